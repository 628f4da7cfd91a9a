"""The token index's MXFP4 form without a GPU: the Python surface names it, and its create refuses a missing context as the other
forms' do."""
from bert_cpp_amd import pybert


def test_the_surface_names_the_form_and_create_wants_a_context(capfd):
    assert pybert.BertTokenIndex.DTYPES["mxfp4"] == 4
    L = pybert.lib()
    capfd.readouterr()
    assert not L.bert_hip_late_index_create(None, 8, 4)
    assert "bert_hip_late_index_create: no context" in capfd.readouterr().err
