// bert-search — the reference's "find similar texts" demo (its README; examples/sample_dylib.py and sample_client.py) in one
// process on the GPU: every line of a text file is embedded straight into an HBM-resident index (bert_hip_index_add_texts),
// then each line read from stdin is a query whose k closest texts are printed in the reference's format.  'q' or the end
// of the input quits.  Public C API of include/bert.h + include/bert_hip.h only.
//
//   bert-search -m MODEL -f TEXTS [-k 3] [--f32 | --i8 | --b1] [--rescore N] [--lists N] [--nprobe P] [-t THREADS] [--save PATH] [--load PATH]
//               [--long [--window W] [--stride S]] [--maxsim N [--token-index] | --cross-model PATH --cross N]
//   bert-search -m MODEL -f TEXTS --late [--i8] [-k 3] [-t THREADS] [--save-tokens PATH] [--load-tokens PATH]
//   bert-search -m MODEL -f TEXTS --sparse [WIDTH] [--inverted] [-k 3] [--f16] [-t THREADS] [--save PATH] [--load PATH]
//   bert-search -m DENSE -f TEXTS --hybrid SPLADE [--postings] [--sparse-width W] [--weights WD,WS] [-k 3] [--f32 | --i8 | --b1] [--f16] [-t THREADS]
//   (--hybrid SPLADE: hybrid search.  SPLADE is a second model file, one with the MLM head, loaded into a context of its own (it may be
//   the same file as DENSE).  Every line goes into an embedding index of DENSE (bert_hip_index_add_texts; --f32 / --i8 / --b1 as
//   below) and, with its W largest terms (--sparse-width, default 128, 1 .. 256), into a sparse index of SPLADE
//   (bert_hip_sparse_index_add_texts; --f16: u16 ids and f16 weights).  Each query line is answered by bert_hip_hybrid_search_texts:
//   the exact top-k of WD * (dense score) + WS * (sparse score) over all lines (--weights, default 1,1; finite numbers), the query's W
//   largest terms on the sparse side.  --postings: the sparse index's postings are built once the lines are in
//   (bert_hip_sparse_index_invert) and each query goes through bert_hip_dense_sparse_search_inverted_texts — the same lines, the same
//   scores; it goes with --hybrid only (the sparse mode's own switch is --inverted).  Not together with --sparse, --lists, --nprobe, --rescore, --long, --maxsim, --cross, --save, --load.)
//   (--sparse [WIDTH]: learned sparse search.  MODEL must carry the MLM head (bert_hip.h "learned sparse embeddings"); every line's WIDTH
//   largest terms (default 128, 1 .. 256) go into a sparse index (bert_hip_sparse_index_add_texts; --f16: u16 ids and f16 weights),
//   each query line is searched with its WIDTH largest terms (bert_hip_sparse_index_search_texts), and the output has the dense mode's
//   shape.  --inverted: the postings are built once the lines are in the index (bert_hip_sparse_index_invert) and the queries go through
//   bert_hip_sparse_index_search_inverted_texts — the same lines, the same scores; not together with --hybrid.
//   Lines without a term in common with the query score 0 and are not printed.  --save: the sparse index goes to PATH once it
//   is built (bert_hip_sparse_index_save); --load: it comes from PATH instead of being encoded (bert_hip_sparse_index_load; its stored
//   type is the file's) — TEXTS is still read, for printing, and must have as many lines as the index has rows.  The dense mode's other
//   options do not apply.)
//   (--cross-model PATH --cross N: cross-encoder reranking.  PATH is a second model file, one with a classification head (bert_hip.h
//   "sentence pairs and scores"), loaded into a context of its own.  The stages above return N candidates per query line instead of k
//   (k <= N <= 256, and N <= --rescore's); bert_hip_score_pairs scores the pairs (query line, candidate line) — each pair read as one
//   sentence, cut at the cross-encoder's position limit —, and the k lines printed are the best by the first label's logit, which is
//   shown; equal scores keep the first stage's order.  Not together with --maxsim.)
//   (--maxsim N: late-interaction reranking.  The stages above return N candidates per query line instead of k (k <= N <= 256, and
//   N <= --rescore's); the query and the N candidate lines go through bert_hip_encode_tokens_batch (token rows, each over its L2
//   norm, lines cut at the model's position limit), bert_hip_maxsim scores the pairs (query, candidate j) — the sum over the query's
//   tokens of the best cosine among the candidate's tokens —, and the k lines printed are the best by that score, which is shown;
//   equal scores keep the first stage's order.  --token-index: the lines' token rows go into a token index while the dense index is
//   built (bert_hip_token_index_add_texts), and the N candidates are scored by bert_hip_token_index_rescore from the stored rows
//   instead of being encoded again: only the query goes through the model.  The printed lines and scores are those of --maxsim N alone.
//   Not together with --long, --sparse, --hybrid, --cross, --save, --load.)
//   (--late: late-interaction search without a dense stage.  Every line's token rows go into a token index; each query line is answered
//   by bert_hip_token_index_search_texts, the exact top-k of the MaxSim score over ALL lines.  A query of more tokens than the index's
//   bert_hip_token_index_max_query_tokens is refused.  With -m, -f, -k, -t, --i8, --save-tokens and --load-tokens only.)
//   (--i8 with --late or with --maxsim N --token-index: the token index is an int8 one (bert_hip_late_index_create with dtype 2: int8
//   codes and a scale per token); with --maxsim N --token-index the dense index is the int8 one too, as --i8 says without a token
//   index.  Not together with --save-tokens or --load-tokens: an int8 token index has no file form.)
//   (--save-tokens PATH / --load-tokens PATH, with --late or with --maxsim N --token-index: the token index goes to PATH once it is built
//   (bert_hip_late_index_save), or comes from PATH instead of the lines being encoded (bert_hip_late_index_load) — TEXTS is still read,
//   for printing, and must have as many lines as the index has documents.  --save and --load are the dense index's and stay refused.)
//   (--long: a line may be longer than the model's position limit: it is cut into overlapping windows of W ids, S inner ids apart,
//   and embedded as ONE row (bert_hip_index_add_long_texts; W defaults to 128 or the model's limit if that is less, S to three
//   quarters of W - 2).  Without --long a line is cut at the model's position limit, like a query;
//   --f32: an f32 index; --i8: an int8 index, one code per element and one scale per row; --b1: one sign bit per element; the
//   default stores the rows as f16; --rescore N: an int8 index of the same texts is kept beside the index, which only picks N
//   candidates per query, and the answer is the int8 index's best k of them (bert_hip_index_search_rescored; k <= N <= 256);
//   --lists N: once the texts are in, the index is partitioned into N lists (bert_hip_index_kmeans, ten iterations from N evenly
//   spaced rows, then bert_hip_index_partition); --nprobe P: each query then scans only its P nearest lists
//   (bert_hip_index_search_probed; 1 <= P <= min(lists, 256)); with --rescore the partitioned index is the coarse one: it picks
//   the N candidates among the P lists, which the int8 index rescores (bert_hip_index_search_rescored_probed);
//   --save: the index goes to PATH (bert_hip_index_save) once it is built, and the partition of a partitioned one to PATH.part
//   (bert_hip_index_partition_save); --load: the index comes from PATH instead of being embedded — TEXTS is still read, for
//   printing, and must have as many lines as the index has rows —, and its partition from PATH.part where that file exists
//   (bert_hip_index_partition_load: --nprobe then needs no --lists))
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "bert.h"
#include "bert_hip.h"

namespace {
void usage(const char *argv0) {
    fprintf(stderr, "usage: %s -m MODEL -f TEXTS [-k 3] [--f32 | --i8 | --b1] [--rescore N] [--lists N] [--nprobe P] [-t THREADS] [--save PATH] [--load PATH] [--long [--window W] [--stride S]] [--maxsim N [--token-index] | --cross-model PATH --cross N] [--save-tokens PATH] [--load-tokens PATH]\n", argv0);
    fprintf(stderr, "       %s -m MODEL -f TEXTS --late [--i8] [-k 3] [-t THREADS] [--save-tokens PATH] [--load-tokens PATH]\n", argv0);
    fprintf(stderr, "       %s -m MODEL -f TEXTS --sparse [WIDTH] [--inverted] [-k 3] [--f16] [-t THREADS] [--save PATH] [--load PATH]\n", argv0);
    fprintf(stderr, "       %s -m DENSE -f TEXTS --hybrid SPLADE [--postings] [--sparse-width W] [--weights WD,WS] [-k 3] [--f32 | --i8 | --b1] [--f16] [-t THREADS]\n", argv0);
    fprintf(stderr, "  --hybrid SPLADE: hybrid search: the lines in an embedding index of DENSE and a sparse index of SPLADE (a model file with the MLM head; W\n"
                    "          terms a line, default 128), each query answered by bert_hip_hybrid_search_texts: the exact top-k of WD * dense + WS * sparse\n"
                    "          (default 1,1).  --postings builds the sparse index's postings and answers through them (the same output).\n"
                    "          Not with --sparse, --lists, --nprobe, --rescore, --long, --maxsim, --cross, --save, --load.\n");
    fprintf(stderr, "  --sparse [WIDTH]: learned sparse search with a model that carries the MLM head: each line's and each query's WIDTH largest terms\n"
                    "          (default 128, 1 .. 256) through a sparse index (bert_hip_sparse_index_*); --f16 stores u16 ids and f16 weights;\n"
                    "          --save PATH writes the sparse index once it is built, --load PATH reads it instead of encoding TEXTS (still read for printing);\n"
                    "          --inverted builds the postings and answers through the inverted search (the same output; not with --hybrid).\n");
    fprintf(stderr, "  --long: lines of any length, cut into overlapping windows of W ids, S inner ids apart, one row per line (defaults: W 128 or the\n"
                    "          model's position limit if that is less, S three quarters of W - 2).  Without --long a line is cut at the model's position limit.\n");
    fprintf(stderr, "  --maxsim N: the search returns N candidates (k <= N <= 256), which are reranked by the MaxSim score of their token rows against the\n"
                    "          query's (bert_hip_encode_tokens_batch + bert_hip_maxsim); the k best by that score are printed with it.\n");
    fprintf(stderr, "  --token-index: with --maxsim N: the lines' token rows are kept in a token index (bert_hip_token_index_add_texts) and the candidates are\n"
                    "          scored from it (bert_hip_token_index_rescore) instead of being encoded again; the same lines and scores are printed.\n");
    fprintf(stderr, "  --late: no dense stage: the lines' token rows in a token index, each query answered by bert_hip_token_index_search_texts, the exact\n"
                    "          top-k by MaxSim score over all lines.  With -m, -f, -k, -t, --i8, --save-tokens and --load-tokens only.\n");
    fprintf(stderr, "  --i8 with --late or with --maxsim N --token-index: the token index stores int8 codes and a scale per token (bert_hip_late_index_create,\n"
                    "          dtype 2); not with --save-tokens or --load-tokens: an int8 token index has no file form.\n");
    fprintf(stderr, "  --save-tokens PATH, --load-tokens PATH: with --late or with --maxsim N --token-index: the token index is written to PATH once it is built\n"
                    "          (bert_hip_late_index_save), or read from PATH instead of encoding TEXTS (bert_hip_late_index_load; TEXTS is still read for printing).\n");
    fprintf(stderr, "  --cross-model PATH --cross N: the search returns N candidates (k <= N <= 256), which a cross-encoder (a model file with a classification\n"
                    "          head) reranks: bert_hip_score_pairs on (query, candidate); the k best by the first label's logit are printed with it.\n");
}

std::string chomp(std::string s) {
    while (!s.empty() && (s.back() == '\n' || s.back() == '\r')) s.pop_back();
    return s;
}
}  // namespace

int main(int argc, char **argv) {
    const char *model = nullptr, *file = nullptr, *save = nullptr, *load = nullptr, *cross_model = nullptr, *hybrid_model = nullptr;
    const char *save_tokens = nullptr, *load_tokens = nullptr;
    float w_dense = 1.f, w_sparse = 1.f;
    bool weights_ok = true;
    int k = 3, n_threads = 6, dtype = 1, n_cand = 0, n_lists = 0, nprobe = 0, window = 0, stride = 0, n_maxsim = 0, n_cross = 0;
    bool long_texts = false, maxsim = false, cross = false, sparse = false, sparse_f16 = false, token_index = false, late = false, inverted = false, postings = false;
    int sparse_width = 128;
    for (int i = 1; i < argc; ++i) {
        const bool has_value = i + 1 < argc;
        if ((!strcmp(argv[i], "-m") || !strcmp(argv[i], "--model")) && has_value) model = argv[++i];
        else if ((!strcmp(argv[i], "-f") || !strcmp(argv[i], "--file")) && has_value) file = argv[++i];
        else if (!strcmp(argv[i], "-k") && has_value) k = atoi(argv[++i]);
        else if ((!strcmp(argv[i], "-t") || !strcmp(argv[i], "--threads")) && has_value) n_threads = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--save") && has_value) save = argv[++i];
        else if (!strcmp(argv[i], "--load") && has_value) load = argv[++i];
        else if (!strcmp(argv[i], "--save-tokens") && has_value) save_tokens = argv[++i];
        else if (!strcmp(argv[i], "--load-tokens") && has_value) load_tokens = argv[++i];
        else if (!strcmp(argv[i], "--f32")) dtype = 0;
        else if (!strcmp(argv[i], "--i8")) dtype = 2;
        else if (!strcmp(argv[i], "--b1")) dtype = 3;
        else if (!strcmp(argv[i], "--rescore") && has_value) n_cand = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--lists") && has_value) n_lists = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--nprobe") && has_value) nprobe = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--long")) long_texts = true;
        else if (!strcmp(argv[i], "--sparse")) {
            sparse = true;
            if (has_value && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') sparse_width = atoi(argv[++i]);
        }
        else if (!strcmp(argv[i], "--f16")) sparse_f16 = true;
        else if (!strcmp(argv[i], "--inverted")) inverted = true;
        else if (!strcmp(argv[i], "--postings")) postings = true;
        else if (!strcmp(argv[i], "--hybrid") && has_value) hybrid_model = argv[++i];
        else if (!strcmp(argv[i], "--sparse-width") && has_value) sparse_width = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--weights") && has_value) {
            char tail = 0;
            weights_ok = sscanf(argv[++i], "%f,%f%c", &w_dense, &w_sparse, &tail) == 2 && std::isfinite(w_dense) && std::isfinite(w_sparse);
        }
        else if (!strcmp(argv[i], "--window") && has_value) window = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--stride") && has_value) stride = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--maxsim") && has_value) { maxsim = true; n_maxsim = atoi(argv[++i]); }
        else if (!strcmp(argv[i], "--token-index")) token_index = true;
        else if (!strcmp(argv[i], "--late")) late = true;
        else if (!strcmp(argv[i], "--cross-model") && has_value) cross_model = argv[++i];
        else if (!strcmp(argv[i], "--cross") && has_value) { cross = true; n_cross = atoi(argv[++i]); }
        else { usage(argv[0]); return strcmp(argv[i], "-h") && strcmp(argv[i], "--help") ? 2 : 0; }
    }
    if (!model || !file) { usage(argv[0]); return 2; }
    if (k < 1 || k > 256) { fprintf(stderr, "search: -k must be 1 .. 256\n"); return 2; }
    for (const char *flag : {token_index ? "--token-index" : nullptr, late ? "--late" : nullptr})
        if (flag && (long_texts || sparse || hybrid_model || cross || cross_model || save || load)) {
            fprintf(stderr, "search: %s does not go with --long, --sparse, --hybrid, --cross, --save or --load\n", flag);
            return 2;
        }
    if (token_index && (!maxsim || late)) { fprintf(stderr, "search: --token-index goes with --maxsim N\n"); return 2; }
    if ((save_tokens || load_tokens) && !late && !token_index) {
        fprintf(stderr, "search: --save-tokens and --load-tokens go with --late or with --maxsim N --token-index\n");
        return 2;
    }
    // (--i8 beside a token index: the token index is an int8 one, which has no file form)
    const bool token_i8 = dtype == 2 && (late || token_index);
    if (token_i8 && (save_tokens || load_tokens)) { fprintf(stderr, "search: --i8 with a token index does not go with --save-tokens or --load-tokens\n"); return 2; }
    if (late && (maxsim || (dtype != 1 && dtype != 2) || n_cand || n_lists || nprobe || sparse_f16)) { fprintf(stderr, "search: --late goes with -m, -f, -k, -t and --i8 only\n"); return 2; }
    if (hybrid_model && (sparse || n_cand || n_lists || nprobe || long_texts || maxsim || cross || cross_model || save || load)) {
        fprintf(stderr, "search: --hybrid goes with -m, -f, -k, -t, --sparse-width, --weights, --f32, --i8, --b1 and --f16 only\n");
        return 2;
    }
    if (inverted && hybrid_model) { fprintf(stderr, "search: --inverted does not go with --hybrid: a hybrid search over the postings is --hybrid SPLADE --postings\n"); return 2; }
    if (postings && !hybrid_model) { fprintf(stderr, "search: --postings goes with --hybrid (the sparse mode's switch is --inverted)\n"); return 2; }
    if (inverted && !sparse) { fprintf(stderr, "search: --inverted goes with --sparse\n"); return 2; }
    if (hybrid_model && (sparse_width < 1 || sparse_width > 256)) { fprintf(stderr, "search: --hybrid: --sparse-width must be 1 .. 256\n"); return 2; }
    if (hybrid_model && !weights_ok) { fprintf(stderr, "search: --hybrid: --weights takes two finite numbers, WD,WS\n"); return 2; }
    if (!hybrid_model && (!weights_ok || w_dense != 1.f || w_sparse != 1.f)) { fprintf(stderr, "search: --weights goes with --hybrid\n"); return 2; }
    if (sparse && (sparse_width < 1 || sparse_width > 256)) { fprintf(stderr, "search: --sparse takes a width of 1 .. 256\n"); return 2; }
    if (sparse && (dtype != 1 || n_cand || n_lists || nprobe || long_texts || maxsim || cross || cross_model)) {
        fprintf(stderr, "search: --sparse goes with -m, -f, -k, -t, --f16, --save and --load only\n");
        return 2;
    }
    if (sparse_f16 && !sparse && !hybrid_model) { fprintf(stderr, "search: --f16 goes with --sparse\n"); return 2; }
    if (!long_texts && (window || stride)) { fprintf(stderr, "search: --window and --stride go with --long\n"); return 2; }
    if (maxsim && (n_maxsim < k || n_maxsim > 256)) { fprintf(stderr, "search: --maxsim must be -k .. 256\n"); return 2; }
    if (cross != (cross_model != nullptr)) { fprintf(stderr, "search: --cross-model and --cross go together\n"); return 2; }
    if (cross && maxsim) { fprintf(stderr, "search: --cross and --maxsim exclude each other\n"); return 2; }
    if (cross && (n_cross < k || n_cross > 256)) { fprintf(stderr, "search: --cross must be -k .. 256\n"); return 2; }
    const int k_print = k;
    if (maxsim) k = n_maxsim;                                 // (what the stages below return; k_print lines come out of the reranking)
    if (cross) k = n_cross;
    const bool two_stage = n_cand != 0;
    if (two_stage && (n_cand < k || n_cand > 256)) { fprintf(stderr, "search: --rescore must be %s .. 256\n", maxsim ? "--maxsim's N" : "-k"); return 2; }
    if (two_stage && cross && n_cand < k) { fprintf(stderr, "search: --rescore must be --cross's N .. 256\n"); return 2; }

    if (n_lists < 0 || n_lists > 65536) { fprintf(stderr, "search: --lists must be 1 .. 65536\n"); return 2; }
    // (against the lists themselves once they are there: they may come from --load PATH's PATH.part)
    if (nprobe != 0 && (nprobe < 1 || nprobe > 256 || (n_lists > 0 && nprobe > n_lists) || (n_lists == 0 && !load))) {
        fprintf(stderr, "search: --nprobe must be 1 .. min(lists, 256), the lists those of --lists or of --load PATH's PATH.part\n");
        return 2;
    }

    bert_ctx *ctx = bert_load_from_file(model);
    if (!ctx) {
        fprintf(stderr, "search: failed to load model from '%s'\n", model);
        return 1;
    }
    // the cross-encoder: a context of its own (frees: at exit, behind ctx)
    bert_ctx *cross_ctx = nullptr;
    if (cross) {
        cross_ctx = bert_load_from_file(cross_model);
        if (!cross_ctx || bert_hip_n_labels(cross_ctx) < 1) {
            fprintf(stderr, "search: '%s' %s\n", cross_model, cross_ctx ? "has no classification head" : "failed to load");
            if (cross_ctx) bert_free(cross_ctx);
            bert_free(ctx);
            return 1;
        }
    }
    printf("Loading texts from %s...\n", file);
    std::ifstream in(file);
    if (!in) {
        fprintf(stderr, "search: cannot read '%s'\n", file);
        bert_free(ctx);
        return 1;
    }
    std::vector<std::string> texts;
    for (std::string line; std::getline(in, line);) texts.push_back(chomp(line));
    std::vector<const char *> ptrs;
    for (auto &t : texts) ptrs.push_back(t.c_str());
    if (hybrid_model) {
        // the hybrid mode: the lines into an embedding index of this model and a sparse index of the second one, each query against both
        bert_ctx *sparse_ctx = bert_load_from_file(hybrid_model);
        if (!sparse_ctx || !bert_hip_has_mlm_head(sparse_ctx)) {
            fprintf(stderr, "search: '%s' %s\n", hybrid_model, sparse_ctx ? "has no MLM head" : "failed to load");
            if (sparse_ctx) bert_free(sparse_ctx);
            bert_free(ctx);
            return 1;
        }
        auto fail = [&](const char *what) {
            fprintf(stderr, "search: %s\n", what);
            bert_free(sparse_ctx);
            bert_free(ctx);
            return 1;
        };
        bert_hip_index *dx = bert_hip_index_create(ctx, 0, dtype);
        if (!dx || bert_hip_index_add_texts(dx, n_threads, (int32_t)ptrs.size(), ptrs.data()) < 0) return fail("could not build the index");
        bert_hip_sparse_index *sx = bert_hip_sparse_index_create(sparse_ctx, 0, sparse_width, sparse_f16 ? 1 : 0);
        if (!sx || bert_hip_sparse_index_add_texts(sx, n_threads, (int32_t)ptrs.size(), ptrs.data()) < 0) return fail("could not build the sparse index");
        if (postings && bert_hip_sparse_index_invert(sx) < 0) return fail("could not build the postings");
        printf("Loaded %zu lines.\n", texts.size());
        std::vector<int32_t> hids((size_t)k);
        std::vector<float> hscores((size_t)k);
        for (;;) {
            printf("Enter a text to find similar texts (enter 'q' to quit): ");
            fflush(stdout);
            std::string q;
            if (!std::getline(std::cin, q)) break;
            q = chomp(q);
            if (q == "q") break;
            const char *qp = q.c_str();
            if ((postings ? bert_hip_dense_sparse_search_inverted_texts(dx, sx, n_threads, 1, &qp, sparse_width, w_dense, w_sparse, k, hids.data(), hscores.data())
                          : bert_hip_hybrid_search_texts(dx, sx, n_threads, 1, &qp, sparse_width, w_dense, w_sparse, k, hids.data(), hscores.data())) != 0)
                return fail("the search failed");
            printf("\nClosest texts:\n");
            for (int i = 0; i < k && hids[i] >= 0; ++i) printf("%d. %s\n (similarity score: %.4f)\n", i + 1, texts[hids[i]].c_str(), hscores[i]);
        }
        printf("\n");
        bert_free(sparse_ctx);                                // (frees the sparse index as well)
        bert_free(ctx);
        return 0;
    }
    if (sparse) {
        // the learned sparse mode: the lines' terms into a sparse index, each query's terms against it; nothing below applies
        if (!bert_hip_has_mlm_head(ctx)) {
            fprintf(stderr, "search: --sparse needs a model with the MLM head, '%s' has none\n", model);
            bert_free(ctx);
            return 1;
        }
        bert_hip_sparse_index *sx;
        if (load) {
            sx = bert_hip_sparse_index_load(ctx, load);
            if (!sx) {
                fprintf(stderr, "search: could not load the sparse index from '%s'\n", load);
                bert_free(ctx);
                return 1;
            }
            if ((size_t)bert_hip_sparse_index_size(sx) != texts.size()) {
                fprintf(stderr, "search: '%s' holds %d rows, '%s' has %zu lines\n", load, bert_hip_sparse_index_size(sx), file, texts.size());
                bert_free(ctx);
                return 1;
            }
        } else {
            sx = bert_hip_sparse_index_create(ctx, 0, sparse_width, sparse_f16 ? 1 : 0);
            if (!sx || bert_hip_sparse_index_add_texts(sx, n_threads, (int32_t)ptrs.size(), ptrs.data()) < 0) {
                fprintf(stderr, "search: could not build the sparse index\n");
                bert_free(ctx);
                return 1;
            }
        }
        if (save && bert_hip_sparse_index_save(sx, save) != 0) {
            fprintf(stderr, "search: could not save the sparse index to '%s'\n", save);
            bert_free(ctx);
            return 1;
        }
        if (inverted && bert_hip_sparse_index_invert(sx) < 0) {
            fprintf(stderr, "search: could not build the postings\n");
            bert_free(ctx);
            return 1;
        }
        printf("Loaded %zu lines.\n", texts.size());
        std::vector<int32_t> sids((size_t)k);
        std::vector<float> sscores((size_t)k);
        for (;;) {
            printf("Enter a text to find similar texts (enter 'q' to quit): ");
            fflush(stdout);
            std::string q;
            if (!std::getline(std::cin, q)) break;
            q = chomp(q);
            if (q == "q") break;
            const char *qp = q.c_str();
            if ((inverted ? bert_hip_sparse_index_search_inverted_texts(sx, n_threads, 1, &qp, sparse_width, k, sids.data(), sscores.data())
                          : bert_hip_sparse_index_search_texts(sx, n_threads, 1, &qp, sparse_width, k, sids.data(), sscores.data())) != 0) {
                fprintf(stderr, "search: the search failed\n");
                bert_free(ctx);
                return 1;
            }
            printf("\nClosest texts:\n");
            // (a line that shares no term with the query scores 0: not a match)
            for (int i = 0; i < k && sids[i] >= 0 && sscores[i] > 0.f; ++i) printf("%d. %s\n (similarity score: %.4f)\n", i + 1, texts[sids[i]].c_str(), sscores[i]);
        }
        printf("\n");
        bert_free(ctx);                                       // (frees the sparse index as well)
        return 0;
    }
    // the lines' token rows in a token index: encoded, or (--load-tokens) from a file; written (--save-tokens) once they are there.
    // NULL after a line on stderr
    auto token_index_of_lines = [&]() -> bert_hip_token_index * {
        bert_hip_token_index *t;
        if (load_tokens) {
            t = bert_hip_late_index_load(ctx, load_tokens);
            if (!t) { fprintf(stderr, "search: could not load the token index from '%s'\n", load_tokens); return nullptr; }
            if ((size_t)bert_hip_token_index_size(t) != texts.size()) {
                fprintf(stderr, "search: '%s' holds %d documents, '%s' has %zu lines\n", load_tokens, bert_hip_token_index_size(t), file, texts.size());
                return nullptr;
            }
        } else {
            t = token_i8 ? bert_hip_late_index_create(ctx, 0, 2) : bert_hip_token_index_create(ctx, 0);
            if (!t || bert_hip_token_index_add_texts(t, n_threads, (int32_t)ptrs.size(), ptrs.data()) < 0) {
                fprintf(stderr, "search: could not build the token index\n");
                return nullptr;
            }
        }
        if (save_tokens && bert_hip_late_index_save(t, save_tokens) != 0) {
            fprintf(stderr, "search: could not save the token index to '%s'\n", save_tokens);
            return nullptr;
        }
        return t;
    };
    if (late) {
        // the late-interaction mode: the lines' token rows into a token index, each query's token rows against all of them
        bert_hip_token_index *tx = token_index_of_lines();
        if (!tx) {
            bert_free(ctx);
            return 1;
        }
        printf("Loaded %zu lines.\n", texts.size());
        std::vector<int32_t> tids((size_t)k);
        std::vector<float> tscores((size_t)k);
        for (;;) {
            printf("Enter a text to find similar texts (enter 'q' to quit): ");
            fflush(stdout);
            std::string q;
            if (!std::getline(std::cin, q)) break;
            q = chomp(q);
            if (q == "q") break;
            const char *qp = q.c_str();
            if (bert_hip_token_index_search_texts(tx, n_threads, 1, &qp, k, tids.data(), tscores.data()) != 0) {
                fprintf(stderr, "search: the search failed\n");
                bert_free(ctx);
                return 1;
            }
            printf("\nClosest texts:\n");
            for (int i = 0; i < k && tids[i] >= 0; ++i) printf("%d. %s\n (MaxSim score: %.4f)\n", i + 1, texts[tids[i]].c_str(), tscores[i]);
        }
        printf("\n");
        bert_free(ctx);                                       // (frees the token index as well)
        return 0;
    }
    if (long_texts) {
        if (!window) window = bert_n_max_tokens(ctx) < 128 ? bert_n_max_tokens(ctx) : 128;
        if (!stride) stride = 3 * (window - 2) / 4 > 1 ? 3 * (window - 2) / 4 : 1;
    }
    // the file's lines into an index: cut at the model's position limit, or (--long) whole, as overlapping windows pooled per line
    auto add_lines = [&](bert_hip_index *to) {
        return long_texts ? bert_hip_index_add_long_texts(to, n_threads, (int32_t)ptrs.size(), ptrs.data(), window, stride)
                          : bert_hip_index_add_texts(to, n_threads, (int32_t)ptrs.size(), ptrs.data());
    };

    bert_hip_index *ix;
    if (load) {
        ix = bert_hip_index_load(ctx, load);
        if (!ix) {
            fprintf(stderr, "search: could not load the index from '%s'\n", load);
            bert_free(ctx);
            return 1;
        }
        if ((size_t)bert_hip_index_size(ix) != texts.size()) {
            fprintf(stderr, "search: '%s' holds %d rows, '%s' has %zu lines\n", load, bert_hip_index_size(ix), file, texts.size());
            bert_free(ctx);
            return 1;
        }
        // the partition saved beside the index, if there is one
        const std::string part = std::string(load) + ".part";
        if (std::ifstream(part).good() && bert_hip_index_partition_load(ix, part.c_str()) != 0) {
            fprintf(stderr, "search: could not load the partition from '%s'\n", part.c_str());
            bert_free(ctx);
            return 1;
        }
    } else {
        ix = bert_hip_index_create(ctx, 0, dtype);
        if (!ix || add_lines(ix) < 0) {
            fprintf(stderr, "search: could not build the index\n");
            bert_free(ctx);
            return 1;
        }
    }
    // --token-index: the lines' token rows, kept for the reranking
    bert_hip_token_index *tx = nullptr;
    if (token_index) {
        tx = token_index_of_lines();
        if (!tx) {
            bert_free(ctx);
            return 1;
        }
    }
    // the finer index of a two-stage search: the same texts as int8 rows
    bert_hip_index *fine = nullptr;
    if (two_stage) {
        fine = bert_hip_index_create(ctx, 0, 2);
        if (!fine || add_lines(fine) < 0) {
            fprintf(stderr, "search: could not build the int8 index to rescore with\n");
            bert_free(ctx);
            return 1;
        }
    }
    if (n_lists > 0) {
        // centroids: ten k-means iterations from n_lists evenly spaced rows
        const int32_t size = bert_hip_index_size(ix);
        if (n_lists > size) {
            fprintf(stderr, "search: --lists %d exceeds the %d texts\n", n_lists, size);
            bert_free(ctx);
            return 1;
        }
        std::vector<int32_t> seeds((size_t)n_lists);
        for (int i = 0; i < n_lists; ++i) seeds[(size_t)i] = (int32_t)((int64_t)i * size / n_lists);
        std::vector<float> centroids((size_t)n_lists * bert_n_embd(ctx));
        if (bert_hip_index_get_rows(ix, n_lists, seeds.data(), centroids.data()) != 0 || bert_hip_index_kmeans(ix, n_lists, 10, centroids.data()) != 0 ||
            bert_hip_index_partition(ix, n_lists, centroids.data()) != 0) {
            fprintf(stderr, "search: could not partition the index\n");
            bert_free(ctx);
            return 1;
        }
    }
    if (nprobe > bert_hip_index_n_lists(ix)) {
        fprintf(stderr, "search: --nprobe %d exceeds the index's %d lists\n", nprobe, bert_hip_index_n_lists(ix));
        bert_free(ctx);
        return 1;
    }
    if (save && bert_hip_index_save(ix, save) != 0) {
        fprintf(stderr, "search: could not save the index to '%s'\n", save);
        bert_free(ctx);
        return 1;
    }
    if (save && bert_hip_index_n_lists(ix) > 0 && bert_hip_index_partition_save(ix, (std::string(save) + ".part").c_str()) != 0) {
        fprintf(stderr, "search: could not save the partition to '%s.part'\n", save);
        bert_free(ctx);
        return 1;
    }
    printf("Loaded %zu lines.\n", texts.size());

    std::vector<int32_t> ids((size_t)k);
    std::vector<float> scores((size_t)k);
    std::vector<float> emb((size_t)bert_n_embd(ctx));
    for (;;) {
        printf("Enter a text to find similar texts (enter 'q' to quit): ");
        fflush(stdout);
        std::string q;
        if (!std::getline(std::cin, q)) break;
        q = chomp(q);
        if (q == "q") break;
        const char *qp = q.c_str();
        int32_t r;
        if (two_stage && nprobe > 0) {
            float *ep = emb.data();
            r = bert_hip_encode_batch(ctx, n_threads, 1, &qp, &ep) == 1
                    ? bert_hip_index_search_rescored_probed(ix, fine, 1, emb.data(), nprobe, n_cand, k, nullptr, 0, ids.data(), scores.data()) : -1;
        } else if (two_stage) {
            float *ep = emb.data();
            r = bert_hip_encode_batch(ctx, n_threads, 1, &qp, &ep) == 1
                    ? bert_hip_index_search_rescored(ix, fine, 1, emb.data(), n_cand, k, ids.data(), scores.data()) : -1;
        } else if (nprobe > 0) {
            float *ep = emb.data();
            r = bert_hip_encode_batch(ctx, n_threads, 1, &qp, &ep) == 1
                    ? bert_hip_index_search_probed(ix, 1, emb.data(), nprobe, k, ids.data(), scores.data()) : -1;
        } else {
            r = bert_hip_index_search_texts(ix, n_threads, 1, &qp, k, ids.data(), scores.data());
        }
        if (r != 0) {
            fprintf(stderr, "search: the search failed\n");
            bert_free(ctx);
            return 1;
        }
        if (maxsim) {
            // token rows of the query and the candidates, then the pairs (query, candidate j)
            int n_found = 0;
            while (n_found < k && ids[n_found] >= 0) ++n_found;
            std::vector<const char *> lines{qp};
            for (int j = 0; j < n_found && !tx; ++j) lines.push_back(texts[ids[j]].c_str());
            const int32_t n_in = (int32_t)lines.size(), H = bert_n_embd(ctx);
            std::vector<int32_t> cu((size_t)n_in + 1), pairs;
            const int64_t total = bert_hip_encode_tokens_batch(ctx, n_threads, n_in, lines.data(), 1, cu.data(), nullptr, 0);
            std::vector<float> rows(total > 0 ? (size_t)total * H : 0), ms((size_t)n_found);
            bool ok = total > 0 && bert_hip_encode_tokens_batch(ctx, n_threads, n_in, lines.data(), 1, cu.data(), rows.data(), total) == total;
            if (ok && n_found > 0 && tx) {
                // the candidates' scores from the stored rows, all n_found of them, back in the first stage's order
                std::vector<int32_t> rid((size_t)n_found);
                std::vector<float> rsc((size_t)n_found);
                ok = bert_hip_token_index_rescore(tx, 1, cu.data(), rows.data(), n_found, ids.data(), n_found, rid.data(), rsc.data()) == 0;
                for (int j = 0; ok && j < n_found; ++j) {
                    const auto at = std::find(rid.begin(), rid.end(), ids[j]);
                    ok = at != rid.end();
                    if (ok) ms[j] = rsc[(size_t)(at - rid.begin())];
                }
            } else if (ok && n_found > 0) {
                const int32_t qcu[2] = {0, cu[1]};
                std::vector<int32_t> dcu((size_t)n_found + 1);
                for (int j = 0; j <= n_found; ++j) { dcu[j] = cu[j + 1] - cu[1]; if (j < n_found) { pairs.push_back(0); pairs.push_back(j); } }
                ok = bert_hip_maxsim(ctx, rows.data(), qcu, 1, rows.data() + (size_t)cu[1] * H, dcu.data(), n_found, H, pairs.data(), n_found, 0, ms.data()) == 0;
            }
            if (!ok) {
                fprintf(stderr, "search: the MaxSim reranking failed\n");
                bert_free(ctx);
                return 1;
            }
            std::vector<int> order((size_t)n_found);
            for (int j = 0; j < n_found; ++j) order[j] = j;
            std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return ms[x] > ms[y]; });
            printf("\nClosest texts:\n");
            for (int i = 0; i < k_print && i < n_found; ++i) printf("%d. %s\n (MaxSim score: %.4f)\n", i + 1, texts[ids[order[i]]].c_str(), ms[order[i]]);
            continue;
        }
        if (cross) {
            int n_found = 0;
            while (n_found < k && ids[n_found] >= 0) ++n_found;
            const int32_t NL = bert_hip_n_labels(cross_ctx);
            std::vector<const char *> qs((size_t)n_found, qp), ds;
            for (int j = 0; j < n_found; ++j) ds.push_back(texts[ids[j]].c_str());
            std::vector<float> cs((size_t)n_found * NL);
            if (n_found > 0 && bert_hip_score_pairs(cross_ctx, n_threads, n_found, qs.data(), ds.data(), 0, cs.data()) != n_found) {
                fprintf(stderr, "search: the cross-encoder reranking failed\n");
                bert_free(cross_ctx);
                bert_free(ctx);
                return 1;
            }
            std::vector<int> order((size_t)n_found);
            for (int j = 0; j < n_found; ++j) order[j] = j;
            std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return cs[(size_t)x * NL] > cs[(size_t)y * NL]; });
            printf("\nClosest texts:\n");
            for (int i = 0; i < k_print && i < n_found; ++i) printf("%d. %s\n (cross-encoder score: %.4f)\n", i + 1, texts[ids[order[i]]].c_str(), cs[(size_t)order[i] * NL]);
            continue;
        }
        printf("\nClosest texts:\n");
        for (int i = 0; i < k && ids[i] >= 0; ++i) printf("%d. %s\n (similarity score: %.4f)\n", i + 1, texts[ids[i]].c_str(), scores[i]);
    }
    printf("\n");
    if (cross_ctx) bert_free(cross_ctx);
    bert_free(ctx);                                           // (frees the index as well)
    return 0;
}
