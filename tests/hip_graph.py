"""Stream capture and graph replay through ctypes on libamdhip64.so, the runtime libbert.so is linked against: device buffers,
streams, a capture that always ends, the kernel nodes of a graph, instantiate / launch / destroy.  Every capture is on ONE stream
(no fork onto a second one, no parallel branches).  A helper module for test_gpu_stream_capture.py, not a conftest."""
import contextlib
import ctypes as C

import numpy as np

HIP_SUCCESS = 0
CAPTURE_MODE_THREAD_LOCAL = 1          # hipStreamCaptureModeThreadLocal
NODE_TYPE_KERNEL = 0                   # hipGraphNodeTypeKernel
H2D, D2H = 1, 2                        # hipMemcpyHostToDevice, hipMemcpyDeviceToHost


class Capture:
    """What `capture` yields: after the block, `status` is hipStreamEndCapture's result and `graph` the graph (None without one)."""
    status = None
    graph = None


class Hip:
    def __init__(self):
        self.lib = C.CDLL("libamdhip64.so")

    # ---- device memory (blocking; never call these inside a capture block) ----
    def malloc(self, nbytes):
        p = C.c_void_p()
        assert self.lib.hipMalloc(C.byref(p), C.c_size_t(max(int(nbytes), 16))) == HIP_SUCCESS
        return p.value

    def write(self, p, arr):
        """arr over the buffer at p, in place, after everything queued on the device has finished"""
        arr = np.ascontiguousarray(arr)
        assert self.lib.hipDeviceSynchronize() == HIP_SUCCESS
        assert self.lib.hipMemcpy(C.c_void_p(p), C.c_void_p(arr.ctypes.data), C.c_size_t(arr.nbytes), H2D) == HIP_SUCCESS

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        p = self.malloc(arr.nbytes)
        self.write(p, arr)
        return p

    def nans(self, shape, dtype=np.float32):
        """a new buffer of that shape, every element NaN (integers: -1)"""
        return self.upload(self._poison(shape, dtype))

    def poison(self, p, shape, dtype=np.float32):
        self.write(p, self._poison(shape, dtype))

    @staticmethod
    def _poison(shape, dtype):
        return np.full(shape, -1 if np.issubdtype(dtype, np.integer) else np.nan, dtype=dtype)

    def download(self, p, shape, dtype=np.float32):
        out = np.empty(shape, dtype=dtype)
        assert self.lib.hipDeviceSynchronize() == HIP_SUCCESS
        assert self.lib.hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(p), C.c_size_t(out.nbytes), D2H) == HIP_SUCCESS
        return out

    def free(self, *ptrs):
        for p in ptrs:
            assert self.lib.hipFree(C.c_void_p(p)) == HIP_SUCCESS

    def sync(self):
        assert self.lib.hipDeviceSynchronize() == HIP_SUCCESS

    # ---- streams ----
    def stream(self):
        s = C.c_void_p()
        assert self.lib.hipStreamCreate(C.byref(s)) == HIP_SUCCESS
        return s.value

    def destroy_stream(self, s):
        assert self.lib.hipStreamDestroy(C.c_void_p(s)) == HIP_SUCCESS

    # ---- capture and graphs ----
    @contextlib.contextmanager
    def capture(self, stream):
        """hipStreamBeginCapture(stream, thread-local) ... hipStreamEndCapture, which runs whatever the block did, also when it raised:
        a failing test must not leave the thread capturing.  Yields a Capture; its fields are set when the block is left."""
        assert stream, "a capture needs a stream of its own, not the null stream"
        assert self.lib.hipStreamBeginCapture(C.c_void_p(stream), CAPTURE_MODE_THREAD_LOCAL) == HIP_SUCCESS
        cap = Capture()
        try:
            yield cap
        finally:
            g = C.c_void_p()
            cap.status = int(self.lib.hipStreamEndCapture(C.c_void_p(stream), C.byref(g)))
            cap.graph = g.value
            if cap.status != HIP_SUCCESS:
                self.lib.hipGetLastError()                   # (the failed capture's error must not show up in a later call's check)

    def capture_status(self, stream):
        """hipStreamIsCapturing: 0 none, 1 active, 2 invalidated"""
        st = C.c_int(-1)
        assert self.lib.hipStreamIsCapturing(C.c_void_p(stream), C.byref(st)) == HIP_SUCCESS
        return st.value

    def kernel_nodes(self, graph):
        """the number of kernel nodes of the graph (hipGraphGetNodes, hipGraphNodeGetType)"""
        n = C.c_size_t(0)
        assert self.lib.hipGraphGetNodes(C.c_void_p(graph), None, C.byref(n)) == HIP_SUCCESS
        if n.value == 0:
            return 0
        nodes = (C.c_void_p * n.value)()
        assert self.lib.hipGraphGetNodes(C.c_void_p(graph), nodes, C.byref(n)) == HIP_SUCCESS
        kernels = 0
        for node in nodes[:n.value]:
            t = C.c_int(-1)
            assert self.lib.hipGraphNodeGetType(C.c_void_p(node), C.byref(t)) == HIP_SUCCESS
            kernels += t.value == NODE_TYPE_KERNEL
        return kernels

    def instantiate(self, graph):
        ex = C.c_void_p()
        assert self.lib.hipGraphInstantiate(C.byref(ex), C.c_void_p(graph), None, None, C.c_size_t(0)) == HIP_SUCCESS
        return ex.value

    def launch(self, graph_exec, stream):
        assert self.lib.hipGraphLaunch(C.c_void_p(graph_exec), C.c_void_p(stream)) == HIP_SUCCESS

    def destroy(self, graph_exec=None, graph=None):
        """after everything queued has finished (a graph may still be running)"""
        self.sync()
        if graph_exec:
            assert self.lib.hipGraphExecDestroy(C.c_void_p(graph_exec)) == HIP_SUCCESS
        if graph:
            assert self.lib.hipGraphDestroy(C.c_void_p(graph)) == HIP_SUCCESS
