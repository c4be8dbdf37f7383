"""ctypes binding of libzkmi_probe.so (csrc/probe.hip), the test-only library that runs single production arithmetic functions on the device,
one test vector per lane, and returns their raw output words.  Test infrastructure only: the package never loads it."""
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(ROOT, "noir_backend_using_gnark_amd", "libzkmi_probe.so")

_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("%s is missing: run `make -C noir_backend_using_gnark_amd/csrc`" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        L.zk_probe_op.argtypes = [C.c_char_p]
        L.zk_probe_op.restype = C.c_int
        L.zk_probe_shape.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.zk_probe_shape.restype = C.c_int
        L.zk_probe.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
        L.zk_probe.restype = C.c_int
        _lib = L
    return _lib


def shape(name):
    """(op code, words per input vector, words per output vector)"""
    L = lib()
    op = L.zk_probe_op(name.encode())
    if op < 0:
        raise KeyError(name)
    i, o = C.c_int(), C.c_int()
    assert L.zk_probe_shape(op, C.byref(i), C.byref(o)) == 0
    return op, i.value, o.value


def run(name, vectors):
    """vectors: a list of word lists (each at most the op's input width; zero-padded) or a uint32 array of shape (n, IN).
    Returns the raw output words as a uint32 array of shape (n, OUT)."""
    op, iw, ow = shape(name)
    if isinstance(vectors, np.ndarray):
        a = np.ascontiguousarray(vectors, dtype=np.uint32)
        assert a.ndim == 2 and a.shape[1] == iw, (a.shape, iw)
    else:
        a = np.zeros((len(vectors), iw), dtype=np.uint32)
        for k, v in enumerate(vectors):
            assert len(v) <= iw, (name, len(v), iw)
            a[k, :len(v)] = v
    n = a.shape[0]
    out = np.zeros((n, ow), dtype=np.uint32)
    rc = lib().zk_probe(op, a.ctypes.data, a.nbytes, out.ctypes.data, n)
    if rc != 0:
        raise RuntimeError("zk_probe(%s) returned %d" % (name, rc))
    return out
