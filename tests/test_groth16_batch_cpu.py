"""The batch Groth16 prover's C ABI and Python wrappers without a device: both symbols are exported and declared, every argument error comes back with the single
prover's code and message before the device is touched, n_proofs = 0 is an empty result, the wrappers refuse ragged shapes before any C call, and a well-formed
call is ZK_ERR_NO_DEVICE -- there is no CPU fallback."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from noir_backend_using_gnark_amd import _lib
from noir_backend_using_gnark_amd import groth16 as zk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH = ("zk_bn254_groth16_prove_batch", "zk_bn254_groth16_prove_r1cs_batch", "zk_bn254_groth16_batch_info", "zk_bn254_r1cs_eval_abc_rows_dev")
BOGUS = C.c_uint64(0x00ffffffffffff)  # no such handle


def _args(n=2, nc=3, nw=5):
    z = lambda *shape: np.zeros(shape, np.uint64)  # noqa: E731
    return z(n, nc, 4), z(n, nc, 4), z(n, nc, 4), z(n, nw, 4), z(n, 4), z(n, 4), (C.c_uint8 * (128 * n))()


def test_symbols_are_exported_and_declared():
    lib = _lib.lib()
    header = open(os.path.join(ROOT, "include", "zkmi.h")).read()
    for s in BATCH:
        assert s in _lib.SYMBOLS and hasattr(lib, s), s
        assert re.search(r"\bint %s\(" % s, header), s
    assert "ProveBatch" in open(os.path.join(ROOT, "include", "zkmi.hpp")).read()


def test_no_proofs_is_ok_and_writes_nothing():
    lib = _lib.lib()
    out = (C.c_uint8 * 128)(*([0xA5] * 128))
    assert lib.zk_bn254_groth16_prove_batch(BOGUS, None, None, None, C.c_size_t(3), None, C.c_size_t(5), None, None, C.c_size_t(0), 0, out) == _lib.ZK_OK
    assert lib.zk_bn254_groth16_prove_r1cs_batch(BOGUS, BOGUS, None, C.c_size_t(5), None, None, C.c_size_t(0), 0, out) == _lib.ZK_OK
    assert bytes(out) == b"\xa5" * 128
    pk = zk.ProvingKey.from_handle(BOGUS.value, 2, 5, 1)
    assert zk.prove_batch(pk, *(np.zeros((0, k, 4), np.uint64) for k in (3, 3, 3, 5)), np.zeros((0, 4), np.uint64), np.zeros((0, 4), np.uint64)) == []


def test_null_pointers_are_argument_errors_before_the_device():
    lib = _lib.lib()
    a, b, c, w, r, s, out = _args()
    vp, n, nc, nw = _lib.vp, C.c_size_t(2), C.c_size_t(3), C.c_size_t(5)
    pb, rb = lib.zk_bn254_groth16_prove_batch, lib.zk_bn254_groth16_prove_r1cs_batch
    for hole in range(7):
        ptrs = [vp(a), vp(b), vp(c), vp(w), vp(r), vp(s), out]
        ptrs[hole] = None
        assert pb(BOGUS, ptrs[0], ptrs[1], ptrs[2], nc, ptrs[3], nw, ptrs[4], ptrs[5], n, 0, ptrs[6]) == _lib.ZK_ERR_ARG, hole
        assert b"null pointer" in lib.zk_last_error()
    # a, b, c may be null when there are no constraints to read
    want = _lib.ZK_ERR_NO_DEVICE if _lib.device_count() <= 0 else _lib.ZK_ERR_HANDLE
    assert pb(BOGUS, None, None, None, C.c_size_t(0), vp(w), nw, vp(r), vp(s), n, 0, out) == want
    for hole in range(4):
        ptrs = [vp(w), vp(r), vp(s), out]
        ptrs[hole] = None
        assert rb(BOGUS, BOGUS, ptrs[0], nw, ptrs[1], ptrs[2], n, 0, ptrs[3]) == _lib.ZK_ERR_ARG, hole
        assert b"null pointer" in lib.zk_last_error()


def test_well_formed_call_has_no_cpu_fallback():
    """without a device: ZK_ERR_NO_DEVICE; with one, the unknown handle is what is wrong (the single prover's message)"""
    lib = _lib.lib()
    a, b, c, w, r, s, out = _args()
    vp, n, nc, nw = _lib.vp, C.c_size_t(2), C.c_size_t(3), C.c_size_t(5)
    no_dev = _lib.device_count() <= 0
    want = _lib.ZK_ERR_NO_DEVICE if no_dev else _lib.ZK_ERR_HANDLE
    assert lib.zk_bn254_groth16_prove_batch(BOGUS, vp(a), vp(b), vp(c), nc, vp(w), nw, vp(r), vp(s), n, 0, out) == want
    if not no_dev:
        assert b"unknown proving-key handle" in lib.zk_last_error()
    assert lib.zk_bn254_groth16_prove_r1cs_batch(BOGUS, BOGUS, vp(w), nw, vp(r), vp(s), n, 0, out) == want
    if not no_dev:
        assert b"unknown R1CS handle" in lib.zk_last_error()
    rows, batched = C.c_size_t(0), C.c_int(0)
    assert lib.zk_bn254_groth16_batch_info(BOGUS, C.byref(rows), C.byref(batched)) == want
    pk = zk.ProvingKey.from_handle(BOGUS.value, 2, 5, 1)
    with pytest.raises(_lib.ZkmiError) as ei:
        zk.prove_batch(pk, a, b, c, w, r, s)
    assert ei.value.code == want


def test_wrappers_refuse_ragged_shapes_before_any_c_call():
    pk = zk.ProvingKey.from_handle(BOGUS.value, 2, 5, 1)
    r1 = zk.R1CS.from_handle(BOGUS.value, 1, 5, 3)
    a, b, c, w, r, s, _ = _args()
    with pytest.raises(ValueError):
        zk.prove_batch(pk, a[:1], b, c, w, r, s)          # a has another row count than b, c
    with pytest.raises(ValueError):
        zk.prove_batch(pk, a[:1], b[:1], c[:1], w, r, s)  # a, b, c have fewer rows than w
    with pytest.raises(ValueError):
        zk.prove_batch(pk, a, b[:, :2], c, w, r, s)       # widths differ
    with pytest.raises(ValueError):
        zk.prove_batch(pk, a, b, c, w, r[:1], s)          # one r for two rows
    with pytest.raises(ValueError):
        zk.prove_batch(pk, a, b, c, w, r, s[:1])
    with pytest.raises(ValueError):
        zk.prove_batch(pk, a[0], b[0], c[0], w[0], r, s)  # 1-D vectors of limbs are the single prover's arguments
    with pytest.raises(ValueError):
        zk.prove_batch(pk, a, b, c, w[:, :, :3], r, s)    # not limbs
    with pytest.raises(ValueError):
        zk.prove_r1cs_batch(r1, pk, w, r[:1], s)
    with pytest.raises(ValueError):
        zk.prove_r1cs_batch(r1, pk, w[0], r, s)
    with pytest.raises(ValueError):
        zk.prove_batch(pk, 1, 2, 3, 4, r, s, on_device=True)  # device matrices need n_constraints


# ---- the row-batched R1CS step on its own (zk_bn254_r1cs_eval_abc_rows_dev) and the device-pointer form of prove_r1cs_batch
def _fake_buffer(nbytes):
    """a DeviceBuffer that owns nothing (no device here): an address no call may reach, forgotten before the object goes"""
    b = _lib.DeviceBuffer.__new__(_lib.DeviceBuffer)
    b.ptr, b.nbytes = 0, nbytes
    return b


def test_eval_abc_rows_argument_errors_before_the_device():
    lib = _lib.lib()
    fn = lib.zk_bn254_r1cs_eval_abc_rows_dev
    w, a, b, c = (np.zeros((2, 5, 4), np.uint64) for _ in range(4))  # stand-ins for device addresses: no call below gets as far as reading them
    vp, nw = _lib.vp, C.c_size_t(5)
    assert fn(BOGUS, None, nw, C.c_size_t(0), None, None, None, None) == _lib.ZK_OK  # no rows: nothing to do, whatever the rest is
    for hole in range(4):
        ptrs = [vp(w), vp(a), vp(b), vp(c)]
        ptrs[hole] = None
        assert fn(BOGUS, ptrs[0], nw, C.c_size_t(2), ptrs[1], ptrs[2], ptrs[3], None) == _lib.ZK_ERR_ARG, hole
        assert b"null pointer" in lib.zk_last_error()
    no_dev = _lib.device_count() <= 0
    for rows in (2, 65536):  # the handle is looked up before the row limit
        assert fn(BOGUS, vp(w), nw, C.c_size_t(rows), vp(a), vp(b), vp(c), None) == (_lib.ZK_ERR_NO_DEVICE if no_dev else _lib.ZK_ERR_HANDLE)
        if not no_dev:
            assert b"unknown R1CS handle" in lib.zk_last_error()


def test_eval_abc_rows_wrapper_refuses_bad_shapes_before_any_c_call():
    r1 = zk.R1CS.from_handle(BOGUS.value, 1, 5, 3)
    w = np.zeros((2, 5, 4), np.uint64)
    with pytest.raises(ValueError):
        r1.eval_abc_rows(w[0])                               # one vector is eval_abc's argument
    with pytest.raises(ValueError):
        r1.eval_abc_rows(w[:, :, :3])                        # not limbs
    with pytest.raises(ValueError):
        r1.eval_abc_rows(w, rows=3)                          # rows contradicts the array
    with pytest.raises(TypeError):
        r1.eval_abc_rows(w, on_device=True, rows=2)          # host rows are not a device buffer
    with pytest.raises(ValueError):
        r1.eval_abc_rows(_fake_buffer(320), on_device=True)  # a device buffer carries no shape
    with pytest.raises(ValueError):
        r1.eval_abc_rows(_fake_buffer(319), on_device=True, rows=2)  # 2 rows of 5 wires are 320 bytes
    with pytest.raises(ValueError):
        r1.eval_abc_rows(_fake_buffer(320), on_device=True, rows=2, out=[_fake_buffer(192)] * 2)          # three outputs
    with pytest.raises(ValueError):
        r1.eval_abc_rows(_fake_buffer(320), on_device=True, rows=2, out=[_fake_buffer(192)] * 2 + [_fake_buffer(191)])  # 2 rows of 3 constraints are 192 bytes


def test_prove_r1cs_batch_on_device_argument_validation():
    pk = zk.ProvingKey.from_handle(BOGUS.value, 2, 5, 1)
    r1 = zk.R1CS.from_handle(BOGUS.value, 1, 5, 3)
    _, _, _, w, r, s, _ = _args()
    with pytest.raises(TypeError):
        zk.prove_r1cs_batch(r1, pk, w, r, s, on_device=True)           # host rows are not a device buffer
    with pytest.raises(TypeError):
        zk.prove_r1cs_batch(r1, pk, _fake_buffer(320), r, s)           # and a device buffer is not host rows
    with pytest.raises(TypeError):
        zk.prove_r1cs_batch(r1, pk, 12345, r, s, on_device=True)       # a bare address carries no size to check
    with pytest.raises(ValueError):
        zk.prove_r1cs_batch(r1, pk, _fake_buffer(320), r, s[:1], on_device=True)   # the row count comes from r: one s for two rows
    with pytest.raises(ValueError):
        zk.prove_r1cs_batch(r1, pk, _fake_buffer(320), r[:, :3], s, on_device=True)  # not limbs
    with pytest.raises(ValueError):
        zk.prove_r1cs_batch(r1, pk, _fake_buffer(319), r, s, on_device=True)       # 2 rows of 5 wires are 320 bytes
    empty = np.zeros((0, 4), np.uint64)
    assert zk.prove_r1cs_batch(r1, pk, _fake_buffer(0), empty, empty, on_device=True) == []
    # a well-formed call reaches the library with on_device = 1: no device here, or no such handle there
    buf = _fake_buffer(320)
    buf.ptr = w.ctypes.data  # never read: the handles are looked up first
    try:
        with pytest.raises(_lib.ZkmiError) as ei:
            zk.prove_r1cs_batch(r1, pk, buf, r, s, on_device=True)
        assert ei.value.code == (_lib.ZK_ERR_NO_DEVICE if _lib.device_count() <= 0 else _lib.ZK_ERR_HANDLE)
    finally:
        buf.ptr = 0
