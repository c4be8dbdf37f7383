"""CPU suite of the row-batched commitments (zk_bn254_msm_bases_rows[_dev], zk_bn254_msm_rows_info, zk_bn254_plonk_commit_batch_dev): every argument error that
can be decided without a registered handle is decided before a device is looked for -- so it has its code and message on a machine without one --, the Python
mirrors reject bad geometry before they call the library, and the library exports the new symbols.  (offset + n beyond the registered bases needs a handle, and
a handle a device: tests/test_gpu_msm_rows.py has it.)"""
import ctypes as C

import numpy as np
import pytest

from noir_backend_using_gnark_amd import _lib
from noir_backend_using_gnark_amd import bn254 as zb
from noir_backend_using_gnark_amd import kzg as zkzg
from noir_backend_using_gnark_amd import plonk as zp

NEW = ("zk_bn254_msm_bases_rows", "zk_bn254_msm_bases_rows_dev", "zk_bn254_msm_rows_info", "zk_bn254_plonk_commit_batch_dev")
UNKNOWN = C.c_uint64(0x123456)  # no such handle on entry 0
FAKE = 0x7F0000001000           # a "device pointer" the library never dereferences on these paths (aligned)


def _err():
    return (_lib.lib().zk_last_error() or b"").decode()


def _rows_dev(handle, offset, ptr, stride, n, rows, flags, out, comp, cfg=None):
    cfg = cfg or _lib.MsmCfg(0, 1, 0, 0)
    return _lib.lib().zk_bn254_msm_bases_rows_dev(handle, C.c_size_t(offset), C.c_void_p(ptr), C.c_size_t(stride), C.c_size_t(n), C.c_size_t(rows), C.byref(cfg),
                                                  C.c_uint32(flags), C.c_void_p(out), C.c_void_p(comp))


def _rows_host(handle, offset, ptr, n, rows, flags, out, comp):
    cfg = _lib.MsmCfg(0, 1, 0, 0)
    return _lib.lib().zk_bn254_msm_bases_rows(handle, C.c_size_t(offset), C.c_void_p(ptr), C.c_size_t(n), C.c_size_t(rows), C.byref(cfg), C.c_uint32(flags),
                                              C.c_void_p(out), C.c_void_p(comp))


def test_new_symbols_are_declared_and_exported():
    lib = _lib.lib()
    for s in NEW:
        assert s in _lib.SYMBOLS, s
        assert hasattr(lib, s), s


@pytest.mark.parametrize("call", [_rows_dev, lambda h, off, p, stride, n, rows, fl, o, c: _rows_host(h, off, p, n, rows, fl, o, c)], ids=["dev", "host"])
def test_rows_entry_argument_errors_need_no_device(call):
    # unknown flag bits
    assert call(UNKNOWN, 0, FAKE, 8, 8, 2, 4, FAKE, 0) == _lib.ZK_ERR_ARG
    assert "flag" in _err()
    # null pointers: the scalars, both outputs, the points without the bit that allows leaving them out
    assert call(UNKNOWN, 0, 0, 8, 8, 2, 0, FAKE, 0) == _lib.ZK_ERR_ARG
    assert "null pointer" in _err()
    assert call(UNKNOWN, 0, FAKE, 8, 8, 2, 0, 0, 0) == _lib.ZK_ERR_ARG
    assert "null pointer" in _err()
    assert call(UNKNOWN, 0, FAKE, 8, 8, 2, zb.MSM_ROWS_SPARSE, 0, FAKE) == _lib.ZK_ERR_ARG
    assert "ZK_MSM_ROWS_NO_POINTS" in _err()
    # with everything in order the handle is looked up -- and is unknown -- before any device
    assert call(UNKNOWN, 0, FAKE, 8, 8, 2, zb.MSM_ROWS_NO_POINTS, 0, FAKE) == _lib.ZK_ERR_HANDLE
    assert "unknown bases handle" in _err()
    assert call(UNKNOWN, 0, FAKE, 8, 8, 2, 0, FAKE, FAKE + 4096) == _lib.ZK_ERR_HANDLE


def test_rows_dev_entry_stride_and_alignment_errors_need_no_device():
    assert _rows_dev(UNKNOWN, 0, FAKE, 7, 8, 2, 0, FAKE + 4096, 0) == _lib.ZK_ERR_ARG
    assert "row_stride = 7 is below n = 8" in _err()
    # one row has no stride to speak of: the call goes on to the handle
    assert _rows_dev(UNKNOWN, 0, FAKE, 0, 8, 1, 0, FAKE + 4096, 0) == _lib.ZK_ERR_HANDLE
    assert _rows_dev(UNKNOWN, 0, FAKE, 8, 8, 2, 0, FAKE + 4096 + 8, 0) == _lib.ZK_ERR_ARG
    assert "aligned" in _err()
    assert _rows_dev(UNKNOWN, 0, FAKE, 8, 8, 2, 0, FAKE + 4096, FAKE + 8192 + 2) == _lib.ZK_ERR_ARG
    assert "aligned" in _err()


def test_rows_info_argument_errors_need_no_device():
    chunk, batched = C.c_size_t(0), C.c_int(0)
    lib = _lib.lib()
    assert lib.zk_bn254_msm_rows_info(UNKNOWN, C.c_size_t(8), C.c_uint32(8), C.byref(chunk), C.byref(batched)) == _lib.ZK_ERR_ARG
    assert "flag" in _err()
    assert lib.zk_bn254_msm_rows_info(UNKNOWN, C.c_size_t(8), C.c_uint32(1), C.byref(chunk), C.byref(batched)) == _lib.ZK_ERR_HANDLE
    assert "unknown bases handle" in _err()
    rb = zb.ResidentBases.__new__(zb.ResidentBases)
    rb.is_g2, rb.handle, rb.n = False, UNKNOWN, 16
    with pytest.raises(_lib.ZkmiError) as ei:
        zb.msm_rows_info(rb, 8)
    assert ei.value.code == _lib.ZK_ERR_HANDLE


def test_plonk_commit_door_argument_errors_need_no_device():
    lib = _lib.lib()
    door = lambda h, rows_ptr, stride, ln, rows, fv, o, c: lib.zk_bn254_plonk_commit_batch_dev(  # noqa: E731
        h, C.c_void_p(rows_ptr), C.c_size_t(stride), C.c_size_t(ln), C.c_size_t(rows), C.c_int(fv), C.c_void_p(o), C.c_void_p(c))
    assert door(UNKNOWN, 0, 8, 8, 2, 0, FAKE, 0) == _lib.ZK_ERR_ARG
    assert "null pointer" in _err()
    assert door(UNKNOWN, FAKE, 8, 8, 2, 0, 0, 0) == _lib.ZK_ERR_ARG
    assert "null pointer" in _err()
    for fv in (0, 1):
        assert door(UNKNOWN, FAKE, 8, 8, 2, fv, FAKE + 4096, 0) == _lib.ZK_ERR_HANDLE
        assert "unknown PLONK proving-key handle" in _err()


# ---- the Python mirrors: every geometry / dtype error before the library is called (the handle is never looked at)
@pytest.fixture()
def bases():
    rb = zb.ResidentBases.__new__(zb.ResidentBases)
    rb.is_g2, rb.handle, rb.n = False, UNKNOWN, 1 << 12
    return rb


def test_multi_exp_rows_rejects_bad_device_geometry(bases):
    with pytest.raises(ValueError, match="n and rows are required"):
        bases.multi_exp_rows(FAKE, n=8)
    with pytest.raises(ValueError, match="n and rows are required"):
        bases.multi_exp_rows(FAKE, rows=2)
    with pytest.raises(ValueError, match="negative"):
        bases.multi_exp_rows(FAKE, n=8, rows=-1)
    with pytest.raises(ValueError, match="row_stride = 7 is below"):
        bases.multi_exp_rows(FAKE, n=8, rows=2, row_stride=7)
    with pytest.raises(ValueError, match="offset"):
        bases.multi_exp_rows(FAKE, n=8, rows=2, offset=-1)
    span = (2 * 9 + 8) * 32  # three rows of 8 at stride 9
    with pytest.raises(ValueError, match="out overlaps scalars"):
        bases.multi_exp_rows(FAKE, n=8, rows=3, row_stride=9, out=FAKE + span - 32)
    with pytest.raises(ValueError, match="compressed overlaps scalars"):
        bases.multi_exp_rows(FAKE, n=8, rows=3, row_stride=9, out=FAKE + span, compressed=FAKE + 64)
    with pytest.raises(ValueError, match="compressed overlaps out"):
        bases.multi_exp_rows(FAKE, n=8, rows=3, row_stride=9, out=FAKE + span, compressed=FAKE + span + 3 * 64 - 32)
    with pytest.raises(TypeError, match="out must be a device buffer"):
        bases.multi_exp_rows(FAKE, n=8, rows=3, out=np.zeros((3, 8), np.uint64))
    with pytest.raises(TypeError, match="compressed must be"):
        bases.multi_exp_rows(FAKE, n=8, rows=3, compressed=np.zeros((3, 32), np.uint8))
    with pytest.raises(ValueError, match="points=False leaves nothing"):
        bases.multi_exp_rows(FAKE, n=8, rows=3, points=False)
    with pytest.raises(ValueError, match="out takes the points"):
        bases.multi_exp_rows(FAKE, n=8, rows=3, points=False, compressed=True, out=FAKE + 4096)


def test_multi_exp_rows_rejects_bad_host_arrays(bases):
    good = np.zeros((3, 8, 4), np.uint64)
    with pytest.raises(TypeError, match="uint64"):
        bases.multi_exp_rows(good.astype(np.int64))
    with pytest.raises(TypeError, match="uint64"):
        bases.multi_exp_rows(good.astype(np.float64))
    with pytest.raises(TypeError, match="C-contiguous"):
        bases.multi_exp_rows(np.zeros((3, 16, 4), np.uint64)[:, ::2])
    with pytest.raises(TypeError):
        bases.multi_exp_rows([[0, 0, 0, 0]])
    with pytest.raises(ValueError, match=r"not \(rows, n, 4\)"):
        bases.multi_exp_rows(np.zeros((3, 8), np.uint64))
    with pytest.raises(ValueError, match="rows = 2 != 3"):
        bases.multi_exp_rows(good, rows=2)
    with pytest.raises(ValueError, match="n = 7 != 8"):
        bases.multi_exp_rows(good, n=7)
    with pytest.raises(ValueError, match="row_stride = 9 != 8"):
        bases.multi_exp_rows(good, row_stride=9)
    with pytest.raises(ValueError, match="device form"):
        bases.multi_exp_rows(good, out=FAKE)
    with pytest.raises(ValueError, match="device form"):
        bases.multi_exp_rows(good, compressed=FAKE)
    # no rows: nothing to ask the library for
    pts, enc = bases.multi_exp_rows(np.zeros((0, 8, 4), np.uint64), compressed=True)
    assert pts.shape == (0, 8) and enc.shape == (0, 32) and enc.dtype == np.uint8


def test_kzg_and_plonk_mirrors_share_the_rules(bases):
    srs = zkzg.SRS(bases, np.zeros((2, 16), np.uint64))
    with pytest.raises(ValueError, match="row_stride = 7 is below"):
        srs.commit_rows(FAKE, n=8, rows=2, row_stride=7)
    with pytest.raises(TypeError, match="uint64"):
        srs.commit_rows(np.zeros((3, 8, 4), np.int32))
    pk = zp.ProvingKey(UNKNOWN.value, bases, {"size": 8, "n_public": 1}, 10)
    pk.free = lambda: None
    with pytest.raises(ValueError, match="row_stride = 9 is below"):
        pk.commit_rows(FAKE, length=10, rows=2, row_stride=9)
    with pytest.raises(ValueError, match="out overlaps scalars"):
        zp.commit_rows(pk, FAKE, length=10, rows=2, out=FAKE + 32)
    with pytest.raises(ValueError, match="two blinders"):
        pk.commit_rows(FAKE, from_values=True, length=11, rows=2)
    with pytest.raises(ValueError, match="two blinders"):
        pk.commit_rows(np.zeros((2, 8, 4), np.uint64), from_values=True)
    with pytest.raises(TypeError, match="uint64"):
        pk.commit_rows(np.zeros((2, 10, 4), np.float32), from_values=True)
    pk.handle = C.c_uint64(0)
