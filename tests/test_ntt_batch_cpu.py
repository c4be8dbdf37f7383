"""Row-batched NTT / computeH without a GPU: the Python mirrors (Domain.fft_batch / fft_inverse_batch, groth16.compute_h_batch) refuse wrong shapes, dtypes and
strides BEFORE the library is called, include/zkmi.h declares the four entries, and the entries answer an argument error (and rows = 0) before they look for a
device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import noir_backend_using_gnark_amd as zk
from noir_backend_using_gnark_amd import _lib, bn254, groth16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def no_library(monkeypatch):
    """any call into the library fails the test"""
    def boom():
        raise AssertionError("the library was called")
    monkeypatch.setattr(bn254, "lib", boom)
    monkeypatch.setattr(groth16, "lib", boom)


def test_fft_batch_rejects_bad_host_arrays_before_the_library(no_library):
    dom = zk.Domain(8)
    good = np.zeros((3, 8, 4), dtype=np.uint64)
    for fn in (dom.fft_batch, dom.fft_inverse_batch):
        with pytest.raises(ValueError):
            fn(good, 2)                                             # decimation
        with pytest.raises(TypeError):
            fn(good.astype(np.int64), zk.DIF)                       # dtype
        with pytest.raises(TypeError):
            fn(np.zeros((3, 8, 8), dtype=np.uint64)[:, :, ::2], zk.DIF)   # not contiguous
        with pytest.raises(TypeError):
            fn([[0] * 4] * 8, zk.DIF)                               # not an array
        for shape in ((8, 4), (3, 4, 4), (3, 16, 4), (3, 8, 5), (3, 32)):
            with pytest.raises(ValueError):
                fn(np.zeros(shape, dtype=np.uint64), zk.DIF)
        with pytest.raises(ValueError):
            fn(good, zk.DIF, rows=2)                                # rows against the array's
        with pytest.raises(ValueError):
            fn(good, zk.DIF, row_stride=9)                          # host rows are contiguous


def test_fft_batch_rejects_bad_device_geometry_before_the_library(no_library):
    dom = zk.Domain(8)
    buf = _lib.DeviceBuffer.__new__(_lib.DeviceBuffer)               # a buffer that owns nothing: no device is needed to describe one
    buf.ptr, buf.nbytes = 0, 3 * 8 * 32
    try:
        for a in (buf, 0x1000):
            with pytest.raises(ValueError):
                dom.fft_batch(a, zk.DIF)                            # rows missing
            with pytest.raises(ValueError):
                dom.fft_batch(a, zk.DIF, rows=-1)
            with pytest.raises(ValueError):
                dom.fft_batch(a, zk.DIF, rows=3, row_stride=7)      # rows would overlap
            with pytest.raises(ValueError):
                dom.fft_inverse_batch(a, 3, rows=3)                 # decimation
        with pytest.raises(ValueError):
            dom.fft_batch(buf, zk.DIF, rows=4)                      # past the end of the buffer
        with pytest.raises(ValueError):
            dom.fft_batch(buf, zk.DIF, rows=3, row_stride=9)
    finally:
        buf.ptr = 0


def test_compute_h_batch_rejects_bad_arrays_before_the_library(no_library):
    good = np.zeros((2, 8, 4), dtype=np.uint64)
    with pytest.raises(TypeError):
        zk.compute_h_batch(good.astype(np.int64), good, good, 3)
    with pytest.raises(TypeError):
        zk.compute_h_batch(good, good.tolist(), good, 3)
    with pytest.raises(ValueError):
        zk.compute_h_batch(good, good, good[:1], 3)                 # row counts differ
    with pytest.raises(ValueError):
        zk.compute_h_batch(good, good[:, :7], good, 3)              # lengths differ
    with pytest.raises(ValueError):
        zk.compute_h_batch(good[0], good[0], good[0], 3)            # one row is not a batch: (n, 4)
    with pytest.raises(ValueError):
        zk.compute_h_batch(good, good, good, 2)                     # n > N
    with pytest.raises(ValueError):
        zk.compute_h_batch(good, good, good, 29)
    with pytest.raises(ValueError):
        zk.compute_h_batch(np.zeros((2, 8, 5), dtype=np.uint64), np.zeros((2, 8, 5), dtype=np.uint64), np.zeros((2, 8, 5), dtype=np.uint64), 3)


def test_header_declares_the_batch_entries():
    hdr = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "zkmi.h")).read())
    for decl in (
        "int zk_bn254_ntt_batch_dev(void *d_a, uint32_t log_n, size_t rows, size_t row_stride, int inverse, int decimation, int coset, void *stream);",
        "int zk_bn254_ntt_batch(zk_fr *a, uint32_t log_n, size_t rows, int inverse, int decimation, int coset);",
        "int zk_bn254_groth16_compute_h_batch_dev(const void *d_a, const void *d_b, const void *d_c, size_t n, size_t in_stride, uint32_t log_N, size_t rows, "
        "void *d_h_out, size_t out_stride, void *stream);",
        "int zk_bn254_groth16_compute_h_batch(const zk_fr *a, const zk_fr *b, const zk_fr *c, size_t n, uint32_t log_N, size_t rows, zk_fr *h_out);",
    ):
        assert decl in hdr, decl
    for name in ("zk_bn254_ntt_batch", "zk_bn254_ntt_batch_dev", "zk_bn254_groth16_compute_h_batch", "zk_bn254_groth16_compute_h_batch_dev"):
        assert name in _lib.SYMBOLS and hasattr(_lib.lib(), name)


def test_argument_errors_and_empty_batches_need_no_device():
    """ZK_ERR_ARG (not ZK_ERR_NO_DEVICE) for a bad argument and ZK_OK for rows = 0: both are decided before the device is looked for"""
    lib = _lib.lib()
    x = np.zeros((2 * 8, 4), dtype=np.uint64)
    p, null = _lib.vp(x), C.c_void_p(0)
    u32, sz, i = C.c_uint32, C.c_size_t, C.c_int
    arg = _lib.ZK_ERR_ARG
    assert lib.zk_bn254_ntt_batch_dev(null, u32(3), sz(2), sz(8), i(0), i(1), i(0), None) == arg
    assert lib.zk_bn254_ntt_batch_dev(p, u32(29), sz(2), sz(1 << 29), i(0), i(1), i(0), None) == arg
    assert lib.zk_bn254_ntt_batch_dev(p, u32(3), sz(2), sz(8), i(0), i(2), i(0), None) == arg
    assert lib.zk_bn254_ntt_batch_dev(p, u32(3), sz(2), sz(7), i(0), i(1), i(0), None) == arg
    assert lib.zk_bn254_ntt_batch(null, u32(3), sz(2), i(0), i(1), i(0)) == arg
    assert lib.zk_bn254_ntt_batch(p, u32(29), sz(2), i(0), i(1), i(0)) == arg
    assert lib.zk_bn254_ntt_batch(p, u32(3), sz(2), i(0), i(7), i(0)) == arg
    h = _lib.vp(np.zeros((2 * 8, 4), dtype=np.uint64))
    for bad in ((null, p, p, h), (p, null, p, h), (p, p, null, h), (p, p, p, null)):
        assert lib.zk_bn254_groth16_compute_h_batch_dev(bad[0], bad[1], bad[2], sz(8), sz(8), u32(3), sz(2), bad[3], sz(8), None) == arg
        assert lib.zk_bn254_groth16_compute_h_batch(bad[0], bad[1], bad[2], sz(8), u32(3), sz(2), bad[3]) == arg
    assert lib.zk_bn254_groth16_compute_h_batch_dev(p, p, p, sz(8), sz(8), u32(29), sz(2), h, sz(1 << 29), None) == arg
    assert lib.zk_bn254_groth16_compute_h_batch_dev(p, p, p, sz(9), sz(9), u32(3), sz(2), h, sz(8), None) == arg      # n > N
    assert lib.zk_bn254_groth16_compute_h_batch_dev(p, p, p, sz(7), sz(6), u32(3), sz(2), h, sz(8), None) == arg      # in_stride < n
    assert lib.zk_bn254_groth16_compute_h_batch_dev(p, p, p, sz(8), sz(8), u32(3), sz(2), h, sz(7), None) == arg      # out_stride < N
    assert lib.zk_bn254_groth16_compute_h_batch_dev(p, p, p, sz(8), sz(8), u32(3), sz(2), p, sz(8), None) == arg      # h_out = a also overlaps b and c
    assert lib.zk_bn254_groth16_compute_h_batch(p, p, p, sz(9), u32(3), sz(2), h) == arg
    assert lib.zk_bn254_groth16_compute_h_batch(p, p, p, sz(8), u32(29), sz(2), h) == arg
    assert lib.zk_bn254_ntt_batch_dev(p, u32(3), sz(0), sz(8), i(0), i(1), i(0), None) == _lib.ZK_OK
    assert lib.zk_bn254_ntt_batch(p, u32(3), sz(0), i(0), i(1), i(0)) == _lib.ZK_OK
    assert lib.zk_bn254_groth16_compute_h_batch_dev(p, p, p, sz(8), sz(8), u32(3), sz(0), h, sz(8), None) == _lib.ZK_OK
    assert lib.zk_bn254_groth16_compute_h_batch(p, p, p, sz(8), u32(3), sz(0), h) == _lib.ZK_OK
    assert not x.any()


CPP_CHECK = r"""
#include <cstdio>
#include "zkmi.hpp"
using namespace zkmi;
int main() {
    fft::Domain d = fft::Domain::NewDomain(8);
    fr::Vector a(3 * 8), empty;
    if (d.FFTBatch(a, 2, fft::DIF).code != ZK_ERR_ARG) return 1;          // 24 elements are not 2 rows of 8
    if (d.FFTInverseBatch(a, 4, fft::DIT, true).code != ZK_ERR_ARG) return 2;
    if (!d.FFTBatch(empty, 0, fft::DIF).ok()) return 3;                     // no rows: nothing to do, no device needed
    if (!d.FFTInverseBatch(empty, 0, fft::DIF).ok()) return 4;
    if (d.FFTBatch(a, 3, (fft::Decimation)2).code != ZK_ERR_ARG) return 5;   // the library's own check
    std::puts("ok");
    return 0;
}
"""


def test_cpp_mirror_batch_methods_check_the_shape(tmp_path):
    """include/zkmi.hpp Domain::FFTBatch / FFTInverseBatch compile against the C ABI and refuse a vector that is not rows x Cardinality"""
    import subprocess
    src, exe = tmp_path / "batch_check.cpp", str(tmp_path / "batch_check")
    src.write_text(CPP_CHECK)
    libdir = os.path.join(ROOT, "noir_backend_using_gnark_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + libdir, "-lzkmi",
                           "-Wl,-rpath," + libdir, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "ok" in out.stdout, (out.returncode, out.stdout + out.stderr)
