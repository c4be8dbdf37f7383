"""Row-batched NTT and computeH (csrc/ntt.hip k_ntt_pass29 / k_ntt_pass29_if with more than one row: the row is blockIdx.z) through the public entries
zk_bn254_ntt_batch[_dev] and zk_bn254_groth16_compute_h_batch[_dev]  (-m gpu).

Every comparison is bit-exact against the C oracle (orc.fr_ntt, orc.groth16_compute_h); computeH rows are also held against the single-vector entry.
Sizes: one per shape a pass can take in the row form -- the copy / scale branch (2^0), tiles with idle lanes, a full tile (2^11), one strided pass of
k = 1, 2, 3, 5 (2^12, 2^13, 2^14, 2^16: the batch prover's ceiling) and two strided passes (2^21).
Rows: every row of a call is a DIFFERENT vector, so a row taken from the wrong place cannot pass: the first is the constant r - 1, the last the complement
alt vector on the lowest bit of the top pass (the module text of tests/test_gpu_ntt_shapes.py says why that vector matters), the rest edge mixes with
distinct seeds.  Strides: 2^log_n and 2^log_n + 1, the gap elements (and the tail of the buffer) filled with a sentinel that must survive.
All inputs are canonical images (< r), the contract include/zkmi.h states for these entries."""
import ctypes as C

import numpy as np
import pytest

import noir_backend_using_gnark_amd as zk
from noir_backend_using_gnark_amd import _lib
from oracle import oracle as orc
from tests import ntt_shapes as S

pytestmark = pytest.mark.gpu

SENTINEL = np.array([0xDEADBEEFDEADBEEF, 0x0123456789ABCDEF, 0xFEEDFACECAFEF00D, 0x1BADB0021BADB002], dtype=np.uint64)   # not a canonical image: never a result
MAX_ROWS = 5
ROW_COUNTS = (1, 2, 3, 5)
NTT_LOG_N = (0, 1, 5, 10, 11, 12, 13, 14, 16)
H_LOG_N = (1, 5, 10, 11, 12, 14, 16)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    _lib.require_device()  # fail loudly: no silent fallback


def _modes(log_n):
    return S.ALL_MODES if log_n < 16 else S.H_MODES


# ---------------------------------------------------------------------------------------------------- inputs and expectations, computed once
_vectors, _expected = {}, {}


def _vector(log_n, j):
    """vector j of the size's pool of MAX_ROWS: 0 = max, MAX_ROWS - 1 = the complement alt on the lowest bit of the top pass, between them edge mixes"""
    if (log_n, j) not in _vectors:
        n = 1 << log_n
        if j == 0:
            v = S.vmax(n)
        elif j == MAX_ROWS - 1:
            v = S.alt(n, S.plan_passes(log_n)[-1][0], True)
        else:
            v = S.edge_mix(n, 0xBA0 + 16 * log_n + j)
        v.setflags(write=False)
        _vectors[(log_n, j)] = v
    return _vectors[(log_n, j)]


def _rows_of(rows):
    """which pool vectors a call of `rows` rows takes: the first is max, the last (from two rows on) the alt vector"""
    return [0] if rows == 1 else [0] + list(range(1, rows - 1)) + [MAX_ROWS - 1]


def _want(log_n, j, mode):
    key = (log_n, j, mode)
    if key not in _expected:
        inverse, dec, coset = mode
        w = orc.fr_ntt(_vector(log_n, j), bool(inverse), dec, bool(coset))
        w.setflags(write=False)
        if log_n >= S.LARGE_FROM:
            return w                       # 64 MiB each: not kept
        _expected[key] = w
    return _expected[key]


def _strided(vectors, stride, width):
    """(len(vectors) * stride + 1, 4): row i's `width` elements at i * stride, everything else the sentinel (one more element behind the last row)"""
    buf = np.tile(SENTINEL, (len(vectors) * stride + 1, 1))
    for i, v in enumerate(vectors):
        buf[i * stride:i * stride + v.shape[0]] = v
    return buf


def _check_strided(got, want_rows, stride, width, what):
    keep = np.ones(got.shape[0], dtype=bool)
    for i, w in enumerate(want_rows):
        assert (got[i * stride:i * stride + width] == w).all(), what + ("row", i)
        keep[i * stride:i * stride + width] = False
    assert (got[keep] == SENTINEL).all(), what + ("sentinel",)


def _ntt_batch_dev(buf, log_n, rows, stride, mode):
    inverse, dec, coset = mode
    d = _lib.DeviceBuffer.from_numpy(buf)
    try:
        _lib.check(_lib.lib().zk_bn254_ntt_batch_dev(C.c_void_p(d.ptr), C.c_uint32(log_n), C.c_size_t(rows), C.c_size_t(stride), C.c_int(inverse), C.c_int(dec),
                                                     C.c_int(coset), None))
        return d.to_numpy(np.uint64, buf.shape)
    finally:
        d.free()


def _ntt_case(log_n, mode, row_counts):
    n = 1 << log_n
    for rows in row_counts:
        idx = _rows_of(rows)
        xs = [_vector(log_n, j) for j in idx]
        want = [_want(log_n, j, mode) for j in idx]
        for stride in (n, n + 1):
            got = _ntt_batch_dev(_strided(xs, stride, n), log_n, rows, stride, mode)
            _check_strided(got, want, stride, n, (log_n, mode, rows, stride))
        y = np.ascontiguousarray(np.stack(xs))
        dom = zk.Domain(n)
        (dom.fft_inverse_batch if mode[0] else dom.fft_batch)(y, mode[1], bool(mode[2]))
        for i, w in enumerate(want):
            assert (y[i] == w).all(), ("host entry", log_n, mode, rows, i)


# -------------------------------------------------------------------------------------------------------------- transforms
@pytest.mark.parametrize("log_n", NTT_LOG_N)
def test_ntt_batch_every_mode_row_count_and_stride(log_n):
    """2^0 .. 2^16: 1, 2, 3 and 5 rows in every mode (computeH's four at 2^16), at both strides through the device entry and contiguous through the host entry"""
    for mode in _modes(log_n):
        _ntt_case(log_n, mode, ROW_COUNTS)


@pytest.mark.parametrize("mode", S.H_MODES)
def test_ntt_batch_two_strided_passes(mode):
    """2^21 (strided passes of k = 5 and 5), two rows: max and the complement alt on the lowest bit of the top pass"""
    _ntt_case(21, mode, (2,))


def test_ntt_batch_more_rows_than_one_grid_holds():
    """65537 rows of four elements: gridDim.z ends at 65535, so the rows go in two launches.  Seven distinct vectors repeated in a fixed non-periodic
    pattern: the oracle runs seven times per mode."""
    log_n, n, rows = 2, 4, 65537
    pool = [S.vmax(n), S.alt(n, 1, True)] + [S.edge_mix(n, 0x7A0 + j) for j in range(5)]
    pick = np.random.default_rng(0x65537).integers(0, len(pool), size=rows)
    pick[[0, 65534, 65535, 65536]] = [0, 3, 5, 1]       # the rows on either side of the launch boundary differ
    x = np.stack(pool)[pick]                              # (rows, n, 4)
    for k, mode in enumerate(S.ALL_MODES):
        inverse, dec, coset = mode
        want = np.stack([orc.fr_ntt(v, bool(inverse), dec, bool(coset)) for v in pool])[pick]
        stride = n + (k & 1)
        buf = np.tile(SENTINEL, (rows * stride + 1, 1))
        view = buf[:rows * stride].reshape(rows, stride, 4)
        view[:, :n] = x
        got = _ntt_batch_dev(buf, log_n, rows, stride, mode)
        assert (got[:rows * stride].reshape(rows, stride, 4)[:, :n] == want).all(), mode
        assert (got[:rows * stride].reshape(rows, stride, 4)[:, n:] == SENTINEL).all() and (got[-1] == SENTINEL).all(), mode
    y = x.copy()
    zk.Domain(n).fft_batch(y, S.DIF)
    assert (y == np.stack([orc.fr_ntt(v, False, S.DIF, False) for v in pool])[pick]).all()


# ---------------------------------------------------------------------------------------------------------------- computeH
_triples, _h_expected = {}, {}


def _fe_mul(x, y):
    return orc.fe_op("mul", 0, x, y)


def _h_triple_names(log_n):
    """five different triples: the three the sweep names (a true quotient, max, alt on the lowest bit of the top pass) and, for the rows beyond them, the edge
    mix and alt on another bit (zeros where the size has no other bit)"""
    top = S.plan_passes(log_n)[-1][0]
    names = [("quotient",), ("max",), ("alt", top), ("edge_mix",)]
    names += [("alt", j) for j in (0, log_n - 1) if j != top][:1] or [("zeros",)]
    return names


def _triple(log_n, t):
    if (log_n, t) not in _triples:
        _triples[(log_n, t)] = S.h_triple(t, log_n, orc.rand_fr, _fe_mul)
    return _triples[(log_n, t)]


def _h_want(log_n, t, n):
    if (log_n, t, n) not in _h_expected:
        a, b, c = (np.ascontiguousarray(v[:n]) for v in _triple(log_n, t))
        _h_expected[(log_n, t, n)] = orc.groth16_compute_h(a, b, c, log_n)
    return _h_expected[(log_n, t, n)]


def _h_batch_dev(bufs, n, in_stride, log_n, rows, out, out_stride, alias=False):
    """-> (h buffer, the three input buffers as they are afterwards)"""
    d_in = [_lib.DeviceBuffer.from_numpy(b) for b in bufs]
    d_out = d_in[0] if alias else _lib.DeviceBuffer.from_numpy(out)
    try:
        _lib.check(_lib.lib().zk_bn254_groth16_compute_h_batch_dev(C.c_void_p(d_in[0].ptr), C.c_void_p(d_in[1].ptr), C.c_void_p(d_in[2].ptr), C.c_size_t(n),
                                                                   C.c_size_t(in_stride), C.c_uint32(log_n), C.c_size_t(rows), C.c_void_p(d_out.ptr),
                                                                   C.c_size_t(out_stride), None))
        return d_out.to_numpy(np.uint64, out.shape), [d.to_numpy(np.uint64, b.shape) for d, b in zip(d_in, bufs)]
    finally:
        for d in d_in + ([] if alias else [d_out]):
            d.free()


def _h_single_dev(a, b, c, log_n):
    N = 1 << log_n
    d = [_lib.DeviceBuffer.from_numpy(v) for v in (a, b, c)]
    h = _lib.DeviceBuffer(N * 32)
    try:
        _lib.check(_lib.lib().zk_bn254_groth16_compute_h_dev(C.c_void_p(d[0].ptr), C.c_void_p(d[1].ptr), C.c_void_p(d[2].ptr), C.c_size_t(a.shape[0]), C.c_uint32(log_n),
                                                             C.c_void_p(h.ptr), None))
        return h.to_numpy(np.uint64, (N, 4))
    finally:
        for x in d + [h]:
            x.free()


@pytest.mark.parametrize("which_n", ["N", "N-1", "1"])
@pytest.mark.parametrize("log_n", H_LOG_N)
def test_compute_h_batch_rows_lengths_and_strides(log_n, which_n):
    """1, 2 and 5 rows of different triples at a length the zero-padding distinguishes, input strides n and n + 3, output strides N and N + 1: every row against
    the oracle and against the single-vector entry; inputs untouched out of place; h_out = a gives the same bytes"""
    N = 1 << log_n
    n = {"N": N, "N-1": N - 1, "1": 1}[which_n]
    names = _h_triple_names(log_n)
    cut = [[np.ascontiguousarray(v[:n]) for v in _triple(log_n, t)] for t in names]       # per triple: a, b, c of length n
    want = [_h_want(log_n, t, n) for t in names]
    for t, (a, b, c), w in zip(names, cut, want):
        assert (_h_single_dev(a, b, c, log_n) == w).all(), ("single entry", log_n, t, n)
    for rows in (1, 2, 5):
        for out_stride in (N, N + 1):
            out = np.tile(SENTINEL, (rows * out_stride + 1, 1))
            for in_stride in (n, n + 3):
                bufs = [_strided([cut[i][m] for i in range(rows)], in_stride, n) for m in range(3)]
                got, after = _h_batch_dev(bufs, n, in_stride, log_n, rows, out, out_stride)
                _check_strided(got, want[:rows], out_stride, N, (log_n, n, rows, in_stride, out_stride))
                for m in range(3):
                    assert (after[m] == bufs[m]).all(), ("input changed", log_n, n, rows, in_stride, out_stride, m)
            # in place: the three inputs at the output's stride, h_out = a
            bufs = [_strided([cut[i][m] for i in range(rows)], out_stride, n) for m in range(3)]
            got, after = _h_batch_dev(bufs, n, out_stride, log_n, rows, bufs[0], out_stride, alias=True)
            _check_strided(got, want[:rows], out_stride, N, (log_n, n, rows, "alias", out_stride))
            for m in (1, 2):
                assert (after[m] == bufs[m]).all(), ("input changed", log_n, n, rows, "alias", out_stride, m)
    if which_n == "N":
        a, b, c = (np.ascontiguousarray(np.stack([cut[i][m] for i in range(5)])) for m in range(3))
        h = zk.compute_h_batch(a, b, c, log_n)
        for i in range(5):
            assert (h[i] == want[i]).all(), ("host entry", log_n, i)


# --------------------------------------------------------------------------------------------------------- argument errors
def test_batch_argument_errors_leave_the_data_alone():
    """every argument error of the four entries returns ZK_ERR_ARG before the device is touched; rows = 0 is ZK_OK and does nothing"""
    lib = _lib.lib()
    log_n, N, rows = 3, 8, 2
    x = np.stack([S.edge_mix(N, 0xE0 + i) for i in range(3 * rows)]).reshape(-1, 4)      # enough for a, b, c below
    d = _lib.DeviceBuffer.from_numpy(x)
    h = _lib.DeviceBuffer.from_numpy(np.tile(SENTINEL, (rows * N, 1)))
    p = C.c_void_p(d.ptr)

    def ntt_dev(ptr=p, log=log_n, r=rows, stride=N, dec=S.DIF):
        return lib.zk_bn254_ntt_batch_dev(ptr, C.c_uint32(log), C.c_size_t(r), C.c_size_t(stride), C.c_int(0), C.c_int(dec), C.c_int(0), None)

    host = x[:rows * N].copy()

    def ntt_host(ptr=_lib.vp(host), log=log_n, r=rows, dec=S.DIF):
        return lib.zk_bn254_ntt_batch(ptr, C.c_uint32(log), C.c_size_t(r), C.c_int(0), C.c_int(dec), C.c_int(0))

    a, b, c = (C.c_void_p(d.ptr + m * rows * N * 32) for m in range(3))
    ho = C.c_void_p(h.ptr)

    def h_dev(pa=a, pb=b, pc=c, n=N, in_stride=N, log=log_n, r=rows, out=ho, out_stride=N):
        return lib.zk_bn254_groth16_compute_h_batch_dev(pa, pb, pc, C.c_size_t(n), C.c_size_t(in_stride), C.c_uint32(log), C.c_size_t(r), out, C.c_size_t(out_stride), None)

    ha, hb, hc = (x[m * rows * N:(m + 1) * rows * N].copy() for m in range(3))
    hh = np.tile(SENTINEL, (rows * N, 1))

    def h_host(pa=_lib.vp(ha), pb=_lib.vp(hb), pc=_lib.vp(hc), n=N, log=log_n, r=rows, out=_lib.vp(hh)):
        return lib.zk_bn254_groth16_compute_h_batch(pa, pb, pc, C.c_size_t(n), C.c_uint32(log), C.c_size_t(r), out)

    null = C.c_void_p(0)
    bad = {
        "ntt_dev null": ntt_dev(ptr=null), "ntt_dev log_n": ntt_dev(log=29), "ntt_dev decimation": ntt_dev(dec=2), "ntt_dev stride": ntt_dev(stride=N - 1),
        "ntt_host null": ntt_host(ptr=null), "ntt_host log_n": ntt_host(log=29), "ntt_host decimation": ntt_host(dec=-1),
        "h_dev null a": h_dev(pa=null), "h_dev null b": h_dev(pb=null), "h_dev null c": h_dev(pc=null), "h_dev null out": h_dev(out=null),
        "h_dev log_N": h_dev(log=29), "h_dev n > N": h_dev(n=N + 1, in_stride=N + 1), "h_dev in_stride": h_dev(n=N - 1, in_stride=N - 2),
        "h_dev out_stride": h_dev(out_stride=N - 1), "h_dev out overlaps b": h_dev(out=b), "h_dev out inside a": h_dev(out=C.c_void_p(d.ptr + 32)),
        "h_dev out = a, other strides": h_dev(n=N - 1, in_stride=N - 1, out=a),
        "h_host null a": h_host(pa=null), "h_host null b": h_host(pb=null), "h_host null c": h_host(pc=null), "h_host null out": h_host(out=null),
        "h_host log_N": h_host(log=29), "h_host n > N": h_host(n=N + 1),
    }
    assert {k: v for k, v in bad.items() if v != _lib.ZK_ERR_ARG} == {}
    # rows = 0 with otherwise good arguments: nothing happens
    assert ntt_dev(r=0) == _lib.ZK_OK and ntt_host(r=0) == _lib.ZK_OK and h_dev(r=0) == _lib.ZK_OK and h_host(r=0) == _lib.ZK_OK
    assert (d.to_numpy(np.uint64, x.shape) == x).all() and (h.to_numpy(np.uint64, hh.shape) == SENTINEL).all()
    assert (host == x[:rows * N]).all() and (hh == SENTINEL).all()
    assert (ha == x[:rows * N]).all() and (hb == x[rows * N:2 * rows * N]).all() and (hc == x[2 * rows * N:]).all()
    d.free()
    h.free()
