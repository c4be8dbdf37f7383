"""The row-batched copy-constraint ratio (csrc/plonk.hip ratio_rows_dev: k_z_terms_rows, one k_batch_inverse for all rows, k_pscan_fused_rows or the three
row scans) through its five public entries  (-m gpu).  Everything is bit-exact.

Sizes: one per shape a launch can take -- 2^0 (Z = [1]), 2^1, 2^3 (one scan lane), 2^5 (one inverse lane), 2^6 (two), 2^11 (the fused scan's ceiling: one full
workgroup), 2^12 (the smallest three-pass scan, nb = 2), 2^13 (one full workgroup of the inverse), 2^16, and 2^22 (K = 16 per lane in the row form, 17 in the
one-row form, which runs the prover's own plan).  Row counts 1, 2, 3, 5 (2^22: 1 and 2).
Rows: every row of a call is a different vector with different challenges (tests/plonk_ratio_ref.py pool_row): row 0 is l = r = o = r - 1 with beta = gamma =
r - 1, the last has gamma = 0, one has beta = 0 (Z all ones), the rest are edge mixes.  Strides n and n + 1 for inputs and output independently; the gaps and
one element behind the last row hold a sentinel that is no canonical image and must survive.  Permutations: identity, a random circuit's, uniformly random.
Expectation up to 2^16: tests/plonk_ratio_ref.ratio (Python integers; tests/test_plonk_ratio_cpu.py holds it against the oracle prover's Z).  At 2^22: the
batched rows equal the one-row calls, z[0] = 1, and the recurrence holds in Python integers at every lane and workgroup boundary of both scan plans and at
4,096 random indices (about 7 s of Python per row: a million indices)."""
import ctypes as C

import numpy as np
import pytest

import noir_backend_using_gnark_amd as zk
from noir_backend_using_gnark_amd import _lib
from noir_backend_using_gnark_amd import bn254 as zb
from noir_backend_using_gnark_amd import plonk as zp
from oracle import bn254_ref as ref
from oracle import oracle as orc
from oracle import plonk_ref as pl
from tests import plonk_ratio_ref as rr
from tests import plonk_shapes as ps

pytestmark = pytest.mark.gpu
R = ref.R
M = pl.ints_to_mont_np
SENTINEL = rr.SENTINEL
LOG_N = (0, 1, 3, 5, 6, 11, 12, 13, 16)
ROW_COUNTS = (1, 2, 3, 5)
ONE = M([1])[0]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    _lib.require_device()  # fail loudly: no silent fallback


# ---------------------------------------------------------------------------------------------------- inputs and expectations, computed once
_perms, _rows, _wants = {}, {}, {}


def _perm(log_n, kind):
    if (log_n, kind) not in _perms:
        _perms[(log_n, kind)] = rr.permutation(kind, 1 << log_n, 0x9E + log_n)
    return _perms[(log_n, kind)]


def _row(log_n, j):
    """pool row j of the size: (dict of integers, dict of Montgomery arrays)"""
    if (log_n, j) not in _rows:
        row = rr.pool_row(1 << log_n, j, 0xA0 + log_n)
        img = {k: M(row[k]) for k in ("l", "r", "o")}
        img.update(beta=M([row["beta"]]), gamma=M([row["gamma"]]))
        for v in img.values():
            v.setflags(write=False)
        _rows[(log_n, j)] = (row, img)
    return _rows[(log_n, j)]


def _want(log_n, kind, j):
    if (log_n, kind, j) not in _wants:
        row = _row(log_n, j)[0]
        w = M(rr.ratio(row["l"], row["r"], row["o"], _perm(log_n, kind), row["beta"], row["gamma"]))
        w.setflags(write=False)
        _wants[(log_n, kind, j)] = w
    return _wants[(log_n, kind, j)]


def _check_strided(got, want_rows, stride, width, what):
    keep = np.ones(got.shape[0], dtype=bool)
    for i, w in enumerate(want_rows):
        assert (got[i * stride:i * stride + width] == w).all(), what + ("row", i)
        keep[i * stride:i * stride + width] = False
    assert (got[keep] == SENTINEL).all(), what + ("sentinel",)


class _Dev:
    """device buffers that are freed together"""

    def __init__(self):
        self.bufs = []

    def up(self, a):
        self.bufs.append(_lib.DeviceBuffer.from_numpy(a))
        return self.bufs[-1]

    def take(self, b):
        self.bufs.append(b)
        return b

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for b in self.bufs:
            b.free()


def _ratio_dev(imgs, n, in_stride, out_stride, sigma=None, key=None):
    """rows = len(imgs) through zk_bn254_iop_ratio_copy_batch_dev (sigma: device buffer) or zk_bn254_plonk_ratio_batch_dev (key) -> the output buffer as it is
    afterwards, (rows * out_stride + 1, 4); asserts that the inputs, gaps included, are unchanged"""
    rows, log_n = len(imgs), n.bit_length() - 1
    ins = [rr.strided([im[k] for im in imgs], in_stride) for k in ("l", "r", "o")]
    ch = [np.concatenate([im[k] for im in imgs] + [SENTINEL[None]]) for k in ("beta", "gamma")]
    out = np.tile(SENTINEL, (rows * out_stride + 1, 1))
    with _Dev() as d:
        dl, dr, do, db, dg, dz = (d.up(a) for a in ins + ch + [out])
        p = lambda b: C.c_void_p(b.ptr)
        if key is None:
            rc = _lib.lib().zk_bn254_iop_ratio_copy_batch_dev(p(dl), p(dr), p(do), C.c_size_t(in_stride), C.c_uint32(log_n), C.c_size_t(rows), p(sigma), p(db), p(dg),
                                                              p(dz), C.c_size_t(out_stride), None)
        else:
            rc = _lib.lib().zk_bn254_plonk_ratio_batch_dev(key.handle, p(dl), p(dr), p(do), C.c_size_t(in_stride), C.c_size_t(rows), p(db), p(dg), p(dz),
                                                           C.c_size_t(out_stride), None)
        _lib.check(rc)
        for buf, a in zip((dl, dr, do, db, dg), ins + ch):
            assert (buf.to_numpy(np.uint64, a.shape) == a).all(), "an input changed"
        return dz.to_numpy(np.uint64, out.shape)


def _host(imgs, perm):
    stack = lambda k: np.ascontiguousarray(np.stack([im[k] for im in imgs]))
    return zk.ratio_copy_batch(stack("l"), stack("r"), stack("o"), np.asarray(perm, dtype=np.uint32), np.concatenate([im["beta"] for im in imgs]),
                               np.concatenate([im["gamma"] for im in imgs]))


# ------------------------------------------------------------------------------------------------------------ 2^0 .. 2^16
@pytest.mark.parametrize("kind", rr.PERMS)
@pytest.mark.parametrize("log_n", LOG_N)
def test_every_row_count_and_stride(log_n, kind):
    """1, 2, 3 and 5 rows at input and output strides n and n + 1: every row equals the Python expectation and the one-row call on the same inputs, through
    the device door; five rows through the host door; sentinel and inputs untouched"""
    n = 1 << log_n
    perm = _perm(log_n, kind)
    with _Dev() as d:
        sigma = d.take(zk.permutation_sigma(np.asarray(perm, dtype=np.uint32)))
        single = []
        for j in range(rr.POOL):
            got = _ratio_dev([_row(log_n, j)[1]], n, n, n, sigma)
            _check_strided(got, [_want(log_n, kind, j)], n, n, (log_n, kind, "one row", j))
            single.append(got[:n])
        if kind == "identity":
            assert all((s == ONE).all() for s in single)
        assert (single[1] == ONE).all(), "beta = 0"
        for rows in ROW_COUNTS:
            idx = rr.rows_of(rows)
            imgs = [_row(log_n, j)[1] for j in idx]
            for in_stride in (n, n + 1):
                for out_stride in (n, n + 1):
                    got = _ratio_dev(imgs, n, in_stride, out_stride, sigma)
                    _check_strided(got, [single[j] for j in idx], out_stride, n, (log_n, kind, rows, in_stride, out_stride))
        z = _host([_row(log_n, j)[1] for j in range(rr.POOL)], perm)
        for j in range(rr.POOL):
            assert (z[j] == single[j]).all(), ("host door", log_n, kind, j)
        assert (_host([_row(log_n, 3)[1]], perm)[0] == single[3]).all(), ("host door, one row", log_n, kind)


@pytest.mark.parametrize("log_n", LOG_N)
def test_zero_terms(log_n):
    """A zero denominator term in one row and a zero numerator term in another, at the first element, either side of a lane and of a workgroup boundary and at
    the last two elements: everything after it is 0 in that row and nowhere else; at i = n - 1 Z is unaffected (the last term is computed and never used)"""
    n = 1 << log_n
    perm = _perm(log_n, "uniform")
    sig = rr.sigma(perm, n)
    base, base_img = _row(log_n, 2)
    num, den = rr.terms(base["l"], base["r"], base["o"], sig, base["beta"], base["gamma"])
    assert 0 not in num and 0 not in den
    other = _row(log_n, 3)[1]
    with _Dev() as d:
        sigma = d.take(zk.permutation_sigma(np.asarray(perm, dtype=np.uint32)))
        for k, i in enumerate(rr.zero_positions(n)):
            imgs, want = [], []
            for which in ("den", "num"):
                row = rr.plant_zero(base, sig, n, i, which)
                t = rr.term(row["l"], row["r"], row["o"], sig, n, row["beta"], row["gamma"], i)
                assert t[which == "den"] == 0 and t[which != "den"] != 0
                nz, dz = list(num), list(den)
                nz[i], dz[i] = t
                z = rr.ratio_from_terms(nz, dz)
                assert z[i + 1:] == [0] * (n - 1 - i) and 0 not in z[:i + 1]
                img = dict(base_img)
                img["l"] = base_img["l"].copy()
                img["l"][i] = M([row["l"][i]])[0]
                imgs.append(img)
                want.append(M(z))
            imgs.append(other)
            want.append(_want(log_n, "uniform", 3))
            if i == n - 1:
                assert (want[0] == _want(log_n, "uniform", 2)).all() and (want[1] == want[0]).all()
            in_stride, out_stride = n + (k & 1), n + ((k >> 1) & 1)
            got = _ratio_dev(imgs, n, in_stride, out_stride, sigma)
            _check_strided(got, want, out_stride, n, (log_n, "zero at", i))
            for m in range(2):
                one = _ratio_dev([imgs[m]], n, n, n, sigma)
                assert (one[:n] == want[m]).all(), (log_n, "zero at", i, "one row", m)


# --------------------------------------------------------------------------------------------------------------------- 2^22
BIG = 22


def _random_images(rng, n):
    a = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64) << np.uint64(1) | rng.integers(0, 2, size=(n, 4), dtype=np.uint64)
    a[:, 3] = rng.integers(0, R >> 192, size=n, dtype=np.uint64)     # below r: a canonical image
    return a


@pytest.fixture(scope="module")
def big():
    """two random rows at 2^22 with a uniformly random permutation: the one-row call of each (the prover's plan, K = 17) and the two-row call (K = 16) at
    strides n + 1"""
    n = 1 << BIG
    rng = np.random.default_rng(0x2222)
    perm = rng.permutation(3 * n).astype(np.uint32)
    ch = [ref.SplitMix64(0x22).felt() for _ in range(4)]
    imgs = [dict(l=_random_images(rng, n), r=_random_images(rng, n), o=_random_images(rng, n), beta=M([ch[2 * v]]), gamma=M([ch[2 * v + 1]])) for v in range(2)]
    with _Dev() as d:
        sigma = d.take(zk.permutation_sigma(perm))
        single = [_ratio_dev([im], n, n, n, sigma)[:n].copy() for im in imgs]
        both = _ratio_dev(imgs, n, n + 1, n + 1, sigma)
    return dict(n=n, perm=perm, imgs=imgs, ch=ch, single=single, both=both)


def test_2p22_batched_rows_equal_the_one_row_calls(big):
    n = big["n"]
    assert rr.boundary_indices(16, (4,)).tolist() == [0, 3, 4, 7, 8, 11, 12] and ps.scan_plan(n + 8)[0] == 17
    _check_strided(big["both"], big["single"], n + 1, n, (BIG, "two rows"))
    for z in big["single"]:
        assert (z[0] == ONE).all()


@pytest.mark.parametrize("v", (0, 1))
def test_2p22_recurrence(big, v):
    """z[i+1] * den_i == z[i] * num_i at every multiple of K and of 256 K and the index before each, for K = 16 and K = 17, and at 4,096 random indices; no term
    there is zero, and none anywhere: z[n - 1] != 0 says so for every i < n - 1 (a zero term zeroes everything after it), the last term is among the indices"""
    n, im, z = big["n"], big["imgs"][v], big["single"][v]
    idx = rr.boundary_indices(n, (16, 17))
    assert np.isin([0, 15, 16, 17, 33, 34, 4095, 4096, 4351, 4352, n - 17, n - 16], idx).all() and not np.isin([1, 18, n - 1], idx).any()
    extra = np.random.default_rng(0x4096 + v).integers(0, n - 1, size=4096)
    bad, zero = rr.recurrence_failures(z, im["l"], im["r"], im["o"], big["perm"], big["ch"][2 * v], big["ch"][2 * v + 1], np.unique(np.concatenate([idx, extra])))
    assert bad == [] and zero == []
    assert z[n - 1].any(), "a zero term somewhere"
    last = np.concatenate([z, z[:1]])        # the term at n - 1 (never used): only that it is not zero
    assert rr.recurrence_failures(last, im["l"], im["r"], im["o"], big["perm"], big["ch"][2 * v], big["ch"][2 * v + 1], [n - 1])[1] == []


# ------------------------------------------------------------------------------------------------------- through a resident key
@pytest.fixture(scope="module")
def fixture_circuit():
    import json
    import os
    e = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plonk_golden.json")))[0]
    return pl.sparse_r1cs_from_acir(e["acir"], [int(v, 16) for v in e["values"]])


def _device_key(spr, n):
    from tests.test_gpu_plonk import _circuit
    rb = zb.ResidentBases(orc.g1_gen_points(0x9E0, n + 3))
    return zp.setup(_circuit(spr), rb), rb


@pytest.mark.parametrize("log_n", (3, 12))
def test_key_door_equals_the_key_free_door(log_n):
    """zk_bn254_plonk_ratio_batch_dev on a key set up at 2^3 and 2^12 equals zk_bn254_iop_ratio_copy_batch_dev given zk_bn254_iop_sigma_dev of the oracle's
    permutation of the same circuit, for 1, 2, 3 and 5 rows; ProvingKey.ratio_batch on host arrays gives the same rows"""
    n = 1 << log_n
    spr, _ = ps.circuit("random", n, 2, "full", 0x6E + log_n)
    perm = pl.build_permutation(spr, n)
    pk, rb = _device_key(spr, n)
    try:
        assert pk.domain_size == n
        with _Dev() as d:
            sigma = d.take(zk.permutation_sigma(np.asarray(perm, dtype=np.uint32)))
            for rows in ROW_COUNTS:
                imgs = [_row(log_n, j)[1] for j in rr.rows_of(rows)]
                free = _ratio_dev(imgs, n, n + 1, n, sigma)
                assert (_ratio_dev(imgs, n, n + 1, n, key=pk) == free).all(), (log_n, rows)
                assert (_ratio_dev(imgs, n, n, n + 1, key=pk)[:rows * (n + 1)].reshape(rows, n + 1, 4)[:, :n] == free[:rows * n].reshape(rows, n, 4)).all()
            stack = lambda k: np.ascontiguousarray(np.stack([im[k] for im in imgs]))
            z = pk.ratio_batch(stack("l"), stack("r"), stack("o"), np.concatenate([im["beta"] for im in imgs]), np.concatenate([im["gamma"] for im in imgs]))
            assert (z.reshape(-1, 4) == free[:-1]).all()
    finally:
        pk.free()
        rb.free()


def _row_any(log_n, j):
    row = rr.pool_row(1 << log_n, j, 0xF1 + log_n)
    img = {k: M(row[k]) for k in ("l", "r", "o")}
    img.update(beta=M([row["beta"]]), gamma=M([row["gamma"]]))
    return img


def test_key_door_gives_a_proofs_own_z(fixture_circuit):
    """fed the l, r, o, beta and gamma of the oracle's proof of a fixture circuit (z blinders 0), the key door returns that proof's Z, in one row and as the
    middle of three"""
    spr, sol = fixture_circuit
    n = ps.domain_size(spr)
    pk_o, _ = pl.plonk_setup(spr, pl.kzg_new_srs(n + 3, 0x5EED))
    trace = {}
    pl.plonk_prove(pk_o, sol, ref.rand_felts(0xB2, 6) + [0, 0, 0], trace=trace)
    z = pk_o["d0"].fft(ref.bit_reverse(trace["bz"][:n]), ref.DIT)
    l, r, o = pl.evaluate_lro(spr, n, sol)
    img = dict(l=M(l), r=M(r), o=M(o), beta=M([trace["beta"]]), gamma=M([trace["gamma"]]))
    log_n = n.bit_length() - 1
    pk, rb = _device_key(spr, n)
    try:
        assert (_ratio_dev([img], n, n, n, key=pk)[:n] == M(z)).all()
        rows = [_row_any(log_n, 3), img, _row_any(log_n, 2)]
        assert (_ratio_dev(rows, n, n + 1, n + 1, key=pk)[n + 1:2 * n + 1] == M(z)).all()
    finally:
        pk.free()
        rb.free()


# ------------------------------------------------------------------------------------------------------------------ sigma
@pytest.mark.parametrize("log_n", (3, 12))
def test_sigma_equals_the_identity_support_permuted(log_n):
    n = 1 << log_n
    spr, _ = ps.circuit("random", n, 2, "full", 0x6E + log_n)
    for perm in (pl.build_permutation(spr, n), rr.uniform_perm(n, log_n)):
        ident = rr.identity_support(n)
        with _Dev() as d:
            got = d.take(zk.permutation_sigma(np.asarray(perm, dtype=np.int64))).to_numpy(np.uint64, (3 * n, 4))
        assert (got == M([ident[p] for p in perm])).all()
    # an entry equal to 3 n is refused: by the library's own status flag (the Python mirror's check is not in the way of a device-resident permutation)
    perm = np.arange(3 * n, dtype=np.uint32)
    for at in (0, n + 1, 3 * n - 1):
        bad = perm.copy()
        bad[at] = 3 * n
        with _Dev() as d:
            src, out = d.up(bad), d.take(_lib.DeviceBuffer(3 * n * 32))
            assert _lib.lib().zk_bn254_iop_sigma_dev(C.c_void_p(src.ptr), C.c_uint32(log_n), C.c_void_p(out.ptr), None) == _lib.ZK_ERR_ARG
            with pytest.raises(ValueError):
                zk.permutation_sigma(src, n)
        z = np.zeros((1, n, 4), dtype=np.uint64)
        one = np.zeros((1, 4), dtype=np.uint64)
        assert _lib.lib().zk_bn254_iop_ratio_copy_batch(_lib.vp(z), _lib.vp(z), _lib.vp(z), C.c_uint32(log_n), C.c_size_t(1), _lib.vp(bad), _lib.vp(one), _lib.vp(one),
                                                        _lib.vp(np.zeros((1, n, 4), dtype=np.uint64))) == _lib.ZK_ERR_ARG


# -------------------------------------------------------------------------------------------------------------- inversion
@pytest.mark.parametrize("n", (1, 31, 32, 33, 8192, 8193))
def test_fr_batch_invert(n):
    """a * inv == 1 where a != 0 and 0 where a == 0, against Python's pow(a, -1, r): zeros at the first, last and lane-boundary positions (the lanes of
    k_batch_inverse are strided: element i belongs to lane i mod T, T the launch's threads), edge values, and an all-zero vector"""
    a = rr.edge_mix(n, 0x1B + n)
    threads = 256 * ((((n + 31) // 32) + 255) // 256)
    for i in {0, n - 1, min(threads - 1, n - 1), min(threads, n - 1), n // 2}:
        a[i] = 0
    if n > 2:
        a[1] = R - 1
    want = [pow(v, -1, R) if v else 0 for v in a]
    assert all((v * w) % R == (1 if v else 0) for v, w in zip(a, want))
    got = zk.fr_batch_invert(M(a))
    assert (got == M(want)).all()
    with _Dev() as d:
        buf = d.up(np.concatenate([M(a), SENTINEL[None]]))
        assert zk.fr_batch_invert(buf, n) is buf
        back = buf.to_numpy(np.uint64, (n + 1, 4))
        assert (back[:n] == M(want)).all() and (back[n] == SENTINEL).all()
    assert not zk.fr_batch_invert(np.zeros((n, 4), dtype=np.uint64)).any()
