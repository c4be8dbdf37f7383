"""Window tables in the accumulate kernel's own domain (csrc/ff29.hpp TabPt: every coordinate x * 2^261 mod p, canonical and packed, a flag for "is a point"):
MSMs against registered bases with tables of width 8 and 13, G1 and G2, byte for byte against the oracle's MSM and against the same call through the
table-less path (raw points in gnark's image) -- at sizes around the workgroup and wave boundaries and on the inputs that take the rare branches of the
table variant of the accumulate kernel: the same-x fallback (equal bases), cancellation to infinity inside a task (P, -P), (0, 0) bases as the first point
of a task and in the middle, the scalars 0 / 1 / r - 1, signed-digit carries in every window, one bucket holding every point.  Then one Groth16 and one
PLONK proof at 2^10 against the oracle's bytes, each with and without tables."""
import numpy as np
import pytest

import noir_backend_using_gnark_amd as zk
from noir_backend_using_gnark_amd import _lib
from noir_backend_using_gnark_amd import bn254 as zb
from noir_backend_using_gnark_amd import plonk as zp
from oracle import bn254_ref as ref
from oracle import oracle as orc
from oracle import plonk_ref as pl

pytestmark = pytest.mark.gpu
R = ref.R
P = 0x30644e72e131a029b85045b68181585d97816a916871ca8d3c208c16d87cfd47
WIDTHS = (8, 13)
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1000)
NMAX = max(SIZES)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    _lib.require_device()


@pytest.fixture(scope="module")
def bases():
    """NMAX points of each group and NMAX random scalars (canonical), generated once; tests slice and copy, never write."""
    d = dict(g1=orc.g1_gen_points(41, NMAX), g2=orc.g2_gen_points(42, NMAX), sc=orc.rand_fr(43, NMAX, mont=False))
    for v in d.values():
        v.setflags(write=False)
    return d


def _neg_points(pts):
    """-P for affine points in gnark's Montgomery image: the image of -y is p - image(y), coordinate by coordinate; (0, 0) stays"""
    out = np.array(pts, dtype=np.uint64)
    half = out.shape[1] // 2
    for i in range(out.shape[0]):
        for k in range(half, out.shape[1], 4):
            y = orc.limbs_to_int(out[i, k:k + 4])
            out[i, k:k + 4] = orc.int_to_limbs((P - y) % P)
    return out


def _check(points, scalars, g2, c, want=None):
    """table of width c == table-less path == oracle, byte for byte; returns the oracle's point"""
    points, scalars = np.ascontiguousarray(points), np.ascontiguousarray(scalars)
    if want is None:
        want = (orc.g2_msm if g2 else orc.g1_msm)(points, scalars, scalars_mont=False)
    tab = zb.ResidentBases(points, is_g2=g2, table_window_bits=c)
    raw = zb.ResidentBases(points, is_g2=g2, table_window_bits=-1)
    try:
        got_tab, got_raw = tab.multi_exp(scalars), raw.multi_exp(scalars)
        assert got_raw.tobytes() == want.tobytes(), "table-less path differs from the oracle"
        assert got_tab.tobytes() == want.tobytes(), "table path (c = %d) differs from the oracle" % c
    finally:
        tab.free()
        raw.free()
    return want


_ORACLE = {}


@pytest.mark.parametrize("g2", [False, True], ids=["g1", "g2"])
@pytest.mark.parametrize("c", WIDTHS)
@pytest.mark.parametrize("n", SIZES)
def test_random_scalars(bases, n, c, g2):
    pts, sc = bases["g2" if g2 else "g1"][:n], bases["sc"][:n]
    _ORACLE[(g2, n)] = _check(pts, sc, g2, c, _ORACLE.get((g2, n)))


@pytest.mark.parametrize("g2", [False, True], ids=["g1", "g2"])
@pytest.mark.parametrize("c", WIDTHS)
def test_all_bases_equal(bases, c, g2):
    """every addition after the first of a task meets the accumulator's own x: the same-x filter fires and the canonical fallback (converted back from the
    table's limbs) doubles"""
    n = 257
    pts = np.repeat(bases["g2" if g2 else "g1"][5:6], n, axis=0)
    _check(pts, bases["sc"][:n], g2, c)
    _check(pts, orc.ints_to_limbs([3] * n), g2, c)   # ... and all of them in ONE bucket: P + P + P + ...


@pytest.mark.parametrize("g2", [False, True], ids=["g1", "g2"])
@pytest.mark.parametrize("c", WIDTHS)
def test_point_and_its_negative_cancel(bases, c, g2):
    """P and -P with equal scalars sit next to each other in every bucket: the accumulator passes through infinity inside a task (and the next point is
    copied in again); the whole sum is the point at infinity, and with one more term it is that term"""
    n = 128
    src = bases["g2" if g2 else "g1"][:n]
    pts = np.empty((2 * n, src.shape[1]), np.uint64)
    pts[0::2], pts[1::2] = src, _neg_points(src)
    sc = np.repeat(bases["sc"][:n], 2, axis=0)
    want = _check(pts, sc, g2, c)
    assert not want.any()
    _check(np.concatenate([pts, src[:1]]), np.concatenate([sc, bases["sc"][7:8]]), g2, c)
    # the same digit with opposite signs: P with scalar s and P with scalar r - s
    neg_sc = orc.ints_to_limbs([(R - orc.limbs_to_int(s)) % R for s in bases["sc"][:n]])
    assert not _check(np.concatenate([src, src]), np.concatenate([bases["sc"][:n], neg_sc]), g2, c).any()


@pytest.mark.parametrize("g2", [False, True], ids=["g1", "g2"])
@pytest.mark.parametrize("c", WIDTHS)
def test_infinity_among_the_bases(bases, c, g2):
    """(0, 0) as the first base, in the middle and last: with equal scalars every bucket's task begins with the flagged entry of index 0"""
    n = 257
    pts = np.array(bases["g2" if g2 else "g1"][:n])
    pts[0] = pts[n // 2] = pts[n - 1] = 0
    _check(pts, bases["sc"][:n], g2, c)
    _check(pts, orc.ints_to_limbs([0x1234567] * n), g2, c)
    _check(pts[:1], bases["sc"][:1], g2, c)   # nothing but the point at infinity


@pytest.mark.parametrize("g2", [False, True], ids=["g1", "g2"])
@pytest.mark.parametrize("c", WIDTHS)
def test_edge_scalars(bases, c, g2):
    n = 255
    pts = bases["g2" if g2 else "g1"][:n]
    _check(pts, orc.ints_to_limbs([(0, 1, R - 1)[i % 3] for i in range(n)]), g2, c)
    _check(pts, orc.ints_to_limbs([0] * n), g2, c)
    _check(pts, orc.ints_to_limbs([R - 1] * n), g2, c)
    # signed digits: a digit of 2^(c-1) becomes -2^(c-1) with a carry into the next window -- in every window the scalar has room for
    half = sum(1 << (c * w + c - 1) for w in range(253 // c))
    assert half < R
    _check(pts, orc.ints_to_limbs([half] * n), g2, c)
    _check(pts, orc.ints_to_limbs([half if i % 2 else half - 1 for i in range(n)]), g2, c)


@pytest.mark.parametrize("g2", [False, True], ids=["g1", "g2"])
@pytest.mark.parametrize("c", WIDTHS)
def test_one_bucket_holds_every_point(bases, c, g2):
    """one digit, one bucket: the bucket is cut into tasks and folded"""
    n = NMAX
    pts = bases["g2" if g2 else "g1"][:n]
    _check(pts, orc.ints_to_limbs([5] * n), g2, c)
    _check(pts, orc.ints_to_limbs([5 << (2 * c)] * n), g2, c)   # ... of the third row of the table


@pytest.mark.parametrize("tables", [True, False], ids=["tables", "no_tables"])
def test_groth16_proof_2p10(tables):
    log_n = 10
    N = 1 << log_n
    nw, npub = N, 3
    pkd = dict(log_domain=log_n, n_wires=nw, n_public=npub,
               g1_alpha=orc.g1_gen_points(1, 1)[0], g1_beta=orc.g1_gen_points(2, 1)[0], g1_delta=orc.g1_gen_points(3, 1)[0],
               g1_a=orc.g1_gen_points(4, nw), g1_b=orc.g1_gen_points(5, nw), g1_k=orc.g1_gen_points(6, nw - npub),
               g1_z=orc.g1_gen_points(7, N), g2_beta=orc.g2_gen_points(8, 1)[0], g2_delta=orc.g2_gen_points(9, 1)[0],
               g2_b=orc.g2_gen_points(10, nw))
    a, b = orc.rand_fr(20, N), orc.rand_fr(21, N)
    c = np.stack([orc.fe_op("mul", 0, a[i], b[i]) for i in range(N)])
    w = orc.rand_fr(22, nw, witness_like=True)
    r, s = orc.rand_fr(23, 1)[0], orc.rand_fr(24, 1)[0]
    want, _ = orc.groth16_prove(pkd, a, b, c, w, r, s)
    pk = zk.ProvingKey(**pkd, precompute_tables=tables)
    try:
        assert pk.info()["tables"] == tables
        assert zk.prove(pk, a, b, c, w, r, s) == want
    finally:
        pk.free()


def _random_circuit(seed, nvars, nc, npub):
    g = ref.SplitMix64(seed)
    sol = [g.felt() for _ in range(nvars)]
    sol[1], sol[2] = 0, 1
    gates = []
    for i in range(nc):
        xa, xb, xc = (int(g.next() % nvars) for _ in range(3))
        ql, qr, qo, qm = (g.felt() for _ in range(4))
        qk = (-(ql * sol[xa] + qr * sol[xb] + qo * sol[xc] + qm * sol[xa] * sol[xb])) % R
        gates.append((ql, qr, qo, qm, qk, xa, xb, xc))
    return pl.SparseR1CS(npub, nvars - npub, gates), sol


@pytest.mark.parametrize("tables", [True, False], ids=["tables", "no_tables"])
def test_plonk_proof_2p10(tables):
    M = pl.ints_to_mont_np
    nc, nvars, npub = 1000, 300, 5
    spr, sol = _random_circuit(2024, nvars, nc, npub)
    n = 1024
    pts = orc.g1_gen_points(1500, n + 3)
    g = spr.constraints
    ck = orc.PlonkKeyC(npub, spr.n_vars, *[M([q[k] for q in g]) for k in (0, 1, 3, 2, 4)], *[[q[k] for q in g] for k in (5, 6, 7)], pts)
    bl = ref.rand_felts(1077, 9)
    want = ck.prove(M(sol), M(bl))
    rb = zb.ResidentBases(pts, table_window_bits=8 if tables else -1)
    col = lambda k: M([q[k] for q in g])
    pk = zp.setup(zp.Circuit(spr.n_public, spr.n_vars, col(0), col(1), col(2), col(3), col(4), [q[5] for q in g], [q[6] for q in g], [q[7] for q in g]), rb)
    try:
        assert zp.prove(pk, M(sol), M(bl)) == want
    finally:
        pk.free()
        rb.free()
