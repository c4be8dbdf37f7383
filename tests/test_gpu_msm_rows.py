"""Row-batched commitments on the device (zk_bn254_msm_bases_rows[_dev]): every row's digest against the CPU oracle AND against the device's own one-row
multi-exp, bit for bit, at every shape where the path can go wrong: rows that end inside / on / after a 256-lane digit block, one row (the finish then folds
up to 64 last-level entries), several rows (one entry each), more rows than a chunk holds (a chunk of 1,024 followed by a chunk of ONE), a row stride wider
than the rows with poison in the gaps, a base offset, scalars at the signed-digit carries, sums that are the point at infinity, both values of the sparse flag,
every combination of outputs, and the paths around the batched one.

Bases are helpers.g1_points_from_scalars(ks) with small ks, so the expected digest of a row is (sum_i s_i k_i mod r) G: one scalar multiplication of the oracle.
Small base arrays get no window table by default, so they are registered with an explicit width: c = 8 (128 buckets, 32 digit windows) and c = 13."""
import random

import numpy as np
import pytest

from noir_backend_using_gnark_amd import _lib
from noir_backend_using_gnark_amd import bn254 as zb
from oracle import bn254_ref as ref
from oracle import oracle as orc
from tests import helpers

pytestmark = pytest.mark.gpu

MONT = zb.MultiExpConfig(scalars_mont=True)
PLAIN = zb.MultiExpConfig(scalars_mont=False)
R = ref.R
OFFSET = 3
NB = 1000 + OFFSET
# base i = KS[i] G: small multipliers (cheap to make on the host); bases 0 and 1 are the same point, base 5 is the point at infinity (0, 0)
KS = [7, 7] + [(i * 7919 + 13) % 2039 + 1 for i in range(2, NB)]
KS[5] = 0
INF_ENC = bytes([0x40]) + bytes(31)


@pytest.fixture(scope="module")
def points():
    pts = helpers.g1_points_from_scalars(KS)
    assert not pts[5].any() and (pts[0] == pts[1]).all()
    return pts


@pytest.fixture(scope="module", params=[8, 13], ids=["c8", "c13"])
def bases(request, points):
    rb = zb.ResidentBases(points, table_window_bits=request.param)
    rb.c = request.param
    assert zb.msm_rows_info(rb, 16) == {"chunk_rows": 1024, "batched": True}
    yield rb
    rb.free()


def expected_points(rows_ints, ks):
    """row -> (sum_i s_i k_i mod r) G, all rows in one call of the oracle: (rows, 8) uint64"""
    es = [sum(s * k for s, k in zip(row, ks)) % R for row in rows_ints]
    return orc.g1_mul_gen_many(helpers.mont_limbs(es))


def compressed_of(pts):
    return np.stack([np.frombuffer(orc.g1_compress(p), np.uint8) for p in pts]) if len(pts) else np.zeros((0, 32), np.uint8)


def matrix(rows_ints, stride):
    """Montgomery images of the rows, `stride` elements apart, every gap (and the tail of the last row's stride) filled with 0xff bytes: no field element"""
    n = len(rows_ints[0])
    m = np.full((len(rows_ints), stride, 4), 0xFFFFFFFFFFFFFFFF, np.uint64)
    for v, row in enumerate(rows_ints):
        m[v, :n] = helpers.mont_limbs(row)
    return m


def run_dev(bases, m, n, *, offset=OFFSET, sparse=False, config=MONT, outputs="both"):
    """the _dev entry on a matrix with stride; -> (points or None, digests or None) as numpy"""
    rows, stride = m.shape[0], m.shape[1]
    d = _lib.DeviceBuffer.from_numpy(m)
    try:
        got = bases.multi_exp_rows(d, n=n, rows=rows, row_stride=stride, offset=offset, sparse=sparse, config=config, compressed=outputs != "points",
                                   points=outputs != "digests")
        out, enc = (got if outputs == "both" else ((got, None) if outputs == "points" else (None, got)))
        res = (out.to_numpy(np.uint64, (rows, 8)) if out is not None else None, enc.to_numpy(np.uint8, (rows, 32)) if enc is not None else None)
        for b in (out, enc):
            if b is not None:
                b.free()
        return res
    finally:
        d.free()


def singles(bases, m, n, *, offset=OFFSET, config=MONT):
    """the device's own one-row multi-exp on every row of the same matrix"""
    d = _lib.DeviceBuffer.from_numpy(m)
    try:
        return np.stack([bases.multi_exp_dev(d.ptr + v * m.shape[1] * 32, n, config, offset) for v in range(m.shape[0])])
    finally:
        d.free()


def check_rows(bases, rows_ints, *, stride_pad=3, sparse=False):
    n = len(rows_ints[0])
    m = matrix(rows_ints, n + stride_pad)
    exp = expected_points(rows_ints, KS[OFFSET:OFFSET + n])
    pts, enc = run_dev(bases, m, n, sparse=sparse)
    assert (pts == exp).all(), np.nonzero((pts != exp).any(axis=1))[0]
    assert (enc == compressed_of(exp)).all()
    assert (singles(bases, m, n) == exp).all()
    return pts, enc


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 1000])
def test_random_rows_with_stride_poison_and_offset(bases, n):
    rng = random.Random(1000 * bases.c + n)
    for rows in (1, 2, 3, 5):
        check_rows(bases, [[rng.randrange(R) for _ in range(n)] for _ in range(rows)])


def test_a_chunk_of_1024_rows_and_a_chunk_of_one(bases):
    """1,025 rows: the finish of several sets (one last-level entry each), then, on the same slot and stream, the finish of ONE set (up to 64 entries)"""
    rng = random.Random(77 + bases.c)
    rows_ints = [[rng.randrange(R) for _ in range(4)] for _ in range(1025)]
    check_rows(bases, rows_ints, stride_pad=1)


def window_scalar(c, digit):
    """`digit` in every c-bit window that fits below r"""
    s, w = 0, 0
    while s + (digit << (c * w)) < R:
        s += digit << (c * w)
        w += 1
    return s


def test_zero_row_between_rows_and_carry_scalars(bases):
    n, c = 257, bases.c
    rng = random.Random(5 + c)
    half = 1 << (c - 1)
    rows_ints = [[rng.randrange(R) for _ in range(n)], [0] * n, [rng.randrange(R) for _ in range(n)], [1] * n, [R - 1] * n,
                 [window_scalar(c, half)] * n, [window_scalar(c, half + 1)] * n, [window_scalar(c, half - 1)] * n]
    pts, enc = check_rows(bases, rows_ints)
    assert not pts[1].any() and enc[1].tobytes() == INF_ENC
    assert pts[0].any() and pts[2].any()


def test_one_scalar_repeated_fills_one_bucket(bases):
    s = random.Random(9).randrange(R)
    check_rows(bases, [[s] * 1000, [R - s] * 1000])


def test_sum_is_infinity_without_a_zero_scalar(bases):
    """bases 0 and 1 are the same point P: 1 P + (r - 1) P"""
    rng = random.Random(11)
    for n in (2, 257):
        rows_ints = [[1, R - 1] + [0] * (n - 2), [rng.randrange(R) for _ in range(n)], [1, R - 1] + [0] * (n - 2)]
        m = matrix(rows_ints, n + 2)
        exp = expected_points(rows_ints, KS[:n])
        pts, enc = run_dev(bases, m, n, offset=0)
        assert (pts == exp).all() and (enc == compressed_of(exp)).all()
        assert not pts[0].any() and not pts[2].any() and enc[0].tobytes() == INF_ENC and pts[1].any()
        assert (singles(bases, m, n, offset=0) == exp).all()


def test_sparse_flag_changes_no_byte(bases):
    rng = random.Random(21 + bases.c)
    n = 1000
    wire = [[rng.choice((0, 0, 0, 1, 1, rng.randrange(1 << 16), rng.randrange(1 << 40))) for _ in range(n)] for _ in range(3)] + [[0] * n]
    dense = [[rng.randrange(R) for _ in range(n)] for _ in range(2)]
    for rows_ints in (wire, dense, wire[:1]):
        a = check_rows(bases, rows_ints, sparse=False)
        b = check_rows(bases, rows_ints, sparse=True)
        assert (a[0] == b[0]).all() and (a[1] == b[1]).all()


def test_outputs_alone_and_together_and_the_host_entry(bases):
    rng = random.Random(31 + bases.c)
    n = 256
    rows_ints = [[rng.randrange(R) for _ in range(n)] for _ in range(3)]
    m = matrix(rows_ints, n + 5)
    exp = expected_points(rows_ints, KS[OFFSET:OFFSET + n])
    both = run_dev(bases, m, n, outputs="both")
    only_pts = run_dev(bases, m, n, outputs="points")
    only_enc = run_dev(bases, m, n, outputs="digests")
    assert (both[0] == exp).all() and (both[1] == compressed_of(exp)).all()
    assert (only_pts[0] == exp).all() and only_pts[1] is None
    assert only_enc[0] is None and (only_enc[1] == both[1]).all()
    host = np.ascontiguousarray(m[:, :n])
    hp, he = bases.multi_exp_rows(host, offset=OFFSET, config=MONT, compressed=True)
    assert (hp == both[0]).all() and (he == both[1]).all()
    assert (bases.multi_exp_rows(host, offset=OFFSET, config=MONT, compressed=True, points=False) == both[1]).all()
    assert (bases.multi_exp_rows(host, offset=OFFSET, config=MONT) == both[0]).all()
    # an empty row (n = 0) is the point at infinity, and no rows are no work
    d = _lib.DeviceBuffer(64)
    out, enc = bases.multi_exp_rows(d, n=0, rows=2, config=MONT, compressed=True)
    assert not out.to_numpy(np.uint64, (2, 8)).any() and enc.to_numpy(np.uint8, (2, 32)).tobytes() == INF_ENC * 2
    for b in (d, out, enc):
        b.free()
    with pytest.raises(ValueError, match=r"len\(points\) != len\(scalars\)"):
        bases.multi_exp_rows(host, offset=NB - n + 1, config=MONT)


def regular_rows(seed, rows, n):
    """random scalars in REGULAR form below 2^252 < r, as (rows, n, 4) uint64, and nothing converted on the host"""
    m = np.random.default_rng(seed).integers(0, 1 << 63, size=(rows, n, 4), dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    m[:, :, 3] >>= np.uint64(12)
    return m


def expected_points_regular(m, ks):
    """(sum_i s_i k_i mod r) G for regular-form rows, through 32-bit halves so that the sums stay below 2^64 (k_i < 2^11, n <= 2^16)"""
    halves = np.ascontiguousarray(m).view(np.uint32).reshape(m.shape[0], m.shape[1], 8).astype(np.uint64)
    sums = np.einsum("vnj,n->vj", halves, np.asarray(ks, np.uint64))
    es = [sum(int(sums[v, j]) << (32 * j) for j in range(8)) % R for v in range(m.shape[0])]
    return orc.g1_mul_gen_many(helpers.mont_limbs(es))


@pytest.fixture(scope="module")
def tiled_points():
    """2^16 bases out of 64 distinct ones"""
    ks = [(i * 31 + 5) % 2039 + 1 for i in range(64)]
    return np.tile(helpers.g1_points_from_scalars(ks), (1 << 10, 1)), ks * (1 << 10)


def test_one_row_of_2_16_against_a_default_table(tiled_points):
    pts, ks = tiled_points
    n = 1 << 16
    rb = zb.ResidentBases(pts)
    try:
        assert zb.msm_rows_info(rb, n)["batched"]
        m = regular_rows(41, 1, n)
        exp = expected_points_regular(m, ks)
        got, enc = run_dev(rb, m, n, offset=0, config=PLAIN)
        assert (got == exp).all() and (enc == compressed_of(exp)).all()
        assert (singles(rb, m, n, offset=0, config=PLAIN) == exp).all()
    finally:
        rb.free()


def test_a_chunk_below_1024_rows_and_one_row_more(tiled_points):
    """A shape whose chunk msm_rows_info reports below 1,024, run at chunk + 1 rows.  (The issue asks for a chunk cut by the 2^31 limit on positions; a chunk's
    workspace -- 16 bytes per position and more -- must fit 1 GiB, which holds the positions below 2^26: the workspace bound always cuts first, and that is the
    bound this shape meets.  The limits on keys and positions stay in the chunk rule as guards.)"""
    pts, ks = tiled_points
    n = 1 << 14
    rb = zb.ResidentBases(pts[:n], table_window_bits=8)
    try:
        info = zb.msm_rows_info(rb, n)
        assert info["batched"] and 1 <= info["chunk_rows"] < 1024, info
        assert info["chunk_rows"] < ((1 << 31) - 1) // (n * 32)
        rows = info["chunk_rows"] + 1
        m = regular_rows(43, rows, n)
        exp = expected_points_regular(m, ks[:n])
        got, enc = run_dev(rb, m, n, offset=0, config=PLAIN)
        assert (got == exp).all(), np.nonzero((got != exp).any(axis=1))[0]
        assert (enc == compressed_of(exp)).all()
        pick = [0, 1, info["chunk_rows"] - 1, info["chunk_rows"]]
        assert (singles(rb, np.ascontiguousarray(m[pick]), n, offset=0, config=PLAIN) == exp[pick]).all()
    finally:
        rb.free()


def test_fallbacks_deliver_the_same_bytes(points, bases):
    rng = random.Random(51)
    n = 257
    rows_ints = [[rng.randrange(R) for _ in range(n)], [0] * n, [rng.randrange(R) for _ in range(n)]]
    m = matrix(rows_ints, n + 3)
    exp = expected_points(rows_ints, KS[OFFSET:OFFSET + n])
    # an explicit window width selects the plain method of the single multi-exp, row after row
    for outputs in ("both", "digests"):
        got, enc = run_dev(bases, m, n, config=zb.MultiExpConfig(scalars_mont=True, window_bits=10), outputs=outputs)
        assert (enc == compressed_of(exp)).all() and (got is None or (got == exp).all())
    # a handle without a table
    plain = zb.ResidentBases(points, table_window_bits=-1)
    try:
        assert zb.msm_rows_info(plain, n) == {"chunk_rows": 1, "batched": False}
        got, enc = run_dev(plain, m, n, sparse=True)
        assert (got == exp).all() and (enc == compressed_of(exp)).all()
        hp = plain.multi_exp_rows(np.ascontiguousarray(m[:, :n]), offset=OFFSET, config=MONT)
        assert (hp == exp).all()
    finally:
        plain.free()
    # G2 bases: rows are G1 only -- the documented error, from every entry; the info entry says "not batched"
    g2 = zb.ResidentBases(helpers.g2_points_from_scalars([1, 2, 3, 4]), is_g2=True)
    try:
        assert zb.msm_rows_info(g2, 4) == {"chunk_rows": 1, "batched": False}
        with pytest.raises(_lib.ZkmiError, match="G1 only") as ei:
            g2.multi_exp_rows(np.zeros((2, 4, 4), np.uint64))
        assert ei.value.code == _lib.ZK_ERR_ARG
        d = _lib.DeviceBuffer(1024)
        with pytest.raises(_lib.ZkmiError, match="G1 only"):
            g2.multi_exp_rows(d, n=4, rows=2)
        d.free()
    finally:
        g2.free()
