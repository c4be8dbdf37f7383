"""The Horner suffix scan stage by stage (csrc/scan.hpp: hscan_local_body, hscan_blocks_body, hscan_apply_body under k_hscan_*_rows), against the host model of
tests/hscan_ref.py, exactly: field arithmetic is exact, so every comparison is of bytes.

zk_bn254_hscan_inspect runs the production launcher hscan_rows_passes over host rows with the CALLER's K and nb and the production point preparation hscan_row
(a -> a, a^K, a^(256 K)), and copies back the lane carries and the workgroup totals of pass 1, the totals of pass 2, f(a) and the quotient.  Every row travels with
guard elements either side and every output array starts as poison, so a store outside [0, len) of a row, or a stage entry that no kernel wrote, shows.

What the planner never asks for and these tests do: K other than max(8, ceil(len / 2^18)) -- odd, not a power of two, 1 -- rows under a K that is not their own
(a row shorter than a lane, a row of one lane), and nb > 1024, where the blocks pass walks more than one chunk of 1024 totals (tests/test_hscan_ref_cpu.py pins why
no planned scan gets there)."""
import random

import numpy as np
import pytest

from noir_backend_using_gnark_amd import _lib, kzg
from oracle import plonk_ref as pl
from tests import hscan_ref as hr

pytestmark = pytest.mark.gpu

R = hr.R
M = pl.ints_to_mont_np
PAD = 4
POISON = np.full(4, 0xDEADBEEFCAFEF00D, np.uint64)

_images = {}  # id(coefficient list) -> (the list, its Montgomery image): rows that share a list share an array, and with it a device buffer
_models = {}  # (id(coefficient list), a, K, nb) -> the model's stages as Montgomery images


def image(f):
    if id(f) not in _images:
        _images[id(f)] = (f, M(f))
    return _images[id(f)][1]


def model(f, a, K, nb):
    key = (id(f), a, K, nb)
    if key not in _models:
        image(f)  # keeps f alive, so its id stays its own
        m = hr.stages(f, a, K, nb)
        _models[key] = dict(btot_local=M(m["btot_local"]), btot=M(m["btot"]), tcarry=M([v for lanes in m["tcarry"] for v in lanes]).reshape(nb, 256, 4),
                            total=M([m["total"]])[0], q=M(m["q"]))
    return _models[key]


def same(got, want, what):
    """exact equality of two arrays of field elements, naming the first entries that differ"""
    got, want = np.asarray(got).reshape(-1, 4), np.asarray(want).reshape(-1, 4)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, "%s: %d of %d entries differ, first at %s" % (what, bad.size, got.shape[0], bad[:8].tolist())


def is_poison(a, what):
    a = np.asarray(a).reshape(-1, 4)
    bad = np.nonzero((a != POISON).any(axis=1))[0]
    assert bad.size == 0, "%s: written at %s" % (what, bad[:8].tolist())


def run(rows, K, nb=0, mode="divide", first=None):
    """inspect `rows` = [(coefficients, point), ...] (python ints) and hold every stage of every row against the model (`first(out)`: a check to make before
    that); returns the entry's output"""
    out = kzg.hscan_inspect([(image(f), M([a])[0]) for f, a in rows], K, nb=nb, mode=mode, pad=PAD, poison=POISON)
    used = out["nb"]
    assert used == max(nb, max(hr.scan_blocks(len(f), K) for f, _ in rows))
    if first:
        first(out)
    for r, (f, a) in enumerate(rows):
        n, m = len(f), model(f, a, K, used)
        tag = "row %d (len %d, K %d, nb %d, %s)" % (r, n, K, used, mode)
        live = hr.scan_blocks(n, K)
        for b in range(live, used):  # a workgroup wholly above the row's end: zeros at every stage (the model says so too: this says it of the device alone)
            assert not out["btot_local"][r, b].any() and not out["btot"][r, b].any(), "%s: totals of workgroup %d above the row's end" % (tag, b)
            assert mode == "eval" or not out["tcarry"][r, b].any(), "%s: lane carries of workgroup %d above the row's end" % (tag, b)
        same(out["btot_local"][r], m["btot_local"], tag + ": btot after pass 1")
        if mode == "eval":
            is_poison(out["tcarry"][r], tag + ": tcarry of an evaluation")
        else:
            same(out["tcarry"][r], m["tcarry"], tag + ": tcarry")
        same(out["btot"][r], m["btot"], tag + ": btot after pass 2")
        same(out["total"][r], m["total"], tag + ": total")
        fb, qb = out["f"][r], out["q"][r]
        assert fb.shape == qb.shape == (n + 2 * PAD, 4)
        is_poison(fb[:PAD], tag + ": guard below f")
        is_poison(fb[PAD + n:], tag + ": guard above f")
        if mode == "in_place":
            assert qb is fb
            same(fb[PAD:PAD + n], m["q"], tag + ": q over f")
            continue
        same(fb[PAD:PAD + n], image(f), tag + ": f after the run")
        if mode == "eval":
            is_poison(qb, tag + ": q of an evaluation")
            continue
        is_poison(qb[:PAD], tag + ": guard below q")
        is_poison(qb[PAD + n:], tag + ": guard above q (q[len] on)")
        assert not qb[PAD + n - 1].any(), tag + ": q[len - 1] is not zero"
        same(qb[PAD:PAD + n], m["q"], tag + ": q")
    return out


def rand_poly(rng, n):
    return [rng.randrange(R) for _ in range(n)]


# ---- K and the boundaries: lane, workgroup, tail lane, live lanes of the top workgroup
@pytest.mark.parametrize("K", [1, 2, 3, 8, 9, 17, 31])
def test_every_k_at_lane_and_workgroup_boundaries(K):
    """one row per launch: a row shorter than a lane, one lane, a tail lane of one coefficient (K + 1, 256 K + 1, 512 K + 1), a top workgroup of one live lane,
    of two (2 * 256 K + K + 1) and of all 256; a^K by square-and-multiply at K that is no power of two"""
    rng = random.Random(1000 + K)
    lengths = hr.lengths_for(K)
    assert 1 in lengths and 256 * K in lengths and 2 * 256 * K + K + 1 in lengths
    for n in lengths:
        run([(rand_poly(rng, n), rng.randrange(R))], K)
    for n in (lengths[0], lengths[-1]):  # the other two modes at the ends of the list
        f, a = rand_poly(rng, n), rng.randrange(R)
        run([(f, a)], K, mode="eval")
        run([(f, a)], K, mode="in_place")


# ---- rows of unequal length in one launch, under the K and nb of the longest
@pytest.mark.parametrize("K", [3, 9])
def test_unequal_rows_share_one_launch(K):
    """eight rows a launch: short rows under a K and an nb that are the longest row's -- their upper workgroups come back zero --, a point per row, one
    polynomial at two points, one point under two polynomials; then nb one above what the longest row needs"""
    rng = random.Random(2000 + K)
    W = 256 * K
    shared = rand_poly(rng, W + 1)
    z = [rng.randrange(R) for _ in range(8)]
    rows = [(shared, z[0]), (shared, z[1]), (rand_poly(rng, 1), z[2]), (rand_poly(rng, K - 1), z[2]), (rand_poly(rng, 2 * W + K + 1), z[4]),
            (rand_poly(rng, K), z[5]), (rand_poly(rng, W), z[6]), (rand_poly(rng, 2 * W), z[7])]
    out = run(rows, K)
    assert out["nb"] == 3 and out["f"][0] is out["f"][1]
    out = run(rows, K, nb=4)
    assert out["nb"] == 4
    run(rows, K, mode="eval")
    rows[1] = (rand_poly(rng, K + 1), z[1])  # in place no two rows share their coefficients
    run(rows, K, mode="in_place")
    run(rows, K, nb=4, mode="in_place")


# ---- the chunk loop of the blocks pass: nb > 1024
CHUNK_LENGTHS = (256 * 1024, 256 * 1024 + 1, 256 * 2048, 256 * 2048 + 1)
_chunk_rows = {}


def chunk_row(n):
    if n not in _chunk_rows:
        rng = random.Random(3000 + n % 1000)
        _chunk_rows[n] = (rand_poly(rng, n), rng.randrange(R))
    return _chunk_rows[n]


def check_chunk_totals(out, rows, K, where):
    """the second btot at the chunk boundaries by name: 1023 closes the bottom chunk, 1024 opens the second, 2047 closes it"""
    for r, (f, a) in enumerate(rows):
        m = model(f, a, K, out["nb"])
        for b in (1023, 1024, 2047):
            if b < out["nb"]:
                assert out["btot"][r, b].tobytes() == m["btot"][b].tobytes(), "%s: row %d (len %d): btot[%d] after pass 2" % (where, r, len(f), b)


@pytest.mark.parametrize("n", CHUNK_LENGTHS)
def test_blocks_pass_chunk_loop(n):
    """K = 1: nb = 1024 (one full chunk, no carry), 1025 (a top chunk of ONE total whose carry runs through all of the chunk below), 2048 (two full chunks),
    2049 (three chunks: M^1024 applied to a carry that is itself carried)"""
    rows = [chunk_row(n)]
    assert hr.scan_blocks(n, 1) == {CHUNK_LENGTHS[0]: 1024, CHUNK_LENGTHS[1]: 1025, CHUNK_LENGTHS[2]: 2048, CHUNK_LENGTHS[3]: 2049}[n]
    run(rows, 1, first=lambda out: check_chunk_totals(out, rows, 1, "one row"))


def test_blocks_pass_chunk_loop_rows_of_unequal_chunk_counts():
    """three chunks and one in the same launch under nb = 2049: the short row's 1025 upper totals are zeros that the chunk loop carries through"""
    rows = [chunk_row(CHUNK_LENGTHS[3]), chunk_row(CHUNK_LENGTHS[0])]
    out = run(rows, 1, first=lambda out: check_chunk_totals(out, rows, 1, "two rows"))
    assert out["nb"] == 2049


# ---- points and coefficients
def _coefficient_kinds(rng, n):
    return dict(zero=[0] * n, max=[R - 1] * n, first=[rng.randrange(1, R)] + [0] * (n - 1), last=[0] * (n - 1) + [rng.randrange(1, R)], random=rand_poly(rng, n))


def _point_kinds(rng, K):
    pts = {"zero": 0, "one": 1, "minus_one": R - 1, "order_256": hr.element_of_order(256), "random": rng.randrange(R)}
    w = hr.element_of_order(K) if K > 1 else None
    if w is not None:
        pts["order_K"] = w  # a^K = 1: A = M = 1
    return pts


@pytest.mark.parametrize("K", [3, 17])
def test_points_and_coefficients(K):
    """every kind of point under every kind of row, three workgroups a row (so that M and its square act): a = 0 (A = M = 0: q_i = f_(i+1)), 1, r - 1, an element
    of order 256 (M = a^(256 K) = 1), a K-th root of unity (A = 1; K = 3 -- Fr has none of order 17, since 17 does not divide r - 1, so K = 17 runs without),
    random; rows of zeros, of r - 1, with one coefficient at either end, random"""
    rng = random.Random(4000 + K)
    n = 2 * 256 * K + K + 1
    pts, kinds = _point_kinds(rng, K), _coefficient_kinds(rng, n)
    assert ("order_K" in pts) == (K == 3)
    assert pow(pts["order_256"], 256 * K, R) == 1 and pow(pts["order_256"], K, R) != 1
    pairs = [(f, a) for a in pts.values() for f in kinds.values()]
    for i in range(0, len(pairs), 8):
        out = run(pairs[i:i + 8], K)
        for r, (f, a) in enumerate(pairs[i:i + 8]):
            if a == 0:
                assert out["q"][r][PAD:PAD + n - 1].tobytes() == image(f)[1:].tobytes()


def test_order_256_point_under_k_256():
    """K a multiple of 256 and a of order 256: A = a^K = 1 already"""
    rng = random.Random(4256)
    w = hr.element_of_order(256)
    n = 256 * 256 + 257
    run([(rand_poly(rng, n), w), (rand_poly(rng, 255), w)], 256)


@pytest.mark.parametrize("K", [3, 9])
def test_root_of_the_polynomial(K):
    """f(a) = 0: total is zero and no stage is -- the totals of pass 1 cancel, they do not vanish"""
    rng = random.Random(5000 + K)
    a = rng.randrange(R)
    f = hr.poly_with_root(rng, 2 * 256 * K + K + 1, a)
    out = run([(f, a), (f, (a + 1) % R)], K)
    assert not out["total"][0].any() and out["total"][1].any()
    assert out["btot_local"][0].any(axis=1).all() and out["btot"][0][:2].any(axis=1).all()


# ---- modes, launches and errors
def test_modes_agree_and_evaluation_leaves_q_alone():
    rng = random.Random(6000)
    K = 9
    rows = [(rand_poly(rng, n), rng.randrange(R)) for n in (2 * 2304 + 10, 2304, 5)]
    sep, inp, ev = run(rows, K), run(rows, K, mode="in_place"), run(rows, K, mode="eval")
    for r, (f, _) in enumerate(rows):
        assert inp["f"][r].tobytes() == sep["q"][r].tobytes()
        assert ev["total"][r].tobytes() == sep["total"][r].tobytes() == inp["total"][r].tobytes()
        assert ev["btot"][r].tobytes() == sep["btot"][r].tobytes()


def test_launches_carry_the_production_names():
    """the entry goes through hscan_rows_passes: three launches under the single prover's profile names for a division, two for an evaluation"""
    rng = random.Random(7000)
    rows = [(image(rand_poly(rng, 5000)), M([rng.randrange(R)])[0]), (image(rand_poly(rng, 7)), M([3])[0])]
    three = {"plonk_horner_local": 1, "plonk_horner_blocks": 1, "plonk_divide_apply": 1}
    for mode, want in (("divide", three), ("in_place", three), ("eval", {"plonk_horner_local": 1, "plonk_horner_blocks": 1})):
        _lib.profile(True)
        _lib.profile_reset()
        try:
            kzg.hscan_inspect(rows, 8, mode=mode)
            kernels, _ = _lib.split_profile(_lib.profile_read())
        finally:
            _lib.profile(False)
        assert {k: v[0] for k, v in kernels.items()} == want, (mode, kernels)


def test_argument_errors_and_the_call_after_them():
    rng = random.Random(8000)
    f, a = rand_poly(rng, 600), rng.randrange(R)
    arr, pt = image(f), M([a])[0]
    for kw in (dict(rows=[], K=8), dict(rows=[(arr.copy(), pt) for _ in range(9)], K=8), dict(rows=[(arr, pt)], K=0), dict(rows=[(arr, pt)], K=1, nb=2),
               dict(rows=[(arr, pt), (arr, pt)], K=8, mode="in_place")):
        with pytest.raises(_lib.ZkmiError) as ei:
            kzg.hscan_inspect(**kw)
        assert ei.value.code == _lib.ZK_ERR_ARG, kw
        run([(f, a)], 1, nb=3)  # the slot went back: the next call runs
