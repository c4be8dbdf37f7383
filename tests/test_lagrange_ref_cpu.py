"""The discrete-log model of the Lagrange-form transform (tests/lagrange_ref.py) against the definition, the oracle's FFTInverse and bn254_ref's own EC arithmetic;
the geometry of every input family that tests/test_gpu_lagrange_stages.py runs, asserted per case by the model's walker; and the argument errors of
zk_bn254_lagrange_inspect, which are decided before a device is looked for.  No device."""
import os
import re

import numpy as np
import pytest

from noir_backend_using_gnark_amd import _lib
from noir_backend_using_gnark_amd import bn254 as zb
from oracle import bn254_ref as ref
from oracle import oracle as orc
from oracle import plonk_ref as pl
from tests import helpers
from tests import lagrange_ref as lr

R = lr.R
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the model is the transform
@pytest.mark.parametrize("log_n", [0, 1, 2, 3, 4, 6])
def test_final_vector_is_the_definition(log_n):
    """final[i] = (1 / n) sum_j w^(-i j) k_j, then k_n - k_0 and k_(n+1) - k_1; the last stage is the same vector in bit-reversed order"""
    n = 1 << log_n
    ks = lr.fam_random(lr.rng_for("definition", log_n), log_n)
    st = lr.stages(ks, log_n)
    ninv, winv = ref.inv(n, R), ref.inv(lr.omega(log_n), R)
    want = [ninv * sum(pow(winv, i * j, R) * ks[j] for j in range(n)) % R for i in range(n)]
    assert st["final"] == want + [(ks[n] - ks[0]) % R, (ks[n + 1] - ks[1]) % R]
    assert len(st["work"]) == log_n + 1 and all(len(a) == n for a in st["work"])
    assert st["work"][0] == [k * ninv % R for k in ks[:n]]
    assert st["work"][-1] == [want[lr.bitrev(i, log_n)] for i in range(n)]


@pytest.mark.parametrize("log_n", [1, 2, 5, 8, 10])
def test_final_vector_is_the_oracles_inverse_transform(log_n):
    """the domain generator is the oracle's: FFTInverse(DIF) + BitReverse of the same vector, as the parity test of zk_bn254_bases_lagrange takes it"""
    n = 1 << log_n
    ks = lr.fam_random(lr.rng_for("oracle", log_n), log_n)
    got = lr.stages(ks, log_n)["final"][:n]
    want = orc.fr_bit_reverse(orc.fr_ntt(pl.ints_to_mont_np(ks[:n]), True, 1))
    assert pl.mont_np_to_ints(want) == got
    assert lr.omega(log_n) == ref.Domain(n).gen and pow(lr.omega(log_n), n // 2, R) == R - 1


def test_n4_points_by_the_reference_curve_arithmetic():
    """for n = 4 the expected POINTS from the points themselves -- sum_j [c_ij] P_j by bn254_ref's ec_add / ec_mul -- equal the discrete-log shortcut"""
    log_n, n = 2, 4
    ks = lr.fam_random(lr.rng_for("n4"), log_n)
    P = [ref.g1_mul(ref.G1_GEN, k) for k in ks]
    ninv, winv = ref.inv(n, R), ref.inv(lr.omega(log_n), R)
    want = []
    for i in range(n):
        acc = None
        for j in range(n):
            acc = ref.g1_add(acc, ref.g1_mul(P[j], ninv * pow(winv, i * j, R) % R))
        want.append(acc)
    want += [ref.g1_add(P[n], ref.g1_neg(P[0])), ref.g1_add(P[n + 1], ref.g1_neg(P[1]))]
    img = np.stack([np.frombuffer(ref.g1_affine_mont_bytes(p), dtype=np.uint64) for p in want])
    assert (lr.points(lr.stages(ks, log_n)["final"]) == img).all()


def test_both_sources_of_expected_points_agree():
    """lr.points takes bn254_ref's double-and-add for few scalars and the oracle's fixed-base multiplication for many: the same images, 0 -> (0, 0)"""
    rng = lr.rng_for("points")
    ks = [0, 1, 2, R - 1, R - 2, (R - 1) // 2] + [rng.randrange(R) for _ in range(18)]
    assert len(set(ks)) > 16
    many, few = lr.points(ks), helpers.g1_points_from_scalars(ks)
    assert (many == few).all() and not many[0].any() and many[1:].any(axis=1).all()
    assert (lr.points(ks[:5] + ks[:5]) == np.concatenate([few[:5], few[:5]])).all()


# ---- every family reaches the cases it is named for
@pytest.mark.parametrize("log_n", lr.SIZES + (4,))
def test_family_random(log_n):
    w = lr.walk(lr.fam_random(lr.rng_for("random", log_n), log_n), log_n)
    assert lr.special_total(w) == 0 and w["inf_out"] == 0


@pytest.mark.parametrize("log_n", lr.SIZES)
def test_family_all_equal(log_n):
    """every first-stage pair is equal (the sum doubles, the difference is infinite and, where e != 0, meets the scalar multiplication); out[0] = [k] G alone"""
    n = 1 << log_n
    ks = lr.fam_all_equal(lr.rng_for("all_equal", log_n), log_n)
    w, st = lr.walk(ks, log_n), lr.stages(ks, log_n)
    assert st["final"][:n] == [ks[0]] + [0] * (n - 1) and w["inf_out"] == n - 1
    if log_n:
        assert w["stage"][0] == dict(equal=n // 2, opposite=0, inf_operand=0, inf_into_mul=n // 2 - 1)
    for s in range(2, log_n + 1):  # the upper half of every block is infinite from then on
        c = w["stage"][s - 1]
        assert c["equal"] == n >> s and c["inf_operand"] == n // 2 - (n >> s) and c["opposite"] == 0


@pytest.mark.parametrize("log_n", lr.SIZES[1:])
def test_family_alternating(log_n):
    """k_j = (-1)^j k: equal pairs until the last stage, whose pairs (neighbours) are opposite; the transform is k at n / 2 alone"""
    n = 1 << log_n
    ks = lr.fam_alternating(lr.rng_for("alternating", log_n), log_n)
    w, st = lr.walk(ks, log_n), lr.stages(ks, log_n)
    assert st["final"][:n] == [ks[0] if i == n // 2 else 0 for i in range(n)]
    assert w["stage"][-1]["opposite"] == 1 and sum(c["opposite"] for c in w["stage"]) == 1
    if log_n > 1:
        assert w["stage"][0]["equal"] == n // 2 and w["stage"][0]["inf_into_mul"] == n // 2 - 1


@pytest.mark.parametrize("log_n", lr.SIZES[1:])
def test_family_half_negated(log_n):
    """k_(j + n/2) = -k_j: every first-stage sum is infinite and every difference a doubling; the lower half is infinite from then on"""
    n = 1 << log_n
    ks = lr.fam_half_negated(lr.rng_for("half_negated", log_n), log_n)
    w, st = lr.walk(ks, log_n), lr.stages(ks, log_n)
    assert w["stage"][0] == dict(equal=0, opposite=n // 2, inf_operand=0, inf_into_mul=0)
    assert st["work"][1][:n // 2] == [0] * (n // 2) and all(st["work"][1][n // 2:])
    assert all(v == 0 for v in st["final"][0:n:2]) and (all(st["final"][1:n:2]))
    if log_n > 1:
        assert w["stage"][1]["inf_operand"] == n // 4 and w["stage"][1]["inf_into_mul"] == n // 4 - 1


@pytest.mark.parametrize("log_n", lr.SIZES)
def test_family_one_hot(log_n):
    """the forward transform of a delta at i0 = 0, 1, n - 1: all inputs distinct (i0 odd), every output but one infinite"""
    n = 1 << log_n
    for i0 in sorted({0, 1 % n, n - 1}):
        ks = lr.fam_one_hot(lr.rng_for("one_hot", log_n, i0), log_n, i0)
        w, st = lr.walk(ks, log_n), lr.stages(ks, log_n)
        assert [i for i in range(n) if st["final"][i]] == [i0] and w["inf_out"] == n - 1 and w["inf_in"] == 0
        if i0 % 2:
            assert len(set(ks[:n])) == n
            assert w["stage"][0]["opposite"] == n // 2   # w^(i0 n / 2) = -1: the first sums vanish


@pytest.mark.parametrize("log_n", lr.SIZES)
def test_family_infinite_bases(log_n):
    n = 1 << log_n
    ks = lr.fam_third_infinite(lr.rng_for("third_infinite", log_n), log_n)
    w = lr.walk(ks, log_n)
    assert w["inf_in"] == max(n // 3, 1) and (log_n < 2 or w["stage"][0]["inf_operand"] > 0)
    assert sum(c["equal"] + c["opposite"] for c in w["stage"]) == 0
    ks = lr.fam_all_infinite(None, log_n)
    w = lr.walk(ks, log_n)
    assert w["inf_in"] == n == w["inf_out"] and all(c["inf_operand"] == n // 2 for c in w["stage"])
    assert all(b["inf_hi"] and b["inf_lo"] for b in w["blind"]) and lr.stages(ks, log_n)["final"] == [0] * (n + 2)


@pytest.mark.parametrize("s", [1, 2, 3, 4])
def test_family_pairs_at_a_chosen_stage(s):
    """log_n = 4: exactly one equal and one opposite butterfly in front of stage s, no special pair and no infinity before it"""
    log_n = 4
    ks = lr.fam_pairs_at_stage(lr.rng_for("pairs_at_stage", s), log_n, s)
    w = lr.walk(ks, log_n)
    assert w["inf_in"] == 0
    for before in range(s - 1):
        assert sum(w["stage"][before].values()) == 0, before
    c = w["stage"][s - 1]
    assert c["equal"] == 1 and c["opposite"] == 1 and c["inf_operand"] == 0
    if s < log_n:
        assert w["stage"][s]["inf_operand"] >= 1   # the infinities those two pairs leave are operands of the next stage


@pytest.mark.parametrize("log_n", lr.SIZES)
def test_family_blinding_lanes(log_n):
    n = 1 << log_n
    for lane in (0, 1):
        for case in lr.BLINDING:
            ks = lr.fam_blinding(lr.rng_for("blinding", log_n, lane, case), log_n, lane, case)
            b, other, fin = lr.walk(ks, log_n)["blind"][lane], lr.walk(ks, log_n)["blind"][1 - lane], lr.stages(ks, log_n)["final"]
            if case in ("equal", "opposite"):
                assert b["kinds"] == {case} and not b["inf_hi"] and not b["inf_lo"]
            else:
                assert b["kinds"] == {"inf_operand"} and (b["inf_hi"], b["inf_lo"]) == (case != "lo_infinite", case != "hi_infinite")
            assert (fin[n + lane] == 0) == (case in ("equal", "both_infinite"))
            if case == "opposite":
                assert fin[n + lane] == 2 * ks[n + lane] % R
            if log_n or case in ("equal", "opposite", "hi_infinite" if lane else "lo_infinite"):  # (at n = 1 P_1 sits in both lanes)
                assert other["kinds"] == set()


# ---- the entry
def test_inspection_entry_argument_errors_need_no_device():
    name = "zk_bn254_lagrange_inspect"
    assert name in _lib.SYMBOLS and hasattr(_lib.lib(), name)
    assert re.search(r"\bint %s\(" % name, open(os.path.join(ROOT, "include", "zkmi.h")).read())
    pts = np.zeros((3, 8), np.uint64)
    for kw in (dict(points=pts, log_n=28), dict(points=pts, log_n=1), dict(points=pts[:2], log_n=0), dict(points=pts, log_n=40)):
        with pytest.raises(_lib.ZkmiError) as ei:
            zb.ResidentBases.lagrange_inspect(**kw)
        assert ei.value.code == _lib.ZK_ERR_ARG, kw
    req, res = _lib.LagrangeRequest(), _lib.LagrangeResult()
    req.points, req.n_points, req.log_n = pts.ctypes.data, 3, 0
    assert _lib.lib().zk_bn254_lagrange_inspect(None, None) == _lib.ZK_ERR_ARG
    import ctypes as C
    assert _lib.lib().zk_bn254_lagrange_inspect(C.byref(req), C.byref(res)) == _lib.ZK_ERR_ARG   # no place for the result
