"""The Lagrange-form transform of a base array stage by stage (csrc/lagrange.hip: k_lag_scale_in, k_lag_dif_stage, k_lag_finish over g1_scalar_mul29 / acc29_add /
acc29_dbl), against the discrete-log model of tests/lagrange_ref.py, exactly: group arithmetic is exact, so after normalisation every comparison is of bytes.

zk_bn254_lagrange_inspect uploads host points, runs the production builder lagrange_srs_build with a trace and returns the work array after the scale-in and
after every stage -- every entry normalised to its affine image on the host, the point at infinity flagged on its own -- and the n + 2 points of the finish.  Every
base is [k_j] G, so the model knows every entry as an integer and says which butterflies see equal, opposite or infinite operands (test_lagrange_ref_cpu.py asserts
that geometry for every family used here).

Sizes: log_n = 0 (its own path: the borrowed 2-point domain, s = 1, no stage), 1 (one lane, e == 0 only), 2 (the first real twiddle), 8 (n + 2 = 258: the second
workgroup of the finish holds the two blinding lanes alone), 9 (one full workgroup of a stage), 10 (two workgroups; the first stage with at least 64 blocks, the
case the lane mapping k = t / blocks is written for); the chosen-stage pairs at 4."""
import ctypes as C

import numpy as np
import pytest

from noir_backend_using_gnark_amd import _lib
from noir_backend_using_gnark_amd import bn254 as zb
from oracle import plonk_ref as pl
from tests import lagrange_ref as lr

pytestmark = pytest.mark.gpu

R = lr.R
MONT = zb.MultiExpConfig(scalars_mont=True)
SIZES = lr.SIZES


def _compare(got_pts, got_inf, want_ints, where, kernel):
    want_pts = lr.points(want_ints)
    want_inf = np.array([v % R == 0 for v in want_ints], np.uint8)
    got_pts, got_inf = np.asarray(got_pts).reshape(-1, 8), np.asarray(got_inf).reshape(-1)
    assert got_pts.shape == want_pts.shape and got_inf.shape == want_inf.shape, (where, got_pts.shape, want_pts.shape)
    bad = np.nonzero((got_pts != want_pts).any(axis=1) | (got_inf != want_inf))[0]
    if bad.size:
        i = int(bad[0])
        raise AssertionError("%s (%s): %d of %d entries differ, first at index %d: expected [k] G with k = %d (infinity: %d), the device says infinity: %d, image %s"
                             % (where, kernel, bad.size, len(want_ints), i, want_ints[i] % R, want_inf[i], got_inf[i],
                                "equal" if (got_pts[i] == want_pts[i]).all() else "different"))


def run(ks, log_n):
    """inspect the bases [k] G for k in ks over 2^log_n points and hold every entry of every stage and of the result against the model; returns the entry's output"""
    n = 1 << log_n
    out = zb.ResidentBases.lagrange_inspect(lr.points(ks), log_n)
    m = lr.stages(ks, log_n)
    assert out["stages"].shape == (log_n + 1, n, 8) and out["final"].shape == (n + 2, 8)
    tag = "log_n %d" % log_n
    _compare(out["stages"][0], out["stage_inf"][0], m["work"][0], tag + ": after the scale-in", "k_lag_scale_in")
    for s in range(1, log_n + 1):
        _compare(out["stages"][s], out["stage_inf"][s], m["work"][s], tag + ": after stage %d (m = %d)" % (s, n >> s), "k_lag_dif_stage")
    _compare(out["final"][:n], out["final_inf"][:n], m["final"][:n], tag + ": transform in natural order", "k_lag_finish")
    _compare(out["final"][n:], out["final_inf"][n:], m["final"][n:], tag + ": blinding points n, n + 1", "k_lag_finish")
    return out


# ---- families
@pytest.mark.parametrize("log_n", SIZES + (4,))
def test_random_bases(log_n):
    """the baseline: distinct random multiples, no special pair anywhere"""
    ks = lr.fam_random(lr.rng_for("random", log_n), log_n)
    assert lr.special_total(lr.walk(ks, log_n)) == 0
    run(ks, log_n)


@pytest.mark.parametrize("log_n", SIZES)
def test_all_bases_equal(log_n):
    """every first-stage sum doubles, every first-stage difference is infinite (and meets the scalar multiplication); out[0] = [k] G, every other out[i] infinite:
    to_affine of infinity and the bit reversal of a mostly infinite array"""
    n = 1 << log_n
    ks = lr.fam_all_equal(lr.rng_for("all_equal", log_n), log_n)
    out = run(ks, log_n)
    assert out["final_inf"][:n].tolist() == [0] + [1] * (n - 1) and not out["final"][1:n].any()


@pytest.mark.parametrize("log_n", SIZES[1:])
def test_alternating_sign(log_n):
    ks = lr.fam_alternating(lr.rng_for("alternating", log_n), log_n)
    assert lr.walk(ks, log_n)["stage"][-1]["opposite"] == 1
    run(ks, log_n)


@pytest.mark.parametrize("log_n", SIZES[1:])
def test_half_period_negation(log_n):
    """every first-stage sum is infinite, every first-stage difference a doubling"""
    n = 1 << log_n
    ks = lr.fam_half_negated(lr.rng_for("half_negated", log_n), log_n)
    assert lr.walk(ks, log_n)["stage"][0]["opposite"] == n // 2
    out = run(ks, log_n)
    assert out["stage_inf"][1][:n // 2].all() and not out["stage_inf"][1][n // 2:].any()


@pytest.mark.parametrize("log_n", SIZES)
def test_one_hot_spectrum(log_n):
    """inputs all distinct, every output but out[i0] infinite; i0 = 0, 1, n - 1"""
    n = 1 << log_n
    for i0 in sorted({0, 1 % n, n - 1}):
        ks = lr.fam_one_hot(lr.rng_for("one_hot", log_n, i0), log_n, i0)
        out = run(ks, log_n)
        assert np.nonzero(out["final_inf"][:n] == 0)[0].tolist() == [i0], i0


@pytest.mark.parametrize("log_n", SIZES)
def test_bases_at_infinity(log_n):
    """a third of the bases infinite at random places; then all of them, the blinding pairs too"""
    n = 1 << log_n
    ks = lr.fam_third_infinite(lr.rng_for("third_infinite", log_n), log_n)
    assert lr.walk(ks, log_n)["inf_in"] == max(n // 3, 1)
    run(ks, log_n)
    out = run(lr.fam_all_infinite(None, log_n), log_n)
    assert out["stage_inf"].all() and out["final_inf"].all() and not out["final"].any() and not out["stages"].any()


@pytest.mark.parametrize("s", [1, 2, 3, 4])
def test_special_pairs_first_met_at_a_chosen_stage(s):
    """log_n = 4: the first equal pair and the first opposite pair sit in front of stage s, with operands that earlier stages computed (projective
    representatives of their own, not copies of an input)"""
    ks = lr.fam_pairs_at_stage(lr.rng_for("pairs_at_stage", s), 4, s)
    w = lr.walk(ks, 4)
    assert all(sum(c.values()) == 0 for c in w["stage"][:s - 1]) and w["stage"][s - 1]["equal"] == 1 and w["stage"][s - 1]["opposite"] == 1
    run(ks, 4)


@pytest.mark.parametrize("lane", [0, 1])
@pytest.mark.parametrize("log_n", SIZES)
def test_blinding_lanes(log_n, lane):
    """P_(n + lane) equal to P_lane, opposite to it, infinite, P_lane infinite, both infinite"""
    n = 1 << log_n
    for case in lr.BLINDING:
        ks = lr.fam_blinding(lr.rng_for("blinding", log_n, lane, case), log_n, lane, case)
        out = run(ks, log_n)
        assert bool(out["final_inf"][n + lane]) == (case in ("equal", "both_infinite")), case


# ---- the public path
def _read_bases(rb):
    """the points of a registered base array: one multi-exp per row of the identity matrix"""
    eye = np.zeros((rb.n, rb.n, 4), np.uint64)
    eye[np.arange(rb.n), np.arange(rb.n)] = pl.ints_to_mont_np([1])[0]
    return rb.multi_exp_rows(eye, config=MONT)


@pytest.mark.parametrize("family", ["random", "all_equal"])
@pytest.mark.parametrize("log_n", [0, 2, 6])
def test_public_entry_returns_the_inspected_points(log_n, family):
    """ResidentBases.lagrange(log_n) registers the n + 2 points that the inspection reports (and the model expects)"""
    n = 1 << log_n
    ks = (lr.fam_random if family == "random" else lr.fam_all_equal)(lr.rng_for("public", family, log_n), log_n)
    pts = lr.points(ks)
    seen = run(ks, log_n)
    rb = zb.ResidentBases(pts, table_window_bits=-1)
    lag = rb.lagrange(log_n)
    try:
        assert lag.n == n + 2
        got = _read_bases(lag)
    finally:
        lag.free()
        rb.free()
    assert got.shape == (n + 2, 8)
    bad = np.nonzero((got != seen["final"]).any(axis=1))[0]
    assert bad.size == 0, "log_n %d, %s: bases %s of the public entry differ from the inspection's" % (log_n, family, bad[:8].tolist())


def _launches(call):
    _lib.profile(True)
    _lib.profile_reset()
    try:
        call()
        kernels, _ = _lib.split_profile(_lib.profile_read())
    finally:
        _lib.profile(False)
    return {k: v[0] for k, v in kernels.items()}


@pytest.mark.parametrize("log_n", [0, 1, 5, 10])
def test_production_launches_are_unchanged(log_n):
    """a production lagrange() call records one scale-in, log_n stages and one finish and nothing else -- the launches it made before the builder took a trace --
    and the inspection records the same"""
    pts = lr.points(lr.fam_random(lr.rng_for("launches", log_n), log_n))
    want = {"lagrange_scale_in": 1, "lagrange_finish": 1}
    if log_n:
        want["lagrange_dif_stage"] = log_n
    rb = zb.ResidentBases(pts, table_window_bits=-1)
    try:
        rb.lagrange(log_n).free()  # the domain's tables are made on first use: not part of the count
        held = []
        assert _launches(lambda: held.append(rb.lagrange(log_n))) == want
        held[0].free()
    finally:
        rb.free()
    assert _launches(lambda: zb.ResidentBases.lagrange_inspect(pts, log_n)) == want


def test_argument_errors_and_the_call_after_them():
    """zk_bn254_bases_lagrange: log_n = 28 is refused, log_n = 0 takes exactly 3 points and refuses 2, a null out_handle is refused; the inspection refuses the
    same and the next call runs"""
    ks = lr.fam_random(lr.rng_for("errors"), 1)
    pts = lr.points(ks)
    three, two = zb.ResidentBases(pts[:3], table_window_bits=-1), zb.ResidentBases(pts[:2], table_window_bits=-1)
    try:
        for rb, log_n in ((three, 28), (two, 0), (three, 1)):
            with pytest.raises(_lib.ZkmiError) as ei:
                rb.lagrange(log_n)
            assert ei.value.code == _lib.ZK_ERR_ARG, log_n
        assert _lib.lib().zk_bn254_bases_lagrange(three.handle, C.c_uint32(0), None) == _lib.ZK_ERR_ARG
        lag = three.lagrange(0)
        try:
            assert lag.n == 3
            want = lr.points(lr.stages(ks[:3], 0)["final"])
            assert (_read_bases(lag) == want).all()
        finally:
            lag.free()
    finally:
        three.free()
        two.free()
    for kw in (dict(points=pts[:3], log_n=28), dict(points=pts[:2], log_n=0), dict(points=pts[:3], log_n=1)):
        with pytest.raises(_lib.ZkmiError) as ei:
            zb.ResidentBases.lagrange_inspect(**kw)
        assert ei.value.code == _lib.ZK_ERR_ARG, kw
        run(ks, 1)
