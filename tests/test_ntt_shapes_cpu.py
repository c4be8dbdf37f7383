"""CPU checks behind tests/test_gpu_ntt_shapes.py: the structured input families and their closed forms (tests/ntt_shapes.py) against the C oracle, the
C oracle against the pure-Python fft.Domain on exactly those inputs, and the coverage of csrc/ntt.hip's pass plans by the swept sizes."""
import numpy as np
import pytest

from oracle import bn254_ref as ref
from oracle import oracle as orc
from tests import ntt_shapes as S


def _fe_mul(x, y):
    return orc.fe_op("mul", 0, x, y)


def _ref_transform(x, inverse, dec, coset):
    """the pure-Python fft.Domain on the images as field elements (the transforms are linear, so this is the image of the transform)"""
    dom = ref.Domain(x.shape[0])
    v = S.to_ints(x)
    return S.from_ints((dom.fft_inverse if inverse else dom.fft)(v, dec, bool(coset)))


# ---------------------------------------------------------------------------------------------------------- builders
def test_builders_give_canonical_images_of_the_stated_shape():
    for log_n in (0, 1, 5, 12, 13):
        n = 1 << log_n
        for fam in S.families(log_n):
            for mode in ((0, S.DIF, 0), (1, S.DIT, 1)):
                x = S.build(fam, n, *mode, rand_fr=orc.rand_fr)
                assert x.shape == (n, 4) and x.dtype == np.uint64 and S.is_canonical(x), (log_n, fam)
    n = 64
    top = S.limbs_of(S.R - 1)
    for j in range(6):
        a, b = S.alt(n, j), S.alt(n, j, True)
        for i in range(n):
            assert (a[i] == (top if not (i >> j) & 1 else 0)).all() and (b[i] == (top if (i >> j) & 1 else 0)).all()
    assert S.to_ints(S.impulse(8, 3)) == [0, 0, 0, S.ONE_IMG, 0, 0, 0, 0]
    assert S.to_ints(S.vmax(3)) == [S.R - 1] * 3 and S.to_ints(S.zeros(2)) == [0, 0]
    assert not S.is_canonical(S.const(2, S.R)) and S.is_canonical(S.const(2, S.R - 1))
    e = S.to_ints(S.edge_mix(1 << 14, 7))
    share = sum(v in (0, 1, S.R - 1) for v in e) / len(e)
    assert 0.12 < share < 0.18 and all(v in e for v in (0, 1, S.R - 1))
    assert S.impulse_positions(1 << 12) == [0, 1, 2047, 2048, 4095] and S.impulse_positions(1) == [0] and S.impulse_positions(2048) == [0, 1, 1024, 2047]


def test_alt_bits_follow_the_pass_plan():
    assert S.alt_bits(12) == list(range(12))
    assert S.alt_bits(20) == [0, 1, 2, 10, 11, 18, 19]
    assert S.alt_bits(25) == [0, 1, 2, 10, 11, 17, 18, 23, 24]          # passes (0, 11), (11, 7), (18, 7)
    for log_n in S.STANDALONE_LOG_N:
        for j in S.alt_bits(log_n):
            assert 0 <= j < log_n
        # every alt bit of the full subset is kept where the sweep thins the alt vectors out
        got = {f[1] for f, _ in S.standalone_cases(log_n) if f[0] == "alt"}
        assert got == set(S.alt_bits(log_n))


# ------------------------------------------------------------------------------------------- closed forms against the oracle
@pytest.mark.parametrize("log_n", range(0, 13))
def test_closed_forms_equal_the_oracle(log_n):
    n = 1 << log_n
    seen = set()
    for fam in S.families(log_n):
        for inverse, dec, coset in S.ALL_MODES:
            want = S.closed_form(fam, n, inverse, dec, coset)
            if want is None:
                assert fam[0] in ("alt", "edge_mix", "random")
                continue
            x = S.build(fam, n, inverse, dec, coset)
            assert (orc.fr_ntt(x, bool(inverse), dec, bool(coset)) == want).all(), (log_n, fam, inverse, dec, coset)
            seen.add(fam[0])
    assert seen == {"zeros", "max", "impulse", "geometric"}


def test_closed_forms_in_the_terms_of_the_residues():
    """the statements of the closed forms on the VALUES: an impulse gives a column of twiddle powers, a geometric input n at one index, the constant
    (r - 1) 2^-256 gives n times itself at index 0"""
    n, log_n = 32, 5
    dom = ref.Domain(n)
    rinv = pow(1 << 256, -1, S.R)
    val = lambda a: [v * rinv % S.R for v in S.to_ints(a)]
    got = val(S.closed_form(("impulse", 3), n, 0, S.DIF, 0))
    assert got == ref.bit_reverse([pow(dom.gen, 3 * k, S.R) for k in range(n)])
    got = val(S.closed_form(("impulse", 3), n, 1, S.DIT, 1))                    # DIT: memory index 3 is logical index bitrev(3)
    i = ref.bitrev(3, log_n)
    assert got == [pow(dom.gen_inv, i * k, S.R) * dom.card_inv * pow(dom.coset_inv, k, S.R) % S.R for k in range(n)]
    got = val(S.closed_form(("geometric", 5), n, 0, S.DIT, 0))
    assert got == [n if k == 5 else 0 for k in range(n)]
    assert val(S.geometric(n, 5, 0, S.DIF, 0)) == [pow(dom.gen_inv, 5 * i, S.R) for i in range(n)]
    got = val(S.closed_form(("max",), n, 0, S.DIF, 0))
    assert got == [(S.R - 1) * rinv * n % S.R] + [0] * (n - 1)


# ------------------------------------------------------------------------------- the oracle against the pure-Python Domain
@pytest.mark.parametrize("log_n", range(0, 9))
def test_oracle_equals_python_domain_on_structured_inputs(log_n):
    n = 1 << log_n
    for fam in S.families(log_n):
        for inverse, dec, coset in S.ALL_MODES:
            x = S.build(fam, n, inverse, dec, coset, rand_fr=orc.rand_fr)
            assert (orc.fr_ntt(x, bool(inverse), dec, bool(coset)) == _ref_transform(x, inverse, dec, coset)).all(), (log_n, fam, inverse, dec, coset)
    x = S.edge_mix(n, 5)
    assert (orc.fr_bit_reverse(x) == S.from_ints(ref.bit_reverse(S.to_ints(x)))).all()


@pytest.mark.parametrize("log_n", range(0, 7))
def test_oracle_compute_h_equals_python_on_structured_triples(log_n):
    """groth16_compute_h on the triples and lengths of the device sweep against bn254_ref.compute_h (on the values behind the images)"""
    dom = ref.Domain(1 << log_n)
    rinv = pow(1 << 256, -1, S.R)
    vals = lambda a: [v * rinv % S.R for v in S.to_ints(a)]
    for t, n in S.h_cases(log_n):
        a, b, c = (v[:n] for v in S.h_triple(t, log_n, orc.rand_fr, _fe_mul))
        want = [v * (1 << 256) % S.R for v in ref.compute_h(vals(a), vals(b), vals(c), dom)]
        assert (orc.groth16_compute_h(a, b, c, log_n) == S.from_ints(want)).all(), (log_n, t, n)


def test_quotient_triple_is_a_product_and_stays_one_when_tiled(monkeypatch):
    monkeypatch.setattr(S, "QUOTIENT_PERIOD", 8)
    a, b, c = S.h_triple(("quotient",), 5, orc.rand_fr, _fe_mul)
    assert a.shape == (32, 4) and (a[:8] == a[16:24]).all() and (a[:8] == a[24:]).all() and not (a[0] == a[1]).all()
    assert not (a[:8] == a[8:16]).any(axis=1).any() and not (b[:8] == b[8:16]).any(axis=1).any()      # the second block is a stretch of its own
    for i in range(32):
        assert (c[i] == _fe_mul(a[i], b[i])).all()
    h = orc.groth16_compute_h(a, b, c, 5)
    assert (orc.fr_bit_reverse(h)[-1] == 0).all()          # a true quotient has degree <= N - 2


# --------------------------------------------------------------------------------------------------- pass-plan coverage
def test_plan_restatement_matches_the_documented_splits():
    for log_n in range(0, 12):
        assert S.plan_passes(log_n) == [(0, log_n, 0)]
    for log_n in range(12, 21):
        k = log_n - 11
        assert S.plan_passes(log_n) == [(0, 11, 0), (11, k, 11 - k)]
    splits = {21: (5, 5), 22: (6, 5), 23: (6, 6), 24: (7, 6), 25: (7, 7), 28: (9, 8)}
    for log_n, (k1, k2) in splits.items():
        assert S.plan_passes(log_n) == [(0, 11, 0), (11, k1, 11 - k1), (11 + k1, k2, 11 - k2)]


def test_swept_sizes_cover_every_pass_shape_up_to_2p25():
    """every (k, logL) a contiguous pass and every (k, logL, bit_lo) a strided pass can take at log_n <= 25 occurs in the stand-alone sweep, and -- up
    to log_n = 22, where computeH's sweep ends -- in computeH's.  The wanted sets come from the same re-statement over 0 .. 25, so this is a guard against
    a later trim of the swept sizes; what is stated independently is the set of contiguous (k, 0) and of strided k.  If TILE_LOG or K_STRIDED change in
    csrc/ntt.hip, plan_passes() in tests/ntt_shapes.py has to follow (the comment at those constants says so)."""
    def shapes(sizes):
        contiguous, strided = set(), set()
        for log_n in sizes:
            plan = S.plan_passes(log_n)
            assert sum(k for _, k, _ in plan) == log_n
            contiguous.add((plan[0][1], plan[0][2]))
            strided |= {(k, logL, bit_lo) for bit_lo, k, logL in plan[1:]}
        return contiguous, strided

    want_c, want_s = shapes(range(0, 26))
    assert want_c == {(k, 0) for k in range(0, S.TILE_LOG + 1)}
    assert {k for k, _, _ in want_s} == set(range(1, S.K_STRIDED + 1))     # every strided k, odd ones (a closing one-stage group) included
    assert shapes(S.STANDALONE_LOG_N) == (want_c, want_s)
    assert {log_n for log_n in S.STANDALONE_LOG_N if any(S.standalone_cases(log_n))} == set(range(0, 26))
    h_c, h_s = shapes(range(0, 23))
    assert shapes(S.H_LOG_N) == (h_c, h_s) and h_c == want_c
    # the idle-lane tiles (fewer than 512 groups of four elements) and full ones both occur
    assert {k + logL < 11 for k, logL in want_c} == {True, False}


def test_sweep_cases_keep_every_family_mode_and_length():
    for log_n in S.STANDALONE_LOG_N:
        cases = S.standalone_cases(log_n)
        names = {f[0] for f, _ in cases}
        modes = {m for _, m in cases}
        if log_n < S.LARGE_FROM:
            assert modes == set(S.ALL_MODES) and {"zeros", "max", "impulse", "geometric", "edge_mix", "random"} <= names
            assert ("alt" in names) == (log_n > 0)
        else:
            assert modes == set(S.H_MODES) and names == {"max", "alt", "edge_mix", "random"}
            for fam in (("max",), ("edge_mix", 0xE00 + log_n), ("random", 0xA00 + log_n)):
                assert all((fam, m) in cases for m in S.H_MODES)
    for log_n in S.H_LOG_N:
        cases = S.h_cases(log_n)
        assert {t[0] for t, _ in cases} == {"zeros", "max", "quotient", "edge_mix"} | ({"alt"} if log_n else set())
        N = 1 << log_n
        assert set(S.h_lengths(log_n)) == {n for n in (N, N - 1, 1, N // 2 + 1) if n >= 1}
        triples = [("zeros",), ("max",), ("quotient",), ("edge_mix",)] + [("alt", j) for j in S.alt_bits(log_n)]
        assert sorted(cases) == sorted((t, n) for t in triples for n in S.h_lengths(log_n))      # the full cross at every size
