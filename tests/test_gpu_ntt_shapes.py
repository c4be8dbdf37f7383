"""Device NTT and computeH (csrc/ntt.hip) at EVERY pass plan and on worst-case inputs (-m gpu).

Sizes: every log_n in 0 .. 25 for the stand-alone transform and 0 .. 22 for computeH, so that every (k, logL, bit_lo) a pass can take runs in a
comparison (tests/test_ntt_shapes_cpu.py checks the coverage against a re-statement of plan_passes()): odd k (a closing one-stage group), the unit-twiddle
group on index bit 0, tiles that leave lanes idle, one or two strided passes.
Inputs: the structured families of tests/ntt_shapes.py -- constants at the largest image, vectors alternating between the extremes at one stage's
pairing distance, impulses, geometric sequences, an edge mix -- next to one random vector.
What the structured inputs add over random ones, from the exact limb model of tools/u29_ntt_model.py run with the production groups of two stages:
  * the bias constants carry so much slack (2^30 per limb; and the group-end reduce leaves an all-sums value below 2 r, so a subtrahend reaches at most
    2 r in a group's first stage and 4 (r - 1) in its second -- max and alt reach exactly that, random data 3.2 r at 2^8 and 3.7 r at 2^11) that lowering
    any single one of u29r_sub<16>, <24> or the DIT <16> to <4> changes no result for ANY canonical input: no input can test them;
  * a missing group-end reduce of the all-sums output in the groups that do not hold index bit 0 (one template branch of ntt_group29) does change results:
    the sums double per stage, and at the stage that pairs index bit j the complement alt(j) subtracts a sum of r - 1 from a sum of zeros, past the 16 r
    or 24 r bias.  In a DIF pass of k = 6 .. 9 stages (every contiguous pass at 2^6 .. 2^9, every strided pass of that length) the complement alt(j) on the
    lowest k - 5 bits of the pass gives a wrong result at every size, while none of 40 random and 20 edge-mix vectors per size does (differences of random
    sums stay within a few r); at k = 10 one random vector in 40 shows it, at k = 11 one in 6 and the constant r - 1 too.
So the value of this module is the pass-plan coverage first, and on the input side the alt family for growth between the stage groups, not bias stress.
Expectations: the C oracle element by element, and closed forms in Python integers where a family has one -- never the device or the library's host code.
All inputs are canonical images (< r), the contract include/zkmi.h states for these entries."""
import ctypes as C
import time

import numpy as np
import pytest

import noir_backend_using_gnark_amd as zk
from noir_backend_using_gnark_amd import _lib
from oracle import oracle as orc
from tests import ntt_shapes as S
from tests.helpers import sha_image

pytestmark = pytest.mark.gpu

SHA_FROM = 23      # from here the images are compared through SHA-256, as the other large-size tests do


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    _lib.require_device()  # fail loudly: no silent fallback


def _fe_mul(x, y):
    return orc.fe_op("mul", 0, x, y)


def _same(got, want, log_n):
    return sha_image(got) == sha_image(want) if log_n >= SHA_FROM else bool((got == want).all())


def _sweep(log_n, run):
    """every (family, mode) of the size: run(x, inverse, dec, coset) -> device result; against the oracle and, where there is one, the closed form"""
    n = 1 << log_n
    t0 = time.time()
    built = {}
    cases = S.standalone_cases(log_n)
    for fam, (inverse, dec, coset) in cases:
        key = (fam, inverse, dec, coset) if fam[0] == "geometric" else fam
        if key not in built:
            if log_n >= S.LARGE_FROM:
                built.clear()                      # a gibibyte per vector at 2^25: keep one
            built[key] = S.build(fam, n, inverse, dec, coset, rand_fr=orc.rand_fr)
        x = built[key]
        got = run(x, inverse, dec, coset)
        want = orc.fr_ntt(x, bool(inverse), dec, bool(coset))
        assert _same(got, want, log_n), ("oracle", log_n, fam, inverse, dec, coset)
        if log_n < S.LARGE_FROM:
            form = S.closed_form(fam, n, inverse, dec, coset)
            assert (form is not None) == (fam[0] in ("zeros", "max", "impulse", "geometric"))
            if form is not None:
                assert (got == form).all(), ("closed form", log_n, fam, inverse, dec, coset)
    print("log_n %d: %d transforms in %.1f s" % (log_n, len(cases), time.time() - t0))


def _host_entry(x, inverse, dec, coset):
    y = x.copy()
    dom = zk.Domain(y.shape[0])
    (dom.fft_inverse if inverse else dom.fft)(y, dec, bool(coset))
    return y


def _resident_entry(x, inverse, dec, coset):
    """zk_bn254_ntt_dev on data already in device memory: always the single-device kernels (the host-copy entry may spread a large vector over several GPUs)"""
    n = x.shape[0]
    d = _lib.DeviceBuffer.from_numpy(x)
    _lib.check(_lib.lib().zk_bn254_ntt_dev(C.c_void_p(d.ptr), C.c_uint32(S.log2(n)), C.c_int(int(inverse)), C.c_int(dec), C.c_int(int(coset)), None))
    return d.to_numpy(np.uint64, (n, 4))


# ------------------------------------------------------------------------------------------------ stand-alone transform
@pytest.mark.parametrize("log_n", [s for s in S.STANDALONE_LOG_N if s < S.LARGE_FROM])
def test_ntt_every_family_and_mode(log_n):
    """2^0 .. 2^20: the eight mode combinations on every family; the oracle element by element, and the closed form of impulse, geometric, max
    and zeros"""
    _sweep(log_n, _host_entry)


@pytest.mark.parametrize("log_n", [s for s in S.STANDALONE_LOG_N if s >= S.LARGE_FROM])
def test_ntt_two_strided_passes_worst_case_inputs(log_n):
    """2^21 .. 2^25, the two-pass splits (5, 5), (6, 5), (6, 6), (7, 6), (7, 7): computeH's four modes on max, alt, edge-mix and random.  From 2^23 each
    alt vector is taken in one mode and only the first bit of each pass keeps both vectors (tests/ntt_shapes.py standalone_cases): the oracle needs
    seconds per transform there"""
    _sweep(log_n, _host_entry)


@pytest.mark.parametrize("log_n", [9, 15, 18, 21])
def test_ntt_resident_entry_per_pass_plan_class(log_n):
    """one size per class of plan (one contiguous pass; plus a strided pass of odd / even k; plus two strided passes) through zk_bn254_ntt_dev"""
    n = 1 << log_n
    top_pass = S.plan_passes(log_n)[-1]
    fams = [("max",), ("alt", top_pass[0], False), ("alt", log_n - 1, True), ("alt", 0, True), ("edge_mix", 0xD00 + log_n), ("impulse", n - 1)]
    for fam in fams:
        x = S.build(fam, n, 0, S.DIF, 0)
        for inverse, dec, coset in (S.ALL_MODES if log_n < S.LARGE_FROM else S.H_MODES):
            got = _resident_entry(x, inverse, dec, coset)
            assert (got == orc.fr_ntt(x, bool(inverse), dec, bool(coset))).all(), (log_n, fam, inverse, dec, coset)
    x = S.edge_mix(n, 0xD80 + log_n)
    d = _lib.DeviceBuffer.from_numpy(x)
    _lib.check(_lib.lib().zk_bn254_bit_reverse_dev(C.c_void_p(d.ptr), C.c_uint32(log_n), None))
    assert (d.to_numpy(np.uint64, (n, 4)) == orc.fr_bit_reverse(x)).all()


# ------------------------------------------------------------------------------------------------------------- computeH
@pytest.mark.parametrize("log_n", S.H_LOG_N)
def test_compute_h_every_size_structured_triples(log_n):
    """computeH (the fused inverse-forward pass, three vectors per launch, the closing step on the last stage's stores) at every size 2^0 .. 2^22:
    zeros, max, a true quotient (c = a * b), alt(j) / its complement / max, and an edge mix, at the lengths the zero-padding distinguishes"""
    t0 = time.time()
    cases = S.h_cases(log_n)
    triples = {}
    for t, n in cases:
        if t not in triples:
            triples.clear()                        # the cases come triple by triple: keep one
            triples[t] = S.h_triple(t, log_n, orc.rand_fr, _fe_mul)
        a, b, c = (np.ascontiguousarray(v[:n]) for v in triples[t])
        got = zk.compute_h(a, b, c, log_n)
        assert (got == orc.groth16_compute_h(a, b, c, log_n)).all(), (log_n, t, n)
        if t[0] == "zeros":
            assert not got.any()
    print("log_n %d: %d computeH calls in %.1f s" % (log_n, len(cases), time.time() - t0))


def test_prove_edge_mix_constraints_at_2p13():
    """a whole proof at a domain size no other proof test takes (2^13: a strided pass of k = 2), with a, b, c an edge mix: computeH's first passes read
    the caller's vectors from a separate buffer (the `src` variant) on a structured input.  Proof bytes against the oracle's."""
    log_n = 13
    N = 1 << log_n
    n_wires, n_public = N - 3, 5
    pkd = dict(log_domain=log_n, n_wires=n_wires, n_public=n_public,
               g1_alpha=orc.g1_gen_points(1, 1)[0], g1_beta=orc.g1_gen_points(2, 1)[0], g1_delta=orc.g1_gen_points(3, 1)[0],
               g1_a=orc.g1_gen_points(4, n_wires), g1_b=orc.g1_gen_points(5, n_wires), g1_k=orc.g1_gen_points(6, n_wires - n_public),
               g1_z=orc.g1_gen_points(7, N), g2_beta=orc.g2_gen_points(8, 1)[0], g2_delta=orc.g2_gen_points(9, 1)[0],
               g2_b=orc.g2_gen_points(10, n_wires))
    n_cons = N - 10
    a, b, c = (S.edge_mix(n_cons, 0xB00 + i) for i in range(3))
    w = orc.rand_fr(22, n_wires, witness_like=True)
    r, s = orc.rand_fr(23, 1)[0], orc.rand_fr(24, 1)[0]
    exp, _ = orc.groth16_prove(pkd, a, b, c, w, r, s)
    pk = zk.ProvingKey(**pkd)
    try:
        assert zk.prove(pk, a, b, c, w, r, s) == exp
    finally:
        pk.free()
