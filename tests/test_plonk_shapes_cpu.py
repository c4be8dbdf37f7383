"""CPU checks behind tests/test_gpu_plonk_shapes.py: every builder of tests/plonk_shapes.py gives a satisfied system on the requested domain with the
wiring it claims; the two oracles -- oracle/plonk_ref.py (Python integers) and orc.PlonkKeyC (C) -- give the same verifying key and the same 548 proof
bytes on every family, blinder family and public-input count, the degenerate proofs included; the Python verifier accepts those proofs; and the sweep
reaches the per-size decisions of csrc/plonk.hip it is meant to reach."""
import functools

import numpy as np
import pytest

from oracle import bn254_ref as ref
from oracle import oracle as orc
from oracle import plonk_ref as pl
from tests import plonk_shapes as ps

R = ref.R
M = pl.ints_to_mont_np
COMBOS = ps.FAMILIES + ("zeros+identity_perm",)


@functools.lru_cache(maxsize=None)
def _points(count):
    return orc.g1_gen_points(0x5A5, count)


@pytest.mark.parametrize("family", COMBOS)
def test_builders_are_satisfied_on_the_requested_domain(family):
    for n in (4, 8, 64):
        for npub in (0,) + tuple(p for p in ps.NPUB_CASES if p):
            for fill in ps.FILLS:
                if ps.rows_of(n, fill) - npub < 1:
                    continue
                spr, sol = ps.circuit(family, n, npub, fill, 7 * n + npub)
                assert spr.is_satisfied(sol), (n, npub, fill)
                assert spr.n_public == npub and len(sol) == spr.n_vars
                assert len(spr.constraints) + npub == ps.rows_of(n, fill) and ps.domain_size(spr) == n, (n, npub, fill)
                traits = family.split("+")
                if "zeros" in traits:
                    assert not any(sol) and not any(c[4] for c in spr.constraints)
                if "max" in traits:
                    assert sol[:npub] == [(R - 1) * (i & 1) for i in range(npub)] and set(sol[npub:]) == {R - 1}
                if "identity_perm" in traits:
                    named = [x for c in spr.constraints for x in c[5:8]]
                    assert spr.n_vars == 3 * (len(spr.constraints) + npub) and len(set(named)) == len(named) and min(named) == npub
                    want = ps.expected_identity_perm(n, npub, ps.rows_of(n, fill))
                    assert pl.build_permutation(spr, n) == want
                    assert (want == list(range(3 * n))) == (npub == 0 and fill == "full")
                if "one_cycle" in traits:
                    assert {x for c in spr.constraints for x in c[5:8]} == {npub}
                    if npub == 0:   # one cycle through all 3n slots
                        perm, seen, s = pl.build_permutation(spr, n), set(), 0
                        while s not in seen:
                            seen.add(s)
                            s = perm[s]
                        assert len(seen) == 3 * n
                if "empty_rows" in traits:
                    assert all(c[:5] == (0, 0, 0, 0, 0) for c in spr.constraints[1::2]) and any(c[2] for c in spr.constraints[0::2])


def test_fill_names_and_blinders():
    assert [ps.rows_of(64, f) for f in ps.FILLS] == [64, 33, 63] and ps.rows_of(64, 43) == 43
    for bad in (32, 65):
        with pytest.raises(AssertionError):
            ps.rows_of(64, bad)
    assert ps.blinders("zeros") == [0] * 9 and ps.blinders("max") == [R - 1] * 9
    b = ps.blinders("random")
    assert len(b) == 9 and len(set(b)) == 9 and b == ps.blinders("random") and all(0 < x < R for x in b)


def test_violation_circuit_changes_exactly_the_named_gates():
    for n in (64, 2048):
        spr, sol, where = ps.violation_circuit(n, 3, 11 + n)
        assert spr.is_satisfied(sol) and ps.domain_size(spr) == n and len(spr.constraints) + 3 == n and set(where) == set(ps.VIOLATIONS)
        uses = lambda v: [i for i, c in enumerate(spr.constraints) if v in c[5:8]]
        assert uses(where["last_gate"]) == [len(spr.constraints) - 1] and uses(where["first_gate"]) == [0] and 1 in uses(where["public_input"])
        assert where["public_input"] < spr.n_public <= where["first_gate"]
        for v in where.values():
            bad = list(sol)
            bad[v] = (bad[v] + 1) % R
            assert not spr.is_satisfied(bad)


def _both_oracles(spr, sol, blinder_sets, srs_np=None):
    """setup and proofs by the Python restatement (NTTs and MSMs of >= 64 elements through the C library's primitives) and by the C prover: equal"""
    n = ps.domain_size(spr)
    srs_np = _points(n + 3) if srs_np is None else srs_np
    opk, ovk = pl.plonk_setup(spr, dict(g1=srs_np, g2=None), fast=True)
    ck = ps.c_key(orc, spr, srs_np)
    assert ck.n == n == opk["n"] and ck.n4 == opk["d1"].n
    assert [pl.g1_from_np(d) for d in ck.vk_digests()] == [*ovk["s"], ovk["ql"], ovk["qr"], ovk["qm"], ovk["qo"], ovk["qk"]]
    assert list(ck.perm()) == list(opk["perm"])
    for name in ck.NAMES:
        assert (ck.poly(name) == M(opk[name])).all(), name
    out = []
    for bl in blinder_sets:
        proof = pl.plonk_prove(opk, sol, bl, fast=True)
        want = pl.plonk_proof_bytes(proof)
        assert ck.prove(M(sol), M(bl)) == want
        out.append((proof, want))
    ck.free()
    return ovk, out


def _infinities(proof_bytes):
    """which of the nine points of Proof.WriteTo are the point at infinity (flag 0b01, all other bits zero): L R O Z H1 H2 H3 BatchH ZShiftH"""
    names = ("L", "R", "O", "Z", "H1", "H2", "H3", "BatchH", "ZShiftH")
    offs = [32 * i for i in range(7)] + [224, 484]
    for o in offs:
        assert (proof_bytes[o] >> 6 == 1) == (proof_bytes[o:o + 32] == bytes([0x40]) + bytes(31))
    return {nm for nm, o in zip(names, offs) if proof_bytes[o] >> 6 == 1}


@pytest.mark.parametrize("family", COMBOS)
def test_oracles_agree_on_every_family_and_blinder_family(family):
    """n = 64 and n = 16 (below 64 the Python side computes its transforms and sums itself), one fill each"""
    for n, fill, npub in ((64, "one_short", 2), (16, "half", 1), (8, "full", 0)):
        spr, sol = ps.circuit(family, n, npub, fill, 0xFA + n)
        _, got = _both_oracles(spr, sol, [ps.blinders(b, n) for b in ps.BLINDER_FAMILIES])
        assert len({w for _, w in got}) == 3
        zero_bl = got[ps.BLINDER_FAMILIES.index("zeros")][1]
        # Zero blinders.  All values zero: l = r = o = 0, three MSMs whose scalars are all zero.  The identity permutation (n = 8 here): z = 1, so Z is the
        # SRS's first point, the shifted opening's quotient is zero, and the quotient is the gate part alone, of degree < 2 (n + 2): H3 = 0.  Both: the
        # quotient is the zero polynomial.  BatchH folds S1 and S2, which are never zero, so no proof is infinity throughout.
        traits = family.split("+")
        identity = "identity_perm" in traits and npub == 0 and fill == "full"
        want = ({"L", "R", "O"} if "zeros" in traits else set()) | ({"H3", "ZShiftH"} if identity else set())
        if want == {"L", "R", "O", "H3", "ZShiftH"}:
            want |= {"H1", "H2"}
        inf = _infinities(zero_bl)
        assert want <= inf and not inf & {"Z", "BatchH"}, (n, inf)
        if family in ("random", "zeros", "zeros+identity_perm"):     # elsewhere a structured wiring may shorten the quotient further (one_cycle at n = 8: H3 = 0)
            assert inf == want, (n, inf)
        if identity:
            assert zero_bl[96:128] == ref.g1_compress(pl.g1_from_np(_points(n + 3)[0]))
        for kind in ("random", "max"):   # any other blinders: nothing vanishes but what the identity permutation's short quotient leaves
            assert _infinities(got[ps.BLINDER_FAMILIES.index(kind)][1]) == set()


@pytest.mark.parametrize("npub", ps.NPUB_CASES)
def test_oracles_agree_at_every_public_input_count(npub):
    spr, sol = ps.edge_public_values(*ps.circuit("random", 128, npub, "full" if npub & 1 else "half", 0xC0 + npub))
    assert spr.is_satisfied(sol) and ps.domain_size(spr) == 128
    if npub >= 2:
        assert {0, R - 1} <= set(sol[:npub])
    _both_oracles(spr, sol, [ps.blinders("random", npub)])


def test_oracles_agree_with_more_public_inputs_than_gates():
    spr, sol = ps.edge_public_values(*ps.circuit("random", 64, 40, 43, 0x40))
    assert len(spr.constraints) == 3 and ps.domain_size(spr) == 64
    _both_oracles(spr, sol, [ps.blinders("random", 40)])


@pytest.mark.parametrize("family", COMBOS)
def test_python_verifier_accepts_each_family(family):
    """n = 8 over an SRS of real powers; zero blinders for the families whose proof is then degenerate, random ones otherwise; another public input is refused"""
    alpha = 0x51F7A11
    srs = pl.kzg_new_srs(8 + 3, alpha, fast=True)
    npub, fill = (0, "full") if family == "zeros+identity_perm" else (1, "one_short")
    spr, sol = ps.circuit(family, 8, npub, fill, 0x88)
    kinds = ("zeros", "random") if family in ps.DEGENERATE else ("random",)
    ovk, got = _both_oracles(spr, sol, [ps.blinders(b, 8) for b in kinds], srs_np=np.ascontiguousarray(srs["g1"]))
    vk = dict(ovk, srs_g2=srs["g2"])
    for proof, wire in got:
        assert ps.decode_proof(wire, pl.g1_decompress) == proof
        assert pl.plonk_verify(vk, proof, sol[:npub])
    if npub:
        assert not pl.plonk_verify(vk, got[-1][0], [(sol[0] + 1) % R])


def test_sweep_reaches_the_per_size_decisions():
    plans = {}
    for log_n in ps.SWEEP_LOG_N:
        for length in ps.scan_lengths(1 << log_n):
            plans[length] = ps.scan_plan(length)
    assert {K for K, _ in plans.values()} == {8}                       # K > 8 needs len > 2^21: the 2^22 test of tests/test_gpu_plonk.py
    assert any(nb == 1 for _, nb in plans.values()) and any(nb >= 32 for _, nb in plans.values())
    # two workgroups, the second ragged: n + 3 = 2051 leaves three elements for the second workgroup's first lane
    ragged = sorted(length for length, (K, nb) in plans.items() if nb == 2 and length % (256 * K))
    assert (1 << 11) + 3 in ragged and plans[(1 << 11) + 3] == (8, 2) and ((1 << 11) + 3) - 256 * 8 == 3
    assert plans[1 << 11] == (8, 1) and plans[(1 << 11) + 8] == (8, 2)  # what scan_bufs() is called with: one workgroup up to 2^10, two at 2^11
    assert ps.scan_plan(256 * 1024 * 8) == (8, 1024) and ps.scan_plan(256 * 1024 * 8 + 1) == (9, 911)
    sizes = [1 << k for k in ps.SWEEP_LOG_N]
    assert any(n + 2 < ps.WINDOW_TABLE_MIN for n in sizes) and any(n + 2 >= ps.WINDOW_TABLE_MIN for n in sizes)
    assert {1 << 11, 1 << 12} <= set(sizes) and (1 << 11) + 2 < ps.WINDOW_TABLE_MIN <= (1 << 12) + 2
    assert ps.PI_DIRECT_MAX in ps.NPUB_CASES and ps.PI_DIRECT_MAX + 1 in ps.NPUB_CASES and ps.PI_DIRECT_MAX - 1 in ps.NPUB_CASES
    assert min(ps.NPUB_CASES) == 0 and max(ps.NPUB_CASES) > ps.PI_DIRECT_MAX + 1
    # the big domain is 8 n below six rows and 4 n from there: both fills of n = 8 differ in it
    assert ps.rows_of(8, "half") < 6 <= ps.rows_of(8, "full")
