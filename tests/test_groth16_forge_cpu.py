"""The tables of tests/groth16_forge.py hold what they claim: every expected verdict, derived there from integer arithmetic and the reference decoders,
is the host verifier's verdict (an error counts as a reject), the premise of every coefficient group holds under the host pairing check, and a few entries
are also decided by the oracle's independent verifier.  No GPU."""
import numpy as np
import pytest

from noir_backend_using_gnark_amd import verify as zv
from oracle import bn254_ref as ref
from oracle import plonk_ref as pl
from tests import groth16_forge as gf
from tests.helpers import g1_points_from_scalars, g2_points_from_scalars


def _host(case):
    try:
        return int(zv.groth16_verify(case.proof, case.key.bytes, case.pub))
    except ValueError:
        return 0


def _check(cases):
    wrong = [c.label for c in cases if _host(c) != c.expect]
    assert not wrong, wrong


@pytest.mark.parametrize("slot", ["Ar", "Bs", "Krs"])
def test_flag_loss_cases_are_refused_and_consistent_with_infinity(slot):
    cases = gf.flag_loss_cases(slot)
    vectors = gf.slot_vectors(slot)
    assert len(cases) == len(vectors) >= 60 and all(c.expect == 0 for c in cases)
    _check(cases)
    # the premise: with the slot's bytes replaced by the encoding of the point at infinity, the proof is accepted
    lo, hi = gf.SLOTS[slot]
    inf = gf.G2_INF if slot == "Bs" else gf.G1_INF
    for c in cases[:4]:                              # the four base proofs
        assert _host(c._replace(proof=c.proof[:lo] + inf + c.proof[hi:])) == 1, c.label
    # the reference decoders refuse every vector
    for lab, b, cls in vectors:
        with pytest.raises(ValueError):
            pl.g2_decompress(b) if slot == "Bs" else pl.g1_decompress(b)
    classes = {cls for _, _, cls in vectors}
    assert classes == {"flags 00", "infinity flag with payload", "x >= q", "x without a point"} | ({"off-subgroup"} if slot == "Bs" else set())
    reps = [c for c in gf.flag_loss_representatives() if c.label.startswith(slot + " <-")]
    assert len(reps) == len(classes)


def test_slot_vectors_hold_every_vector_of_the_codec_tables():
    from tests import codec_edges as ce
    n1 = sum(kind == "invalid" for _, _, kind in ce.g1_decompress_vectors())
    n2 = sum(kind == "invalid" for _, _, kind in ce.g2_decompress_vectors())
    off = sum(not m for m in ce.g2_decompress_membership().values()) + sum(not m for _, _, _, m in ce.subgroup_vectors())
    assert len(gf.slot_vectors("Ar")) == len(gf.slot_vectors("Krs")) == n1 and len(gf.slot_vectors("Bs")) == n2 + off
    shifted = [lab for lab, _, _ in gf.slot_vectors("Bs") if "G + torsion point" in lab]
    assert any("order 10069" in lab for lab in shifted) and any("order 5864401" in lab for lab in shifted)


def test_coefficient_groups_cancel_together_and_fail_alone():
    groups = gf.coefficient_groups()
    assert [g.label for g in groups] == ["Krs +- D", "Ar +- D", "w +- e", "Krs + 2 D, - D, - D"]
    for g in groups:
        assert len(g.members) == len(g.pairs) and all(c.expect == 0 for c in g.members)
        _check(g.members)
        everything = [p for eq in g.pairs for p in eq]
        assert zv.pairing_check(g1_points_from_scalars([a for a, _ in everything]), g2_points_from_scalars([b for _, b in everything])), g.label
        for c, eq in zip(g.members, g.pairs):
            assert not zv.pairing_check(g1_points_from_scalars([a for a, _ in eq]), g2_points_from_scalars([b for _, b in eq])), c.label
            # the pairs are this member's equation: -Ar and Krs as the proof's bytes have them
            assert ref.g1_compress(ref.g1_neg(gf.g1(eq[0][0]))) == c.proof[:32] and ref.g2_compress(gf.g2(eq[0][1])) == c.proof[32:96], c.label
            assert ref.g1_compress(gf.g1(eq[3][0])) == c.proof[96:], c.label


def test_accept_cases_and_the_plain_ones():
    acc = gf.accept_cases()
    assert set(acc) == {"two public inputs", "K_1 at infinity", "K_0 at infinity", "no public input"}
    for name, cases in acc.items():
        assert all(c.expect == 1 for c in cases)
        _check(cases)
        labels = " | ".join(c.label for c in cases)
        for what in ("Ar at infinity", "Bs at infinity", "Krs at infinity"):
            assert what in labels
    assert gf.key(2, 1).bytes[292 + 32:292 + 64] == gf.G1_INF and gf.key(0).bytes[288:292] == b"\0\0\0\1"
    plus_r = [c for c in acc["two public inputs"] if "+ r" in c.label]
    assert plus_r and all(int.from_bytes(np.asarray(row, dtype=np.uint64).tobytes(), "little") >= ref.R for c in plus_r for row in c.pub)
    for npub in (0, 1, 2, 33):
        k = gf.key(npub)
        _check(gf.good_cases(k, 3) + [gf.reject_case(k)])


def _oracle(case):
    p = case.proof
    proof = (pl.g1_decompress(p[:32]), pl.g2_decompress(p[32:96]), pl.g1_decompress(p[96:]))
    w = [1] + [int.from_bytes(np.asarray(x, dtype=np.uint64).tobytes(), "little") * pow(1 << 256, -1, ref.R) % ref.R for x in case.pub]
    return int(ref.groth16_verify(case.key.points(), proof, w))


def test_the_oracle_decides_four_entries_the_same_way():
    acc = gf.accept_cases()["two public inputs"]
    at_inf = next(c for c in acc if "Ar at infinity" in c.label)
    for c in (acc[0], at_inf, gf.reject_case(gf.KEY), gf.coefficient_groups()[1].members[0]):
        assert _oracle(c) == c.expect, c.label
