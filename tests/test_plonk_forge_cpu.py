"""The tables of tests/plonk_forge.py hold what they claim: every expected verdict, derived there from integer arithmetic and the reference decoder, is the
host verifier's verdict (zk_bn254_plonk_verify; an error counts as a reject), the premises of the flag-loss, identity-only and cancelling cases hold, a few
entries are also decided by the oracle's independent verifier, and the KZG lanes get the host zk_bn254_kzg_verify's verdicts.  No GPU."""
import numpy as np
import pytest

from noir_backend_using_gnark_amd import kzg
from noir_backend_using_gnark_amd import verify as zv
from oracle import bn254_ref as ref
from oracle import plonk_ref as pl
from tests import plonk_forge as pf

R = ref.R


def _host(case, pub=None):
    try:
        return int(zv.plonk_verify(case.proof, case.key.bytes, case.key.g2, case.pub if pub is None else pub))
    except ValueError:
        return 0


def _check(cases):
    cases = list(cases)
    wrong = [c.label for c in cases if _host(c) != c.expect]
    assert not wrong, wrong
    return len(cases)


def test_every_entry_of_the_table_gets_the_host_verdict():
    table = pf.table()
    assert list(table) == pf.KEY_NAMES
    total = sum(_check(cases) for cases in table.values())
    assert total == sum(len(cs) for cs in table.values()) >= 9 * len(pf.refused_encodings()) + 100
    kinds = {c.kind for cs in table.values() for c in cs}
    assert kinds == {"accept", "identity", "flag", "header", "opening"}
    for cs in table.values():
        assert all(c.expect == (c.kind == "accept") for c in cs)
        assert any(c.expect for c in cs) and not all(c.expect for c in cs)      # every key has accepts and a reject
    names = set(table)
    assert {"n_public %d" % n for n in pf.N_PUBLIC} <= names and {"log_n %d" % n for n in pf.LOG_N} <= names
    assert {"%s at infinity" % p for p in pf.KEY_POINTS} <= names and "Ql Qr Qm Qo Qk at infinity" in names


def test_the_keys_are_what_their_names_say():
    for p, k in zip(pf.KEY_POINTS, pf.infinity_keys()):
        at = 112 + 32 * pf.KEY_POINTS.index(p)
        assert k.bytes[at:at + 32] == pf.G1_INF and k.bytes.count(pf.G1_INF) == 1, k.name
    assert pf.infinity_keys()[-1].bytes[112 + 96:] == pf.G1_INF * 5
    k = pf.double_key()
    assert k.bytes[112 + 96:112 + 128] == k.bytes[112 + 128:112 + 160] != pf.G1_INF
    for n in pf.LOG_N:
        k = pf.log_n_key(n)
        assert int.from_bytes(k.bytes[:8], "big") == 1 << n and pow(k.omega, 1 << n, R) == 1 and (n == 0 or pow(k.omega, 1 << (n - 1), R) == R - 1)
    # the key reader's limit: 2^28 is read, 2^29 is not
    assert pf.MAX_LOG_N == 28 == max(pf.LOG_N)
    c = pf.log_n_cases(28)[0]
    beyond = (1 << 29).to_bytes(8, "big") + c.key.bytes[8:]
    with pytest.raises(ValueError, match="power of two"):
        zv.plonk_verify(c.proof, beyond, c.key.g2, c.pub)
    for n in pf.N_PUBLIC:
        assert int.from_bytes(pf.n_public_key(n).bytes[72:80], "big") == n


def test_accepts_hold_the_edges_they_are_named_for():
    cs = {c.label.split(": ", 1)[1]: c for c in pf.base_accepts()}
    for slot, off in pf.POINT_SLOTS.items():
        c = cs["%s at infinity" % slot]
        assert c.proof[off:off + 32] == pf.G1_INF and c.proof.count(pf.G1_INF) == 1, slot
    assert cs["L R O Z H0 H1 H2 at infinity"].proof[:224] == pf.G1_INF * 7
    for s, off in pf.VALUE_SLOTS.items():
        assert cs["%s = 0" % s].proof[off:off + 32] == bytes(32) and cs["%s = r - 1" % s].proof[off:off + 32] == (R - 1).to_bytes(32, "big")
        plus, top = cs["%s written as v + r" % s], cs["%s written as the largest v + k r" % s]
        a, b = int.from_bytes(plus.proof[off:off + 32], "big"), int.from_bytes(top.proof[off:off + 32], "big")
        assert R <= a < 2 * R and b + R >= 1 << 256 and a % R == b % R
        canon = plus.proof[:off] + (a % R).to_bytes(32, "big") + plus.proof[off + 32:]       # the canonical writing is accepted as well
        assert _host(plus._replace(proof=canon)) == 1
    every = cs["every value written as v + r"]
    assert all(int.from_bytes(every.proof[off:off + 32], "big") >= R for off in pf.VALUE_SLOTS.values())
    # public inputs as Montgomery images + r: the same verdicts
    for n in pf.N_PUBLIC:
        for c in pf.n_public_cases(n):
            assert _host(c, pf.plus_r(c.pub)) == 1, c.label
    for c in pf.n_public_cases(33):
        assert c.pub.shape == (33, 4)
    edges = pf.n_public_cases(64)[1].pub
    assert not edges[0].any() and edges[1].tobytes() == pf.limbs([R - 1])[0].tobytes()


@pytest.mark.parametrize("slot", list(pf.POINT_SLOTS))
def test_flag_loss_cases_are_refused_and_accepted_with_infinity(slot):
    cases, vectors = pf.flag_loss_cases(slot), pf.refused_encodings()
    assert len(cases) == len(vectors) >= 59 and all(c.expect == 0 and c.kind == "flag" for c in cases)
    off = pf.POINT_SLOTS[slot]
    for c, (lab, b) in zip(cases, vectors):
        assert c.proof[off:off + 32] == b
        with pytest.raises(ValueError):
            pl.g1_decompress(b)
    # the premise: with the slot's bytes replaced by the encoding of the point at infinity the proof is one of the two accepted bases
    bases = [c for _, _, c in pf.flag_loss_bases(slot)]
    assert [_host(c) for c in bases] == [1, 1]
    for i, c in enumerate(cases):
        assert c.proof[:off] + pf.G1_INF + c.proof[off + 32:] == bases[i % 2].proof
    assert {pf.encoding_class(lab) for lab, _ in vectors} == {"flags 00", "infinity flag with payload", "x >= q", "x without a point"}
    assert sum(c.label.split(": ", 1)[1].startswith(slot + " <-") for c in pf.flag_loss_representatives()) == 4


def _parse(case):
    p = case.proof
    g = lambda off: pl.g1_decompress(p[off:off + 32])
    f = lambda off: int.from_bytes(p[off:off + 32], "big") % R
    proof = dict(lro=[g(0), g(32), g(64)], z=g(96), h=[g(128), g(160), g(192)], batch_h=g(224), claimed=[f(260 + 32 * k) for k in range(7)],
                 z_open_h=g(484), zu=f(516))
    w = [int.from_bytes(np.asarray(x, dtype=np.uint64).tobytes(), "little") * pow(1 << 256, -1, R) % R for x in case.pub]
    return proof, w


def test_identity_rejects_have_both_openings_right():
    """both KZG checks of plonk.Verify pass on these proofs, so only the identity refuses them; they fail on an opening reject, so the check can fail"""
    cases = pf.identity_rejects()
    assert len(cases) == 5 and all(c.expect == 0 for c in cases)
    _check(cases)
    for c in (cases[0], cases[3]):                  # quot + 1; lin_z made without PI
        proof, w = _parse(c)
        assert _openings(c.key, proof, w), c.label
    proof, w = _parse(pf.opening_rejects()[0])
    assert not _openings(pf.base_key(), proof, w)


def _openings(key, proof, w):
    """the two KZG checks of plonk.Verify alone, restated with the oracle's parts (the digests from public data, kzg_derive_gamma, _kzg_check)"""
    vk = key.vk
    fs = pl.Transcript("gamma", "beta", "alpha", "zeta")
    pl._bind_public_data(fs, vk, w)
    gamma = fs.challenge_fr("gamma", *proof["lro"])
    beta = fs.challenge_fr("beta")
    alpha = fs.challenge_fr("alpha", proof["z"])
    zeta = fs.challenge_fr("zeta", *proof["h"])
    n, u = vk["size"], vk["coset_shift"]
    l1 = (pow(zeta, n, R) - 1) * vk["size_inv"] % R * pow(zeta - 1, -1, R) % R
    _, _, lz, rz, oz, s1z, s2z = proof["claimed"]
    zu = proof["zu"]
    zp = pow(zeta, n + 2, R)
    mul, add = ref.g1_mul, ref.g1_add
    folded_h = add(mul(add(mul(proof["h"][2], zp), proof["h"][1]), zp), proof["h"][0])
    c_s3 = (lz + beta * s1z + gamma) * (rz + beta * s2z + gamma) % R * zu % R * beta % R * alpha % R
    c_z = (-(lz + beta * zeta + gamma) * (rz + beta * u % R * zeta + gamma) % R * (oz + beta * u * u % R * zeta + gamma) % R * alpha + alpha * alpha % R * l1) % R
    lin = None
    for p, k in zip([vk["ql"], vk["qr"], vk["qm"], vk["qo"], vk["qk"], vk["s"][2], proof["z"]], [lz, rz, lz * rz % R, oz, 1, c_s3, c_z]):
        lin = add(lin, mul(p, k))
    digests = [folded_h, lin, *proof["lro"], vk["s"][0], vk["s"][1]]
    kg = pl.kzg_derive_gamma(zeta, digests, proof["claimed"])
    fd, fe, acc = None, 0, 1
    for d, v in zip(digests, proof["claimed"]):
        fd, fe, acc = add(fd, mul(d, acc)), (fe + v * acc) % R, acc * kg % R
    return pl._kzg_check(fd, proof["batch_h"], fe, zeta, vk["srs_g2"]) and pl._kzg_check(proof["z"], proof["z_open_h"], zu, zeta * vk["generator"] % R, vk["srs_g2"])


def test_the_oracle_decides_a_spread_of_entries_the_same_way():
    acc = {c.label.split(": ", 1)[1]: c for c in pf.base_accepts()}
    spread = [acc["baseline"], acc["L R O Z H0 H1 H2 at infinity"], acc["W at infinity"], acc["lin_z written as the largest v + k r"],
              pf.identity_rejects()[0], pf.rho_cases()[0], pf.key_accepts()["Qm at infinity"][0], pf.cancelling_pairs()[0].members[1]]
    assert len(spread) == 8
    for c in spread:
        proof, w = _parse(c)
        assert int(pl.plonk_verify(c.key.vk, proof, w)) == c.expect, c.label


def test_header_opening_and_pair_cases():
    assert [c.proof[256:260] for c in pf.header_rejects()] == [b"\0\0\0\6", b"\0\0\0\x08"]
    for c in pf.header_rejects():                                                        # with the count word put right they are accepted
        assert _host(c._replace(proof=c.proof[:256] + b"\0\0\0\7" + c.proof[260:])) == 1
    assert len(pf.opening_rejects()) == 4 and len(pf.rho_cases()) == 2
    pairs = pf.cancelling_pairs()
    assert len(pairs) == 3 and all(len(p.members) == 2 for p in pairs)
    _check(pf.opening_rejects() + pf.header_rejects() + [m for p in pairs for m in p.members])


def test_kzg_lanes_get_the_host_verdicts():
    lanes = pf.kzg_accepts() + pf.kzg_rejects() + [l for p in pf.kzg_cancelling_pairs() for l in p]
    D, H, V, Z, want, g2 = pf.kzg_arrays(lanes)
    got = [int(kzg.verify(D[i], H[i], V[i], Z[i], g2)) for i in range(len(lanes))]
    assert got == list(want), [l.label for l, a, b in zip(lanes, got, want) if a != b]
    by = {l.label: i for i, l in enumerate(lanes)}
    assert not D[by["C at infinity"]].any() and H[by["C at infinity"]].any()
    assert not H[by["c = v: X and C - v G + z X at infinity"]].any()
    i = by["C at infinity, v = 0: X at infinity too"]
    assert not D[i].any() and not H[i].any()
    assert H[by["z = tau, c = v, X arbitrary"]].any()
    assert sum(want) == len(pf.kzg_accepts()) and len(pf.kzg_accepts()) >= 24 + 7
