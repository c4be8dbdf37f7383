"""Device pairing values (zk_bn254_pair) and batch Groth16 verification (zk_bn254_groth16_verify_batch) against the host pairing and the host verifier."""
import json
import os

import numpy as np
import pytest

import noir_backend_using_gnark_amd as zk
from noir_backend_using_gnark_amd import _lib
from noir_backend_using_gnark_amd import verify as zv
from oracle import bn254_ref as ref
from oracle import plonk_ref as pl
from tests.helpers import g1_points_from_scalars, g2_points_from_scalars, h2i, mont_limbs

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    with open(os.path.join(HERE, "golden", name)) as f:
        return json.load(f)


def _host_verdicts(proofs, vk, pubs):
    out = []
    for p, w in zip(proofs, pubs):
        try:
            out.append(zv.groth16_verify(p, vk, w))
        except ValueError:
            out.append(False)
    return np.array(out, dtype=bool)


@pytest.mark.parametrize("n", [0, 1, 2, 3, 7, 64])
def test_device_pairing_equals_host_value(n):
    g = ref.SplitMix64(0xBA7 + n)
    ka = [g.felt() for _ in range(n)]
    kb = [g.felt() for _ in range(n)]
    if n >= 3:
        ka[0], kb[0] = 1, 1        # the generators
        ka[1] = 0                  # G1 infinity
        kb[2] = 0                  # G2 infinity
    P, Q = g1_points_from_scalars(ka), g2_points_from_scalars(kb)
    dev = zv.pair(P, Q)
    assert (dev == zv.pair(P, Q, on_device=False)).all()


@pytest.fixture(scope="module")
def tile_of_eight():
    """eight pairs (a_i G, b_i H) with a = 0, b = 0, a = r - 1 and the generators among them, and the host's e(a_i b_i G, H) per pair's worth"""
    g = ref.SplitMix64(0x7113)
    ka = [1, 0, g.felt(), ref.R - 1, g.felt(), g.felt(), g.felt(), g.felt()]
    kb = [1, g.felt(), 0, g.felt(), ref.R - 1, g.felt(), g.felt(), g.felt()]
    return ka, kb, g1_points_from_scalars(ka), g2_points_from_scalars(kb)


@pytest.mark.parametrize("n", [65, 128, 129, 257, 1 << 16, (1 << 16) + 1])
def test_device_pairing_beyond_one_workgroup_and_one_chunk(n, tile_of_eight):
    """a second workgroup of k_miller (64 lanes each), odd levels of the product tree, and past 2^16 pairs the chunk products multiplied on the host:
    prod e(a_i G, b_i H) = e(s G, H), s = sum a_i b_i mod r, by bilinearity -- the host's value of that one pair (test_pair_cpu.py pins it to the oracle)"""
    ka, kb, P8, Q8 = tile_of_eight
    idx = np.arange(n) % 8
    s = sum(ka[i] * kb[i] for i in idx[:8]) * (n // 8) + sum(ka[i] * kb[i] for i in idx[:n % 8])
    want = zv.pair(g1_points_from_scalars([s % ref.R]), g2_points_from_scalars([1]), on_device=False)
    P, Q = P8[idx], Q8[idx]
    dev = zv.pair(P, Q)
    assert (dev == want).all()
    if n <= 257:
        assert (zv.pair(P, Q, on_device=False) == want).all()


def test_device_pairing_bilinearity():
    a, b = 0x1234567, 0x7654321
    lhs = zv.pair(g1_points_from_scalars([a]), g2_points_from_scalars([b]))
    rhs = zv.pair(g1_points_from_scalars([a * b % ref.R]), g2_points_from_scalars([1]))
    assert (lhs == rhs).all()


def _golden():
    g = _load("bn254_golden.json")
    wire = {e["name"]: e for e in _load("groth16_wire_golden.json")}
    out = {}
    for e in g["groth16"]:
        name = e["name"].replace("_r0", "")
        out.setdefault(name, (wire[name]["vk_hex"], []))[1].append((bytes.fromhex(e["proof"]), mont_limbs([h2i(v) for v in e["w"][1:e["n_public"]]])))
    return out


def test_golden_proofs_in_batches():
    gold = _golden()
    names = sorted(gold)
    for name in names:
        vk, items = gold[name]
        proofs, pubs = [p for p, _ in items], np.stack([w for _, w in items])
        got = zv.groth16_verify_batch(proofs, vk, pubs)
        assert got.all() and (got == _host_verdicts(proofs, vk, pubs)).all()
        assert (zv.groth16_verify_batch(proofs, bytes.fromhex(vk), pubs) == got).all()   # hex and bytes keys
    # a proof under the other key (same number of public inputs: a reject, not an error)
    (vk0, it0), (vk1, it1) = gold[names[0]], gold[names[1]]
    if len(it0[0][1]) == len(it1[0][1]):
        got = zv.groth16_verify_batch([it0[0][0]], vk1, np.stack([it0[0][1]]))
        assert not got[0] and got[0] == _host_verdicts([it0[0][0]], vk1, [it0[0][1]])[0]


def test_chunk_boundary():
    """2^16 + 3 proofs (the golden proofs of one key, tiled): two chunks, the second one three proofs long, and a bad proof in the second chunk only --
    the first chunk is decided by its combined check, the second one proof by proof; every chunk decompresses its own G2 points in the same scratch"""
    vk, items = _golden()["seq_r1cs_13"]
    base, bpubs = [p for p, _ in items], np.stack([w for _, w in items])
    bad = bytearray(base[0])
    bad[96] ^= 0x40                                      # -Krs: still a valid encoding, a rejected proof
    distinct = base + [bytes(bad)]
    dpubs = np.concatenate([bpubs, bpubs[:1]])
    host = _host_verdicts(distinct, vk, dpubs)
    assert list(host) == [True] * len(base) + [False]
    n = (1 << 16) + 3
    idx = np.arange(n) % len(base)
    idx[(1 << 16) + 1] = len(base)
    ps = b"".join(distinct[i] for i in idx)
    ws = dpubs[idx]
    _lib.profile(True)
    _lib.profile_reset()
    try:
        got = zv.groth16_verify_batch(ps, vk, ws)
        prof = _lib.profile_read()
    finally:
        _lib.profile(False)
    assert (got == host[idx]).all()
    assert prof["vb_prep"][0] == 2 and prof["vb_single"][0] == 1 and prof["miller_loop"][0] == 3 and prof["fe_easy"][0] == 3
    assert (zv.groth16_verify_batch(ps, vk, ws) == got).all()


def _fresh(n_proofs, npub, seed):
    """n_proofs distinct proofs of one small random R1CS (256 constraints), each with its own witness and (r, s), made on the GPU."""
    g = ref.SplitMix64(seed)
    nc, n_in = 256, 24
    shape = [tuple(int(g.next() % n_in) for _ in range(4)) + (1 + int(g.next() % 7), 1 + int(g.next() % 7)) for _ in range(nc)]
    one = mont_limbs([1])[0]
    cons = []
    for j, (la, lb, ra, rb, c1, c2) in enumerate(shape):
        L = {la: mont_limbs([c1])[0]}
        L[lb] = mont_limbs([(c2 + (c1 if lb == la else 0)) % ref.R])[0]
        Rr = {ra: one}
        if rb != ra:
            Rr[rb] = one
        cons.append((L, Rr, {n_in + j: one}))
    r1 = zk.R1CS(npub, n_in + nc, cons)
    pk, vk = zk.setup(r1, mont_limbs(ref.rand_felts(seed + 1, 5)))
    vkb = pk.vk_write_to(vk)
    proofs, pubs = [], []
    for k in range(n_proofs):
        w = [1] + [g.felt() for _ in range(n_in - 1)]
        for (la, lb, ra, rb, c1, c2) in shape:
            w.append((c1 * w[la] + c2 * w[lb]) % ref.R * ((w[ra] + (w[rb] if rb != ra else 0)) % ref.R) % ref.R)
        wm = mont_limbs(w)
        r, s = mont_limbs([g.felt(), g.felt()])
        proofs.append(zk.prove_r1cs(r1, pk, wm, r, s))
        pubs.append(wm[1:npub])
    pk.free()
    r1.free()
    return vkb, proofs, np.stack(pubs)


def test_fresh_proofs_batched_then_tampered():
    vk, proofs, pubs = _fresh(257, 4, 0xF00D)
    assert len(set(proofs)) == 257
    _lib.profile(True)
    _lib.profile_reset()
    try:
        got = zv.groth16_verify_batch(proofs, vk, pubs)
        prof = _lib.profile_read()
    finally:
        _lib.profile(False)
    assert got.all()
    assert "vb_prep" in prof and "vb_single" not in prof        # the batched path alone decided
    # tampering, each at its own index
    proofs = list(proofs)
    pubs = pubs.copy()
    pubs[3][0] = mont_limbs([5])[0]                       # a wrong public input
    proofs[10] = proofs[11][:32] + proofs[10][32:]                              # Ar of another proof
    proofs[20] = proofs[20][:96] + proofs[21][96:]                              # Krs of another proof
    proofs[30] = bytes([proofs[30][0] & 0x3F]) + proofs[30][1:]                 # invalid G1 flags
    X = (2, 1)                                                                  # on the twist, outside the r-torsion
    y = pl.f2_sqrt(ref.f2_add(ref.f2_mul(ref.f2_sqr(X), X), ref.B_G2))
    proofs[40] = proofs[40][:32] + ref.g2_compress((X, y)) + proofs[40][96:]
    proofs[50] = ref.g1_compress(None) + proofs[50][32:]                        # Ar at infinity
    _lib.profile(True)
    _lib.profile_reset()
    try:
        got = zv.groth16_verify_batch(proofs, vk, pubs)
        prof = _lib.profile_read()
    finally:
        _lib.profile(False)
    assert "vb_single" in prof
    bad = {3, 10, 20, 30, 40, 50}
    assert [i for i in range(257) if not got[i]] == sorted(bad)
    assert (got == _host_verdicts(proofs, vk, pubs)).all()
    # determinism
    assert (zv.groth16_verify_batch(proofs, vk, pubs) == got).all()
    # n_proofs = 1 and 0, a wrong n_public
    for i in (0, 10, 30):
        assert zv.groth16_verify_batch([proofs[i]], vk, pubs[i:i + 1])[0] == _host_verdicts([proofs[i]], vk, pubs[i:i + 1])[0]
    assert len(zv.groth16_verify_batch([], vk, np.zeros((0, 3, 4), np.uint64))) == 0
    with pytest.raises(ValueError, match="invalid witness size"):
        zv.groth16_verify_batch(proofs[:2], vk, pubs[:2, :2])


def test_fresh_proofs_one_public_input_and_the_oracle():
    vk, proofs, pubs = _fresh(16, 2, 0xBEEF)
    proofs[5] = proofs[6][:32] + proofs[5][32:]
    got = zv.groth16_verify_batch(proofs, vk, pubs)
    assert (got == _host_verdicts(proofs, vk, pubs)).all() and got.sum() == 15 and not got[5]
    # the oracle's independent verifier decides one tampered and one valid proof the same way
    kb = bytes.fromhex(vk) if isinstance(vk, str) else bytes(vk)
    nk = int.from_bytes(kb[288:292], "big")
    ovk = dict(g1_alpha=pl.g1_decompress(kb[0:32]), g2_beta=pl.g2_decompress(kb[64:128]), g2_gamma=pl.g2_decompress(kb[128:192]),
               g2_delta=pl.g2_decompress(kb[224:288]), g1_ic=[pl.g1_decompress(kb[292 + 32 * i:324 + 32 * i]) for i in range(nk)])
    for i in (4, 5):
        p = proofs[i]
        proof = (pl.g1_decompress(p[:32]), pl.g2_decompress(p[32:96]), pl.g1_decompress(p[96:]))
        w = [1] + [int.from_bytes(np.asarray(x, dtype=np.uint64).tobytes(), "little") * pow(1 << 256, -1, ref.R) % ref.R for x in pubs[i]]
        assert ref.groth16_verify(ovk, proof, w) == bool(got[i])


def _plus_r(pubs):
    """the same public inputs as NON-canonical Montgomery images: each limb vector increased by r (value unchanged mod r, limbs >= r)"""
    out = pubs.copy()
    for idx in np.ndindex(pubs.shape[:-1]):
        v = int.from_bytes(np.asarray(pubs[idx], dtype=np.uint64).tobytes(), "little") + ref.R
        assert v < 1 << 256
        out[idx] = np.frombuffer(v.to_bytes(32, "little"), dtype=np.uint64)
    return out


def test_non_canonical_public_inputs_match_the_host_verifier():
    vk, proofs, pubs = _fresh(12, 4, 0xACE)
    wide = _plus_r(pubs)
    assert (wide != pubs).any()
    wide[7] = pubs[7]                                                            # a canonical one in the same batch
    wide[9][1] = mont_limbs([3])[0]                                              # a wrong value
    got = zv.groth16_verify_batch(proofs, vk, wide)
    assert (got == _host_verdicts(proofs, vk, wide)).all()
    assert (got == zv.groth16_verify_batch(proofs, vk, pubs) & (np.arange(12) != 9)).all()
