"""Batch PLONK verification on the device (zk_bn254_plonk_verify_batch) against the host verifier zk_bn254_plonk_verify, which test_verify_cpu.py pins
to the oracle: the reference's fixtures with their tampers, many fresh proofs under one key, a mixed batch that takes the per-proof fallback, coefficients
that must differ between proofs, and a chunk boundary."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from noir_backend_using_gnark_amd import _lib
from noir_backend_using_gnark_amd import kzg
from noir_backend_using_gnark_amd import plonk as zp
from noir_backend_using_gnark_amd import verify as zv
from oracle import bn254_ref as ref
from oracle import plonk_ref as pl
from tests.helpers import h2i, mont_limbs

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
R = ref.R
M = pl.ints_to_mont_np


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    _lib.require_device()


def g2_img(P):
    return np.frombuffer(ref.g2_affine_mont_bytes(P), dtype=np.uint64)


def _host(proofs, vk, g2, pubs):
    """the host verifier's verdicts; an error (a malformed proof) counts as a reject"""
    out = []
    for p, w in zip(proofs, pubs):
        try:
            out.append(zv.plonk_verify(p, vk, g2, w))
        except ValueError:
            out.append(False)
    return np.array(out, dtype=bool)


def _batch(proofs, vk, g2, pubs):
    _lib.profile(True)
    _lib.profile_reset()
    try:
        got = zv.plonk_verify_batch(proofs, vk, g2, pubs)
        prof = _lib.profile_read()
    finally:
        _lib.profile(False)
    return got, prof


def _with(proof, off, b):
    return proof[:off] + b + proof[off + len(b):]


def _flip(proof, off):
    return _with(proof, off, bytes([proof[off] ^ 1]))


def test_reference_fixtures_and_their_tampers():
    with open(os.path.join(HERE, "golden", "plonk_golden.json")) as f:
        gold = json.load(f)
    for e in gold:
        alpha = h2i(e["srs_alpha"])
        g2 = np.stack([g2_img(ref.G2_GEN), g2_img(ref.g2_mul(ref.G2_GEN, alpha))])
        g2_other = np.stack([g2[0], g2_img(ref.g2_mul(ref.G2_GEN, alpha + 1))])
        proof = bytes.fromhex(e["proof"])
        pub_i = [h2i(v) for v in e["solution"][:e["n_public"]]]
        pub = mont_limbs(pub_i) if pub_i else np.zeros((0, 4), np.uint64)
        vk = e["vk_hex"]
        assert list(zv.plonk_verify_batch([proof], vk, g2, pub[None])) == [True], e["name"]
        assert list(zv.plonk_verify_batch([proof], bytes.fromhex(vk), g2, pub[None])) == [True]
        other = ref.g1_compress(ref.g1_mul(ref.G1_GEN, 9))
        cases = [(_flip(proof, 260 + 31), pub), (_flip(proof, 547), pub), (_with(proof, 96, other), pub),
                 (bytes.fromhex(e["proof_pinned"]), pub), (_with(proof, 256, b"\0\0\0\x08"), pub)]
        if pub_i:
            cases.append((proof, mont_limbs([(pub_i[0] + 1) % R] + pub_i[1:])))
        for p, w in cases:
            want = _host([p], vk, g2, [w])
            assert not want[0]
            assert list(zv.plonk_verify_batch([p], vk, g2, w[None])) == [False], e["name"]
        assert list(zv.plonk_verify_batch([proof], vk, g2_other, pub[None])) == [False]
        assert not zv.plonk_verify(proof, vk, g2_other, pub)
        # all of them in one batch, around the valid proof
        ps = [proof] + [p for p, _ in cases] + [proof]
        ws = np.stack([pub] + [w for _, w in cases] + [pub]) if pub_i else np.zeros((len(ps), 0, 4), np.uint64)
        got = zv.plonk_verify_batch(ps, vk, g2, ws)
        assert (got == _host(ps, vk, g2, ws)).all() and got[0] and got[-1] and got.sum() == 2


class Key:
    """a circuit with free public inputs: per public input p_j the gate p_j + s_j - t_j = 0 (s_j, t_j secret), and the gates a + b - c = 0,
    c + b - d = 0, d + a - e = 0 of secrets (n_public = 0 has gates too; the domain has at least 4 rows); the key from kzg.new_srs (known alpha) + plonk.setup"""

    def __init__(self, npub, seed):
        self.npub, self.g = npub, ref.SplitMix64(seed)
        nv, a = 3 * npub + 5, 3 * npub
        xa = [j for j in range(npub)] + [a, a + 2, a + 3]
        xb = [npub + j for j in range(npub)] + [a + 1, a + 1, a]
        xc = [2 * npub + j for j in range(npub)] + [a + 2, a + 3, a + 4]
        nc = npub + 3
        circ = zp.Circuit(npub, nv, M([1] * nc), M([1] * nc), M([R - 1] * nc), M([0] * nc), M([0] * nc), xa, xb, xc)
        n = 1
        while n < nc + npub:
            n <<= 1
        self.alpha = self.g.felt()
        self.srs = kzg.new_srs(n + 3, M([self.alpha])[0])
        self.pk = zp.setup(circ, self.srs.g1)
        self.vk = self.pk.write()[:368]
        self.g2 = np.ascontiguousarray(self.srs.g2, dtype=np.uint64).reshape(2, 16)

    def proof(self):
        g = self.g
        p = [g.felt() for _ in range(self.npub)]
        s = [g.felt() for _ in range(self.npub)]
        a, b = g.felt(), g.felt()
        sol = p + s + [(x + y) % R for x, y in zip(p, s)] + [a, b, (a + b) % R, (a + 2 * b) % R, (2 * a + 2 * b) % R]
        pr = zp.prove(self.pk, M(sol), M([g.felt() for _ in range(9)]))
        return pr, (M(p) if p else np.zeros((0, 4), np.uint64))

    def proofs(self, k):
        items = [self.proof() for _ in range(k)]
        return [p for p, _ in items], np.stack([w for _, w in items])

    def free(self):
        self.pk.free()
        self.srs.free()


@pytest.fixture(scope="module")
def keys():
    ks = {npub: Key(npub, 0x5EED + npub) for npub in (0, 1, 3)}
    yield ks
    for k in ks.values():
        k.free()


def test_one_key_many_proofs(keys):
    for npub, key in keys.items():
        m = 1000 if npub == 3 else 64
        proofs, pubs = key.proofs(m)
        assert len(set(proofs)) == m
        assert _host(proofs[:4], key.vk, key.g2, pubs[:4]).all()
        for n in (1, 2, 64, 1000):
            idx = [i % m for i in range(n)]
            ps, ws = [proofs[i] for i in idx], pubs[idx]
            got, prof = _batch(ps, key.vk, key.g2, ws)
            assert got.all() and len(got) == n, (npub, n)
            assert "pv_kzg" in prof and "pv_single" not in prof  # the batched check alone decided
        acc, n_acc = np.zeros(2, np.uint8), C.c_size_t(0)
        blob = b"".join(proofs[:2])
        w = np.ascontiguousarray(pubs[:2]) if npub else None
        rc = _lib.lib().zk_bn254_plonk_verify_batch(C.c_char_p(blob), C.c_size_t(2), C.c_char_p(key.vk), C.c_size_t(368), C.c_int(0), _lib.vp(key.g2),
                                                     _lib.vp(w) if npub else None, C.c_size_t(npub), _lib.vp(acc), C.byref(n_acc))
        assert rc == _lib.ZK_OK and n_acc.value == 2 and list(acc) == [1, 1]


def _x_is_q():
    """a compressed G1 encoding with x = q (x >= q)"""
    b = bytearray(ref.Q.to_bytes(32, "big"))
    b[0] |= 0x80
    return bytes(b)


def test_mixed_batch_matches_the_host(keys):
    key = keys[3]
    proofs, pubs = key.proofs(256)
    proofs, pubs = list(proofs), pubs.copy()
    other = ref.g1_compress(ref.g1_mul(ref.G1_GEN, 7))
    proofs[5] = _flip(proofs[5], 260 + 2 * 32 + 31)                                # a claimed value (l(zeta))
    pubs[17][1] = mont_limbs([5])[0]                                               # a wrong public input
    pubs[[30, 31]] = pubs[[31, 30]]                                                # two rows swapped
    proofs[44] = _with(proofs[44], 0, _x_is_q())            # x >= q
    proofs[60] = _with(proofs[60], 128, bytes([proofs[60][128] & 0x3F]))           # invalid flag bits (H0)
    proofs[77] = _with(proofs[77], 224, other)                                     # BatchH: only the folded opening is wrong
    proofs[91] = _with(proofs[91], 484, other)                                     # ZShiftH: only the shifted opening is wrong
    proofs[103] = _flip(proofs[103], 516 + 31)                                     # zu: the quotient identity rejects
    v = int.from_bytes(proofs[150][260 + 32:260 + 64], "big") + R                  # a claimed value + r: reduced, accepted
    proofs[150] = _with(proofs[150], 260 + 32, v.to_bytes(32, "big"))
    proofs[200] = _with(proofs[200], 256, b"\0\0\0\x08")                           # a count of 8
    want = _host(proofs, key.vk, key.g2, pubs)
    assert [i for i in range(256) if not want[i]] == [5, 17, 30, 31, 44, 60, 77, 91, 103, 200]
    got, prof = _batch(proofs, key.vk, key.g2, pubs)
    assert "pv_single" in prof
    assert (got == want).all(), [i for i in range(256) if got[i] != want[i]]
    assert (zv.plonk_verify_batch(proofs, key.vk, key.g2, pubs) == got).all()


POINT_SLOTS = [("L", 0), ("R", 32), ("O", 64), ("Z", 96), ("H0", 128), ("H1", 160), ("H2", 192), ("BatchH", 224), ("ZShiftH", 484)]


def test_every_point_slot_with_every_refused_encoding(keys):
    """every refused G1 encoding of the codec tables, the point at infinity and four other points, in each of the nine point slots, untouched proofs
    between them.  A refused encoding gives 0 whatever else holds (the reference decoder says so, not the host verifier); the rest gets the host's verdict"""
    from tests import codec_edges as ce
    key = keys[1]
    base, bpubs = key.proofs(8)
    vectors = [(lab, b, kind) for lab, b, kind in ce.g1_decompress_vectors() if kind in ("invalid", "inf")]
    vectors += [v for v in ce.g1_decompress_vectors() if v[2] == "valid"][3:42:11]
    assert sum(kind == "invalid" for _, _, kind in vectors) >= 59 and sum(kind == "valid" for _, _, kind in vectors) == 4
    for _, b, kind in vectors:
        if kind == "invalid":
            with pytest.raises(ValueError):
                pl.g1_decompress(b)
    ps, ws, labels, kinds = [], [], [], []
    for slot, off in POINT_SLOTS:
        for lab, b, kind in vectors:
            j = len(ps) % 8
            if len(ps) % 5 == 0:
                ps.append(base[j]), ws.append(bpubs[j]), labels.append("untouched"), kinds.append("untouched")
            ps.append(_with(base[j], off, b)), ws.append(bpubs[j]), labels.append("%s <- %s" % (slot, lab)), kinds.append(kind)
    ws = np.stack(ws)
    want = _host(ps, key.vk, key.g2, ws)
    got, prof = _batch(ps, key.vk, key.g2, ws)
    assert "pv_single" in prof
    for i, (lab, kind) in enumerate(zip(labels, kinds)):
        if kind == "untouched":
            assert got[i] and want[i], (i, lab)
        elif kind == "invalid":
            assert not got[i], (i, lab)
        assert got[i] == want[i], (i, lab, kind)
    assert (zv.plonk_verify_batch(ps, key.vk, key.g2, ws) == got).all()


def test_coefficients_are_independent(keys):
    """ZShiftH + P in one copy of a proof and ZShiftH - P in another: no transcript binds that point, so equal coefficients would cancel the errors"""
    key = keys[1]
    proof, w = key.proof()
    ws = pl.g1_decompress(proof[484:516])
    P = ref.g1_mul(ref.G1_GEN, 0xC0FFEE)
    a = _with(proof, 484, ref.g1_compress(ref.g1_add(ws, P)))
    b = _with(proof, 484, ref.g1_compress(ref.g1_add(ws, ref.g1_neg(P))))
    ps, pubs = [proof, a, b, proof], np.stack([w] * 4)
    want = _host(ps, key.vk, key.g2, pubs)
    assert list(want) == [True, False, False, True]
    assert list(zv.plonk_verify_batch(ps, key.vk, key.g2, pubs)) == list(want)
    assert list(zv.plonk_verify_batch(ps[1:3], key.vk, key.g2, pubs[1:3])) == [False, False]


def test_chunk_boundary(keys):
    key = keys[1]
    base, bpubs = key.proofs(5)
    bad = _with(base[2], 484, ref.g1_compress(ref.g1_mul(ref.G1_GEN, 3)))
    distinct = list(base) + [bad]
    dpubs = np.concatenate([bpubs, bpubs[2:3]])
    host = _host(distinct, key.vk, key.g2, dpubs)
    assert list(host) == [True] * 5 + [False]
    n = (1 << 16) + 3
    idx = np.arange(n) % 5
    idx[(1 << 16) + 1] = 5  # the bad proof only in the second chunk
    ps = b"".join(distinct[i] for i in idx)
    ws = dpubs[idx]
    got = zv.plonk_verify_batch(ps, key.vk, key.g2, ws)
    assert (got == host[idx]).all()
    assert (zv.plonk_verify_batch(ps, key.vk, key.g2, ws) == got).all()


def test_non_canonical_public_inputs_match_the_host(keys):
    """public inputs given as Montgomery images increased by r (limbs >= r, the same value): the device verdicts equal the host verifier's, proof by proof"""
    key = keys[3]
    proofs, pubs = key.proofs(16)
    wide = pubs.copy()
    for i in range(16):
        for j in range(3):
            v = int.from_bytes(np.asarray(pubs[i][j], dtype=np.uint64).tobytes(), "little") + R
            assert v < 1 << 256
            wide[i][j] = np.frombuffer(v.to_bytes(32, "little"), dtype=np.uint64)
    wide[4] = pubs[4]                                                              # a canonical row in the same batch
    wide[11][2] = mont_limbs([5])[0]                                               # a wrong value
    want = _host(proofs, key.vk, key.g2, wide)
    got = zv.plonk_verify_batch(proofs, key.vk, key.g2, wide)
    assert (got == want).all(), [i for i in range(16) if got[i] != want[i]]
    assert (got == zv.plonk_verify_batch(proofs, key.vk, key.g2, pubs) & (np.arange(16) != 11)).all()
