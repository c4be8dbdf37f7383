"""KZG openings without a GPU: the new entries are declared and exported and zkmi.hpp's mirror compiles; the host verifiers zk_bn254_kzg_verify /
_fold_proof / _batch_verify_single_point against openings computed by the oracle (oracle/plonk_ref.py: poly_eval, divide_by_x_minus_a, kzg_derive_gamma,
_kzg_check) over kzg_new_srs(64, alpha); the golden PLONK proofs cut into their two openings; the device entries' argument errors and ZK_ERR_NO_DEVICE."""
import ctypes as C
import json
import os
import random
import re
import subprocess

import numpy as np
import pytest

from noir_backend_using_gnark_amd import _lib, kzg
from noir_backend_using_gnark_amd import verify as zv
from oracle import bn254_ref as ref
from oracle import plonk_ref as pl
from tests.helpers import from_mont_limbs, h2i, mont_limbs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = ref.R
ALPHA = 0x1f3a5c7e9b2d4f60718293a4b5c6d7e8f9010203040506070809aabbccddeeff % R
NEW = ("zk_bn254_kzg_open", "zk_bn254_kzg_batch_open_single_point", "zk_bn254_kzg_verify", "zk_bn254_kzg_fold_proof",
       "zk_bn254_kzg_batch_verify_single_point", "zk_bn254_kzg_verify_batch")


def g1_img(P):
    return np.frombuffer(ref.g1_affine_mont_bytes(P), dtype=np.uint64).copy()


def g2_img(P):
    return np.frombuffer(ref.g2_affine_mont_bytes(P), dtype=np.uint64)


def fr_img(x):
    return mont_limbs([x])[0]


@pytest.fixture(scope="module")
def srs():
    s = pl.kzg_new_srs(64, ALPHA)
    s["g2_img"] = np.stack([g2_img(s["g2"][0]), g2_img(s["g2"][1])])
    return s


def commit(srs, p):
    return ref.msm_naive(pl.FP, srs["g1"][:len(p)], list(p)) if p else None


def oracle_open(srs, p, z):
    v = pl.poly_eval(p, z)
    return commit(srs, pl.divide_by_x_minus_a(p, v, z)), v


def rand_poly(rng, n):
    return [rng.randrange(R) for _ in range(n)]


def poly_with_root(rng, n, root):
    """(X - root) * q, n coefficients (n >= 2)"""
    q = rand_poly(rng, n - 1)
    p = [0] * n
    for i, c in enumerate(q):
        p[i] = (p[i] - root * c) % R
        p[i + 1] = (p[i + 1] + c) % R
    return p


def test_symbols_declared_and_exported():
    with open(os.path.join(ROOT, "include", "zkmi.h")) as f:
        hdr = f.read()
    lib = _lib.lib()
    for s in NEW:
        assert re.search(r"\bint %s\(" % s, hdr), s
        assert s in _lib.SYMBOLS and hasattr(lib, s), s
    assert "zk_kzg_opening" in hdr and "SHA-256 ONLY" in hdr


def test_cpp_mirror_compiles(tmp_path):
    src = tmp_path / "kzg_mirror.cpp"
    src.write_text("""
#include "zkmi.hpp"
using namespace zkmi;
int main(int argc, char**) {
    kzg::SRS srs;
    fr::Vector p(4), points(2);
    fr::Element z = {};
    kzg::OpeningProof o = {};
    kzg::BatchOpeningProof b;
    kzg::Digest d = {};
    std::vector<kzg::Digest> ds(2);
    std::vector<kzg::OpeningProof> os(2);
    std::vector<uint8_t> acc;
    if (argc > 100) {  // compiled and linked, never run
        Error e = kzg::Open(p, z, srs, &o);
        e = kzg::BatchOpenSinglePoint({p, p}, ds, z, srs, &b);
        e = kzg::FoldProof(ds, b, z, &o, &d);
        e = kzg::Verify(d, o, z, srs);
        e = kzg::BatchVerifySinglePoint(ds, b, z, srs);
        e = kzg::BatchVerifyMultiPoints(ds, os, points, srs, &acc);
        return e.code;
    }
    return 0;
}
""")
    pkg = os.path.join(ROOT, "noir_backend_using_gnark_amd")
    exe = tmp_path / "kzg_mirror"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + pkg, "-lzkmi", "-Wl,-rpath," + pkg,
                           "-o", str(exe)])
    assert subprocess.call([str(exe)]) == 0


LENGTHS = (1, 2, 33, 64)


def _points(rng, p):
    pts = [0, 1, R - 1, rng.randrange(R)]
    return pts


def test_verify_accepts_true_openings_and_rejects_every_single_replacement(srs):
    rng = random.Random(11)
    g2 = srs["g2_img"]
    other_g2 = g2_img(ref.g2_mul(ref.G2_GEN, 7))
    checked_by_pairing = 0
    for n in LENGTHS:
        cases = [(rand_poly(rng, n), z) for z in _points(rng, None)]
        if n >= 2:
            root = rng.randrange(R)
            cases.append((poly_with_root(rng, n, root), root))
        else:
            cases.append(([0], rng.randrange(R)))  # the zero constant: every point is a root
        for p, z in cases:
            Cd = commit(srs, p)
            H, v = oracle_open(srs, p, z)
            if n == 1:
                assert H is None and v == p[0]
            if n >= 2 and z not in (0, 1, R - 1) and pl.poly_eval(p, z) == 0:
                assert v == 0
            d, h, vv, zz = g1_img(Cd), g1_img(H), fr_img(v), fr_img(z)
            assert kzg.verify(d, h, vv, zz, g2), (n, z)
            # another valid value in each position
            assert not kzg.verify(g1_img(ref.g1_add(Cd, ref.G1_GEN)), h, vv, zz, g2)
            assert not kzg.verify(d, g1_img(ref.g1_add(H, ref.G1_GEN)), vv, zz, g2)
            assert not kzg.verify(d, h, fr_img((v + 1) % R), zz, g2)
            if n >= 2:  # (a constant's true opening is C - v G = infinity with H = infinity: it holds at every point and under every G2 pair)
                assert not kzg.verify(d, h, vv, fr_img((z + 1) % R), g2)
                assert not kzg.verify(d, h, vv, zz, np.stack([g2[0], other_g2]))
                assert not kzg.verify(d, h, vv, zz, np.stack([other_g2, g2[1]]))
            if checked_by_pairing < 3 and n in (2, 33):  # the library's verdicts are the oracle's pairing check's
                assert pl._kzg_check(Cd, H, v, z, srs["g2"])
                assert not pl._kzg_check(Cd, H, (v + 1) % R, z, srs["g2"])
                checked_by_pairing += 1


def test_fold_proof_and_batch_verify_single_point(srs):
    rng = random.Random(12)
    g2 = srs["g2_img"]
    for z in (0, 1, R - 1, rng.randrange(R)):
        polys = [rand_poly(rng, n) for n in LENGTHS]
        polys.append(poly_with_root(rng, 33, z))
        digests = [commit(srs, p) for p in polys]
        claimed = [pl.poly_eval(p, z) for p in polys]
        assert claimed[-1] == 0
        kg = pl.kzg_derive_gamma(z, digests, claimed)
        folded = [0] * 64
        fd, fe, acc = None, 0, 1
        for p, d, v in zip(polys, digests, claimed):
            for j, c in enumerate(p):
                folded[j] = (folded[j] + c * acc) % R
            fd = ref.g1_add(fd, ref.g1_mul(d, acc))
            fe = (fe + v * acc) % R
            acc = acc * kg % R
        H = commit(srs, pl.divide_by_x_minus_a(folded, fe, z))
        D, V, h, zz = np.stack([g1_img(d) for d in digests]), mont_limbs(claimed), g1_img(H), fr_img(z)
        (oh, ov), od = kzg.fold_proof(D, h, V, zz)
        assert oh.tobytes() == h.tobytes() and from_mont_limbs(ov) == [fe] and od.tobytes() == g1_img(fd).tobytes()
        assert kzg.verify(od, oh, ov, zz, g2)
        assert kzg.batch_verify_single_point(D, h, V, zz, g2)
        for k in (0, len(polys) - 1):
            bad = V.copy()
            bad[k] = fr_img((claimed[k] + 1) % R)
            assert not kzg.batch_verify_single_point(D, h, bad, zz, g2)
            bad = D.copy()
            bad[k] = g1_img(ref.g1_add(digests[k], ref.G1_GEN))
            assert not kzg.batch_verify_single_point(bad, h, V, zz, g2)
        assert not kzg.batch_verify_single_point(D, g1_img(ref.g1_add(H, ref.G1_GEN)), V, zz, g2)
        assert not kzg.batch_verify_single_point(D, h, V, fr_img((z + 1) % R), g2)
        assert not kzg.batch_verify_single_point(D, h, V, zz, np.stack([g2[0], g2_img(ref.g2_mul(ref.G2_GEN, 7))]))
        assert not kzg.batch_verify_single_point(D, h, V, zz, np.stack([g2_img(ref.g2_mul(ref.G2_GEN, 7)), g2[1]]))
    lib = _lib.lib()
    ok = C.c_int(5)
    assert lib.zk_bn254_kzg_batch_verify_single_point(_lib.vp(D), C.c_size_t(0), _lib.vp(h), _lib.vp(V), _lib.vp(zz), _lib.vp(g2), C.byref(ok)) == _lib.ZK_ERR_ARG
    assert lib.zk_bn254_kzg_verify(None, _lib.vp(np.zeros(12, np.uint64)), _lib.vp(zz), _lib.vp(g2), C.byref(ok)) == _lib.ZK_ERR_ARG


def golden_openings(e):
    """a golden proof cut into its BatchedProof and ZShiftedOpening, with the seven digests rebuilt as plonk_ref.plonk_verify does"""
    b = bytes.fromhex(e["proof"])
    pts = [pl.g1_decompress(b[32 * k:32 * k + 32]) for k in range(7)]
    proof = dict(lro=pts[:3], z=pts[3], h=pts[4:7], batch_h=pl.g1_decompress(b[224:256]),
                 claimed=[int.from_bytes(b[260 + 32 * k:292 + 32 * k], "big") for k in range(7)], z_open_h=pl.g1_decompress(b[484:516]),
                 zu=int.from_bytes(b[516:548], "big"))
    assert b[256:260] == (7).to_bytes(4, "big") and pl.plonk_proof_bytes(proof) == b
    P = lambda h: pl.g1_from_np(np.frombuffer(bytes.fromhex(h), dtype=np.uint64))
    vkb = bytes.fromhex(e["vk_hex"])
    n, npub = int.from_bytes(vkb[:8], "big"), int.from_bytes(vkb[72:80], "big")
    vk = dict(size=n, size_inv=int.from_bytes(vkb[8:40], "big"), generator=int.from_bytes(vkb[40:72], "big"), n_public=npub,
              coset_shift=int.from_bytes(vkb[80:112], "big"), s=[P(p) for p in e["vk"]["s"]], **{k: P(e["vk"][k]) for k in ("ql", "qr", "qm", "qo", "qk")})
    pub = [h2i(v) for v in e["solution"][:npub]]
    fs = pl.Transcript("gamma", "beta", "alpha", "zeta")
    pl._bind_public_data(fs, vk, pub)
    gamma = fs.challenge_fr("gamma", *proof["lro"])
    beta = fs.challenge_fr("beta")
    alpha = fs.challenge_fr("alpha", proof["z"])
    zeta = fs.challenge_fr("zeta", *proof["h"])
    u = vk["coset_shift"]
    zz = (pow(zeta, n, R) - 1) % R
    l1 = zz * vk["size_inv"] % R * pl.inv((zeta - 1) % R, R) % R
    _, _, lz, rz, oz, s1z, s2z = proof["claimed"]
    zu = proof["zu"]
    zp = pow(zeta, n + 2, R)
    folded_h = ref.g1_add(ref.g1_mul(ref.g1_add(ref.g1_mul(proof["h"][2], zp), proof["h"][1]), zp), proof["h"][0])
    c_s3 = (lz + beta * s1z + gamma) * (rz + beta * s2z + gamma) % R * zu % R * beta % R * alpha % R
    c_z = ((-(lz + beta * zeta + gamma) * (rz + beta * u % R * zeta + gamma) % R * (oz + beta * u * u % R * zeta + gamma)) % R * alpha + alpha * alpha % R * l1) % R
    lin = ref.msm_naive(pl.FP, [vk["ql"], vk["qr"], vk["qm"], vk["qo"], vk["qk"], vk["s"][2], proof["z"]], [lz, rz, lz * rz % R, oz, 1, c_s3, c_z])
    digests = [folded_h, lin, *proof["lro"], vk["s"][0], vk["s"][1]]
    return proof, digests, zeta, zeta * vk["generator"] % R, pub


def test_golden_plonk_proofs_are_two_kzg_openings():
    with open(os.path.join(ROOT, "tests", "golden", "plonk_golden.json")) as f:
        golden = json.load(f)
    for e in golden:
        proof, digests, zeta, zeta_sh, pub = golden_openings(e)
        g2 = np.stack([g2_img(ref.G2_GEN), g2_img(ref.g2_mul(ref.G2_GEN, h2i(e["srs_alpha"])))])
        D, V = np.stack([g1_img(d) for d in digests]), mont_limbs(proof["claimed"])
        assert kzg.batch_verify_single_point(D, g1_img(proof["batch_h"]), V, fr_img(zeta), g2)
        assert kzg.verify(g1_img(proof["z"]), g1_img(proof["z_open_h"]), fr_img(proof["zu"]), fr_img(zeta_sh), g2)
        assert not kzg.verify(g1_img(proof["z"]), g1_img(proof["z_open_h"]), fr_img(proof["zu"]), fr_img(zeta), g2)
        # the PLONK verifier, which now goes through the same two functions, says what it said
        pubm = mont_limbs(pub) if pub else np.zeros((0, 4), np.uint64)
        assert zv.plonk_verify(bytes.fromhex(e["proof"]), e["vk_hex"], g2, pubm) is True
        bad = bytearray(bytes.fromhex(e["proof"]))
        bad[547] ^= 1  # z(omega zeta)
        assert zv.plonk_verify(bytes(bad), e["vk_hex"], g2, pubm) is False
        bad = bytearray(bytes.fromhex(e["proof"]))
        bad[260 + 32 * 3 + 31] ^= 1  # r(zeta)
        assert zv.plonk_verify(bytes(bad), e["vk_hex"], g2, pubm) is False


def test_device_entries_argument_errors_then_no_device():
    lib = _lib.lib()
    p = mont_limbs([1, 2, 3])
    polys, lens, z = (C.c_void_p * 1)(p.ctypes.data), (C.c_size_t * 1)(3), fr_img(5)
    out, d, h, claimed = np.zeros(12, np.uint64), np.zeros(8, np.uint64), np.zeros(8, np.uint64), np.zeros(4, np.uint64)
    vp, n0, n1 = _lib.vp, C.c_size_t(0), C.c_size_t(1)
    op, bo = lib.zk_bn254_kzg_open, lib.zk_bn254_kzg_batch_open_single_point
    bogus = C.c_uint64(0x00ffffffffffff)  # no such handle
    assert op(bogus, polys, lens, vp(z), n0, 0, vp(out)) == _lib.ZK_ERR_ARG
    assert op(bogus, None, lens, vp(z), n1, 0, vp(out)) == _lib.ZK_ERR_ARG
    assert op(bogus, polys, None, vp(z), n1, 0, vp(out)) == _lib.ZK_ERR_ARG
    assert op(bogus, polys, lens, None, n1, 0, vp(out)) == _lib.ZK_ERR_ARG
    assert op(bogus, polys, lens, vp(z), n1, 0, None) == _lib.ZK_ERR_ARG
    assert op(bogus, (C.c_void_p * 1)(None), lens, vp(z), n1, 0, vp(out)) == _lib.ZK_ERR_ARG
    assert op(bogus, polys, (C.c_size_t * 1)(0), vp(z), n1, 0, vp(out)) == _lib.ZK_ERR_LEN
    assert b"kzg: invalid polynomial size (larger than SRS or == 0)" in lib.zk_last_error()
    assert bo(bogus, polys, lens, vp(d), n0, vp(z), 0, vp(h), vp(claimed)) == _lib.ZK_ERR_ARG
    assert bo(bogus, polys, lens, None, n1, vp(z), 0, vp(h), vp(claimed)) == _lib.ZK_ERR_ARG
    assert bo(bogus, polys, lens, vp(d), n1, None, 0, vp(h), vp(claimed)) == _lib.ZK_ERR_ARG
    assert bo(bogus, polys, lens, vp(d), n1, vp(z), 0, None, vp(claimed)) == _lib.ZK_ERR_ARG
    assert bo(bogus, polys, (C.c_size_t * 1)(0), vp(d), n1, vp(z), 0, vp(h), vp(claimed)) == _lib.ZK_ERR_LEN
    g2 = np.stack([g2_img(ref.G2_GEN), g2_img(ref.G2_GEN)])
    acc, n_acc = np.zeros(1, np.uint8), C.c_size_t(9)
    vb = lib.zk_bn254_kzg_verify_batch
    assert vb(None, vp(out), vp(z), n1, vp(g2), vp(acc), C.byref(n_acc)) == _lib.ZK_ERR_ARG
    assert vb(vp(d), vp(out), vp(z), n1, None, vp(acc), C.byref(n_acc)) == _lib.ZK_ERR_ARG
    assert vb(vp(d), vp(out), vp(z), n1, vp(g2), None, C.byref(n_acc)) == _lib.ZK_ERR_ARG
    assert vb(vp(d), vp(out), vp(z), n1, vp(g2), vp(acc), None) == _lib.ZK_ERR_ARG
    assert vb(None, None, None, n0, vp(g2), None, C.byref(n_acc)) == _lib.ZK_OK and n_acc.value == 0
    # with well-formed arguments: no device -> ZK_ERR_NO_DEVICE (no CPU fallback); with one, the unknown handle is what is wrong
    want = _lib.ZK_ERR_NO_DEVICE if _lib.device_count() <= 0 else _lib.ZK_ERR_HANDLE
    assert op(bogus, polys, lens, vp(z), n1, 0, vp(out)) == want
    assert bo(bogus, polys, lens, vp(d), n1, vp(z), 0, vp(h), vp(claimed)) == want
    if _lib.device_count() <= 0:
        assert vb(vp(d), vp(out), vp(z), n1, vp(g2), vp(acc), C.byref(n_acc)) == _lib.ZK_ERR_NO_DEVICE
