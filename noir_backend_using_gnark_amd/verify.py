"""Host-side verifiers of libzkmi (no GPU needed): groth16.Verify, plonk.Verify and the pairing check they are built on -- the counterpart of the
reference's PlonkVerifyWithVK (gnark_backend_ffi/main.go:44-56) and the intended Groth16 VerifyWithVK (backend/groth16/r1cs.go:176-212).
Proofs and keys are gnark's wire images (Proof.WriteTo / VerifyingKey.WriteTo as bytes, or hex str); public inputs are Montgomery limbs (n, 4) uint64."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, lib, vp


def _blob(x):
    if isinstance(x, str):
        return x.encode("ascii"), 1
    return bytes(x), 0


def _call(fn, *args) -> bool:
    ok = C.c_int(0)
    rc = fn(*args, C.byref(ok))
    if rc in (_lib.ZK_ERR_LEN, _lib.ZK_ERR_ARG):
        raise ValueError((lib().zk_last_error() or b"").decode())
    check(rc)
    return bool(ok.value)


def groth16_verify(proof: bytes, vk, public_inputs) -> bool:
    """groth16.Verify(proof, vk, publicWitness); public_inputs WITHOUT the constant wire."""
    proof = bytes(proof)
    if len(proof) != 128:
        raise ValueError("a Groth16 proof is 128 bytes (Proof.WriteTo)")
    k, is_hex = _blob(vk)
    pub = np.ascontiguousarray(public_inputs, dtype=np.uint64).reshape(-1, 4)
    return _call(lib().zk_bn254_groth16_verify, C.c_char_p(proof), C.c_char_p(k), C.c_size_t(len(k)), C.c_int(is_hex), vp(pub) if len(pub) else None, C.c_size_t(len(pub)))


def plonk_verify(proof: bytes, vk, srs_g2, public_inputs) -> bool:
    """plonk.Verify(proof, vk, publicWitness) with vk.InitKZG(srs): srs_g2 = the SRS's two G2 points ((2, 16) uint64, kzg.SRS.g2)."""
    proof = bytes(proof)
    if len(proof) != _lib.PLONK_PROOF_BYTES:
        raise ValueError("a PLONK proof is %d bytes (Proof.WriteTo)" % _lib.PLONK_PROOF_BYTES)
    k, is_hex = _blob(vk)
    g2 = np.ascontiguousarray(srs_g2, dtype=np.uint64).reshape(2, 16)
    pub = np.ascontiguousarray(public_inputs, dtype=np.uint64).reshape(-1, 4)
    return _call(lib().zk_bn254_plonk_verify, C.c_char_p(proof), C.c_char_p(k), C.c_size_t(len(k)), C.c_int(is_hex), vp(g2), vp(pub) if len(pub) else None, C.c_size_t(len(pub)))


def pairing_check(g1_points, g2_points) -> bool:
    """prod_i e(P_i, Q_i) == 1 for affine Montgomery images ((n, 8) and (n, 16) uint64)."""
    p = np.ascontiguousarray(g1_points, dtype=np.uint64).reshape(-1, 8)
    q = np.ascontiguousarray(g2_points, dtype=np.uint64).reshape(-1, 16)
    if len(p) != len(q):
        raise ValueError("as many G1 as G2 points")
    return _call(lib().zk_bn254_pairing_check, vp(p) if len(p) else None, vp(q) if len(q) else None, C.c_size_t(len(p)))


def pair(g1_points, g2_points, on_device: bool = True) -> np.ndarray:
    """prod_i e(P_i, Q_i), the reduced optimal ate pairing, as bn254.GT's memory image ((48,) uint64: E12 C0.B0 .. C1.B2, Montgomery).
    on_device=False computes the same value on the host.  The value is exactly f^((q^12 - 1) / r) for the host Miller product f; it is not claimed to
    equal gnark-crypto's bn254.Pair value (a fixed power of it may differ), only products tested against one are comparable across libraries."""
    p = np.ascontiguousarray(g1_points, dtype=np.uint64).reshape(-1, 8)
    q = np.ascontiguousarray(g2_points, dtype=np.uint64).reshape(-1, 16)
    if len(p) != len(q):
        raise ValueError("as many G1 as G2 points")
    out = np.zeros(48, np.uint64)
    fn = lib().zk_bn254_pair if on_device else lib().zk_bn254_pair_host
    check(fn(vp(p) if len(p) else None, vp(q) if len(q) else None, C.c_size_t(len(p)), vp(out)))
    return out


def groth16_verify_batch(proofs, vk, public_inputs) -> np.ndarray:
    """groth16.Verify for many proofs against ONE verifying key, on the device: one verdict per proof, equal to groth16_verify's, except that a
    malformed proof encoding gives False instead of an error.  proofs: a sequence of 128-byte proofs (or their concatenation); public_inputs:
    (n_proofs, n_public, 4) Montgomery limbs, without the constant wire."""
    blob = bytes(proofs) if isinstance(proofs, (bytes, bytearray)) else b"".join(bytes(x) for x in proofs)
    if len(blob) % 128:
        raise ValueError("a Groth16 proof is 128 bytes (Proof.WriteTo)")
    n = len(blob) // 128
    k, is_hex = _blob(vk)
    pub = np.ascontiguousarray(public_inputs, dtype=np.uint64)
    if pub.size == 0:
        n_public = pub.shape[1] if pub.ndim == 3 and pub.shape[0] == n else 0
        pub = np.zeros((max(n, 1), max(n_public, 1), 4), np.uint64)
    else:
        pub = pub.reshape(n, -1, 4)
        n_public = pub.shape[1]
    acc = np.zeros(max(n, 1), np.uint8)
    n_acc = C.c_size_t(0)
    rc = lib().zk_bn254_groth16_verify_batch(C.c_char_p(blob), C.c_size_t(n), C.c_char_p(k), C.c_size_t(len(k)), C.c_int(is_hex),
                                             vp(pub) if n_public else None, C.c_size_t(n_public), vp(acc), C.byref(n_acc))
    if rc in (_lib.ZK_ERR_LEN, _lib.ZK_ERR_ARG):
        raise ValueError((lib().zk_last_error() or b"").decode())
    check(rc)
    return acc[:n].astype(bool)


def plonk_verify_batch(proofs, vk, srs_g2, public_inputs) -> np.ndarray:
    """plonk.Verify for many proofs against ONE verifying key, on the device: one verdict per proof, equal to plonk_verify's, except that a malformed
    proof (an invalid point encoding, a batched-opening count other than 7) gives False instead of an error.  proofs: a sequence of 548-byte proofs (or
    their concatenation); srs_g2: the SRS's two G2 points ((2, 16) uint64); public_inputs: (n_proofs, n_public, 4) Montgomery limbs."""
    pb = _lib.PLONK_PROOF_BYTES
    blob = bytes(proofs) if isinstance(proofs, (bytes, bytearray)) else b"".join(bytes(x) for x in proofs)
    if len(blob) % pb:
        raise ValueError("a PLONK proof is %d bytes (Proof.WriteTo)" % pb)
    n = len(blob) // pb
    k, is_hex = _blob(vk)
    g2 = np.ascontiguousarray(srs_g2, dtype=np.uint64).reshape(2, 16)
    pub = np.ascontiguousarray(public_inputs, dtype=np.uint64)
    if pub.size == 0:
        n_public = pub.shape[1] if pub.ndim == 3 and pub.shape[0] == n else 0
        pub = np.zeros((max(n, 1), max(n_public, 1), 4), np.uint64)
    else:
        pub = pub.reshape(n, -1, 4)
        n_public = pub.shape[1]
    acc = np.zeros(max(n, 1), np.uint8)
    n_acc = C.c_size_t(0)
    rc = lib().zk_bn254_plonk_verify_batch(C.c_char_p(blob), C.c_size_t(n), C.c_char_p(k), C.c_size_t(len(k)), C.c_int(is_hex), vp(g2),
                                           vp(pub) if n_public else None, C.c_size_t(n_public), vp(acc), C.byref(n_acc))
    if rc in (_lib.ZK_ERR_LEN, _lib.ZK_ERR_ARG):
        raise ValueError((lib().zk_last_error() or b"").decode())
    check(rc)
    return acc[:n].astype(bool)


def _keys_args(vks, key_of, n: int):
    """(key blobs kept alive, char*[n_keys], size_t[n_keys], n_keys, is_hex, key_of as contiguous uint32) of the many-key entries"""
    blobs = [_blob(k) for k in vks]
    if len({h for _, h in blobs}) > 1:
        raise ValueError("the keys are all bytes or all hex text")
    raw = [b for b, _ in blobs]
    ptrs = (C.c_char_p * max(len(raw), 1))(*raw)
    lens = (C.c_size_t * max(len(raw), 1))(*[len(b) for b in raw])
    ko = np.asarray(key_of)
    if ko.shape != (n,) or (n and (ko.min() < 0 or ko.max() >= 1 << 32)):
        raise ValueError("key_of holds one key index per proof")
    return raw, ptrs, lens, len(raw), blobs[0][1] if blobs else 0, np.ascontiguousarray(ko, dtype=np.uint32)


def plonk_verify_batch_keys(proofs, vks, key_of, srs_g2, public_inputs) -> np.ndarray:
    """plonk_verify_batch against MANY verifying keys of one SRS in one device call (zk_bn254_plonk_verify_batch_keys): proof i is verified against
    vks[key_of[i]], all openings of all keys in one two-pairing check.  vks: a sequence of keys (all bytes or all hex str); key_of: n_proofs key indices;
    public_inputs: (n_proofs, pub_stride, 4) Montgomery limbs, of which row i's first n_public(key_of[i]) elements are read, or a list of per-row arrays of
    each row's own length, which is padded here.  The verdicts are plonk_verify's per row, a malformed proof being False instead of an error."""
    pb = _lib.PLONK_PROOF_BYTES
    blob = bytes(proofs) if isinstance(proofs, (bytes, bytearray)) else b"".join(bytes(x) for x in proofs)
    if len(blob) % pb:
        raise ValueError("a PLONK proof is %d bytes (Proof.WriteTo)" % pb)
    n = len(blob) // pb
    raw, ptrs, lens, n_keys, is_hex, ko = _keys_args(vks, key_of, n)
    g2 = np.ascontiguousarray(srs_g2, dtype=np.uint64).reshape(2, 16)
    if isinstance(public_inputs, (list, tuple)):
        rows = [np.ascontiguousarray(r, dtype=np.uint64).reshape(-1, 4) for r in public_inputs]
        if len(rows) != n:
            raise ValueError("one row of public inputs per proof")
        pub = np.zeros((n, max([len(r) for r in rows] + [0]), 4), np.uint64)
        for i, r in enumerate(rows):
            pub[i, :len(r)] = r
    else:
        pub = np.ascontiguousarray(public_inputs, dtype=np.uint64)
        pub = pub.reshape(n, -1, 4) if pub.size else np.zeros((n, 0, 4), np.uint64)
    stride = pub.shape[1]
    acc = np.zeros(max(n, 1), np.uint8)
    n_acc = C.c_size_t(0)
    rc = lib().zk_bn254_plonk_verify_batch_keys(blob, n, ptrs, lens, n_keys, is_hex, vp(g2), vp(ko) if n else None, vp(pub) if pub.size else None, stride,
                                                vp(acc), C.addressof(n_acc))
    return _verdicts(rc, acc, n)


def plonk_verify_batch_keys_dev(d_proofs, proof_stride: int, n_proofs: int, vks, key_of, srs_g2, d_public_inputs, pub_stride: int) -> np.ndarray:
    """plonk_verify_batch_keys for rows that already lie in HBM (zk_bn254_plonk_verify_batch_keys_dev): proof v is the 548 bytes at d_proofs + v * proof_stride,
    its public inputs the first n_public(key_of[v]) Montgomery elements at element v * pub_stride of d_public_inputs (None when no key has any); vks and key_of
    are host data."""
    raw, ptrs, lens, n_keys, is_hex, ko = _keys_args(vks, key_of, n_proofs)
    g2 = np.ascontiguousarray(srs_g2, dtype=np.uint64).reshape(2, 16)
    p, q = _dev_rows(d_proofs, d_public_inputs, None)
    acc = np.zeros(max(n_proofs, 1), np.uint8)
    n_acc = C.c_size_t(0)
    rc = lib().zk_bn254_plonk_verify_batch_keys_dev(p, proof_stride, n_proofs, ptrs, lens, n_keys, is_hex, vp(g2), vp(ko) if n_proofs else None, q or None,
                                                    pub_stride, vp(acc), C.addressof(n_acc))
    return _verdicts(rc, acc, n_proofs)


def _padded_rows(public_inputs, n: int) -> np.ndarray:
    """(n, pub_stride, 4) uint64 of the many-key entries: an array as it is, or per-row arrays of each row's own length padded to the longest"""
    if isinstance(public_inputs, (list, tuple)):
        rows = [np.ascontiguousarray(r, dtype=np.uint64).reshape(-1, 4) for r in public_inputs]
        if len(rows) != n:
            raise ValueError("one row of public inputs per proof")
        pub = np.zeros((n, max([len(r) for r in rows] + [0]), 4), np.uint64)
        for i, r in enumerate(rows):
            pub[i, :len(r)] = r
        return pub
    pub = np.ascontiguousarray(public_inputs, dtype=np.uint64)
    return pub.reshape(n, -1, 4) if pub.size else np.zeros((n, 0, 4), np.uint64)


def groth16_verify_batch_keys(proofs, vks, key_of, public_inputs) -> np.ndarray:
    """groth16_verify_batch against MANY verifying keys in one device call (zk_bn254_groth16_verify_batch_keys): proof i is verified against
    vks[key_of[i]], every key's pairings in one product with one final exponentiation.  vks: a sequence of keys (all bytes or all hex str); key_of: n_proofs
    key indices; public_inputs: (n_proofs, pub_stride, 4) Montgomery limbs, of which row i's first n_public(key_of[i]) elements are read, or a list of per-row
    arrays of each row's own length, which is padded here.  The verdicts are groth16_verify's per row, a malformed proof being False instead of an error."""
    blob = bytes(proofs) if isinstance(proofs, (bytes, bytearray)) else b"".join(bytes(x) for x in proofs)
    if len(blob) % 128:
        raise ValueError("a Groth16 proof is 128 bytes (Proof.WriteTo)")
    n = len(blob) // 128
    raw, ptrs, lens, n_keys, is_hex, ko = _keys_args(vks, key_of, n)
    pub = _padded_rows(public_inputs, n)
    acc = np.zeros(max(n, 1), np.uint8)
    n_acc = C.c_size_t(0)
    rc = lib().zk_bn254_groth16_verify_batch_keys(blob, n, ptrs, lens, n_keys, is_hex, vp(ko) if n else None, vp(pub) if pub.size else None, pub.shape[1],
                                                  vp(acc), C.addressof(n_acc))
    return _verdicts(rc, acc, n)


def groth16_verify_batch_keys_dev(d_proofs, proof_stride: int, n_proofs: int, vks, key_of, d_public_inputs, pub_stride: int) -> np.ndarray:
    """groth16_verify_batch_keys for rows that already lie in HBM (zk_bn254_groth16_verify_batch_keys_dev): proof v is the 128 bytes at
    d_proofs + v * proof_stride, its public inputs the first n_public(key_of[v]) Montgomery elements at element v * pub_stride of d_public_inputs (None when
    no key has any); vks and key_of are host data."""
    raw, ptrs, lens, n_keys, is_hex, ko = _keys_args(vks, key_of, n_proofs)
    p, q = _dev_rows(d_proofs, d_public_inputs, None)
    acc = np.zeros(max(n_proofs, 1), np.uint8)
    n_acc = C.c_size_t(0)
    rc = lib().zk_bn254_groth16_verify_batch_keys_dev(p, proof_stride, n_proofs, ptrs, lens, n_keys, is_hex, vp(ko) if n_proofs else None, q or None,
                                                      pub_stride, vp(acc), C.addressof(n_acc))
    return _verdicts(rc, acc, n_proofs)


def _dev_rows(proofs, public_inputs, n_public: int | None):
    """(device pointer or DeviceBuffer, rows) pair of arguments of the device forms -> raw pointers (0 for no public inputs)"""
    p = proofs.ptr if isinstance(proofs, _lib.DeviceBuffer) else int(proofs)
    if public_inputs is None or n_public == 0:
        return p, 0
    return p, public_inputs.ptr if isinstance(public_inputs, _lib.DeviceBuffer) else int(public_inputs)


def _verdicts(rc: int, acc: np.ndarray, n: int) -> np.ndarray:
    if rc in (_lib.ZK_ERR_LEN, _lib.ZK_ERR_ARG):
        raise ValueError((lib().zk_last_error() or b"").decode())
    check(rc)
    return acc[:n].astype(bool)


def groth16_verify_batch_dev(d_proofs, proof_stride: int, n_proofs: int, vk, d_public_inputs, pub_stride: int, n_public: int) -> np.ndarray:
    """groth16_verify_batch for rows that already lie in HBM (zk_bn254_groth16_verify_batch_dev): proof v is the 128 bytes at d_proofs + v * proof_stride,
    its public inputs the n_public Montgomery elements at element v * pub_stride of d_public_inputs (DeviceBuffer or raw device pointers).  The verdicts are
    groth16_verify_batch's for the same bytes; the coefficients come from one SHA-256 per row computed on the device."""
    k, is_hex = _blob(vk)
    p, q = _dev_rows(d_proofs, d_public_inputs, n_public)
    acc = np.zeros(max(n_proofs, 1), np.uint8)
    n_acc = C.c_size_t(0)
    rc = lib().zk_bn254_groth16_verify_batch_dev(p, proof_stride, n_proofs, k, len(k), is_hex, q, pub_stride, n_public, vp(acc), C.addressof(n_acc))
    return _verdicts(rc, acc, n_proofs)


def plonk_verify_batch_dev(d_proofs, proof_stride: int, n_proofs: int, vk, srs_g2, d_public_inputs, pub_stride: int, n_public: int) -> np.ndarray:
    """plonk_verify_batch for rows that already lie in HBM (zk_bn254_plonk_verify_batch_dev): proof v is the 548 bytes at d_proofs + v * proof_stride, its
    public inputs the n_public Montgomery elements at element v * pub_stride of d_public_inputs.  srs_g2 as in plonk_verify_batch."""
    k, is_hex = _blob(vk)
    g2 = np.ascontiguousarray(srs_g2, dtype=np.uint64).reshape(2, 16)
    p, q = _dev_rows(d_proofs, d_public_inputs, n_public)
    acc = np.zeros(max(n_proofs, 1), np.uint8)
    n_acc = C.c_size_t(0)
    rc = lib().zk_bn254_plonk_verify_batch_dev(p, proof_stride, n_proofs, k, len(k), is_hex, vp(g2), q, pub_stride, n_public, vp(acc), C.addressof(n_acc))
    return _verdicts(rc, acc, n_proofs)
