"""The coefficients of the device forms of the batch verifiers (include/zkmi.h: zk_bn254_groth16_verify_batch_dev / zk_bn254_plonk_verify_batch_dev), restated in
plain Python over a SHA-256 written out here (FIPS 180-4) -- nothing of the library under test, and hashlib only in the test that checks this file:
    d_v   = SHA-256(row v's proof bytes || row v's public inputs as they lie in memory: n_public x 32 bytes, the Montgomery images, little-endian limbs)
    D     = SHA-256(d_0 || .. || d_{n-1})
    r_i   = low128(SHA-256("zkmi-groth16-batch-rows" || SHA-256(vk) || D || u64 i LE)), forced non-zero
    rho_i, rho'_i = low128(SHA-256("zkmi-plonk-batch-rows" || SHA-256(vk) || SHA-256(srs_g2) || D || u64 i LE || 0 / 1)), forced non-zero
low128: the digest read as a big-endian integer, its low 128 bits."""
import numpy as np

_K = [
    0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be, 0x550c7dc3,
    0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da,
    0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, 0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13,
    0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070,
    0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208,
    0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2]
_IV = [0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19]
_M = 0xffffffff


def _rotr(x, n):
    return ((x >> n) | (x << (32 - n))) & _M


def sha256(msg: bytes) -> bytes:
    msg = bytes(msg)
    padded = msg + b"\x80" + b"\0" * ((55 - len(msg)) % 64) + (8 * len(msg)).to_bytes(8, "big")
    h = list(_IV)
    for off in range(0, len(padded), 64):
        w = [int.from_bytes(padded[off + 4 * i:off + 4 * i + 4], "big") for i in range(16)]
        for i in range(16, 64):
            s0 = _rotr(w[i - 15], 7) ^ _rotr(w[i - 15], 18) ^ (w[i - 15] >> 3)
            s1 = _rotr(w[i - 2], 17) ^ _rotr(w[i - 2], 19) ^ (w[i - 2] >> 10)
            w.append((w[i - 16] + s0 + w[i - 7] + s1) & _M)
        a, b, c, d, e, f, g, hh = h
        for i in range(64):
            t1 = (hh + (_rotr(e, 6) ^ _rotr(e, 11) ^ _rotr(e, 25)) + ((e & f) ^ (~e & g & _M)) + _K[i] + w[i]) & _M
            t2 = ((_rotr(a, 2) ^ _rotr(a, 13) ^ _rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c))) & _M
            a, b, c, d, e, f, g, hh = (t1 + t2) & _M, a, b, c, (d + t1) & _M, e, f, g
        h = [(x + y) & _M for x, y in zip(h, (a, b, c, d, e, f, g, hh))]
    return b"".join(x.to_bytes(4, "big") for x in h)


def pub_bytes(pub) -> bytes:
    """a row's public inputs ((n_public, 4) uint64 Montgomery limbs) as they lie in memory"""
    return np.ascontiguousarray(pub, dtype="<u8").tobytes()


def row_digests(proofs, pubs) -> list:
    """[d_v]: proofs a list of byte strings, pubs a list of (n_public, 4) limb arrays (or None: no public inputs)"""
    return [sha256(bytes(p) + (pub_bytes(pubs[v]) if pubs is not None else b"")) for v, p in enumerate(proofs)]


def data_digest(proofs, pubs) -> bytes:
    return sha256(b"".join(row_digests(proofs, pubs)))


def low128(digest: bytes) -> int:
    v = int.from_bytes(digest, "big") & ((1 << 128) - 1)
    return v or 1


def groth16_rows_coefficients(vk: bytes, proofs, pubs) -> list:
    """[r_i] for the n rows of one call"""
    pre = b"zkmi-groth16-batch-rows" + sha256(vk) + data_digest(proofs, pubs)
    return [low128(sha256(pre + i.to_bytes(8, "little"))) for i in range(len(proofs))]


def plonk_rows_coefficients(vk: bytes, srs_g2, proofs, pubs) -> list:
    """[(rho_i, rho'_i)] for the n rows of one call; srs_g2: the (2, 16) uint64 image of ([1]2, [alpha]2)"""
    g2 = np.ascontiguousarray(srs_g2, dtype="<u8").tobytes()
    assert len(g2) == 256
    pre = b"zkmi-plonk-batch-rows" + sha256(vk) + sha256(g2) + data_digest(proofs, pubs)
    return [tuple(low128(sha256(pre + i.to_bytes(8, "little") + bytes([tag]))) for tag in (0, 1)) for i in range(len(proofs))]
