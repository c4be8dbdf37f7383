"""The five Fiat-Shamir stages of the batch PLONK prover (csrc/plonk_batch.hip k_pb_transcript; zk_bn254_plonk_challenges_batch_dev) restated with hashlib
alone.  The messages are the single prover's (csrc/plonk.hip zk_bn254_plonk_prove, csrc/proofio.hpp FsTranscript and kzg_derive_gamma):
    0  gamma = H("gamma" || S1 S2 S3 Ql Qr Qm Qo Qk || public inputs || L R O)     1  beta = H("beta" || gamma's digest)
    2  alpha = H("alpha" || beta's digest || Z)                                    3  zeta = H("zeta" || alpha's digest || H0 H1 H2)
    4  kzg's folding gamma = H("gamma" || zeta || foldedH lin L R O S1 S2 || the seven claimed values), a transcript of its own
A point is an (x, y) pair of integers or None (infinity) and is bound as G1Affine.RawBytes(), a field element as 32 big-endian bytes; a challenge is its
digest read big-endian and reduced mod r.  tests/test_plonk_batch_cpu.py holds this against oracle/plonk_ref.py, so a device mismatch points at the device."""
import hashlib

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
NAMES = (b"gamma", b"beta", b"alpha", b"zeta", b"gamma")


def raw_point(p) -> bytes:
    return bytes([0x40]) + bytes(63) if p is None else p[0].to_bytes(32, "big") + p[1].to_bytes(32, "big")


def fr_bytes(x: int) -> bytes:
    return (x % R).to_bytes(32, "big")


def stage(k: int, key, *, public=(), points=(), prev=None, values=()):
    """-> (challenge, raw digest).  key: the verifying key's eight digests S1 S2 S3 Ql Qr Qm Qo Qk; prev: the previous stage's raw digest (stages 1 to 3) or
    zeta as an integer (stage 4); points: the stage's own (3, 0, 1, 3, 5); values: the eight of the proof, the first seven are bound (stage 4)"""
    h = hashlib.sha256(NAMES[k])
    if k == 0:
        for d in key:
            h.update(raw_point(d))
        for w in public:
            h.update(fr_bytes(w))
    else:
        h.update(fr_bytes(prev) if k == 4 else prev)
    for p in list(points) + ([key[0], key[1]] if k == 4 else []):
        h.update(raw_point(p))
    for v in list(values)[:7] if k == 4 else ():
        h.update(fr_bytes(v))
    d = h.digest()
    return int.from_bytes(d, "big") % R, d


def five(key, public, lro, z, hd, fh, lin, values):
    """the five challenges of a proof from its digests and values, in the prover's order"""
    gamma, d = stage(0, key, public=public, points=lro)
    beta, d = stage(1, key, prev=d)
    alpha, d = stage(2, key, prev=d, points=[z])
    zeta, d = stage(3, key, prev=d, points=hd)
    return gamma, beta, alpha, zeta, stage(4, key, prev=zeta, points=[fh, lin] + list(lro), values=values)[0]
