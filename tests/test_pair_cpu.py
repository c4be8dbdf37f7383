"""The pairing value entries (zk_bn254_pair_host here; zk_bn254_pair on the GPU: test_gpu_verify_batch.py): the host value against the oracle's
independent final_exp(prod miller_loop), bilinearity on values, agreement with zk_bn254_pairing_check, and the device entries' argument errors."""
import ctypes as C

import numpy as np
import pytest

from noir_backend_using_gnark_amd import _lib
from noir_backend_using_gnark_amd import verify as zv
from oracle import bn254_ref as ref

RINV = pow(1 << 256, -1, ref.Q)


def g1_img(P):
    return np.frombuffer(ref.g1_affine_mont_bytes(P), dtype=np.uint64)


def g2_img(P):
    return np.frombuffer(ref.g2_affine_mont_bytes(P), dtype=np.uint64)


def gt_to_flat(gt):
    """zk_gt (gnark's E12 order C0.B0, C0.B1, C0.B2, C1.B0, C1.B1, C1.B2; Montgomery) -> the oracle's w^12 - 18 w^6 + 82 basis: the w-basis
    coefficient c_i = a_i + b_i u (C0 = c0, c2, c4; C1 = c1, c3, c5) gives flat[i] = a_i - 9 b_i, flat[i + 6] = b_i, since u = w^6 - 9."""
    limbs = [int.from_bytes(np.asarray(gt[4 * k:4 * k + 4], dtype=np.uint64).tobytes(), "little") * RINV % ref.Q for k in range(12)]
    pos = [0, 2, 4, 1, 3, 5]
    flat = [0] * 12
    for k in range(6):
        a, b = limbs[2 * k], limbs[2 * k + 1]
        i = pos[k]
        flat[i] = (a - 9 * b) % ref.Q
        flat[i + 6] = b
    return flat


def oracle_pair(pairs):
    f = [1] + [0] * 11
    for P, Qp in pairs:
        f = ref._p12_mul(f, ref.miller_loop(Qp, P))
    return ref.final_exp(f)


def pair_host(pairs):
    return zv.pair([g1_img(p) for p, _ in pairs], [g2_img(q) for _, q in pairs], on_device=False)


def test_host_pairing_equals_the_oracle_value():
    """The exact reduced pairing value, pinned by the oracle's independent implementation (three pairings: the oracle is slow)."""
    G, H = ref.G1_GEN, ref.G2_GEN
    assert gt_to_flat(pair_host([(G, H)])) == oracle_pair([(G, H)])
    P, Qp = ref.g1_mul(G, 0x1234567890ABCDEF), ref.g2_mul(H, 0xFEDCBA987654321)
    assert gt_to_flat(pair_host([(P, H), (G, Qp)])) == oracle_pair([(P, H), (G, Qp)])


def test_host_pairing_values_are_bilinear():
    G, H = ref.G1_GEN, ref.G2_GEN
    one = pair_host([])
    assert gt_to_flat(one) == [1] + [0] * 11
    for a in (2, 7, 123456789123456789):
        assert (pair_host([(ref.g1_mul(G, a), H)]) == pair_host([(G, ref.g2_mul(H, a))])).all()
    P = ref.g1_mul(G, 99)
    assert (pair_host([(P, H), (ref.g1_neg(P), H)]) == one).all()
    assert not (pair_host([(G, H)]) == one).all()
    # infinity on either side contributes one
    assert (pair_host([(None, H), (G, H)]) == pair_host([(G, H)])).all()
    assert (pair_host([(G, None)]) == one).all()


def test_host_pairing_decisions_agree_with_pairing_check():
    G, H = ref.G1_GEN, ref.G2_GEN
    one = pair_host([])
    cases = [[(ref.g1_mul(G, 6), H), (ref.g1_neg(G), ref.g2_mul(H, 6))], [(ref.g1_mul(G, 6), H), (ref.g1_neg(G), ref.g2_mul(H, 5))], [(G, H)], []]
    for pairs in cases:
        ps, qs = [g1_img(p) for p, _ in pairs], [g2_img(q) for _, q in pairs]
        assert zv.pairing_check(ps, qs) == bool((pair_host(pairs) == one).all())


def test_new_symbols_exist():
    for s in ("zk_bn254_pair", "zk_bn254_pair_host", "zk_bn254_groth16_verify_batch"):
        assert s in _lib.SYMBOLS and hasattr(_lib.lib(), s)


def test_device_entries_without_gpu():
    if _lib.device_count() > 0:
        pytest.skip("a GPU is present")
    lib = _lib.lib()
    G, H = g1_img(ref.G1_GEN), g2_img(ref.G2_GEN)
    out = np.zeros(48, np.uint64)
    assert lib.zk_bn254_pair(None, None, C.c_size_t(1), _lib.vp(out)) == _lib.ZK_ERR_ARG
    assert lib.zk_bn254_pair(_lib.vp(G), _lib.vp(H), C.c_size_t(1), None) == _lib.ZK_ERR_ARG
    assert lib.zk_bn254_pair(_lib.vp(G), _lib.vp(H), C.c_size_t(1), _lib.vp(out)) == _lib.ZK_ERR_NO_DEVICE
    with pytest.raises(_lib.ZkmiError) as ei:
        zv.pair([G], [H])
    assert ei.value.code == _lib.ZK_ERR_NO_DEVICE
    # a toy verifying key with one K point (no public input)
    vk = (ref.g1_compress(ref.G1_GEN) * 2 + ref.g2_compress(ref.G2_GEN) * 2 + ref.g1_compress(ref.G1_GEN) + ref.g2_compress(ref.G2_GEN)
          + (1).to_bytes(4, "big") + ref.g1_compress(ref.G1_GEN))
    proof = ref.g1_compress(ref.G1_GEN) + ref.g2_compress(ref.G2_GEN) + ref.g1_compress(ref.G1_GEN)
    acc, n_acc = (C.c_uint8 * 2)(), C.c_size_t(7)
    vb = lib.zk_bn254_groth16_verify_batch
    assert vb(None, C.c_size_t(1), vk, C.c_size_t(len(vk)), 0, None, C.c_size_t(0), acc, C.byref(n_acc)) == _lib.ZK_ERR_ARG
    assert vb(proof, C.c_size_t(1), vk, C.c_size_t(len(vk)), 0, None, C.c_size_t(0), None, C.byref(n_acc)) == _lib.ZK_ERR_ARG
    pub = np.zeros((1, 4), np.uint64)
    with pytest.raises(ValueError, match="invalid witness size"):
        zv.groth16_verify_batch([proof], vk, pub.reshape(1, 1, 4))               # n_public + 1 != len(K)
    with pytest.raises(ValueError):
        zv.groth16_verify_batch([proof], vk[:-1], np.zeros((1, 0, 4), np.uint64))  # malformed key
    assert vb(proof, C.c_size_t(0), vk, C.c_size_t(len(vk)), 0, None, C.c_size_t(0), None, C.byref(n_acc)) == _lib.ZK_OK and n_acc.value == 0
    with pytest.raises(_lib.ZkmiError) as ei:
        zv.groth16_verify_batch([proof], vk, np.zeros((1, 0, 4), np.uint64))
    assert ei.value.code == _lib.ZK_ERR_NO_DEVICE
