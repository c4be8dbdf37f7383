"""zk_bn254_plonk_verify_batch without a GPU: the symbol is declared and exported, key and witness-size errors come before any device work (with the host
verifier's messages), n_proofs = 0 is an empty result, and otherwise the call is ZK_ERR_NO_DEVICE -- there is no CPU fallback."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from noir_backend_using_gnark_amd import _lib
from noir_backend_using_gnark_amd import verify as zv
from oracle import bn254_ref as ref
from tests.helpers import h2i, mont_limbs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def g2_img(P):
    return np.frombuffer(ref.g2_affine_mont_bytes(P), dtype=np.uint64)


@pytest.fixture(scope="module")
def fixture():
    """the reference's first demo circuit (one public input): proof, key, srs_g2, public inputs"""
    with open(os.path.join(ROOT, "tests", "golden", "plonk_golden.json")) as f:
        e = json.load(f)[0]
    g2 = np.stack([g2_img(ref.G2_GEN), g2_img(ref.g2_mul(ref.G2_GEN, h2i(e["srs_alpha"])))])
    pub = mont_limbs([h2i(v) for v in e["solution"][:e["n_public"]]])
    assert e["n_public"] == 1
    return bytes.fromhex(e["proof"]), e["vk_hex"], g2, pub


def test_symbol_declared_and_exported():
    with open(os.path.join(ROOT, "include", "zkmi.h")) as f:
        hdr = f.read()
    assert re.search(r"\bint zk_bn254_plonk_verify_batch\(", hdr)
    assert "zk_bn254_plonk_verify_batch" in _lib.SYMBOLS
    assert hasattr(_lib.lib(), "zk_bn254_plonk_verify_batch")


def test_key_and_witness_errors(fixture):
    proof, vk, g2, pub = fixture
    with pytest.raises(ValueError, match="invalid hex text"):
        zv.plonk_verify_batch([proof], "zz" + vk[2:], g2, pub[None])
    with pytest.raises(ValueError, match="367 bytes, 368 expected"):
        zv.plonk_verify_batch([proof], bytes.fromhex(vk)[:-1], g2, pub[None])
    with pytest.raises(ValueError, match="invalid witness size, got 2, expected 1"):
        zv.plonk_verify_batch([proof], vk, g2, np.stack([pub, pub], axis=1))
    with pytest.raises(ValueError, match="invalid witness size, got 0, expected 1"):
        zv.plonk_verify_batch([proof], vk, g2, np.zeros((1, 0, 4), np.uint64))
    # the same messages as the host verifier
    for bad_vk in ("zz" + vk[2:], bytes.fromhex(vk)[:-1]):
        with pytest.raises(ValueError) as host:
            zv.plonk_verify(proof, bad_vk, g2, pub)
        with pytest.raises(ValueError) as batch:
            zv.plonk_verify_batch([proof], bad_vk, g2, pub[None])
        assert str(host.value) == str(batch.value)
    with pytest.raises(ValueError):
        zv.plonk_verify_batch(proof[:-1], vk, g2, pub[None])  # not a whole number of proofs


def test_no_proofs_is_an_empty_result(fixture):
    _, vk, g2, _ = fixture
    got = zv.plonk_verify_batch([], vk, g2, np.zeros((0, 1, 4), np.uint64))
    assert got.dtype == bool and len(got) == 0
    n_acc = C.c_size_t(7)
    rc = _lib.lib().zk_bn254_plonk_verify_batch(None, C.c_size_t(0), C.c_char_p(vk.encode()), C.c_size_t(len(vk)), C.c_int(1), _lib.vp(g2), None,
                                                 C.c_size_t(1), None, C.byref(n_acc))
    assert rc == _lib.ZK_OK and n_acc.value == 0


def test_device_entry_without_gpu(fixture):
    if _lib.device_count() > 0:
        pytest.skip("a GPU is present")
    proof, vk, g2, pub = fixture
    lib = _lib.lib()
    kb = bytes.fromhex(vk)
    acc, n_acc = (C.c_uint8 * 2)(), C.c_size_t(7)
    vb = lib.zk_bn254_plonk_verify_batch
    assert vb(None, C.c_size_t(1), kb, C.c_size_t(len(kb)), 0, _lib.vp(g2), _lib.vp(pub), C.c_size_t(1), acc, C.byref(n_acc)) == _lib.ZK_ERR_ARG
    assert vb(proof, C.c_size_t(1), kb, C.c_size_t(len(kb)), 0, None, _lib.vp(pub), C.c_size_t(1), acc, C.byref(n_acc)) == _lib.ZK_ERR_ARG
    assert vb(proof, C.c_size_t(1), kb, C.c_size_t(len(kb)), 0, _lib.vp(g2), _lib.vp(pub), C.c_size_t(1), None, C.byref(n_acc)) == _lib.ZK_ERR_ARG
    assert vb(proof, C.c_size_t(1), kb, C.c_size_t(len(kb)), 0, _lib.vp(g2), _lib.vp(pub), C.c_size_t(1), acc, C.byref(n_acc)) == _lib.ZK_ERR_NO_DEVICE
    with pytest.raises(_lib.ZkmiError) as ei:
        zv.plonk_verify_batch([proof], vk, g2, pub[None])
    assert ei.value.code == _lib.ZK_ERR_NO_DEVICE
