"""CPU suite for the verifying side of the export path: the device forms of the batch verifiers, the rows' digests, the text-row decoders and the two
zk_*_verify_batch_with_vk entries.  The symbols are there with their signatures, every argument error is decided without a device, without a GPU the
entries answer ZK_ERR_NO_DEVICE only after validation, and tests/verify_rows_ref.py (the rows coefficient derivation in plain Python) agrees with hashlib."""
import ctypes as C
import hashlib
import os
import re

import numpy as np
import pytest

from noir_backend_using_gnark_amd import _lib
from tests import groth16_forge as gf
from tests import plonk_forge as pf
from tests import verify_rows_ref as vr
from tools import synth_acir as sa
from tools import synth_raw_r1cs as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("zk_bn254_groth16_verify_batch_dev", "zk_bn254_plonk_verify_batch_dev", "zk_bn254_rows_sha256_dev", "zk_bn254_bytes_decode_hex_rows_dev",
       "zk_bn254_felts_public_hex_rows_dev", "zk_plonk_verify_batch_with_vk", "zk_groth16_verify_batch_with_vk")
ARG, LEN, OK = _lib.ZK_ERR_ARG, _lib.ZK_ERR_LEN, _lib.ZK_OK


def _after_validation():
    """what a well-formed call returns here: the work's result with a GPU, ZK_ERR_NO_DEVICE without one"""
    return (OK,) if _lib.device_count() > 0 else (_lib.ZK_ERR_NO_DEVICE,)


def test_symbols_are_exported_with_signatures():
    lib = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "zkmi.h")).read()
    for s in NEW:
        assert s in _lib.SYMBOLS and hasattr(lib, s), s
        assert getattr(lib, s).argtypes == _lib.ARGTYPES[s]
        decl = re.search(r"\bint %s\s*\(([^;]*)\);" % s, hdr)
        assert decl, s
        assert len(decl.group(1).split(",")) == len(_lib.ARGTYPES[s]), s   # as many parameters as the header declares
    from noir_backend_using_gnark_amd import bn254, frontend, verify, wire
    for mod, name in ((verify, "groth16_verify_batch_dev"), (verify, "plonk_verify_batch_dev"), (wire, "decode_hex_bytes_rows"), (wire, "decode_public_rows"),
                      (bn254, "rows_sha256"), (frontend, "plonk_verify_batch_with_vk"), (frontend, "groth16_verify_batch_with_vk")):
        assert callable(getattr(mod, name)), name


def test_the_new_row_status_is_appended_to_the_enum():
    """ZK_ROW_BAD_PROOF_HEX follows ZK_ROW_BAD_COUNT = 4 without a value of its own: five, by the rule of C's enumerations"""
    hdr = open(os.path.join(ROOT, "include", "zkmi.h")).read()
    body = re.search(r"enum \{\s*(ZK_ROW_OK[^}]*)\}", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    value, got = -1, {}
    for item in (x.strip() for x in body.split(",") if x.strip()):
        name, _, v = (p.strip() for p in item.partition("="))
        value = int(v) if v else value + 1
        got[name] = value
    assert got == {"ZK_ROW_OK": 0, "ZK_ROW_UNSATISFIED": 1, "ZK_ROW_BAD_HEX": 2, "ZK_ROW_NOT_CANONICAL": 3, "ZK_ROW_BAD_COUNT": 4, "ZK_ROW_BAD_PROOF_HEX": 5}
    assert _lib.ROW_BAD_PROOF_HEX == 5


# ------------------------------------------------------------------------------------------------ the export-path entries
def _plonk(acir, proofs, pstride, text, vlen, vstride, rows, vk, g2, acc, status, n_acc, chunk_rows=0):
    return _lib.lib().zk_plonk_verify_batch_with_vk(acir, len(acir) if acir else 0, 0, proofs, pstride, text, vlen, vstride, rows, vk, len(vk) if vk else 0, g2, chunk_rows,
                                                    acc, status, n_acc)


def _g16(raw, proofs, pstride, text, vlen, vstride, rows, vk, g2, acc, status, n_acc, chunk_rows=0):
    return _lib.lib().zk_groth16_verify_batch_with_vk(raw, len(raw) if raw else 0, proofs, pstride, text, vlen, vstride, rows, vk, len(vk) if vk else 0, chunk_rows, acc,
                                                      status, n_acc)


def test_export_entries_decide_their_argument_errors_before_a_device_is_looked_for():
    """Every case returns its code whether or not a GPU is present; the well-formed call at the end gets past all of them (ZK_ERR_NO_DEVICE without a GPU)."""
    acir, w = sa.synth(8, 2)
    raw, w2 = sr.synth(8, 2)
    row = sa.felts_wire_hex(w).encode()
    row2 = sr.felts_wire_hex(w2).encode()
    assert len(row) == len(row2)
    vlen = len(row)
    g2 = np.ascontiguousarray(pf.n_public_key(2).g2, dtype=np.uint64)
    acc = np.full(2, 0xEE, np.uint8)
    status = np.full(2, 77, np.int32)
    n_acc = C.c_size_t(12345)
    a, s, n = acc.ctypes.data, status.ctypes.data, C.addressof(n_acc)
    for call, circuit, text, width, vk, vk_other in ((_plonk, acir.encode(), row * 2, 1096, pf.n_public_key(2).bytes.hex().encode(), pf.n_public_key(1).bytes.hex().encode()),
                                                     (_g16, raw.encode(), row2 * 2, 256, gf.key(2).bytes.hex().encode(), gf.key(0).bytes.hex().encode())):
        g = g2.ctypes.data
        proofs = b"0" * (2 * width)
        # a null pointer: the circuit, the proofs, the values, the key, the verdicts, the statuses, the count
        assert call(None, proofs, width, text, vlen, vlen, 2, vk, g, a, s, n) == ARG
        assert call(circuit, None, width, text, vlen, vlen, 2, vk, g, a, s, n) == ARG
        assert call(circuit, proofs, width, None, vlen, vlen, 2, vk, g, a, s, n) == ARG
        assert call(circuit, proofs, width, text, vlen, vlen, 2, None, g, a, s, n) == ARG
        assert call(circuit, proofs, width, text, vlen, vlen, 2, vk, g, None, s, n) == ARG
        assert call(circuit, proofs, width, text, vlen, vlen, 2, vk, g, a, None, n) == ARG
        assert call(circuit, proofs, width, text, vlen, vlen, 2, vk, g, a, s, None) == ARG
        if call is _plonk:
            assert call(circuit, proofs, width, text, vlen, vlen, 2, vk, None, a, s, n) == ARG
        # rows a stride apart that is shorter than a row (one row's stride may be anything: those calls get as far as the length check)
        assert call(circuit, proofs, width, text, vlen, vlen - 1, 2, vk, g, a, s, n) == ARG
        assert call(circuit, proofs, width - 1, text, vlen, vlen, 2, vk, g, a, s, n) == ARG
        assert call(circuit, proofs, 0, text, vlen - 64, 0, 1, vk, g, a, s, n) == LEN
        # values_len that is not 8 + 64 * (row 0's count)
        assert call(circuit, proofs, width, text, vlen - 64, vlen, 2, vk, g, a, s, n) == LEN
        assert call(circuit, proofs, width, text, vlen + 64, vlen + 64, 1, vk, g, a, s, n) == LEN
        assert call(circuit, proofs, width, b"0000000g" + text[8:], vlen, vlen, 2, vk, g, a, s, n) == ARG   # no count at all
        # a malformed key, and the key of a circuit with another number of public inputs: upstream's message
        assert call(circuit, proofs, width, text, vlen, vlen, 2, b"zz" + vk[2:], g, a, s, n) == ARG
        assert call(circuit, proofs, width, text, vlen, vlen, 2, vk[:-2], g, a, s, n) in (ARG, LEN)
        assert call(circuit, proofs, width, text, vlen, vlen, 2, vk_other, g, a, s, n) == LEN
        assert b"invalid witness size" in _lib.lib().zk_last_error()
        # no rows: nothing to do, nothing written (not even looked at: the length is wrong)
        assert call(circuit, proofs, 0, text, 5, 0, 0, vk, g, a, s, n) == OK
        assert (acc == 0xEE).all() and (status == 77).all() and n_acc.value == 12345
        # everything in order: only now is a device looked for
        assert call(circuit, proofs, width, text, vlen, vlen, 2, vk, g, a, s, n) in _after_validation()
        if _lib.device_count() <= 0:
            assert (acc == 0xEE).all() and (status == 77).all() and n_acc.value == 12345
        else:                                   # rows of '0' are no proofs: decoded, verified, rejected
            assert (acc == 0).all() and (status == 0).all() and n_acc.value == 0
            acc[:], status[:], n_acc.value = 0xEE, 77, 12345


# ------------------------------------------------------------------------------------------------ the device forms and the codecs
def test_device_forms_decide_their_argument_errors_before_a_device_is_looked_for():
    lib = _lib.lib()
    acc = np.full(2, 0xEE, np.uint8)
    n_acc = C.c_size_t(7)
    a, n = acc.ctypes.data, C.addressof(n_acc)
    d = 4096                                    # stands for a device address: no call below gets as far as reading it
    kp, kg = pf.n_public_key(2), gf.key(2)
    g2 = np.ascontiguousarray(kp.g2, dtype=np.uint64).ctypes.data
    P, G = lib.zk_bn254_plonk_verify_batch_dev, lib.zk_bn254_groth16_verify_batch_dev
    assert P(None, 548, 2, kp.bytes, len(kp.bytes), 0, g2, d, 2, 2, a, n) == ARG
    assert P(d, 548, 2, None, 0, 0, g2, d, 2, 2, a, n) == ARG
    assert P(d, 548, 2, kp.bytes, len(kp.bytes), 0, None, d, 2, 2, a, n) == ARG
    assert P(d, 548, 2, kp.bytes, len(kp.bytes), 0, g2, None, 2, 2, a, n) == ARG
    assert P(d, 548, 2, kp.bytes, len(kp.bytes), 0, g2, d, 2, 2, None, n) == ARG
    assert P(d, 548, 2, kp.bytes, len(kp.bytes), 0, g2, d, 2, 2, a, None) == ARG
    assert P(d, 547, 2, kp.bytes, len(kp.bytes), 0, g2, d, 2, 2, a, n) == ARG            # proof_stride below a proof
    assert P(d, 548, 2, kp.bytes, len(kp.bytes), 0, g2, d, 1, 2, a, n) == ARG            # pub_stride below a row
    assert P(d, 548, 2, kp.bytes[:-1], len(kp.bytes) - 1, 0, g2, d, 2, 2, a, n) in (ARG, LEN)
    assert P(d, 548, 2, kp.bytes, len(kp.bytes), 0, g2, d, 3, 3, a, n) == LEN and b"invalid witness size, got 3, expected 2" in lib.zk_last_error()
    assert P(None, 0, 0, kp.bytes, len(kp.bytes), 0, g2, None, 0, 2, None, n) == OK and n_acc.value == 0
    if _lib.device_count() <= 0:                 # (with a GPU the well-formed call would read the made-up address: tests/test_gpu_verify_dev.py has real rows)
        assert P(d, 548, 2, kp.bytes, len(kp.bytes), 0, g2, d, 2, 2, a, n) == _lib.ZK_ERR_NO_DEVICE
        assert (acc == 0xEE).all()
    n_acc.value = 7
    assert G(None, 128, 2, kg.bytes, len(kg.bytes), 0, d, 2, 2, a, n) == ARG
    assert G(d, 128, 2, None, 0, 0, d, 2, 2, a, n) == ARG
    assert G(d, 128, 2, kg.bytes, len(kg.bytes), 0, None, 2, 2, a, n) == ARG
    assert G(d, 128, 2, kg.bytes, len(kg.bytes), 0, d, 2, 2, None, n) == ARG
    assert G(d, 128, 2, kg.bytes, len(kg.bytes), 0, d, 2, 2, a, None) == ARG
    assert G(d, 127, 2, kg.bytes, len(kg.bytes), 0, d, 2, 2, a, n) == ARG
    assert G(d, 128, 2, kg.bytes, len(kg.bytes), 0, d, 1, 2, a, n) == ARG
    assert G(d, 128, 2, kg.bytes, len(kg.bytes), 0, d, 1, 1, a, n) == LEN and b"invalid witness size, got 1, expected 2" in lib.zk_last_error()
    assert G(None, 0, 0, kg.bytes, len(kg.bytes), 0, None, 0, 2, None, n) == OK and n_acc.value == 0
    if _lib.device_count() <= 0:
        assert G(d, 128, 2, kg.bytes, len(kg.bytes), 0, d, 2, 2, a, n) == _lib.ZK_ERR_NO_DEVICE
        assert (acc == 0xEE).all()


def test_codec_entries_decide_their_argument_errors_before_a_device_is_looked_for():
    lib = _lib.lib()
    d = 4096
    sha, dec, pub = lib.zk_bn254_rows_sha256_dev, lib.zk_bn254_bytes_decode_hex_rows_dev, lib.zk_bn254_felts_public_hex_rows_dev
    assert sha(None, 4, 4, d, 4, 4, 2, d, None) == ARG
    assert sha(d, 4, 4, None, 4, 4, 2, d, None) == ARG
    assert sha(d, 4, 4, d, 4, 4, 2, None, None) == ARG
    assert sha(d, 4, 3, d, 4, 4, 2, d, None) == ARG and sha(d, 4, 4, d, 4, 3, 2, d, None) == ARG
    assert sha(d, 4, 4, d, 4, 4, 0, d, None) == OK
    assert sha(None, 0, 0, None, 0, 0, 0, None, None) == OK
    assert dec(None, 256, 2, 128, d, 128, d, None) == ARG
    assert dec(d, 256, 2, 128, None, 128, d, None) == ARG
    assert dec(d, 256, 2, 128, d, 128, None, None) == ARG
    assert dec(d, 255, 2, 128, d, 128, d, None) == ARG                # pitch below a row
    assert dec(d, 256, 2, 128, d, 127, d, None) == ARG                # out_stride below a row
    assert dec(d, 256, 65536, 128, d, 128, d, None) == ARG            # the row is a grid dimension
    assert dec(d, 256, 0, 128, d, 128, d, None) == OK
    assert pub(None, 8 + 64 * 3, 2, 3, d, 1, d, 1, d, None) == ARG
    assert pub(d, 8 + 64 * 3, 2, 3, None, 1, d, 1, d, None) == ARG
    assert pub(d, 8 + 64 * 3, 2, 3, d, 1, None, 1, d, None) == ARG
    assert pub(d, 8 + 64 * 3, 2, 3, d, 1, d, 1, None, None) == ARG
    assert pub(d, 7 + 64 * 3, 2, 3, d, 1, d, 1, d, None) == ARG        # pitch below a row
    assert pub(d, 8 + 64 * 3, 2, 3, d, 2, d, 1, d, None) == ARG        # pub_stride below the public inputs
    assert pub(d, 8 + 64 * 3, 65536, 3, d, 1, d, 1, d, None) == ARG
    assert pub(d, 8 + 64 * 3, 0, 3, d, 1, d, 1, d, None) == OK
    if _lib.device_count() <= 0:
        assert sha(d, 4, 4, d, 4, 4, 2, d, None) == _lib.ZK_ERR_NO_DEVICE
        assert dec(d, 256, 2, 128, d, 128, d, None) == _lib.ZK_ERR_NO_DEVICE
        assert pub(d, 8 + 64 * 3, 2, 3, d, 1, d, 1, d, None) == _lib.ZK_ERR_NO_DEVICE


# ------------------------------------------------------------------------------------------------ the derivation's restatement
def test_reference_sha256_matches_hashlib_at_the_padding_edges():
    for n in (0, 1, 55, 56, 63, 64, 65, 119, 120, 128, 548, 644):
        msg = bytes((7 * i + n) & 0xFF for i in range(n))
        assert vr.sha256(msg) == hashlib.sha256(msg).digest(), n


def test_rows_coefficients_on_a_fixed_vector():
    """three rows of a fixed pattern: the restatement against the same composition over hashlib, and against digests written down when this file was made"""
    H = lambda b: hashlib.sha256(b).digest()
    vk = bytes(range(200))
    g2 = np.arange(32, dtype=np.uint64).reshape(2, 16) * np.uint64(0x0101010101010101)
    proofs = [bytes((i * 3 + v) & 0xFF for i in range(548)) for v in range(3)]
    pubs = [np.arange(8, dtype=np.uint64).reshape(2, 4) + np.uint64(v << 40) for v in range(3)]
    d = [H(proofs[v] + pubs[v].astype("<u8").tobytes()) for v in range(3)]
    assert vr.row_digests(proofs, pubs) == d
    D = H(b"".join(d))
    assert vr.data_digest(proofs, pubs) == D
    assert D.hex() == FIXED["D"]
    low = lambda dg: (int.from_bytes(dg, "big") & ((1 << 128) - 1)) or 1
    want = [(low(H(b"zkmi-plonk-batch-rows" + H(vk) + H(g2.tobytes()) + D + i.to_bytes(8, "little") + b"\0")),
             low(H(b"zkmi-plonk-batch-rows" + H(vk) + H(g2.tobytes()) + D + i.to_bytes(8, "little") + b"\1"))) for i in range(3)]
    assert vr.plonk_rows_coefficients(vk, g2, proofs, pubs) == want
    assert ["%032x" % x for x in want[2]] == FIXED["plonk row 2"]
    g16 = [p[:128] for p in proofs]
    D16 = H(b"".join(H(g16[v] + pubs[v].tobytes()) for v in range(3)))
    want16 = [low(H(b"zkmi-groth16-batch-rows" + H(vk) + D16 + i.to_bytes(8, "little"))) for i in range(3)]
    assert vr.groth16_rows_coefficients(vk, g16, pubs) == want16
    assert "%032x" % want16[1] == FIXED["groth16 row 1"]
    # no public inputs: the row's digest is the proof's alone; a digest whose low 128 bits are zero gives the coefficient one
    assert vr.row_digests(g16, None) == [H(p) for p in g16]
    assert vr.low128(b"\xff" * 16 + b"\0" * 16) == 1 and vr.low128(b"\0" * 31 + b"\2") == 2


FIXED = {
    "D": "883ec552f1000a6c17f1b99cde9167def962ab24216acc63f0439141bf1f28d5",
    "plonk row 2": ["bb778e030099250de689ca37d8a9ad25", "c3a853893f924ddc6dceabb5dade4778"],
    "groth16 row 1": "c40cd4713334a072b237a194859f0010",
}
