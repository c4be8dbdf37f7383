"""CPU suite for the batch entries of the export path (many witness-value texts of one circuit per call): the symbols are there, the argument errors are
decided without a device, the row-status enum is what include/zkmi.h documents, and tools/synth_acir.synth's new `first` changes nothing but the witness."""
import ctypes as C
import hashlib
import json
import os
import re

import numpy as np
import pytest

from noir_backend_using_gnark_amd import _lib
from oracle import plonk_ref as pl
from tools import synth_acir as sa
from tools import synth_raw_r1cs as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("zk_bn254_felts_decode_hex_rows_dev", "zk_plonk_solutions_rows", "zk_groth16_wires_rows", "zk_plonk_prove_batch_with_pk", "zk_groth16_prove_batch_with_pk")


def test_symbols_are_exported_with_signatures():
    lib = _lib.lib()
    for s in NEW:
        assert s in _lib.SYMBOLS and hasattr(lib, s), s
        assert getattr(lib, s).argtypes == _lib.ARGTYPES[s]


def test_row_status_enum_is_as_documented():
    hdr = open(os.path.join(ROOT, "include", "zkmi.h")).read()
    got = {k: int(v) for k, v in re.findall(r"\b(ZK_ROW_[A-Z_]+) = (\d+)", hdr)}
    assert got == {"ZK_ROW_OK": 0, "ZK_ROW_UNSATISFIED": 1, "ZK_ROW_BAD_HEX": 2, "ZK_ROW_NOT_CANONICAL": 3, "ZK_ROW_BAD_COUNT": 4}
    assert (_lib.ROW_OK, _lib.ROW_UNSATISFIED, _lib.ROW_BAD_HEX, _lib.ROW_NOT_CANONICAL, _lib.ROW_BAD_COUNT) == (0, 1, 2, 3, 4)


def _plonk_batch(acir, text, vlen, stride, rows, pk, handle, out, status):
    return _lib.lib().zk_plonk_prove_batch_with_pk(acir, len(acir) if acir else 0, 0, text, vlen, stride, rows, pk, len(pk) if pk else 0, handle, 0, None, 0, out, status)


def _g16_batch(raw, text, vlen, stride, rows, pk, handle, out, status):
    return _lib.lib().zk_groth16_prove_batch_with_pk(raw, len(raw) if raw else 0, text, vlen, stride, rows, pk, len(pk) if pk else 0, handle, None, 0, out, status)


def test_argument_errors_are_decided_before_a_device_is_looked_for():
    """Every case returns its code whether or not a GPU is present: none of them reaches the device."""
    acir, w = sa.synth(8, 2)
    raw, w2 = sr.synth(8, 2)
    row = sa.felts_wire_hex(w).encode()
    a, r = acir.encode(), raw.encode()
    text = row * 2
    vlen = len(row)
    out = C.create_string_buffer(b"\x55" * (2 * 1096), 2 * 1096)
    status = np.full(2, 77, np.int32)
    o, s = C.addressof(out), status.ctypes.data
    pk = b"00"
    for call, circuit in ((_plonk_batch, a), (_g16_batch, r)):
        # a null pointer: the circuit, the values, the proofs, the statuses
        assert call(None, text, vlen, vlen, 2, pk, 0, o, s) == _lib.ZK_ERR_ARG
        assert call(circuit, None, vlen, vlen, 2, pk, 0, o, s) == _lib.ZK_ERR_ARG
        assert call(circuit, text, vlen, vlen, 2, pk, 0, None, s) == _lib.ZK_ERR_ARG
        assert call(circuit, text, vlen, vlen, 2, pk, 0, o, None) == _lib.ZK_ERR_ARG
        # rows a stride apart that is shorter than a row (one row's stride may be anything: that call gets as far as the length check below)
        assert call(circuit, text, vlen, vlen - 1, 2, pk, 0, o, s) == _lib.ZK_ERR_ARG
        assert call(circuit, text, vlen - 64, 0, 1, pk, 0, o, s) == _lib.ZK_ERR_LEN
        # values_len that is not 8 + 64 * (row 0's count)
        assert call(circuit, text, vlen - 64, vlen, 2, pk, 0, o, s) == _lib.ZK_ERR_LEN
        assert call(circuit, text, vlen + 64, vlen + 64, 1, pk, 0, o, s) == _lib.ZK_ERR_LEN
        assert call(circuit, b"0000000g" + text[8:], vlen, vlen, 2, pk, 0, o, s) == _lib.ZK_ERR_ARG   # no count at all
        # neither a key text nor a resident key
        assert call(circuit, text, vlen, vlen, 2, None, 0, o, s) == _lib.ZK_ERR_ARG
        # no rows: nothing to do, nothing written (not even looked at: the length is wrong)
        assert call(circuit, text, 5, 0, 0, pk, 0, o, s) == _lib.ZK_OK
        assert out.raw == b"\x55" * (2 * 1096) and (status == 77).all()
    lib = _lib.lib()
    # the assembly entries and the codec entry
    assert lib.zk_plonk_solutions_rows(None, 0, 0, text, vlen, vlen, 2, 256, 64, s) == _lib.ZK_ERR_ARG
    assert lib.zk_plonk_solutions_rows(a, len(a), 0, text, vlen, vlen, 2, None, 64, s) == _lib.ZK_ERR_ARG
    assert lib.zk_plonk_solutions_rows(a, len(a), 0, text, vlen, vlen - 1, 2, 256, 64, s) == _lib.ZK_ERR_ARG
    assert lib.zk_plonk_solutions_rows(a, len(a), 0, text, vlen - 64, vlen, 2, 256, 64, s) == _lib.ZK_ERR_LEN
    assert lib.zk_plonk_solutions_rows(a, len(a), 0, text, vlen, vlen, 2, 256, 1, s) == _lib.ZK_ERR_ARG     # sol_stride below the circuit's variables
    assert lib.zk_plonk_solutions_rows(a, len(a), 0, text, vlen, vlen, 0, 256, 64, s) == _lib.ZK_OK
    assert lib.zk_groth16_wires_rows(r, len(r), None, vlen, vlen, 2, 256, 64, s) == _lib.ZK_ERR_ARG
    assert lib.zk_groth16_wires_rows(r, len(r), text, vlen, vlen - 1, 2, 256, 64, s) == _lib.ZK_ERR_ARG
    assert lib.zk_groth16_wires_rows(r, len(r), text, vlen - 64, vlen, 2, 256, 64, s) == _lib.ZK_ERR_LEN   # not the length the circuit was read with
    assert lib.zk_groth16_wires_rows(r, len(r), text, vlen, vlen, 2, 256, 1, s) == _lib.ZK_ERR_ARG          # wire_stride below the circuit's wires
    assert lib.zk_groth16_wires_rows(r, len(r), text, vlen, vlen, 0, 256, 64, s) == _lib.ZK_OK
    dec = lib.zk_bn254_felts_decode_hex_rows_dev
    n = 3
    assert dec(None, 64 * n + 16, 2, n, 4096, n, 1, 8192, None) == _lib.ZK_ERR_ARG
    assert dec(1024 + 8, 64 * n + 16, 2, n, None, n, 1, 8192, None) == _lib.ZK_ERR_ARG
    assert dec(1024 + 8, 64 * n + 16, 2, n, 4096, n, 1, None, None) == _lib.ZK_ERR_ARG
    assert dec(1024 + 8, 64 * n + 16, 65536, n, 4096, n, 1, 8192, None) == _lib.ZK_ERR_ARG       # the row is a grid dimension
    assert dec(1024 + 8, 64 * n + 8, 2, n, 4096, n, 1, 8192, None) == _lib.ZK_ERR_ARG            # pitch not a multiple of 16
    assert dec(1024 + 8, 64 * n, 2, n, 4096, n, 1, 8192, None) == _lib.ZK_ERR_ARG                # pitch below a row
    assert dec(1024 + 8, 64 * n + 16, 2, n, 4096, n - 1, 1, 8192, None) == _lib.ZK_ERR_ARG       # out_stride below a row
    assert dec(1024, 64 * n + 16, 2, n, 4096, n, 1, 8192, None) == _lib.ZK_ERR_ARG               # the felts would not start 16-byte aligned
    assert dec(1024 + 8, 64 * n + 16, 0, n, 4096, n, 1, 8192, None) == _lib.ZK_OK
    assert dec(1024 + 8, 16, 2, 0, 4096, 0, 1, 8192, None) == _lib.ZK_OK
    assert (status == 77).all()


def test_synth_acir_first_changes_the_witness_and_nothing_else():
    """synth(40, 3) without `first` is byte for byte what the tool gave before it had the argument: sha256 of the circuit text
    d3955f41de22968c55ca1f13c96acf80e9551d4c1fee0f74f043a0feed451f42 and of felts_wire_hex(values)
    5497fbda1b6ef5cd75e2f6e4edcaee28ee6923a37c3b8a39162d7cef6742ce74, both computed with the parent commit's tools/synth_acir.py.  With `first` the text is the
    same and the values are another satisfying assignment (the oracle's lowering, both layouts)."""
    acir, w = sa.synth(40, 3)
    assert hashlib.sha256(acir.encode()).hexdigest() == "d3955f41de22968c55ca1f13c96acf80e9551d4c1fee0f74f043a0feed451f42"
    assert hashlib.sha256(sa.felts_wire_hex(w).encode()).hexdigest() == "5497fbda1b6ef5cd75e2f6e4edcaee28ee6923a37c3b8a39162d7cef6742ce74"
    assert sa.synth(40, 3, first=None) == (acir, w)
    for first in ((1, 2), (0, 0), (pl.R - 1, pl.R + 5)):
        acir2, w2 = sa.synth(40, 3, first=first)
        assert acir2 == acir and w2[:2] == [first[0] % pl.R, first[1] % pl.R] and w2 != w and len(w2) == len(w)
        for layout in ("reference", "one_var"):
            spr, sol = pl.sparse_r1cs_from_acir(json.loads(acir), w2, layout)
            assert spr.is_satisfied(sol)
    spr, sol = pl.sparse_r1cs_from_acir(json.loads(acir), w[:5] + [(w[5] + 1) % pl.R] + w[6:])
    assert not spr.is_satisfied(sol)
