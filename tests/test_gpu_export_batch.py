"""GPU suite for the batch entries of the export path (-m gpu): many witness-value texts of ONE circuit per call.
  zk_plonk_solutions_rows / zk_groth16_wires_rows          the assembly alone, against the oracle's HandleValues / buildR1CS
  zk_plonk_prove_batch_with_pk / zk_groth16_prove_batch_with_pk   row v's characters are exactly the single entry's for that row's text, key and randomness; a bad
                                                           row (violated circuit, non-canonical felt, bad hex, wrong count header) has its status and no
                                                           proof, and its neighbours are what they are without it
The rows of a call are satisfying assignments of one circuit text: tools/synth_acir.synth / tools/synth_raw_r1cs.synth with different `first`."""
import ctypes as C
import json
import os
import threading

import numpy as np
import pytest

from noir_backend_using_gnark_amd import _lib, kzg
from noir_backend_using_gnark_amd import frontend as fe
from noir_backend_using_gnark_amd import verify as zv
from oracle import bn254_ref as ref
from oracle import plonk_ref as pl
from tools import synth_acir as sa
from tools import synth_raw_r1cs as sr

pytestmark = pytest.mark.gpu
R = ref.R
M = pl.ints_to_mont_np
HERE = os.path.dirname(os.path.abspath(__file__))
h2i = lambda h: int(h, 16)
LAYOUTS = {"reference": fe.LAYOUT_REFERENCE, "one_var": fe.LAYOUT_ONE_VAR_PER_WITNESS}
FIRSTS = [None, (0x1111, 0x2222), (R - 1, 0), (5, R - 2), (0xABCDEF << 200, 7)]
ZEROS = "0" * (2 * _lib.PLONK_PROOF_BYTES)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    _lib.require_device()


@pytest.fixture(scope="module")
def plonk_golden():
    return json.load(open(os.path.join(HERE, "golden", "plonk_golden.json")))


def _enc(values) -> str:
    return sa.felts_wire_hex(values)


class _Plonk:
    """one circuit text, `rows` satisfying assignments of it, a resident SRS and key, pinned blinders and the single entry's proof of every row"""

    def __init__(self, n_opcodes, rows, seed):
        self.acir, _ = sa.synth(n_opcodes, 3)
        self.values = [sa.synth(n_opcodes, 3, first=FIRSTS[v])[1] for v in range(rows)]
        self.texts = [_enc(w) for w in self.values]
        n = 1
        while n < n_opcodes + 3:
            n <<= 1
        self.srs = kzg.new_srs(n + 3, M([0x5EED0000 + seed])[0])
        self.pk_hex, self.vk_hex, self.h = fe.plonk_preprocess(self.acir, self.texts[0], self.srs, keep_resident=True)
        self.bl = np.stack([M(ref.rand_felts(0xB100 + seed + v, 9)) for v in range(rows)])
        self.single = [fe.plonk_prove_with_pk(self.acir, self.texts[v], None, self.srs, blinders=self.bl[v], pk_handle=self.h) for v in range(rows)]

    def free(self):
        _lib.check(_lib.lib().zk_bn254_plonk_pk_free(C.c_uint64(self.h)))
        self.srs.free()


@pytest.fixture(scope="module")
def p64():
    p = _Plonk(40, 5, 1)
    yield p
    p.free()


# ------------------------------------------------------------------------------------------------ the assembly alone
def _check_solutions(acir_dict, acir_text, value_rows):
    for lname, layout in LAYOUTS.items():
        try:
            want = [pl.sparse_r1cs_from_acir(acir_dict, w, lname)[1] for w in value_rows]
        except KeyError:  # a term names a witness without a variable: an error in this layout, there as here
            with pytest.raises(ValueError):
                fe.plonk_solutions_rows(acir_text, [_enc(w) for w in value_rows], layout)
            continue
        got, status = fe.plonk_solutions_rows(acir_text, [_enc(w) for w in value_rows], layout)
        assert status == [0] * len(value_rows)
        assert got.shape == (len(value_rows), len(want[0]), 4)
        for v, sol in enumerate(want):
            assert (got[v] == M(sol)).all(), (lname, v)


def test_solution_rows_on_the_reference_fixtures(plonk_golden):
    """HandleValues does not look at the gates: rows 1 and 2 are other value vectors of the fixture's length"""
    assert len(plonk_golden) == 3
    for k, e in enumerate(plonk_golden):
        values = [h2i(v) for v in e["values"]]
        rows = [values, ref.rand_felts(0x50 + k, len(values)), [R - 1 - i for i in range(len(values))]]
        _check_solutions(e["acir"], json.dumps(e["acir"]), rows)


@pytest.mark.parametrize("n_public", [0, 1, 3])
def test_solution_rows_with_duplicated_secret_variables(n_public):
    """the reference layout's duplicated variables only appear with two or more public inputs"""
    acir, _ = sa.synth(40, n_public)
    rows = [sa.synth(40, n_public, first=FIRSTS[v])[1] for v in range(3)]
    _check_solutions(json.loads(acir), acir, rows)
    if n_public == 3:
        assert fe.acir_to_sparse_r1cs(acir, 42, fe.LAYOUT_REFERENCE)["n_vars"] > 42 == fe.acir_to_sparse_r1cs(acir, 42, fe.LAYOUT_ONE_VAR_PER_WITNESS)["n_vars"]


def test_wire_rows_against_build_r1cs():
    raw, _ = sr.synth(24, 3)
    rows = [sr.synth(24, 3, first=FIRSTS[v + 1])[1] for v in range(3)]
    got, status = fe.groth16_wires_rows(raw, [_enc(w) for w in rows], 1 + 26 + 24)
    assert status == [0, 0, 0]
    for v, w in enumerate(rows):
        r1, wires = pl.r1cs_from_raw(json.loads(sr.with_values(raw, w)))
        assert len(wires) == 51 and (got[v] == M(wires)).all(), v
    # a bad felt becomes zero in its own row's wires (and in the products that read it), the neighbours do not notice
    bad = _enc(rows[1])
    bad = bad[:8 + 64 * 4] + "%064x" % R + bad[8 + 64 * 5:]
    got2, status = fe.groth16_wires_rows(raw, [_enc(rows[0]), bad, _enc(rows[2])], 51)
    assert status == [0, _lib.ROW_NOT_CANONICAL, 0]
    assert (got2[0] == got[0]).all() and (got2[2] == got[2]).all()
    _, zeroed = pl.r1cs_from_raw(json.loads(sr.with_values(raw, rows[1][:4] + [0] + rows[1][5:])))
    assert (got2[1] == M(zeroed)).all()


# ------------------------------------------------------------------------------------------------ PLONK
def test_plonk_batch_of_one_row_gives_the_golden_proofs(plonk_golden):
    for e in plonk_golden:
        acir = json.dumps(e["acir"])
        enc = ref.felts_wire([h2i(v) for v in e["values"]]).hex()
        srs = kzg.new_srs(e["srs_size"], M([h2i(e["srs_alpha"])])[0])
        bl = M([h2i(v) for v in e["blinders"]])
        proofs, status = fe.plonk_prove_batch_with_pk(acir, [enc], e["pk_hex"], srs, blinders=bl)
        assert status == [0] and proofs == [e["proof"]], e["name"]
        srs.free()
    fe.export_cache_clear()


def _raw_plonk_batch(p, texts, bl, chunk_rows=0):
    """the C entry itself: the rows' characters as they are written (the Python mirror turns a row without a proof into None)"""
    rows = len(texts)
    a, text = p.acir.encode(), "".join(texts).encode()
    out = C.create_string_buffer(b"\x55" * (rows * 1096), rows * 1096)
    status = np.full(rows, -1, np.int32)
    bl = np.ascontiguousarray(bl, dtype=np.uint64)
    _lib.check(_lib.lib().zk_plonk_prove_batch_with_pk(a, len(a), 0, text, len(texts[0]), len(texts[0]), rows, None, 0, p.h, p.srs.handle, _lib.vp(bl), chunk_rows,
                                                       C.addressof(out), _lib.vp(status)))
    return [out.raw[1096 * v:1096 * (v + 1)].decode() for v in range(rows)], list(status)


@pytest.mark.parametrize("chunk_rows", [0, 2])
@pytest.mark.parametrize("key", ["text", "handle"])
def test_plonk_batch_rows_are_the_single_entry_s_proofs(p64, key, chunk_rows):
    pk, h = (p64.pk_hex, 0) if key == "text" else (None, p64.h)
    proofs, status = fe.plonk_prove_batch_with_pk(p64.acir, p64.texts, pk, p64.srs, blinders=p64.bl, pk_handle=h, chunk_rows=chunk_rows)
    assert status == [0] * 5 and proofs == p64.single
    if key == "text":
        fe.export_cache_clear()


@pytest.mark.parametrize("chunk_rows", [0, 2])
def test_plonk_batch_bad_rows_have_a_status_and_no_proof(p64, chunk_rows):
    violated = list(p64.values[1])
    violated[5] = (violated[5] + 1) % R
    not_canonical = p64.texts[3][:8 + 64 * 7] + "%064x" % R + p64.texts[3][8 + 64 * 8:]
    wrong_count = "%08x" % 41 + p64.texts[4][8:]
    texts = [p64.texts[0], _enc(violated), p64.texts[2], not_canonical, wrong_count]
    raw, status = _raw_plonk_batch(p64, texts, p64.bl, chunk_rows)
    assert status == [0, _lib.ROW_UNSATISFIED, 0, _lib.ROW_NOT_CANONICAL, _lib.ROW_BAD_COUNT]
    assert raw == [p64.single[0], ZEROS, p64.single[2], ZEROS, ZEROS]
    proofs, status2 = fe.plonk_prove_batch_with_pk(p64.acir, texts, None, p64.srs, blinders=p64.bl, pk_handle=p64.h, chunk_rows=chunk_rows)
    assert status2 == status and proofs == [p64.single[0], None, p64.single[2], None, None]
    # an invalid character is the row's own too
    texts = [p64.texts[0][:-1] + "g"] + p64.texts[1:]
    proofs, status = fe.plonk_prove_batch_with_pk(p64.acir, texts, None, p64.srs, blinders=p64.bl, pk_handle=p64.h, chunk_rows=chunk_rows)
    assert status == [_lib.ROW_BAD_HEX, 0, 0, 0, 0] and proofs == [None] + p64.single[1:]


def test_plonk_batch_draws_its_blinders_when_none_are_given(p64):
    proofs, status = fe.plonk_prove_batch_with_pk(p64.acir, p64.texts, None, p64.srs, pk_handle=p64.h)
    assert status == [0] * 5 and all(a != b for a, b in zip(proofs, p64.single)) and len(set(proofs)) == 5
    pub = np.stack([M(w[:3]) for w in p64.values])
    assert zv.plonk_verify_batch([bytes.fromhex(x) for x in proofs], p64.vk_hex, p64.srs.g2, pub).all()


def test_plonk_batch_with_several_workgroups_per_row():
    p = _Plonk(1000, 3, 2)  # domain 2^10: the decode and the gather of a row span four workgroups
    try:
        proofs, status = fe.plonk_prove_batch_with_pk(p.acir, p.texts, None, p.srs, blinders=p.bl, pk_handle=p.h, chunk_rows=2)
        assert status == [0, 0, 0] and proofs == p.single
    finally:
        p.free()


def test_a_batch_and_a_single_proof_on_the_same_circuit_and_key_overlap(p64):
    got = {}

    def batch():
        got["batch"] = [fe.plonk_prove_batch_with_pk(p64.acir, p64.texts, None, p64.srs, blinders=p64.bl, pk_handle=p64.h, chunk_rows=2) for _ in range(2)]

    def single():
        got["single"] = [fe.plonk_prove_with_pk(p64.acir, p64.texts[v], None, p64.srs, blinders=p64.bl[v], pk_handle=p64.h) for v in (3, 0, 4)]

    ths = [threading.Thread(target=batch), threading.Thread(target=single)]
    [t.start() for t in ths]
    [t.join() for t in ths]
    assert got["batch"] == [(p64.single, [0] * 5)] * 2
    assert got["single"] == [p64.single[3], p64.single[0], p64.single[4]]


def test_text_keyed_batches_share_one_resident_circuit_and_key_with_the_single_entry(p64):
    """four batches of five rows also take the cached key past its sixteenth proof: the Lagrange form of its SRS is built in front of that batch, no byte changes"""
    fe.export_cache_clear()
    assert fe.export_cache_info()["circuits"] == 0 and fe.export_cache_info()["keys"] == 0
    for chunk_rows in (0, 2, 0, 2):
        proofs, status = fe.plonk_prove_batch_with_pk(p64.acir, p64.texts, p64.pk_hex, p64.srs, blinders=p64.bl, chunk_rows=chunk_rows)
        assert status == [0] * 5 and proofs == p64.single
        info = fe.export_cache_info()
        assert (info["circuits"], info["keys"]) == (1, 1)
    assert fe.plonk_prove_with_pk(p64.acir, p64.texts[2], p64.pk_hex, p64.srs, blinders=p64.bl[2]) == p64.single[2]
    info = fe.export_cache_info()
    assert (info["circuits"], info["keys"]) == (1, 1)
    fe.export_cache_clear()


# ------------------------------------------------------------------------------------------------ Groth16
def test_groth16_batch_rows_are_the_single_entry_s_proofs_with_and_without_window_tables():
    raw, _ = sr.synth(1 << 10, 3)
    values = [sr.synth(1 << 10, 3, first=FIRSTS[v + 1])[1] for v in range(4)]
    texts = [_enc(w) for w in values]
    rs = np.stack([M(ref.rand_felts(0xE100 + v, 2)) for v in range(4)])
    pk_hex, vk_hex, h = fe.groth16_preprocess(raw, M(ref.rand_felts(0xE2, 5)), keep_resident=True)
    single = [fe.groth16_prove_with_pk(sr.with_values(raw, values[v]), None, rs[v], pk_handle=h) for v in range(4)]
    assert len(set(single)) == 4
    lib = _lib.lib()

    def batched():
        b = C.c_int(-1)
        _lib.check(lib.zk_bn254_groth16_batch_info(C.c_uint64(h), None, C.byref(b)))
        return b.value

    bad_hex = texts[1][:100] + "G0g" + texts[1][103:]
    for tables in (0, 1):
        if tables:
            built = C.c_int(0)
            _lib.check(lib.zk_bn254_groth16_pk_build_tables(C.c_uint64(h), C.c_int(0), C.byref(built)))
        assert batched() == tables  # row by row inside the prover without them, the batched route with them
        for chunk_rows in (0, 3):
            proofs, status = fe.groth16_prove_batch_with_pk(raw, texts, None, rs, pk_handle=h, chunk_rows=chunk_rows)
            assert status == [0] * 4 and proofs == single, (tables, chunk_rows)
        proofs, status = fe.groth16_prove_batch_with_pk(raw, [texts[0], bad_hex, texts[2], texts[3]], None, rs, pk_handle=h)
        assert status == [0, _lib.ROW_BAD_HEX, 0, 0] and proofs == [single[0], None, single[2], single[3]], tables
    # drawn (r, s): other proofs, all different
    proofs, status = fe.groth16_prove_batch_with_pk(raw, texts, None, None, pk_handle=h)
    assert status == [0] * 4 and len(set(proofs + single)) == 8
    # the key as text: found (made) resident by content; its second proof queues its window tables in the background -- before, during and after: the same bytes
    fe.export_cache_clear()
    for _ in range(2):
        proofs, status = fe.groth16_prove_batch_with_pk(raw, texts, pk_hex, rs)
        assert status == [0] * 4 and proofs == single
    assert lib.zk_background_wait(C.c_int(-1)) == 1
    proofs, status = fe.groth16_prove_batch_with_pk(raw, texts, pk_hex, rs, chunk_rows=3)
    assert status == [0] * 4 and proofs == single
    assert fe.groth16_prove_with_pk(sr.with_values(raw, values[1]), pk_hex, rs[1]) == single[1]
    info = fe.export_cache_info()
    assert (info["circuits"], info["keys"]) == (1, 1)
    fe.export_cache_clear()
    _lib.check(lib.zk_bn254_groth16_pk_free(C.c_uint64(h)))
