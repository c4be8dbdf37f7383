"""GPU suite for the verifying batch entries of the export path (-m gpu): zk_plonk_verify_batch_with_vk / zk_groth16_verify_batch_with_vk take N proof texts and
N values texts of ONE circuit and one verifying-key text.  For a row with status ZK_ROW_OK the verdict is what the single sequence gives for that row's texts --
hex-decode the proof, take the public values, verify.plonk_verify / verify.groth16_verify: restated once below --; a bad row has its status, accepted = 0, and
leaves its neighbours what they are without it.  The proofs come from the prove-batch entries with pinned randomness."""
import ctypes as C
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
LAYOUTS = {"reference": fe.LAYOUT_REFERENCE, "one_var": fe.LAYOUT_ONE_VAR_PER_WITNESS}
FIRSTS = [None, (0x1111, 0x2222), (R - 1, 0), (5, R - 2), (0xABCDEF << 200, 7)]
OK, BAD_HEX, NOT_CANONICAL, BAD_COUNT, BAD_PROOF_HEX = _lib.ROW_OK, _lib.ROW_BAD_HEX, _lib.ROW_NOT_CANONICAL, _lib.ROW_BAD_COUNT, _lib.ROW_BAD_PROOF_HEX
HEX = set("0123456789abcdefABCDEF")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    _lib.require_device()


# ------------------------------------------------------------------------------------------------ the single sequence (goffi.cpp: PlonkVerifyWithVK / VerifyWithVK)
def _values_status(text, n_values):
    """DeserializeFelts' view of a values text, as far as a status: the count, then every character (hex.DecodeString sees the whole text)"""
    if set(text[:8]) - HEX or int(text[:8], 16) != n_values or len(text) != 8 + 64 * n_values:
        return BAD_COUNT
    return BAD_HEX if set(text[8:]) - HEX else OK


def _public_witnesses(acir, n_values, layout):
    a = acir.encode()
    out, n = np.zeros(64, np.uint32), C.c_size_t(0)
    _lib.check(_lib.lib().zk_acir_public_witnesses(C.c_char_p(a), C.c_size_t(len(a)), C.c_size_t(n_values), C.c_int(layout), _lib.vp(out), C.c_size_t(64), C.byref(n)))
    return [int(x) for x in out[:n.value]]


def _single_plonk(p, proof_text, values_text):
    """-> (status, accepted)"""
    if set(proof_text) - HEX:
        return BAD_PROOF_HEX, False
    st = _values_status(values_text, p.n_values)
    if st != OK:
        return st, False
    vals = [int(values_text[8 + 64 * k:8 + 64 * (k + 1)], 16) for k in _public_witnesses(p.acir, p.n_values, p.layout)]
    if any(v >= R for v in vals):
        return NOT_CANONICAL, False
    try:
        return OK, zv.plonk_verify(bytes.fromhex(proof_text), p.vk_hex, p.srs.g2, M(vals).reshape(len(vals), 4))
    except ValueError:                           # an encoding the host verifier refuses: a 0 from the batch
        return OK, False


def _single_groth16(g, proof_text, values_text):
    if set(proof_text) - HEX:
        return BAD_PROOF_HEX, False
    st = _values_status(values_text, g.n_values)
    if st != OK:
        return st, False
    try:
        pub = fe.groth16_public_inputs(g.raw[:g.at] + values_text + g.raw[g.at + len(values_text):])
    except ValueError as e:
        assert ">= r" in str(e), e
        return NOT_CANONICAL, False
    try:
        return OK, zv.groth16_verify(bytes.fromhex(proof_text), g.vk_hex, pub)
    except ValueError:
        return OK, False


def _cached(c, sequence, proof, text):
    """the single sequence's answer for a pair of texts, computed once per circuit (most rows of most calls below are the untouched ones)"""
    memo = c.__dict__.setdefault("_memo", {})
    if (proof, text) not in memo:
        memo[(proof, text)] = sequence(c, proof, text)
    return memo[(proof, text)]


class _Plonk:
    def __init__(self, n_public, layout, seed, rows=5, n_opcodes=40):
        self.layout, self.n_public = layout, n_public
        self.acir, _ = sa.synth(n_opcodes, n_public)
        self.values = [sa.synth(n_opcodes, n_public, first=FIRSTS[v])[1] for v in range(rows)]
        self.n_values = len(self.values[0])
        self.texts = [sa.felts_wire_hex(w) for w in self.values]
        self.srs = kzg.new_srs(64 + 3, M([0x5EED1000 + seed])[0])
        self.pk_hex, self.vk_hex, self.h = fe.plonk_preprocess(self.acir, self.texts[0], self.srs, keep_resident=True, layout=layout)
        self.bl = np.stack([M(ref.rand_felts(0xB200 + seed + v, 9)) for v in range(rows)])
        self.proofs, status = fe.plonk_prove_batch_with_pk(self.acir, self.texts, None, self.srs, blinders=self.bl, pk_handle=self.h, layout=layout)
        assert status == [0] * rows and len(set(self.proofs)) == rows

    def verify(self, proofs, texts, chunk_rows=0, vk=None):
        acc, status = fe.plonk_verify_batch_with_vk(self.acir, proofs, texts, vk or self.vk_hex, self.srs.g2, chunk_rows=chunk_rows, layout=self.layout)
        return [bool(x) for x in acc], status

    def single(self, proof, text):
        return _cached(self, _single_plonk, proof, text)

    def free(self):
        _lib.check(_lib.lib().zk_bn254_plonk_pk_free(C.c_uint64(self.h)))
        self.srs.free()


class _Groth16:
    def __init__(self, rows):
        self.raw, _ = sr.synth(24, 3)
        self.at = self.raw.index('"values":"') + len('"values":"')
        self.values = [sr.synth(24, 3, first=FIRSTS[v])[1] for v in range(rows)]
        self.n_values = len(self.values[0])
        self.texts = [sr.felts_wire_hex(w) for w in self.values]
        rs = np.stack([M(ref.rand_felts(0xE300 + v, 2)) for v in range(rows)])
        self.pk_hex, self.vk_hex, self.h = fe.groth16_preprocess(self.raw, M(ref.rand_felts(0xE4, 5)), keep_resident=True)
        self.proofs, status = fe.groth16_prove_batch_with_pk(self.raw, self.texts, None, rs, pk_handle=self.h)
        assert status == [0] * rows and len(set(self.proofs)) == rows

    def verify(self, proofs, texts, chunk_rows=0, vk=None):
        acc, status = fe.groth16_verify_batch_with_vk(self.raw, proofs, texts, vk or self.vk_hex, chunk_rows=chunk_rows)
        return [bool(x) for x in acc], status

    def single(self, proof, text):
        return _cached(self, _single_groth16, proof, text)

    def free(self):
        _lib.check(_lib.lib().zk_bn254_groth16_pk_free(C.c_uint64(self.h)))


@pytest.fixture(scope="module", params=[(np_, ln) for np_ in (0, 1, 3) for ln in LAYOUTS], ids=lambda p: "%d public, %s" % p)
def plonk(request):
    n_public, lname = request.param
    p = _Plonk(n_public, LAYOUTS[lname], 16 * n_public + len(lname))
    yield p
    p.free()
    fe.export_cache_clear()


@pytest.fixture(scope="module", params=[3, 5], ids=lambda r: "%d rows" % r)
def groth16(request):
    g = _Groth16(request.param)
    yield g
    g.free()
    fe.export_cache_clear()


def _put(text, k, v):
    return text[:8 + 64 * k] + "%064x" % v + text[8 + 64 * (k + 1):]


def _flip(proof, at):
    """another hex digit at `at`"""
    return proof[:at] + ("1" if proof[at] != "1" else "2") + proof[at + 1:]


def _against_single(c, proofs, texts, chunk_rows=0):
    """the batch entry's (accepted, status) for these rows, checked row by row against the single sequence"""
    acc, status = c.verify(proofs, texts, chunk_rows)
    want = [c.single(p, t) for p, t in zip(proofs, texts)]
    assert status == [w[0] for w in want] and acc == [w[1] for w in want], (acc, status, want)
    return acc, status


def _chunkings(j):
    """chunk_rows 1, 2 and 0 (no cap) for the first case of a kind, one of them in turn for the others"""
    return (1, 2, 0) if j == 0 else ((2, 0, 1)[j % 3],)


def _the_checks(c, public_at):
    """what both proof systems are asked: c is a _Plonk or a _Groth16; public_at: the position, in the values text, of a public value (None: there is none)"""
    rows = len(c.proofs)
    everyone = [True] * rows
    # all rows are accepted, and each verdict is the single sequence's; chunk_rows changes nothing
    for chunk_rows in (1, 2, 0):
        acc, status = _against_single(c, c.proofs, c.texts, chunk_rows)
        assert acc == everyone and status == [OK] * rows, chunk_rows
    assert c.verify([p.upper() for p in c.proofs], c.texts) == (everyone, [OK] * rows)           # either letter case, as hex.DecodeString
    # row v's proof with row w's values is rejected (where the circuit has public values: without them nothing binds a proof to its values), its neighbours accepted
    texts = list(c.texts)
    texts[1], texts[2] = c.texts[2], c.texts[1]
    acc, status = _against_single(c, c.proofs, texts)
    swapped = public_at is None
    assert acc == [True, swapped, swapped] + everyone[3:] and status == [OK] * rows
    # one flipped proof character (still hex): rejected -- as an equation that fails or as an encoding that is refused -- and the neighbours do not notice
    for j, (v, at) in enumerate(((0, 5), (rows - 1, len(c.proofs[0]) - 1), (1, 70))):
        proofs = list(c.proofs)
        proofs[v] = _flip(proofs[v], at)
        for chunk_rows in _chunkings(j):
            acc, status = _against_single(c, proofs, c.texts, chunk_rows)
            assert acc == [i != v for i in range(rows)] and status == [OK] * rows, (v, at, chunk_rows)
    # a non-hex proof character: status 5
    for j, (v, at, ch) in enumerate(((0, 0, "g"), (2, len(c.proofs[0]) - 1, "x"), (1, 16, "\x10"))):
        proofs = list(c.proofs)
        proofs[v] = proofs[v][:at] + ch + proofs[v][at + 1:]
        for chunk_rows in _chunkings(j):
            acc, status = _against_single(c, proofs, c.texts, chunk_rows)
            assert acc == [i != v for i in range(rows)] and status == [BAD_PROOF_HEX if i == v else OK for i in range(rows)], (v, at, chunk_rows)
    # a bad value row of each kind: its status, accepted = 0, the neighbours unchanged
    private = c.n_values - 1                       # (the last witness is never public in these circuits)
    kinds = [(BAD_COUNT, "%08x" % (c.n_values + 1) + c.texts[1][8:]), (BAD_COUNT, "0000000G" + c.texts[1][8:]),
             (BAD_HEX, c.texts[1][:8 + 64 * private + 9] + "g" + c.texts[1][8 + 64 * private + 10:]), (BAD_HEX, c.texts[1][:-1] + "/")]
    if public_at is not None:
        kinds += [(NOT_CANONICAL, _put(c.texts[1], public_at, R)), (NOT_CANONICAL, _put(c.texts[1], public_at, (1 << 256) - 1)),
                  (BAD_HEX, _put(c.texts[1], public_at, R)[:-1] + "z")]                        # hex.DecodeString runs before the felts are read
    for j, (want, text) in enumerate(kinds):
        texts = [c.texts[0], text] + c.texts[2:]
        for chunk_rows in _chunkings(j):
            acc, status = _against_single(c, c.proofs, texts, chunk_rows)
            assert acc == [True, False] + everyone[2:] and status == [OK, want] + [OK] * (rows - 2), (want, chunk_rows)
    # a felt >= r at a position that is not public is not an error: the single path never decodes it
    texts = [c.texts[0], _put(c.texts[1], private, R)] + c.texts[2:]
    acc, status = _against_single(c, c.proofs, texts)
    assert acc == everyone and status == [OK] * rows
    # both texts of a row bad: the proof's status comes first; every row bad: nothing is accepted
    # (row 0's header is the call's n_values: the bad count goes into row 1)
    proofs = [c.proofs[0], c.proofs[1][:-1] + "g"] + c.proofs[2:]
    acc, status = _against_single(c, proofs, [c.texts[0], "%08x" % 1 + c.texts[1][8:]] + c.texts[2:])
    assert acc == [True, False] + everyone[2:] and status == [OK, BAD_PROOF_HEX] + [OK] * (rows - 2)
    acc, status = _against_single(c, ["0" * len(c.proofs[0])] * rows, c.texts, 2)
    assert acc == [False] * rows and status == [OK] * rows


def test_plonk_rows_against_the_single_sequence(plonk):
    where = _public_witnesses(plonk.acir, plonk.n_values, plonk.layout)
    assert len(where) == plonk.n_public
    _the_checks(plonk, where[-1] if where else None)


def test_groth16_rows_against_the_single_sequence(groth16):
    _the_checks(groth16, 2)                      # witnesses 1..3 are public


def test_a_key_of_another_circuit_with_other_public_inputs_is_err_len():
    a = _Plonk(1, fe.LAYOUT_REFERENCE, 0x41, rows=2)
    b = _Plonk(3, fe.LAYOUT_REFERENCE, 0x42, rows=2)
    try:
        with pytest.raises(ValueError, match="invalid witness size, got 1, expected 3"):
            a.verify(a.proofs, a.texts, vk=b.vk_hex)
        n_acc, acc, status = C.c_size_t(99), np.full(2, 0xEE, np.uint8), np.full(2, 77, np.int32)
        ac, pr, tx, vk = a.acir.encode(), "".join(a.proofs).encode(), "".join(a.texts).encode(), b.vk_hex.encode()
        g2 = np.ascontiguousarray(a.srs.g2, dtype=np.uint64)
        rc = _lib.lib().zk_plonk_verify_batch_with_vk(ac, len(ac), 0, pr, 1096, tx, len(a.texts[0]), len(a.texts[0]), 2, vk, len(vk), _lib.vp(g2), 0, _lib.vp(acc), _lib.vp(status),
                                                      C.addressof(n_acc))
        assert rc == _lib.ZK_ERR_LEN and (acc == 0xEE).all() and (status == 77).all() and n_acc.value == 99
        assert a.verify(a.proofs, a.texts) == ([True, True], [OK, OK])
    finally:
        a.free()
        b.free()
        fe.export_cache_clear()
    g = _Groth16(3)
    try:
        other_raw, _ = sr.synth(24, 2)
        _, other_vk = fe.groth16_preprocess(other_raw, M(ref.rand_felts(0xE5, 5)))
        with pytest.raises(ValueError, match="invalid witness size, got 3, expected 2"):
            g.verify(g.proofs, g.texts, vk=other_vk)
        assert g.verify(g.proofs, g.texts) == ([True] * 3, [OK] * 3)
    finally:
        g.free()
        fe.export_cache_clear()


def test_two_batches_from_two_threads_beside_a_single_proof():
    p = _Plonk(3, fe.LAYOUT_REFERENCE, 0x51)
    got = {}
    tampered = [p.proofs[0], _flip(p.proofs[1], 9)] + p.proofs[2:]

    def batch(name, proofs, chunk_rows):
        got[name] = [p.verify(proofs, p.texts, chunk_rows) for _ in range(3)]

    def single():
        got["single"] = [fe.plonk_prove_with_pk(p.acir, p.texts[v], None, p.srs, blinders=p.bl[v], pk_handle=p.h, layout=p.layout) for v in (3, 0, 4)]

    try:
        ths = [threading.Thread(target=batch, args=("a", p.proofs, 2)), threading.Thread(target=batch, args=("b", tampered, 0)), threading.Thread(target=single)]
        [t.start() for t in ths]
        [t.join() for t in ths]
        assert got["a"] == [([True] * 5, [OK] * 5)] * 3
        assert got["b"] == [([True, False, True, True, True], [OK] * 5)] * 3
        assert got["single"] == [p.proofs[3], p.proofs[0], p.proofs[4]]
    finally:
        p.free()
        fe.export_cache_clear()


def test_more_rows_than_a_verifier_workgroup():
    """70 rows (the verifier's lanes come in workgroups of 64): the five proofs repeated, every seventh tampered with, in chunks of 64 + 6, 33 + 33 + 4 and all"""
    p = _Plonk(3, fe.LAYOUT_REFERENCE, 0x61)
    try:
        proofs = [p.proofs[v % 5] if v % 7 else _flip(p.proofs[v % 5], 3 + v) for v in range(70)]
        texts = [p.texts[v % 5] for v in range(70)]
        for chunk_rows in (64, 33, 0):
            acc, status = p.verify(proofs, texts, chunk_rows)
            assert acc == [bool(v % 7) for v in range(70)] and status == [OK] * 70, chunk_rows
    finally:
        p.free()
        fe.export_cache_clear()
