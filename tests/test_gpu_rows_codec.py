"""GPU suite for the row utilities in front of the device batch verifiers (-m gpu):
  zk_bn254_rows_sha256_dev             one SHA-256 per row of a || b, against hashlib at the padding edges, with strides and poison between the rows
  zk_bn254_bytes_decode_hex_rows_dev   hex.DecodeString per row: both letter cases, an invalid character at the row's ends and across a word, any pitch
  zk_bn254_felts_public_hex_rows_dev   the verifier's reading of a values text: count header, every character, only the public felts decoded"""
import hashlib

import numpy as np
import pytest

from noir_backend_using_gnark_amd import _lib, wire
from noir_backend_using_gnark_amd import bn254 as zb
from oracle import bn254_ref as ref
from oracle import plonk_ref as pl

pytestmark = pytest.mark.gpu
R = ref.R
OK, BAD_HEX, NOT_CANONICAL, BAD_COUNT = _lib.ROW_OK, _lib.ROW_BAD_HEX, _lib.ROW_NOT_CANONICAL, _lib.ROW_BAD_COUNT


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    _lib.require_device()


def _bytes(seed, rows, n):
    return np.random.default_rng(seed).integers(0, 256, (rows, n), dtype=np.uint8)


# ------------------------------------------------------------------------------------------------ rows_sha256
@pytest.mark.parametrize("a_len,b_len", [(0, 0), (55, 0), (56, 0), (63, 1), (64, 0), (119, 9), (128, 0), (128, 96), (548, 0), (548, 32)])
def test_rows_sha256_matches_hashlib(a_len, b_len):
    for rows in (1, 63, 64, 65, 257):
        a, b = _bytes(1000 * a_len + rows, rows, a_len), _bytes(77 + b_len + rows, rows, b_len)
        want = np.stack([np.frombuffer(hashlib.sha256(a[v].tobytes() + b[v].tobytes()).digest(), dtype=np.uint8) for v in range(rows)])
        assert (zb.rows_sha256(a, b) == want).all(), rows
        # strides larger than the rows (odd ones: no row but the first is aligned), poison between them
        got = zb.rows_sha256(a, b, a_stride=a_len + 13, b_stride=b_len + 7, fill=0xA5)
        assert (got == want).all(), rows


def test_rows_sha256_with_one_span_only():
    a = _bytes(5, 3, 100)
    want = np.stack([np.frombuffer(hashlib.sha256(a[v].tobytes()).digest(), dtype=np.uint8) for v in range(3)])
    assert (zb.rows_sha256(a, None) == want).all()
    assert (zb.rows_sha256(None, a) == want).all()


# ------------------------------------------------------------------------------------------------ proof-hex rows
def _proof_rows(rows, n_bytes, seed):
    raw = _bytes(seed, rows, n_bytes)
    texts = [raw[v].tobytes().hex() for v in range(rows)]
    for v in range(rows):                       # lower, upper and mixed case
        if v % 3 == 1:
            texts[v] = texts[v].upper()
        elif v % 3 == 2:
            texts[v] = "".join(c.upper() if i % 2 else c for i, c in enumerate(texts[v]))
    return raw, texts


@pytest.mark.parametrize("n_bytes", [128, 548])
@pytest.mark.parametrize("rows", [1, 65])
def test_proof_hex_rows(rows, n_bytes):
    raw, texts = _proof_rows(rows, n_bytes, 11 * rows + n_bytes)
    chars = 2 * n_bytes
    for pitch, lead, stride in ((chars, 0, n_bytes), (chars + 7, 3, n_bytes + 5), (chars + 16, 8, n_bytes + 16)):   # 7: not a multiple of 16, nor of 4
        got, status = wire.decode_hex_bytes_rows(texts, pitch=pitch, out_stride=stride, fill=0xC3, lead=lead)
        assert status == [OK] * rows
        assert (got[:, :n_bytes] == raw).all() and (got[:, n_bytes:] == 0xC3).all()
    # an invalid character at the first character of a row, at the last, and at characters 15 / 16 / 17
    for at in (0, chars - 1, 15, 16, 17):
        for bad_char in ("g", "G", "/", ":", "@", "`", "\x10", " "):
            for victim in sorted({0, rows - 1, rows // 2}):
                t = list(texts)
                t[victim] = t[victim][:at] + bad_char + t[victim][at + 1:]
                got, status = wire.decode_hex_bytes_rows(t, pitch=chars + 7, out_stride=n_bytes + 5, fill=0xC3, lead=1)
                want = raw.copy()
                want[victim] = 0                # a rejected row is all zero, its neighbours are untouched
                assert status == [BAD_HEX if v == victim else OK for v in range(rows)], (at, bad_char, victim)
                assert (got[:, :n_bytes] == want).all() and (got[:, n_bytes:] == 0xC3).all(), (at, bad_char, victim)
            if rows > 1:
                break                           # (every refused character on the single row; one of them at 65 rows)


def test_proof_hex_rows_accept_exactly_the_hex_characters():
    """every byte value in a row of its own: only 0-9, a-f, A-F decode"""
    texts = [bytes([c]) + b"0" * 7 for c in range(256)]
    got, status = wire.decode_hex_bytes_rows(texts)
    for c in range(256):
        if chr(c) in "0123456789abcdefABCDEF":
            assert status[c] == OK and got[c, 0] == int(chr(c), 16) << 4, c
        else:
            assert status[c] == BAD_HEX and (got[c] == 0).all(), c


# ------------------------------------------------------------------------------------------------ public values
def _enc(values):
    return "%08x" % len(values) + "".join("%064x" % v for v in values)


@pytest.mark.parametrize("n_public", [0, 1, 3])
def test_public_values_rows(n_public):
    n = 9
    rows = 5
    vals = [[v % R for v in ref.rand_felts(0x9A + 10 * n_public + r, n)] for r in range(rows)]
    vals[1][0] = R - 1
    vals[2][n - 1] = R - 1
    vals[3][4] = 0
    for where in ([], [0], [n - 1], [0, 4, n - 1], [n - 1, 0, 4]):           # the public position is the first / the last value
        if len(where) != n_public:
            continue
        texts = [_enc(w) for w in vals]
        texts[4] = texts[4].upper()
        want = np.stack([pl.ints_to_mont_np([w[k] for k in where]).reshape(len(where), 4) for w in vals]) if where else np.zeros((rows, 0, 4), np.uint64)
        for pitch, lead, stride in ((len(texts[0]), 0, len(where)), (len(texts[0]) + 5, 3, len(where) + 2), (len(texts[0]) + 24, 8, len(where) + 1)):
            got, status = wire.decode_public_rows(texts, where, pitch=pitch, pub_stride=stride, fill=0x5A5A, lead=lead)
            assert status == [OK] * rows, (where, pitch)
            assert (got[:, :len(where)] == want).all() and (got[:, len(where):] == 0x5A5A).all(), (where, pitch)

        def one(victim, text, expect):
            t = list(texts)
            t[victim] = text
            got, status = wire.decode_public_rows(t, where, pitch=len(t[0]) + 5, pub_stride=len(where) + 2, fill=0x5A5A, lead=3)
            w2 = want.copy()
            if expect != OK:
                w2[victim] = 0                  # a rejected row's public inputs are zeros
            assert status == [expect if v == victim else OK for v in range(rows)], (where, victim, expect, status)
            assert (got[:, :len(where)] == w2).all() and (got[:, len(where):] == 0x5A5A).all()
            return got

        def put(text, k, v):
            return text[:8 + 64 * k] + "%064x" % v + text[8 + 64 * (k + 1):]

        private = [k for k in range(n) if k not in where]
        # r at a public position is refused, at a private one it is not looked at; r - 1 is a value like any other
        for k in where:
            one(2, put(texts[2], k, R), NOT_CANONICAL)
            one(0, put(texts[0], k, (1 << 256) - 1), NOT_CANONICAL)
        for k in (private[0], private[-1]):
            one(1, put(texts[1], k, R), OK)
            one(1, put(texts[1], k, (1 << 256) - 1), OK)
        # a wrong count header (another count, a character that is no digit), whatever else the row holds
        one(0, "%08x" % (n + 1) + texts[0][8:], BAD_COUNT)
        one(4, "0000000g" + texts[4][8:], BAD_COUNT)
        one(2, "%08x" % (n - 1) + put(texts[2], private[0], R)[8:-1] + "z", BAD_COUNT)
        # an invalid character in a private felt, at the text's first and last felt character, and across a word of the text
        for at in (8 + 64 * private[0] + 5, 8, len(texts[0]) - 1, 8 + 64 * private[-1] + 63, 23, 24, 25):
            for c in ("g", "\x10", "G"):
                one(3, texts[3][:at] + c + texts[3][at + 1:], BAD_HEX)
        # bad hex comes before a public felt >= r in the same row (hex.DecodeString runs first)
        if where:
            t = put(texts[1], where[0], R)
            at = 8 + 64 * private[0]
            one(1, t[:at] + "x" + t[at + 1:], BAD_HEX)


def test_public_values_r_minus_one_at_a_public_position_is_accepted():
    n = 4
    vals = [[R - 1, 5, 6, R - 1], [0, R - 1, R - 1, 0]]
    got, status = wire.decode_public_rows([_enc(w) for w in vals], [0, 3])
    assert status == [OK, OK]
    assert (got == np.stack([pl.ints_to_mont_np([w[0], w[3]]).reshape(2, 4) for w in vals])).all()


def test_public_values_rows_longer_than_a_workgroup_s_stride():
    """1030 values: the whole-text check walks 65,920 characters in strides of 256 lanes, the public felts sit at both ends and in the middle"""
    n, rows = 1030, 3
    vals = [[v % R for v in ref.rand_felts(0x77 + r, n)] for r in range(rows)]
    where = [0, 515, n - 1]
    texts = [_enc(w) for w in vals]
    want = np.stack([pl.ints_to_mont_np([w[k] for k in where]).reshape(3, 4) for w in vals])
    got, status = wire.decode_public_rows(texts, where, pitch=len(texts[0]) + 3, lead=1)
    assert status == [OK] * rows and (got == want).all()
    t = list(texts)
    at = 8 + 64 * 700 + 31
    t[1] = t[1][:at] + "h" + t[1][at + 1:]
    got, status = wire.decode_public_rows(t, where, pitch=len(texts[0]) + 3, lead=1)
    want[1] = 0
    assert status == [OK, BAD_HEX, OK] and (got == want).all()
