"""GPU suite for the row-batched felt decoder (-m gpu): zk_bn254_felts_decode_hex_rows_dev -- `rows` texts of the same count in ONE launch, the row as a grid
dimension -- against Python big-integer decoding of the same texts and against zk_bn254_felts_decode_hex of every row alone.  n in {1, 255, 256, 257} x rows
in {1, 2, 3}: a text is 8 + 64 n characters and the staging pitch 64 n + 16, so both parities of a row's alignment and a partial last workgroup occur."""
import numpy as np
import pytest

from noir_backend_using_gnark_amd import _lib, wire
from oracle import bn254_ref as ref
from oracle import plonk_ref as pl

pytestmark = pytest.mark.gpu
R = ref.R
M = pl.ints_to_mont_np
FILL = 0xA5A5A5A55A5A5A5A


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    _lib.require_device()


def _values(n, rows, seed):
    vals = [list(ref.rand_felts(seed + 16 * z, n)) for z in range(rows)]
    vals[0][0] = R - 1          # the largest canonical value
    vals[-1][n // 2] = 0 if (rows > 1 or n > 1) else R - 1
    return vals


def _text(values, upper=False):
    body = "".join("%064x" % v for v in values)
    return "%08x" % len(values) + (body.upper() if upper else body)


def _limbs(values, mont=True):
    return M(values) if mont else np.frombuffer(b"".join(v.to_bytes(32, "little") for v in values), dtype=np.uint64).reshape(-1, 4)


@pytest.mark.parametrize("rows", [1, 2, 3])
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_rows_decode_equals_big_integers_and_the_one_row_kernel(n, rows):
    vals = _values(n, rows, 0x5100 + n)
    texts = [_text(v, upper=(z == 1)) for z, v in enumerate(vals)]      # row 1 in upper-case digits
    out, status = wire.decode_hex_rows(texts, out_stride=n + 3, fill=FILL)
    assert status == [_lib.ROW_OK] * rows
    assert out.shape == (rows, n + 3, 4) and (out[:, n:] == FILL).all()          # the gap behind every row is not written
    for z in range(rows):
        assert (out[z, :n] == _limbs(vals[z])).all(), z
        assert out[z, :n].tobytes() == wire.deserialize_felts_to_numpy(texts[z].lower()).tobytes(), z
    if rows == 2:  # canonical limbs (no Montgomery conversion), packed rows
        out, status = wire.decode_hex_rows(texts, to_mont=False)
        assert status == [0, 0] and all((out[z] == _limbs(vals[z], mont=False)).all() for z in range(2))


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_a_bad_row_fails_neither_the_call_nor_its_neighbours(n):
    vals = _values(n, 3, 0x5200 + n)
    good = [_text(v) for v in vals]
    alone = [wire.deserialize_felts_to_numpy(t) for t in good]
    zero_at = lambda v, i: _limbs(v[:i] + [0] + v[i + 1:])
    # r itself in the first felt of the LAST row: not canonical, that row only; the felt decodes to zero, the row's other felts as they are
    bad = list(vals[2])
    bad[0] = R
    texts = good[:2] + ["%08x" % n + "".join("%064x" % v for v in bad)]
    out, status = wire.decode_hex_rows(texts, out_stride=n + 1, fill=FILL)
    assert status == [_lib.ROW_OK, _lib.ROW_OK, _lib.ROW_NOT_CANONICAL]
    assert out[0, :n].tobytes() == alone[0].tobytes() and out[1, :n].tobytes() == alone[1].tobytes()
    assert (out[2, :n] == zero_at(vals[2], 0)).all() and (out[:, n:] == FILL).all()
    # 'g', and the control byte 0x10 (whose low nibble would decode), as the last character of the MIDDLE row
    for ch in ("g", "\x10"):
        texts = [good[0], good[1][:-1] + ch, good[2]]
        out, status = wire.decode_hex_rows(texts)
        assert status == [_lib.ROW_OK, _lib.ROW_BAD_HEX, _lib.ROW_OK], ch
        assert out[0].tobytes() == alone[0].tobytes() and out[2].tobytes() == alone[2].tobytes()
        assert (out[1] == zero_at(vals[1], n - 1)).all()
    # both kinds in one row: the larger code (not canonical) is the row's verdict; a wrong count header is the caller's finding
    both = "f" * 64 + good[2][72:-1] + "z" if n > 1 else "f" * 63 + "z"
    texts = [good[0][:-1] + "G", "%08x" % (n + 1) + good[1][8:], "%08x" % n + both]
    out, status = wire.decode_hex_rows(texts)
    assert status == [_lib.ROW_BAD_HEX, _lib.ROW_BAD_COUNT, _lib.ROW_NOT_CANONICAL if n > 1 else _lib.ROW_BAD_HEX]
    assert out[1].tobytes() == alone[1].tobytes()
