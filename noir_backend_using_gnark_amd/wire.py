"""Felt-vector wire codec, host-side mirror of the reference's helpers
(`DeserializeFelts` in gnark_backend_ffi/internal/backend/helpers.go:24-33, `encode_felts` in
src/gnark_backend_wrapper/serialize.rs:33-47): hex(u32 BE count || count x 32 B BE canonical felts) <-> a Montgomery
fr.Element vector resident in HBM (decoded on the device by one fused kernel, csrc/wire.hip)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, lib


def deserialize_felts(encoded: str | bytes, capacity: int | None = None) -> tuple[_lib.DeviceBuffer, int]:
    """DeserializeFelts: returns (device buffer of n Montgomery fr.Elements, n).  Raises on bad hex, a length that does not match
    the count, or a non-canonical felt (gnark-crypto: "invalid fr.Element encoding")."""
    text = encoded.encode("ascii") if isinstance(encoded, str) else bytes(encoded)
    if len(text) < 8:
        raise ValueError("felt vector shorter than its 4-byte count")
    cap = capacity if capacity is not None else max(1, (len(text) - 8) // 64)
    out = _lib.DeviceBuffer(cap * 32)
    n = C.c_size_t(0)
    check(lib().zk_bn254_felts_decode_hex(C.c_char_p(text), C.c_size_t(len(text)), C.c_void_p(out.ptr), C.c_size_t(cap), C.byref(n)))
    return out, int(n.value)


def serialize_felts(d_vec, n: int) -> str:
    """encode_felts of a Montgomery vector resident in HBM (DeviceBuffer or raw device pointer)."""
    ptr = d_vec.ptr if isinstance(d_vec, _lib.DeviceBuffer) else int(d_vec)
    buf = C.create_string_buffer(8 + 64 * n)
    check(lib().zk_bn254_felts_encode_hex(C.c_void_p(ptr), C.c_size_t(n), buf, C.c_size_t(8 + 64 * n)))
    return buf.raw.decode("ascii")


def decode_hex_rows(texts: list, to_mont: bool = True, out_stride: int | None = None, fill: int | None = None) -> tuple[np.ndarray, list]:
    """DeserializeFelts of many texts of the same count in one launch (zk_bn254_felts_decode_hex_rows_dev) -> ((rows, out_stride, 4) limbs, [status per row]).
    The rows are staged at the pitch the kernel asks for (64 n + 16: every row's felts 16-byte aligned).  Status: _lib.ROW_OK / ROW_BAD_HEX / ROW_NOT_CANONICAL /
    ROW_BAD_COUNT (the header is checked here, on the host, as the entry leaves it to its caller); a rejected felt decodes to zero.  out_stride > n leaves a gap
    behind every row that the kernel does not write: it keeps `fill` (every limb), with which the output is filled first when given."""
    rows = [t.encode("ascii") if isinstance(t, str) else bytes(t) for t in texts]
    if not rows:
        return np.zeros((0, 0, 4), np.uint64), []
    if any(len(r) != len(rows[0]) for r in rows) or len(rows[0]) < 8 or (len(rows[0]) - 8) % 64:
        raise ValueError("the texts of a batch must all be 8 + 64 n characters long")
    n = (len(rows[0]) - 8) // 64
    stride = n if out_stride is None else out_stride
    pitch = 64 * n + 16
    staged = b"\0" * 8 + b"".join(r + b"\0" * 8 for r in rows)  # row z's header at 8 + z * pitch
    d_text = _lib.DeviceBuffer.from_numpy(np.frombuffer(staged, dtype=np.uint8))
    init = np.zeros((len(rows), max(stride, 1), 4), np.uint64) if fill is None else np.full((len(rows), max(stride, 1), 4), fill, np.uint64)
    d_out = _lib.DeviceBuffer.from_numpy(init)
    d_status = _lib.DeviceBuffer.from_numpy(np.zeros(len(rows), np.int32))
    check(lib().zk_bn254_felts_decode_hex_rows_dev(d_text.ptr + 8, pitch, len(rows), n, d_out.ptr, stride, int(to_mont), d_status.ptr, None))
    out = d_out.to_numpy(np.uint64, init.shape)
    wire_status = d_status.to_numpy(np.int32, (len(rows),))  # 0, 1 = invalid hex character, 2 = not canonical
    status = []
    for r, ws in zip(rows, wire_status):
        try:
            header_ok = int(r[:8], 16) == n and not r[:8].strip(b"0123456789abcdefABCDEF")
        except ValueError:
            header_ok = False
        status.append(_lib.ROW_BAD_COUNT if not header_ok else (_lib.ROW_OK, _lib.ROW_BAD_HEX, _lib.ROW_NOT_CANONICAL)[int(ws)])
    return out[:, :stride] if stride else out[:, :0], status


def deserialize_felts_to_numpy(encoded) -> np.ndarray:
    d, n = deserialize_felts(encoded)
    return d.to_numpy(np.uint64, (max(n, 1), 4))[:n]


def decode_hex_bytes_rows(texts: list, pitch: int | None = None, out_stride: int | None = None, fill: int = 0, lead: int = 0) -> tuple[np.ndarray, list]:
    """hex.DecodeString of many texts of one length in one launch (zk_bn254_bytes_decode_hex_rows_dev) -> ((rows, out_stride) bytes, [status per row: _lib.ROW_OK or
    ROW_BAD_HEX]).  pitch (default: the text's length) is the distance between the rows' texts on the device and `lead` the offset of row 0 from an aligned
    address: any values will do.  A rejected row's bytes are zeros; the out_stride - n_bytes bytes behind every row are not written and keep `fill`."""
    rows = [t.encode("ascii") if isinstance(t, str) else bytes(t) for t in texts]
    if not rows:
        return np.zeros((0, 0), np.uint8), []
    if any(len(r) != len(rows[0]) for r in rows) or len(rows[0]) % 2:
        raise ValueError("the texts of a batch must all have the same even length")
    n_bytes = len(rows[0]) // 2
    pitch = len(rows[0]) if pitch is None else pitch
    stride = n_bytes if out_stride is None else out_stride
    if pitch < len(rows[0]) or stride < n_bytes:
        raise ValueError("pitch / out_stride below a row")
    staged = b"\xee" * lead + b"".join(r + b"\xee" * (pitch - len(r)) for r in rows)
    d_text = _lib.DeviceBuffer.from_numpy(np.frombuffer(staged, dtype=np.uint8))
    init = np.full((len(rows), max(stride, 1)), fill, np.uint8)
    d_out = _lib.DeviceBuffer.from_numpy(init)
    d_status = _lib.DeviceBuffer.from_numpy(np.full(len(rows), -1, np.int32))
    check(lib().zk_bn254_bytes_decode_hex_rows_dev(d_text.ptr + lead, pitch, len(rows), n_bytes, d_out.ptr, stride, d_status.ptr, None))
    return d_out.to_numpy(np.uint8, init.shape), [int(x) for x in d_status.to_numpy(np.int32, (len(rows),))]


def decode_public_rows(texts: list, where, pitch: int | None = None, pub_stride: int | None = None, fill: int = 0, lead: int = 0) -> tuple[np.ndarray, list]:
    """The verifier's reading of many felt-vector texts of one count in one launch (zk_bn254_felts_public_hex_rows_dev): the count header, every character, and
    of the felts only those at the 0-based positions `where` -> ((rows, pub_stride, 4) Montgomery limbs, [status per row: _lib.ROW_OK / ROW_BAD_COUNT / ROW_BAD_HEX /
    ROW_NOT_CANONICAL]).  pitch / lead / fill as in decode_hex_bytes_rows; a rejected row's public inputs are zeros."""
    rows = [t.encode("ascii") if isinstance(t, str) else bytes(t) for t in texts]
    where = np.ascontiguousarray(where, dtype=np.uint32).reshape(-1)
    if not rows:
        return np.zeros((0, len(where), 4), np.uint64), []
    if any(len(r) != len(rows[0]) for r in rows) or len(rows[0]) < 8 or (len(rows[0]) - 8) % 64:
        raise ValueError("the texts of a batch must all be 8 + 64 n characters long")
    n = (len(rows[0]) - 8) // 64
    pitch = len(rows[0]) if pitch is None else pitch
    stride = len(where) if pub_stride is None else pub_stride
    if pitch < len(rows[0]) or stride < len(where):
        raise ValueError("pitch / pub_stride below a row")
    staged = b"\xee" * lead + b"".join(r + b"\xee" * (pitch - len(r)) for r in rows)
    d_text = _lib.DeviceBuffer.from_numpy(np.frombuffer(staged, dtype=np.uint8))
    d_where = _lib.DeviceBuffer.from_numpy(where) if len(where) else None
    init = np.full((len(rows), max(stride, 1), 4), fill, np.uint64)
    d_pub = _lib.DeviceBuffer.from_numpy(init)
    d_status = _lib.DeviceBuffer.from_numpy(np.full(len(rows), -1, np.int32))
    check(lib().zk_bn254_felts_public_hex_rows_dev(d_text.ptr + lead, pitch, len(rows), n, d_where.ptr if d_where else None, len(where), d_pub.ptr, stride,
                                                   d_status.ptr, None))
    out = d_pub.to_numpy(np.uint64, init.shape)
    return (out[:, :stride] if stride else out[:, :0]), [int(x) for x in d_status.to_numpy(np.int32, (len(rows),))]
