"""Host-side mirror of gnark-crypto v0.9.1's kzg package for the hot path (ecc/bn254/fr/kzg; pinned at /root/reference/gnark_backend_ffi/go.mod:5):
    kzg.NewSRS(size, alpha)         reached at /root/reference/gnark_backend_ffi/backend/common.go:137      -> new_srs(size, alpha)
    (*SRS).ReadFrom / WriteTo       what LoadSRS / SaveSRS move through srs.hex (backend/common.go:86-125) -> read_srs / SRS.write
    kzg.Commit(p, srs)              reached through plonk.Setup / plonk.Prove (backend/plonk/plonk.go:21,67) -> SRS.commit
    kzg.Open(p, point, srs)         plonk.Prove's opening of Z at omega zeta                                  -> SRS.open (SRS.open_many: several at once)
    kzg.BatchOpenSinglePoint        plonk.Prove's batched opening of seven polynomials at zeta               -> SRS.batch_open_single_point
    kzg.Verify / FoldProof / BatchVerifySinglePoint   the end of plonk.Verify (host, no device)              -> verify / fold_proof / batch_verify_single_point
    kzg.BatchVerifyMultiPoints      many openings in one check, a verdict each (device)                      -> batch_verify_multi_points
    (tests)                         the Horner scan under Open and plonk.Prove, every stage copied back       -> hscan_inspect
The G1 side lives in HBM as a registered base array with its window tables; decoding a serialised SRS decompresses the points on the
device (one square root each) instead of on the host cores, and happens once instead of on every prove / verify call."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, lib, vp
from .bn254 import MultiExpConfig, ResidentBases


class SRS:
    def __init__(self, g1: ResidentBases, g2: np.ndarray, keep=None):
        self.g1, self.g2, self._keep = g1, g2, keep  # g2: (2, 16) uint64 = [G2, alpha * G2]

    @property
    def handle(self):
        return self.g1.handle

    def commit(self, poly, n: int | None = None) -> np.ndarray:
        """kzg.Commit: MultiExp(srs.G1[:len(p)], p); p = Montgomery coefficients (numpy (n, 4)) or a DeviceBuffer with n."""
        cfg = MultiExpConfig(scalars_mont=True)
        if isinstance(poly, _lib.DeviceBuffer):
            return self.g1.multi_exp_dev(poly, n, cfg)
        return self.g1.multi_exp(poly, cfg)

    def commit_rows(self, polys, *, n: int | None = None, rows: int | None = None, row_stride: int | None = None, sparse: bool = False, out=None, compressed=False,
                    points: bool = True):
        """kzg.Commit of every row of a matrix of Montgomery coefficients in one launch set per chunk of rows (ResidentBases.multi_exp_rows says the rest):
        a (rows, n, 4) uint64 array, or device rows with n, rows and row_stride.  Row v is commit's digest of that row."""
        return self.g1.multi_exp_rows(polys, n=n, rows=rows, row_stride=row_stride, sparse=sparse, out=out, compressed=compressed, points=points,
                                      config=MultiExpConfig(scalars_mont=True))

    @staticmethod
    def _rows(polys, lens):
        """host arrays or DeviceBuffers (then lens[k] = their coefficient counts) -> (pointer array, length array, on_device, keep-alive)"""
        dev = [isinstance(p, _lib.DeviceBuffer) for p in polys]
        if dev and any(dev) != all(dev):
            raise TypeError("polynomials must be all host arrays or all DeviceBuffers")
        if dev and dev[0]:
            if lens is None or len(lens) != len(polys):
                raise ValueError("DeviceBuffer polynomials need their lengths")
            keep, ptrs, ns = list(polys), [p.ptr for p in polys], [int(n) for n in lens]
        else:
            keep = [np.ascontiguousarray(p, dtype=np.uint64).reshape(-1, 4) for p in polys]
            ptrs, ns = [a.ctypes.data for a in keep], [a.shape[0] for a in keep]
        k = len(polys)
        return (C.c_void_p * max(k, 1))(*ptrs), (C.c_size_t * max(k, 1))(*ns), int(bool(dev and dev[0])), keep

    def open_many(self, polys, points, lens=None):
        """`len(polys)` independent kzg.Open calls in one launch set: polynomial k at points[k] ((k, 4) Montgomery).  Returns (H (k, 8), claimed values (k, 4))."""
        ptrs, ns, on_dev, keep = self._rows(polys, lens)
        z = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 4)
        if z.shape[0] != len(polys):
            raise ValueError("one point per polynomial")
        out = np.zeros((max(len(polys), 1), 12), np.uint64)
        _check_open(lib().zk_bn254_kzg_open(self.g1.handle, ptrs, ns, vp(z), C.c_size_t(len(polys)), C.c_int(on_dev), vp(out)))
        out = out[:len(polys)]
        return out[:, :8].copy(), out[:, 8:].copy()

    def open(self, poly, point, n: int | None = None):
        """kzg.Open(p, point, srs) -> (H (8,), claimed value (4,)); poly: Montgomery coefficients or a DeviceBuffer with n."""
        h, v = self.open_many([poly], np.ascontiguousarray(point, dtype=np.uint64).reshape(1, 4), None if n is None else [n])
        return h[0], v[0]

    def batch_open_single_point(self, polys, digests, point, lens=None):
        """kzg.BatchOpenSinglePoint(polys, digests, point, sha256, srs) -> (H (8,), claimed values (k, 4))."""
        ptrs, ns, on_dev, keep = self._rows(polys, lens)
        d = np.ascontiguousarray(digests, dtype=np.uint64).reshape(-1, 8)
        if d.shape[0] != len(polys):
            raise ValueError("kzg: number of digests differs from the number of polynomials")  # ErrInvalidNbDigests
        h, claimed = np.zeros(8, np.uint64), np.zeros((max(len(polys), 1), 4), np.uint64)
        _check_open(lib().zk_bn254_kzg_batch_open_single_point(self.g1.handle, ptrs, ns, vp(d), C.c_size_t(len(polys)),
                                                               vp(np.ascontiguousarray(point, dtype=np.uint64)), C.c_int(on_dev), vp(h), vp(claimed)))
        return h, claimed[:len(polys)]

    def write(self, as_hex: bool = False) -> bytes:
        """(*SRS).WriteTo (as_hex: the text SaveSRS writes to srs.hex)"""
        nbytes = 132 + 32 * self.g1.n
        cap = 2 * nbytes if as_hex else nbytes
        buf = C.create_string_buffer(cap)
        n = C.c_size_t(0)
        check(lib().zk_bn254_kzg_srs_write(self.g1.handle, vp(np.ascontiguousarray(self.g2, dtype=np.uint64)), C.c_int(int(as_hex)), buf, C.c_size_t(cap), C.byref(n)))
        return buf.raw[:n.value]

    def free(self):
        self.g1.free()


def _check_open(rc: int) -> None:
    """ZK_ERR_LEN is upstream's ErrInvalidPolynomialSize: a ValueError, like SRS.commit's length errors"""
    if rc == _lib.ZK_ERR_LEN:
        raise ValueError((lib().zk_last_error() or b"").decode())
    check(rc)


def _opening(h, claimed) -> np.ndarray:
    o = np.zeros(12, np.uint64)
    o[:8], o[8:] = np.asarray(h, np.uint64).reshape(8), np.asarray(claimed, np.uint64).reshape(4)
    return o


def verify(digest, h, claimed, point, g2) -> bool:
    """kzg.Verify(digest, proof{H, ClaimedValue}, point, srs) on the host: e(C - v G + z H, [1]2) e(-H, [alpha]2) == 1; g2 = SRS.g2."""
    ok = C.c_int(0)
    check(lib().zk_bn254_kzg_verify(vp(np.ascontiguousarray(digest, dtype=np.uint64)), vp(_opening(h, claimed)), vp(np.ascontiguousarray(point, dtype=np.uint64)),
                                    vp(np.ascontiguousarray(g2, dtype=np.uint64)), C.byref(ok)))
    return bool(ok.value)


def fold_proof(digests, h, claimed, point):
    """kzg.FoldProof(digests, batchOpeningProof{H, ClaimedValues}, point, sha256) -> ((H, folded claimed value), folded digest)."""
    d = np.ascontiguousarray(digests, dtype=np.uint64).reshape(-1, 8)
    v = np.ascontiguousarray(claimed, dtype=np.uint64).reshape(-1, 4)
    if d.shape[0] != v.shape[0]:
        raise ValueError("kzg: number of digests differs from the number of claimed values")
    o, fd = np.zeros(12, np.uint64), np.zeros(8, np.uint64)
    check(lib().zk_bn254_kzg_fold_proof(vp(d), C.c_size_t(d.shape[0]), vp(np.ascontiguousarray(h, dtype=np.uint64)), vp(v),
                                        vp(np.ascontiguousarray(point, dtype=np.uint64)), vp(o), vp(fd)))
    return (o[:8].copy(), o[8:].copy()), fd


def batch_verify_single_point(digests, h, claimed, point, g2) -> bool:
    """kzg.BatchVerifySinglePoint on the host: fold, then verify."""
    d = np.ascontiguousarray(digests, dtype=np.uint64).reshape(-1, 8)
    v = np.ascontiguousarray(claimed, dtype=np.uint64).reshape(-1, 4)
    if d.shape[0] != v.shape[0]:
        raise ValueError("kzg: number of digests differs from the number of claimed values")
    ok = C.c_int(0)
    check(lib().zk_bn254_kzg_batch_verify_single_point(vp(d), C.c_size_t(d.shape[0]), vp(np.ascontiguousarray(h, dtype=np.uint64)), vp(v),
                                                       vp(np.ascontiguousarray(point, dtype=np.uint64)), vp(np.ascontiguousarray(g2, dtype=np.uint64)), C.byref(ok)))
    return bool(ok.value)


def batch_verify_multi_points(digests, hs, claimed, points, g2) -> np.ndarray:
    """kzg.BatchVerifyMultiPoints on the device with a verdict per opening: digests (n, 8), hs (n, 8), claimed (n, 4), points (n, 4) -> (n,) uint8."""
    d = np.ascontiguousarray(digests, dtype=np.uint64).reshape(-1, 8)
    n = d.shape[0]
    o = np.zeros((n, 12), np.uint64)
    o[:, :8], o[:, 8:] = np.asarray(hs, np.uint64).reshape(n, 8), np.asarray(claimed, np.uint64).reshape(n, 4)
    z = np.ascontiguousarray(points, dtype=np.uint64).reshape(n, 4)
    acc, cnt = np.zeros(max(n, 1), np.uint8), C.c_size_t(0)
    check(lib().zk_bn254_kzg_verify_batch(vp(d), vp(o), vp(z), C.c_size_t(n), vp(np.ascontiguousarray(g2, dtype=np.uint64)), vp(acc), C.byref(cnt)))
    return acc[:n]


def hscan_inspect(rows, K: int, nb: int = 0, mode: str = "divide", pad: int = 4, poison=None) -> dict:
    """The Horner suffix scan under the openings and the PLONK prover, alone (zk_bn254_hscan_inspect; for tests): the production launcher over up to eight host
    rows with the caller's K (and nb, 0 = what the longest row needs), every stage copied back.
    rows: (f, a) pairs -- f (len, 4) Montgomery coefficients, a (4,) the point; the SAME array object twice is one device array.  mode: "divide" (the quotient
    into a buffer of its own), "in_place" (over f) or "eval" (two launches, no quotient).  Every row gets `pad` guard elements either side and every output
    array starts as `poison` (4 limbs), so that what no kernel wrote shows.
    Returns nb, tcarry (rows, nb, 256, 4), btot_local / btot (rows, nb, 4): the workgroup totals after pass 1 / pass 2, total (rows, 4), and per row f and q as
    they came back, guards included ((pad + len + pad, 4) each; in place q is f)."""
    if mode not in ("divide", "in_place", "eval"):
        raise ValueError("mode: divide, in_place or eval")
    poison = np.full(4, 0xDEADBEEFCAFEF00D, np.uint64) if poison is None else np.asarray(poison, np.uint64).reshape(4)
    req, res = _lib.HscanRequest(), _lib.HscanResult()
    req.rows, req.K, req.nb, req.pad, req.eval_only = len(rows), K, nb, pad, int(mode == "eval")
    fs, qs, padded = [], [], {}
    for k, (f, a) in enumerate(rows[:_lib.HSCAN_ROWS_MAX]):
        c = np.ascontiguousarray(f, dtype=np.uint64).reshape(-1, 4)
        if id(f) not in padded:
            padded[id(f)] = np.concatenate([np.tile(poison, (pad, 1)), c, np.tile(poison, (pad, 1))])
        fs.append(padded[id(f)])
        qs.append(fs[k] if mode == "in_place" else np.tile(poison, (c.shape[0] + 2 * pad, 1)))
        req.f[k], req.q[k], req.len[k] = fs[k].ctypes.data, qs[k].ctypes.data, c.shape[0]
        req.a[k][:] = [int(x) for x in np.asarray(a, np.uint64).reshape(4)]
    # the geometry the entry will use (csrc/scan.hpp scan_blocks); arguments it refuses get arrays of one workgroup, which it never touches
    longest = max([int(n) for n in req.len[:len(fs)]] + [1])
    n, used = len(rows), max(nb, ((longest + K - 1) // K + 255) // 256) if K >= 1 else 1
    out = dict(nb=used, tcarry=np.tile(poison, (n, used, 256, 1)), btot_local=np.tile(poison, (n, used, 1)), btot=np.tile(poison, (n, used, 1)),
               total=np.tile(poison, (n, 1)))
    for key in ("tcarry", "btot_local", "btot", "total"):
        setattr(res, key, out[key].ctypes.data)
    check(lib().zk_bn254_hscan_inspect(C.byref(req), C.byref(res)))
    if int(res.nb) != used:
        raise RuntimeError("scan inspection ran %d workgroups a row, %d were expected" % (res.nb, used))
    out["f"], out["q"] = fs, qs
    return out


def new_srs(size: int, alpha_mont, table_window_bits: int = 0) -> SRS:
    """kzg.NewSRS(size, alpha) on the device; alpha: Montgomery fr.Element (4 limbs)."""
    d = _lib.DeviceBuffer(max(size, 1) * 64)
    g2 = np.zeros((2, 16), np.uint64)
    check(lib().zk_bn254_kzg_new_srs_dev(C.c_void_p(d.ptr), C.c_size_t(size), vp(np.ascontiguousarray(alpha_mont, dtype=np.uint64)), vp(g2), None))
    rb = ResidentBases(d, n=size, table_window_bits=table_window_bits)
    d.free()
    return SRS(rb, g2)


def read_srs(data: bytes | str, is_hex: bool = False, table_window_bits: int = 0) -> SRS:
    """(*SRS).ReadFrom: bytes of WriteTo (or their hex text)."""
    raw = data.encode("ascii") if isinstance(data, str) else bytes(data)
    h, n = C.c_uint64(0), C.c_size_t(0)
    g2 = np.zeros((2, 16), np.uint64)
    rc = lib().zk_bn254_kzg_srs_read(C.c_char_p(raw), C.c_size_t(len(raw)), C.c_int(int(is_hex)), C.c_int(table_window_bits), C.byref(h), C.byref(n), vp(g2))
    if rc in (_lib.ZK_ERR_LEN, _lib.ZK_ERR_ARG):
        raise ValueError((lib().zk_last_error() or b"").decode())
    check(rc)
    rb = ResidentBases.__new__(ResidentBases)
    rb.is_g2, rb.handle, rb.n = False, h, int(n.value)
    return SRS(rb, g2)


def read_srs_g2(data: bytes | str, is_hex: bool = False) -> np.ndarray:
    """The two G2 points of an SRS image ([1]2, [alpha]2), decoded on the HOST (zk_bn254_kzg_srs_g2): all that plonk.Verify needs of the SRS; no device is touched."""
    raw = data.encode("ascii") if isinstance(data, str) else bytes(data)
    g2 = np.zeros((2, 16), np.uint64)
    rc = lib().zk_bn254_kzg_srs_g2(C.c_char_p(raw), C.c_size_t(len(raw)), C.c_int(int(is_hex)), vp(g2))
    if rc in (_lib.ZK_ERR_LEN, _lib.ZK_ERR_ARG):
        raise ValueError((lib().zk_last_error() or b"").decode())
    check(rc)
    return g2
