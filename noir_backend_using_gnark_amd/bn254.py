"""Host-side mirror of the gnark-crypto v0.9.1 interface for the hot path (names and argument meaning follow upstream;
pinned at /root/reference/gnark_backend_ffi/go.mod:5 and reached through groth16.Prove main.go:131 / plonk.Prove
backend/plonk/plonk.go:67):

    ecc.MultiExpConfig{NbTasks, ScalarsMont}      -> MultiExpConfig
    (*G1Jac).MultiExp(points, scalars, config)    -> g1_multi_exp(points, scalars, config)   (affine result)
    (*G2Jac).MultiExp                             -> g2_multi_exp
    fft.NewDomain(m); (*Domain).FFT / FFTInverse  -> Domain(m).fft / .fft_inverse (in place, returns the array)
    fft.BitReverse                                -> bit_reverse
    fft.DIT / fft.DIF                             -> DIT / DIF

Containers are numpy uint64 arrays holding gnark's memory images: fr.Vector (n, 4); []G1Affine (n, 8);
[]G2Affine (n, 16) -- or `_lib.DeviceBuffer` / raw device pointers for data already resident in HBM.
Everything here dispatches to libzkmi.so; nothing is computed on the host."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._lib import MsmCfg, check, lib, vp

DIT, DIF = 0, 1


@dataclass
class MultiExpConfig:
    nb_tasks: int = 0          # upstream NbTasks; > 1024 is an error like upstream, otherwise ignored on the GPU
    scalars_mont: bool = False  # upstream's zero value: scalars in regular form (gnark v0.8.0 calls FromMont() before MultiExp); True = Montgomery images
    window_bits: int = 0       # 0 = auto
    device_mask: int = 0       # several GPUs in one process (zk_init_devices): bit i = device entry i; 0 = the process default

    def _c(self) -> MsmCfg:
        return MsmCfg(self.nb_tasks, 1 if self.scalars_mont else 0, self.window_bits, self.device_mask)


def _as_u64(a, width) -> np.ndarray:
    a = np.ascontiguousarray(a, dtype=np.uint64)
    if a.size % width:
        raise ValueError("array size %d is not a multiple of %d limbs" % (a.size, width))
    return a.reshape(-1, width)


def _multi_exp(fn, width, points, scalars, config):
    config = config or MultiExpConfig()
    points, scalars = _as_u64(points, width), _as_u64(scalars, 4)
    if points.shape[0] != scalars.shape[0]:
        # upstream: errors.New("len(points) != len(scalars)") -- raised by the library, not here, so that the C ABI is what is tested
        pass
    out = np.zeros(width, dtype=np.uint64)
    cfg = config._c()
    rc = fn(vp(points), C.c_size_t(points.shape[0]), vp(scalars), C.c_size_t(scalars.shape[0]), C.byref(cfg), vp(out))
    if rc in (_lib.ZK_ERR_LEN, _lib.ZK_ERR_NB_TASKS):
        raise ValueError((lib().zk_last_error() or b"").decode())
    check(rc)
    return out


def g1_multi_exp(points, scalars, config: MultiExpConfig | None = None) -> np.ndarray:
    """sum_i scalars[i] * points[i] on G1; returns the G1Affine image (8 limbs)."""
    return _multi_exp(lib().zk_bn254_g1_msm, 8, points, scalars, config)


def g2_multi_exp(points, scalars, config: MultiExpConfig | None = None) -> np.ndarray:
    """sum_i scalars[i] * points[i] on G2; returns the G2Affine image (16 limbs)."""
    return _multi_exp(lib().zk_bn254_g2_msm, 16, points, scalars, config)


def g1_multi_exp_dev(d_points: int, d_scalars: int, n: int, config: MultiExpConfig | None = None, stream: int = 0, partial=False):
    """Device-pointer variant (inputs resident in HBM).  partial=True returns the un-normalised XYZZ sum (16 limbs)."""
    cfg = (config or MultiExpConfig())._c()
    out = np.zeros(16 if partial else 8, dtype=np.uint64)
    fn = lib().zk_bn254_g1_msm_partial_dev if partial else lib().zk_bn254_g1_msm_dev
    check(fn(C.c_void_p(d_points), C.c_void_p(d_scalars), C.c_size_t(n), C.byref(cfg), vp(out), C.c_void_p(stream)))
    return out


def g2_multi_exp_dev(d_points: int, d_scalars: int, n: int, config: MultiExpConfig | None = None, stream: int = 0, partial=False):
    cfg = (config or MultiExpConfig())._c()
    out = np.zeros(32 if partial else 16, dtype=np.uint64)
    fn = lib().zk_bn254_g2_msm_partial_dev if partial else lib().zk_bn254_g2_msm_dev
    check(fn(C.c_void_p(d_points), C.c_void_p(d_scalars), C.c_size_t(n), C.byref(cfg), vp(out), C.c_void_p(stream)))
    return out


def g1_sum_partials(partials) -> np.ndarray:
    """Combine XYZZ partial sums (k, 16) from range-sharded MSMs into one affine point (host, O(k))."""
    p = _as_u64(partials, 16)
    out = np.zeros(8, dtype=np.uint64)
    check(lib().zk_bn254_g1_sum_xyzz(vp(p), C.c_size_t(p.shape[0]), vp(out)))
    return out


def g2_sum_partials(partials) -> np.ndarray:
    p = _as_u64(partials, 32)
    out = np.zeros(16, dtype=np.uint64)
    check(lib().zk_bn254_g2_sum_xyzz(vp(p), C.c_size_t(p.shape[0]), vp(out)))
    return out


def _msm_prep_request(req, vectors, n, window_bits, scalars_mont, table_c, stride, row_first, row_step, rows, row_stride, drop_zero_digits):
    """fills a _lib.MsmPrepRequest; returns the arrays it points into (keep them alive across the call)"""
    if rows:
        mat = _as_u64(vectors, 4)
        row_stride = row_stride if row_stride is not None else mat.shape[0] // rows
        if n is None:
            n = row_stride
        if mat.shape[0] < (rows - 1) * row_stride + n:
            raise ValueError("the matrix is shorter than rows * row_stride")
        keep, sets = [mat], rows
    else:
        keep, seen = [], {}
        for v in (vectors if isinstance(vectors, (list, tuple)) else [vectors]):
            if id(v) not in seen:
                seen[id(v)] = _as_u64(v, 4)
            keep.append(seen[id(v)])
        sets = len(keep)
        if n is None:
            n = keep[0].shape[0]
        if any(k.shape[0] < n for k in keep):
            raise ValueError("a scalar vector is shorter than n")
    req.n, req.window_bits, req.scalars_mont, req.table, req.drop_zero_digits = n, window_bits, int(scalars_mont), int(table_c != 0), int(drop_zero_digits)
    req.c, req.row_first, req.row_step, req.sets, req.stride = table_c, row_first, row_step, sets, (stride if stride is not None else n)
    req.by_rows, req.row_stride = int(rows > 0), (row_stride or 0)
    for i, k in enumerate(keep[:3]):
        req.vec[i] = k.ctypes.data
    return keep


def _msm_prep_plan(res) -> dict:
    return dict({k: int(getattr(res, k)) for k in _lib.MSM_PREP_PLAN}, total=int(res.total), max_tasks=int(res.max_tasks))


def _msm_prep_arrays(res, plan, arrays) -> dict:
    sizes = dict(keys=plan["total"], vals=plan["total"], start=plan["nb"] + 1, task_off=plan["nb"] + 1, task_begin=plan["max_tasks"], len_keys=plan["max_tasks"],
                 task_ids=plan["max_tasks"], multi_list=plan["nb"])
    wanted = _lib.MSM_PREP_ARRAYS if arrays is None else tuple(arrays)
    out = {k: np.zeros(sizes[k] if k in wanted else 0, np.uint32) for k in _lib.MSM_PREP_ARRAYS}
    for k in wanted:
        setattr(res, k, out[k].ctypes.data)
    return out


def msm_prep_inspect(vectors, n: int | None = None, window_bits: int = 0, scalars_mont: bool = False, table_c: int = 0, stride: int | None = None,
                     row_first: int = 0, row_step: int = 1, rows: int = 0, row_stride: int | None = None, drop_zero_digits: bool = False,
                     plan_only: bool = False, arrays=None) -> dict:
    """The scalar-side half of an MSM alone (zk_bn254_msm_prep_inspect; for tests): the plan and, unless plan_only (host work, no device), the pair count as the
    device knows it, the control block and every intermediate array of the production preparation.
    vectors: one (n, 4) array (plain method, or one vector against a table of width table_c), a list of up to three of them (a batch by pointers; the same
    array object twice is the same device vector twice), or -- with rows > 0 -- one (rows, row_stride, 4) matrix whose rows' first n elements are the vectors.
    arrays: names of the arrays to copy back (default: all of _lib.MSM_PREP_ARRAYS; the others come back empty)."""
    req = _lib.MsmPrepRequest()
    keep = _msm_prep_request(req, vectors, n, window_bits, scalars_mont, table_c, stride, row_first, row_step, rows, row_stride, drop_zero_digits)  # noqa: F841
    res = _lib.MsmPrepResult()
    check(lib().zk_bn254_msm_prep_inspect(C.byref(req), C.byref(res)))
    out = _msm_prep_plan(res)
    if plan_only or out["total"] == 0:
        out.update(device_total=0, dropped=False, ctl=np.zeros(64, np.uint32), **{k: np.zeros(0, np.uint32) for k in _lib.MSM_PREP_ARRAYS})
        return out
    arrays = _msm_prep_arrays(res, out, arrays)
    check(lib().zk_bn254_msm_prep_inspect(C.byref(req), C.byref(res)))
    assert _msm_prep_plan(res) == out
    out.update(device_total=int(res.device_total), dropped=bool(res.dropped), ctl=np.array(res.ctl[:], dtype=np.uint32), **arrays)
    return out


def msm_tail_inspect(points, vectors, is_g2: bool = False, l1_m: int = 0, l2_m: int = 0, quad_tail: bool = False, keep_final: bool = False, skip_below: int = 0,
                     plan_only: bool = False, **prep) -> dict:
    """The base-side half of an MSM behind the production preparation (zk_bn254_msm_tail_inspect; for tests): window table, accumulate, folds, every reduction
    level and the finishers, with every intermediate array back as AFFINE points ((k, 8) uint64 on G1, (k, 16) on G2; (0, 0) = infinity).
    points: (n, 8) / (n, 16) affine bases; vectors and **prep: as for msm_prep_inspect (n, window_bits, scalars_mont, table_c, stride, row_first, row_step,
    rows, row_stride, drop_zero_digits).  Returns msm_prep_inspect's dictionary FROM THIS RUN plus m2, tasks, n_final, sh_final, levels (a list of dictionaries:
    kind 'l1' / 'l2' / 'wave' / 'wave_quad', n_in, n_out, sh_in, sh_out, m and, after a run, the level's A and S as (W, n_out, width)), table, partial_acc,
    partial_fold, and set_values / total (host finish) or final_affine / final_bytes (keep_final: the device finish).  plan_only: host work, no device."""
    width = 16 if is_g2 else 8
    pts = _as_u64(points, width)
    req = _lib.MsmTailRequest()
    keep = _msm_prep_request(req.prep, vectors, prep.pop("n", None), prep.pop("window_bits", 0), prep.pop("scalars_mont", False), prep.pop("table_c", 0),  # noqa: F841
                             prep.pop("stride", None), prep.pop("row_first", 0), prep.pop("row_step", 1), prep.pop("rows", 0), prep.pop("row_stride", None),
                             prep.pop("drop_zero_digits", False))
    if prep:
        raise TypeError("unknown arguments: %s" % sorted(prep))
    if pts.shape[0] < req.prep.n:
        raise ValueError("fewer points than scalars")
    req.points, req.is_g2, req.quad_tail, req.keep_final = pts.ctypes.data, int(is_g2), int(quad_tail), int(keep_final)
    req.l1_m, req.l2_m, req.skip_below = l1_m, l2_m, skip_below
    res = _lib.MsmTailResult()
    check(lib().zk_bn254_msm_tail_inspect(C.byref(req), C.byref(res)))

    def plan():
        d = _msm_prep_plan(res.prep)
        d.update({k: int(getattr(res, k)) for k in ("m2", "n_final", "sh_final", "table_entries", "level_entries")})
        d["levels"] = [dict({k: int(getattr(res.level[i], k)) for k in _lib.MSM_TAIL_LEVEL}, kind=_lib.MSM_TAIL_KINDS[int(res.level[i].kind)])
                       for i in range(res.n_levels)]
        return d
    out = plan()
    sets = int(req.prep.sets) if req.prep.table else 1
    if plan_only or (out["total"] == 0 and not keep_final):
        return out
    arrays = _msm_prep_arrays(res.prep, out, None) if out["total"] else {}
    W = out["W"]
    shapes = dict(table=(out["table_entries"], width), partial_acc=(out["max_tasks"], width), partial_fold=(out["max_tasks"], width),
                  level_a=(out["level_entries"], width), level_s=(out["level_entries"], width))
    if keep_final:
        shapes.update(final_affine=(sets, 8), final_bytes=(sets, 32))
    else:
        shapes.update(set_values=(W, width), total=(1, width))
    tail = {k: np.zeros(shp, np.uint8 if k == "final_bytes" else np.uint64) for k, shp in shapes.items()}
    for k, a in tail.items():
        setattr(res, k, a.ctypes.data)
    check(lib().zk_bn254_msm_tail_inspect(C.byref(req), C.byref(res)))
    assert plan() == out
    if out["total"]:
        out.update(device_total=int(res.prep.device_total), dropped=bool(res.prep.dropped), ctl=np.array(res.prep.ctl[:], dtype=np.uint32), **arrays)
    out["tasks"] = int(res.tasks)
    at = 0
    for lv in out["levels"]:
        cnt = W * lv["n_out"]
        lv["A"] = tail["level_a"][at:at + cnt].reshape(W, lv["n_out"], width)
        lv["S"] = tail["level_s"][at:at + cnt].reshape(W, lv["n_out"], width)
        at += cnt
    out.update({k: v for k, v in tail.items() if k not in ("level_a", "level_s")})
    return out


MSM_ROWS_SPARSE, MSM_ROWS_NO_POINTS = 1, 2
_DEV = (int, _lib.DeviceBuffer)


def _dptr(a) -> int:
    return a if isinstance(a, int) else a.ptr


def _check_len(rc: int) -> None:
    if rc in (_lib.ZK_ERR_LEN, _lib.ZK_ERR_NB_TASKS):
        raise ValueError((lib().zk_last_error() or b"").decode())
    check(rc)


def rows_digests(dev_call, host_call, scalars, n, rows, row_stride, out, compressed, points):
    """The argument rules of a row-batched commitment (ResidentBases.multi_exp_rows, plonk.commit_rows), checked before the library is called, and the call.
      dev_call(ptr, row_stride, n, rows, out_ptr, compressed_ptr) -> rc on device rows; host_call(array, n, rows, points or None, digests or None) -> rc on a
      host matrix (None: the matrix goes to the device and dev_call runs).
      host    scalars: C-contiguous (rows, n, 4) uint64; n / rows / row_stride, when given, must agree with it; out belongs to the device form
              -> points (rows, 8) uint64, or (points, digests (rows, 32) uint8) with compressed=True, or the digests alone with points=False
      device  scalars: device buffer / pointer with n and rows, row v at element v * row_stride (default n); out: where the points go (rows x 64 bytes; made
              here when None); compressed: False, True (a buffer is made here) or the buffer for rows x 32 bytes; nothing written overlaps anything else
              -> out, or (out, compressed), or compressed alone with points=False"""
    if not isinstance(compressed, bool) and not isinstance(compressed, _DEV):
        raise TypeError("compressed must be False, True or a device buffer / pointer")
    if not points and compressed is False:
        raise ValueError("points=False leaves nothing to return: ask for the compressed digests")
    if not points and out is not None:
        raise ValueError("out takes the points: there are none with points=False")
    if isinstance(scalars, _DEV):
        if n is None or rows is None:
            raise ValueError("n and rows are required with device-resident scalars")
        n, rows = int(n), int(rows)
        if n < 0 or rows < 0:
            raise ValueError("n and rows must not be negative")
        row_stride = int(n if row_stride is None else row_stride)
        if row_stride < n and rows > 1:
            raise ValueError("row_stride = %d is below the n = %d scalars of a row" % (row_stride, n))
        span = ((rows - 1) * row_stride + n) * 32 if rows and n else 0
        if isinstance(scalars, _lib.DeviceBuffer) and span > scalars.nbytes:
            raise ValueError("scalars: %d bytes do not fit the device buffer (%d bytes)" % (span, scalars.nbytes))
        seen = [("scalars", scalars, span)]
        for name, b, nbytes in (("out", out, rows * 64), ("compressed", compressed, rows * 32)):
            if b is None or isinstance(b, bool):
                continue
            if not isinstance(b, _DEV):
                raise TypeError("%s must be a device buffer or a device pointer" % name)
            if isinstance(b, _lib.DeviceBuffer) and nbytes > b.nbytes:
                raise ValueError("%s: %d bytes do not fit the device buffer (%d bytes)" % (name, nbytes, b.nbytes))
            for other, c, cb in seen:
                if nbytes and cb and _dptr(b) < _dptr(c) + cb and _dptr(c) < _dptr(b) + nbytes:
                    raise ValueError("%s overlaps %s" % (name, other))
            seen.append((name, b, nbytes))
        made = []
        if points and out is None:
            out = _lib.DeviceBuffer(max(rows * 64, 64))
            made.append(out)
        if compressed is True:
            compressed = _lib.DeviceBuffer(max(rows * 32, 32))
            made.append(compressed)
        enc = None if compressed is False else compressed
        if rows:
            try:
                _check_len(dev_call(_dptr(scalars), row_stride, n, rows, _dptr(out) if points else 0, _dptr(enc) if enc is not None else 0))
            except Exception:
                for b in made:
                    b.free()
                raise
        return out if enc is None else ((out, enc) if points else enc)
    if not (isinstance(scalars, np.ndarray) and scalars.dtype == np.uint64 and scalars.flags["C_CONTIGUOUS"]):
        raise TypeError("scalars must be a C-contiguous uint64 numpy array (or a device buffer)")
    if scalars.ndim != 3 or scalars.shape[2] != 4:
        raise ValueError("scalars has shape %s, not (rows, n, 4)" % (scalars.shape,))
    cnt, width = scalars.shape[0], scalars.shape[1]
    for name, v, want in (("rows", rows, cnt), ("n", n, width), ("row_stride", row_stride, width)):
        if v is not None and int(v) != want:
            raise ValueError("%s = %d != %d of the host array (its rows are contiguous)" % (name, v, want))
    if out is not None or not isinstance(compressed, bool):
        raise ValueError("out and a compressed buffer belong to the device form: the host form returns new arrays")
    pts = np.zeros((cnt, 8), np.uint64) if points else None
    enc = np.zeros((cnt, 32), np.uint8) if compressed else None
    if cnt and host_call is not None:
        _check_len(host_call(scalars, width, cnt, pts, enc))
    elif cnt:
        bufs = [_lib.DeviceBuffer.from_numpy(scalars), _lib.DeviceBuffer(cnt * 64), _lib.DeviceBuffer(cnt * 32)]
        try:
            _check_len(dev_call(bufs[0].ptr, width, width, cnt, bufs[1].ptr if points else 0, bufs[2].ptr if compressed else 0))
            pts = bufs[1].to_numpy(np.uint64, (cnt, 8)) if points else None
            enc = bufs[2].to_numpy(np.uint8, (cnt, 32)) if compressed else None
        finally:
            for b in bufs:
                b.free()
    return pts if enc is None else ((pts, enc) if points else enc)


def msm_rows_info(bases: "ResidentBases", n: int, sparse: bool = False) -> dict:
    """zk_bn254_msm_rows_info: {"chunk_rows": rows per launch set of multi_exp_rows at n scalars per row, "batched": whether the batched path serves these bases}"""
    chunk, batched = C.c_size_t(0), C.c_int(0)
    _check_len(lib().zk_bn254_msm_rows_info(bases.handle, C.c_size_t(n), C.c_uint32(MSM_ROWS_SPARSE if sparse else 0), C.byref(chunk), C.byref(batched)))
    return {"chunk_rows": int(chunk.value), "batched": bool(batched.value)}


class ResidentBases:
    """pk / SRS bases kept in HBM across calls (zk_bn254_bases_register)."""

    def __init__(self, points, is_g2: bool = False, n: int | None = None, table_window_bits: int = 0):
        """points: gnark memory images (numpy) -- or a DeviceBuffer / raw device pointer together with `n` (bases already in HBM).
        table_window_bits: 0 = the planner decides (window tables for >= 4096 bases), -1 = none, else the tables' window width."""
        self.is_g2, self.handle = is_g2, C.c_uint64(0)
        if isinstance(points, (_lib.DeviceBuffer, int)):
            if n is None:
                raise ValueError("n is required with device-resident points")
            self.n = n
            ptr = points.ptr if isinstance(points, _lib.DeviceBuffer) else int(points)
            check(lib().zk_bn254_bases_register_cfg(C.c_void_p(ptr), C.c_size_t(n), C.c_int(int(is_g2)), C.c_int(1), C.c_int(table_window_bits), C.byref(self.handle)))
            return
        points = _as_u64(points, 16 if is_g2 else 8)
        self.n = points.shape[0]
        check(lib().zk_bn254_bases_register_cfg(vp(points), C.c_size_t(self.n), C.c_int(int(is_g2)), C.c_int(0), C.c_int(table_window_bits), C.byref(self.handle)))

    def multi_exp_dev(self, d_scalars, n: int, config: MultiExpConfig | None = None, offset: int = 0) -> np.ndarray:
        """kzg.Commit of a polynomial that already lives in HBM (DeviceBuffer or raw device pointer)."""
        out = np.zeros(16 if self.is_g2 else 8, dtype=np.uint64)
        cfg = (config or MultiExpConfig())._c()
        ptr = d_scalars.ptr if isinstance(d_scalars, _lib.DeviceBuffer) else int(d_scalars)
        rc = lib().zk_bn254_msm_bases_dev(self.handle, C.c_size_t(offset), C.c_void_p(ptr), C.c_size_t(n), C.byref(cfg), vp(out))
        if rc in (_lib.ZK_ERR_LEN, _lib.ZK_ERR_NB_TASKS):
            raise ValueError((lib().zk_last_error() or b"").decode())
        check(rc)
        return out

    def multi_exp(self, scalars, config: MultiExpConfig | None = None, offset: int = 0) -> np.ndarray:
        scalars = _as_u64(scalars, 4)
        out = np.zeros(16 if self.is_g2 else 8, dtype=np.uint64)
        cfg = (config or MultiExpConfig())._c()
        rc = lib().zk_bn254_msm_bases(self.handle, C.c_size_t(offset), vp(scalars), C.c_size_t(scalars.shape[0]), C.byref(cfg), vp(out))
        if rc in (_lib.ZK_ERR_LEN, _lib.ZK_ERR_NB_TASKS):
            raise ValueError((lib().zk_last_error() or b"").decode())
        check(rc)
        return out

    def lagrange(self, log_n: int) -> "ResidentBases":
        """The Lagrange form of these G1 bases over the domain of 2^log_n points (zk_bn254_bases_lagrange): 2^log_n + 2 bases of their own."""
        rb = ResidentBases.__new__(ResidentBases)
        rb.is_g2, rb.handle, rb.n = False, C.c_uint64(0), (1 << log_n) + 2
        check(lib().zk_bn254_bases_lagrange(self.handle, C.c_uint32(log_n), C.byref(rb.handle)))
        return rb

    @staticmethod
    def lagrange_inspect(points, log_n: int) -> dict:
        """The transform under lagrange(), alone and stage by stage (zk_bn254_lagrange_inspect; for tests): host G1 points (at least 2^log_n + 2, gnark's images)
        through the production builder with a trace.  Returns stages (log_n + 1, n, 8): the work array after the scale-in and after every stage, in the device's
        order, every entry normalised to its affine image; stage_inf (log_n + 1, n): 1 where the entry is the point at infinity (a flag of its own: the image is
        then zeros, and zeros under a flag of 0 are a wrong point); final (n + 2, 8) and final_inf (n + 2,): the points the finish wrote."""
        points = _as_u64(points, 8)
        n = 1 << log_n if 0 <= log_n < 32 else 1
        fits = 0 <= log_n <= 27 and points.shape[0] >= n + 2   # arguments the entry refuses get arrays of one point, which it never touches
        k, m = (log_n + 1, n) if fits else (1, 1)
        out = dict(stages=np.zeros((k, m, 8), np.uint64), stage_inf=np.full((k, m), 0xEE, np.uint8), final=np.zeros((m + 2, 8), np.uint64),
                   final_inf=np.full(m + 2, 0xEE, np.uint8))
        req, res = _lib.LagrangeRequest(), _lib.LagrangeResult()
        req.points, req.n_points, req.log_n = points.ctypes.data, points.shape[0], log_n & 0xFFFFFFFF
        res.stage_points, res.stage_inf, res.final_points, res.final_inf = (out[key].ctypes.data for key in ("stages", "stage_inf", "final", "final_inf"))
        check(lib().zk_bn254_lagrange_inspect(C.byref(req), C.byref(res)))
        return out

    def build_table(self, table_window_bits: int = 0) -> None:
        """Window tables for bases registered without them (zk_bn254_bases_build_table); a no-op when they exist."""
        check(lib().zk_bn254_bases_build_table(self.handle, C.c_int(table_window_bits)))

    def multi_exp_batch(self, vectors, n: int | None = None, config: MultiExpConfig | None = None, offset: int = 0) -> np.ndarray:
        """Several scalar vectors of one length against these bases in one call (zk_bn254_msm_bases_batch[_dev]): numpy (n, 4) arrays, or DeviceBuffers / raw
        device pointers together with n.  Returns (len(vectors), 8 or 16) affine points -- the same as one multi_exp per vector."""
        cnt = len(vectors)
        out = np.zeros((cnt, 16 if self.is_g2 else 8), dtype=np.uint64)
        cfg = (config or MultiExpConfig())._c()
        on_dev = cnt > 0 and isinstance(vectors[0], (_lib.DeviceBuffer, int))
        if on_dev:
            if n is None:
                raise ValueError("n is required with device-resident scalars")
            ptrs = (C.c_void_p * cnt)(*[v.ptr if isinstance(v, _lib.DeviceBuffer) else int(v) for v in vectors])
            rc = lib().zk_bn254_msm_bases_batch_dev(self.handle, C.c_size_t(offset), ptrs, C.c_uint32(cnt), C.c_size_t(n), C.byref(cfg), vp(out))
        else:
            keep = [_as_u64(v, 4) for v in vectors]
            if any(k.shape[0] != keep[0].shape[0] for k in keep):
                raise ValueError("the scalar vectors of one batch have one length")
            ptrs = (C.c_void_p * cnt)(*[k.ctypes.data for k in keep])
            rc = lib().zk_bn254_msm_bases_batch(self.handle, C.c_size_t(offset), ptrs, C.c_uint32(cnt), C.c_size_t(keep[0].shape[0] if cnt else 0), C.byref(cfg), vp(out))
        if rc in (_lib.ZK_ERR_LEN, _lib.ZK_ERR_NB_TASKS):
            raise ValueError((lib().zk_last_error() or b"").decode())
        check(rc)
        return out

    def multi_exp_rows(self, scalars, *, n: int | None = None, rows: int | None = None, row_stride: int | None = None, offset: int = 0, sparse: bool = False,
                       out=None, compressed=False, points: bool = True, config: MultiExpConfig | None = None):
        """kzg.Commit for many polynomials at once (zk_bn254_msm_bases_rows[_dev]; include/zkmi.h says the rest): the rows of one matrix against
        bases[offset : offset + n], one launch set per chunk of rows, points and / or their 32-byte G1Affine.Bytes() encodings.  Row v is multi_exp_dev's point
        for that row, byte for byte.  sparse: the scalars are wire-like (zero digits dropped before the sort; same result).  rows_digests says what the two
        forms (host matrix / device rows) take and return; every shape / dtype / stride / overlap error is raised before the library is called."""
        cfg = (config or MultiExpConfig())._c()
        flags = C.c_uint32((MSM_ROWS_SPARSE if sparse else 0) | (0 if points else MSM_ROWS_NO_POINTS))
        if int(offset) < 0:
            raise ValueError("offset must not be negative")

        def dev(ptr, stride, n_, rows_, o, c):
            return lib().zk_bn254_msm_bases_rows_dev(self.handle, C.c_size_t(offset), C.c_void_p(ptr), C.c_size_t(stride), C.c_size_t(n_), C.c_size_t(rows_), C.byref(cfg),
                                                     flags, C.c_void_p(o), C.c_void_p(c))

        def host(a, n_, rows_, o, c):
            return lib().zk_bn254_msm_bases_rows(self.handle, C.c_size_t(offset), vp(a), C.c_size_t(n_), C.c_size_t(rows_), C.byref(cfg), flags, vp(o), vp(c))

        return rows_digests(dev, host, scalars, n, rows, row_stride, out, compressed, points)

    def multi_exp_prepared(self, scalars: "PreparedScalars", skip: int = 0, offset: int = 0, config: MultiExpConfig | None = None) -> np.ndarray:
        """sum_{i >= skip} scalars[i] * bases[offset + i - skip] against scalars that were uploaded and are recoded once (zk_bn254_msm_bases_prepared)."""
        out = np.zeros(16 if self.is_g2 else 8, dtype=np.uint64)
        cfg = (config or MultiExpConfig())._c()
        rc = lib().zk_bn254_msm_bases_prepared(self.handle, C.c_size_t(offset), scalars.handle, C.c_size_t(skip), C.byref(cfg), vp(out))
        if rc in (_lib.ZK_ERR_LEN, _lib.ZK_ERR_NB_TASKS):
            raise ValueError((lib().zk_last_error() or b"").decode())
        check(rc)
        return out

    def free(self):
        if self.handle.value:
            lib().zk_bn254_bases_free(self.handle)
            self.handle = C.c_uint64(0)


class PreparedScalars:
    """A scalar vector uploaded once and recoded once per table geometry (zk_bn254_scalars_register): what groth16.Prove's A, B1, K and G2.B MultiExp calls share."""

    def __init__(self, scalars, config: MultiExpConfig | None = None):
        scalars = _as_u64(scalars, 4)
        self.n, self.handle = scalars.shape[0], C.c_uint64(0)
        cfg = (config or MultiExpConfig())._c()
        check(lib().zk_bn254_scalars_register(vp(scalars), C.c_size_t(self.n), C.byref(cfg), C.byref(self.handle)))

    def free(self):
        if self.handle.value:
            lib().zk_bn254_scalars_free(self.handle)
            self.handle = C.c_uint64(0)


class Domain:
    """fft.NewDomain(m): Cardinality = next power of two >= m.  The generator / coset / twiddle tables live on the device
    (built lazily per size by the library)."""

    def __init__(self, m: int):
        n = 1
        while n < m:
            n <<= 1
        self.cardinality = n
        self.log_n = n.bit_length() - 1
        if self.log_n > 28:
            raise ValueError("domain size 2^%d exceeds the Fr two-adicity 2^28" % self.log_n)

    def _run(self, a, inverse, decimation, coset):
        if decimation not in (DIT, DIF):
            raise ValueError("decimation must be DIT or DIF")
        if isinstance(a, (int, _lib.DeviceBuffer)):
            ptr = a if isinstance(a, int) else a.ptr
            check(lib().zk_bn254_ntt_dev(C.c_void_p(ptr), C.c_uint32(self.log_n), C.c_int(int(inverse)), C.c_int(decimation),
                                         C.c_int(int(bool(coset))), C.c_void_p(0)))
            return a
        if not (isinstance(a, np.ndarray) and a.dtype == np.uint64 and a.flags["C_CONTIGUOUS"]):
            raise TypeError("in-place transform needs a C-contiguous uint64 numpy array (or a device buffer)")
        if a.size != 4 * self.cardinality:
            raise ValueError("len(a) = %d != domain cardinality %d" % (a.size // 4, self.cardinality))
        check(lib().zk_bn254_ntt(vp(a), C.c_uint32(self.log_n), C.c_int(int(inverse)), C.c_int(decimation), C.c_int(int(bool(coset)))))
        return a

    def _run_batch(self, a, inverse, decimation, coset, rows, row_stride):
        """`rows` vectors of this domain in one launch per pass (zk_bn254_ntt_batch[_dev]); every shape / dtype / stride error is raised before the library is called"""
        if decimation not in (DIT, DIF):
            raise ValueError("decimation must be DIT or DIF")
        n = self.cardinality
        if isinstance(a, (int, _lib.DeviceBuffer)):
            if rows is None:
                raise ValueError("rows is required with device-resident data")
            rows, row_stride = int(rows), int(n if row_stride is None else row_stride)
            if rows < 0:
                raise ValueError("rows must not be negative")
            if row_stride < n:
                raise ValueError("row_stride = %d is below the domain cardinality %d" % (row_stride, n))
            if isinstance(a, _lib.DeviceBuffer) and rows and ((rows - 1) * row_stride + n) * 32 > a.nbytes:
                raise ValueError("%d rows at stride %d do not fit the device buffer (%d bytes)" % (rows, row_stride, a.nbytes))
            ptr = a if isinstance(a, int) else a.ptr
            check(lib().zk_bn254_ntt_batch_dev(C.c_void_p(ptr), C.c_uint32(self.log_n), C.c_size_t(rows), C.c_size_t(row_stride), C.c_int(int(inverse)),
                                               C.c_int(decimation), C.c_int(int(bool(coset))), C.c_void_p(0)))
            return a
        if not (isinstance(a, np.ndarray) and a.dtype == np.uint64 and a.flags["C_CONTIGUOUS"]):
            raise TypeError("in-place transform needs a C-contiguous uint64 numpy array (or a device buffer)")
        if a.ndim != 3 or a.shape[1:] != (n, 4):
            raise ValueError("a has shape %s, not (rows, %d, 4)" % (a.shape, n))
        if rows is not None and int(rows) != a.shape[0]:
            raise ValueError("rows = %d != %d rows of the array" % (rows, a.shape[0]))
        if row_stride is not None and int(row_stride) != n:
            raise ValueError("the rows of a host array are contiguous: row_stride must be %d" % n)
        check(lib().zk_bn254_ntt_batch(vp(a), C.c_uint32(self.log_n), C.c_size_t(a.shape[0]), C.c_int(int(inverse)), C.c_int(decimation), C.c_int(int(bool(coset)))))
        return a

    def fft_batch(self, a, decimation: int, coset: bool = False, rows: int | None = None, row_stride: int | None = None):
        """(*Domain).FFT on every row of a -- an (rows, N, 4) uint64 array, or a device buffer / pointer with `rows` rows `row_stride` elements apart (default N) --
        in place, one launch per pass for all rows.  Row i's result is fft's on that row."""
        return self._run_batch(a, False, decimation, coset, rows, row_stride)

    def fft_inverse_batch(self, a, decimation: int, coset: bool = False, rows: int | None = None, row_stride: int | None = None):
        """(*Domain).FFTInverse on every row of a, as fft_batch."""
        return self._run_batch(a, True, decimation, coset, rows, row_stride)

    def fft(self, a, decimation: int, coset: bool = False):
        """(*Domain).FFT(a, decimation, coset...) -- in place."""
        return self._run(a, False, decimation, coset)

    def fft_inverse(self, a, decimation: int, coset: bool = False):
        """(*Domain).FFTInverse(a, decimation, coset...) -- in place, includes the 1/N scaling."""
        return self._run(a, True, decimation, coset)


def bit_reverse(a):
    """fft.BitReverse(a) -- in place."""
    if not (isinstance(a, np.ndarray) and a.dtype == np.uint64 and a.flags["C_CONTIGUOUS"]):
        raise TypeError("needs a C-contiguous uint64 numpy array")
    n = a.size // 4
    log_n = n.bit_length() - 1
    if n == 0 or (1 << log_n) != n:
        raise ValueError("BitReverse needs a power-of-two length")
    check(lib().zk_bn254_bit_reverse(vp(a), C.c_uint32(log_n)))
    return a


def fr_batch_invert(a, n: int | None = None):
    """fr.BatchInvert(a): every element's inverse, zeros stay zeros (zk_bn254_fr_batch_invert_dev).  An (n, 4) uint64 array of Montgomery images gives a new
    array; a device buffer / pointer together with n is inverted in place and returned."""
    if isinstance(a, (int, _lib.DeviceBuffer)):
        if n is None:
            raise ValueError("n is required with device-resident data")
        n = int(n)
        if n < 0:
            raise ValueError("n must not be negative")
        if isinstance(a, _lib.DeviceBuffer) and n * 32 > a.nbytes:
            raise ValueError("%d elements do not fit the device buffer (%d bytes)" % (n, a.nbytes))
        check(lib().zk_bn254_fr_batch_invert_dev(C.c_void_p(a if isinstance(a, int) else a.ptr), C.c_size_t(n), C.c_void_p(0)))
        return a
    if not (isinstance(a, np.ndarray) and a.dtype == np.uint64 and a.flags["C_CONTIGUOUS"]):
        raise TypeError("needs a C-contiguous uint64 numpy array (or a device buffer)")
    if a.ndim != 2 or a.shape[1] != 4:
        raise ValueError("a has shape %s, not (n, 4)" % (a.shape,))
    if n is not None and int(n) != a.shape[0]:
        raise ValueError("n = %d != %d elements of the array" % (n, a.shape[0]))
    if a.shape[0] == 0:
        return a.copy()
    d = _lib.DeviceBuffer.from_numpy(a)
    try:
        check(lib().zk_bn254_fr_batch_invert_dev(C.c_void_p(d.ptr), C.c_size_t(a.shape[0]), C.c_void_p(0)))
        return d.to_numpy(np.uint64, a.shape)
    finally:
        d.free()


def rows_sha256(a, b=None, a_stride: int | None = None, b_stride: int | None = None, fill: int = 0) -> np.ndarray:
    """SHA-256(a_v || b_v) for every row v, one lane per row on the device (zk_bn254_rows_sha256_dev) -> (rows, 32) uint8.  a, b: (rows, len) uint8 arrays
    (either may be None or of length 0); they are staged a_stride / b_stride bytes apart (default: packed), the gaps filled with `fill`, which no digest sees."""
    a = np.zeros((0, 0), np.uint8) if a is None else np.ascontiguousarray(a, dtype=np.uint8)
    b = np.zeros((len(a), 0), np.uint8) if b is None else np.ascontiguousarray(b, dtype=np.uint8)
    if a.shape[1] == 0 and len(a) != len(b):
        a = np.zeros((len(b), 0), np.uint8)
    if len(a) != len(b):
        raise ValueError("as many rows of a as of b")
    rows = len(a)

    def stage(x, stride):
        stride = x.shape[1] if stride is None else stride
        if stride < x.shape[1]:
            raise ValueError("stride below a row")
        buf = np.full((max(rows, 1), max(stride, 1)), fill, np.uint8)
        buf[:rows, :x.shape[1]] = x
        return _lib.DeviceBuffer.from_numpy(buf), stride

    d_a, sa = stage(a, a_stride)
    d_b, sb = stage(b, b_stride)
    d_out = _lib.DeviceBuffer(max(rows, 1) * 32)
    check(lib().zk_bn254_rows_sha256_dev(d_a.ptr if a.shape[1] else None, a.shape[1], sa, d_b.ptr if b.shape[1] else None, b.shape[1], sb, rows, d_out.ptr, None))
    return d_out.to_numpy(np.uint8, (rows, 32))
