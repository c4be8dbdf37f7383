"""The row-batched openings (PLONK rounds 4 and 5) without a GPU: the expectation of the device tests (tests/plonk_open_ref.py) reproduces the oracle prover's
linearised polynomial, claimed values and opening commitments; the row with zeta = 1, where the oracle's inverse raises, is held to the division identity and to
lag = 0; poly_open_rows, ProvingKey.linearize_batch and ProvingKey.open_batch refuse wrong shapes, dtypes, strides, counts and overlap BEFORE the library is
called; include/zkmi.h declares the three entries, libzkmi.so exports them, they answer their argument errors (and rows = 0) before they look for a device, and
the mirrors in zkmi.hpp compile over them."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import noir_backend_using_gnark_amd as zk
from noir_backend_using_gnark_amd import _lib, bn254, plonk
from oracle import bn254_ref as ref
from oracle import plonk_ref as pl
from tests import plonk_open_ref as po
from tests import plonk_quotient_ref as qr
from tests import plonk_shapes as ps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = ref.R
FAMILIES = ("random", "max", "zeros+identity_perm")
NPUB = (0, 1, 33)
CASES = [(log_n, family, npub) for log_n in range(2, 7) for family in FAMILIES for npub in NPUB if npub < (1 << log_n)]

_srs = {}


def _srs_for(n):
    if n not in _srs:
        _srs[n] = pl.kzg_new_srs(n + 3, 0x5EED + n, fast=True)
    return _srs[n]


def _mul_x_minus_a(q, a, v):
    """q (X - a) + v"""
    f = [0] * (len(q) + 1)
    for i, c in enumerate(q):
        f[i + 1] = (f[i + 1] + c) % R
        f[i] = (f[i] - a * c) % R
    f[0] = (f[0] + v) % R
    return f


# ------------------------------------------------------------------------------------------------------- the restatement against the oracle
@pytest.mark.parametrize("log_n,family,npub", CASES)
def test_restatement_reproduces_the_oracle_provers_openings(log_n, family, npub):
    """the oracle's trace holds bl, br, bo, bz, h, the challenges and lin, its proof the claimed values, z(omega zeta) and the two opening commitments:
    linearize() and open_batch() on the trace's inputs give all of them"""
    n = 1 << log_n
    spr, sol = ps.circuit(family, n, npub, "full", 0x4B0 + 7 * log_n + npub)
    pk, _ = pl.plonk_setup(spr, _srs_for(n), fast=True)
    t = {}
    proof = pl.plonk_prove(pk, sol, ps.blinders("max" if family == "max" else "random", log_n), fast=True, trace=t)
    commit = lambda p: pl._Backend(True).msm_g1(pk["srs"]["g1"], p)
    got = po.linearize(pk, t["bl"], t["br"], t["bo"], t["bz"], t["h"], t["alpha"], t["beta"], t["gamma"], t["zeta"])
    assert got["lin"] == t["lin"] and len(got["lin"]) == n + 3
    assert got["values"][:7] == proof["claimed"] and got["values"][7] == proof["zu"]
    assert len(got["zquot"]) == n + 2 and commit(got["zquot"]) == proof["z_open_h"]
    assert len(got["fh"]) == n + 2 and commit(got["fh"]) == t["folded_h_digest"]
    q, value = po.open_batch(pk, got["fh"], got["lin"], t["bl"], t["br"], t["bo"], t["zeta"], t["kzg_gamma"])
    assert len(q) == n + 2 and commit(q) == proof["batch_h"]
    acc = 0
    for v in reversed(proof["claimed"]):
        acc = (acc * t["kzg_gamma"] + v) % R
    assert value == acc


@pytest.mark.parametrize("log_n,npub", [(2, 0), (3, 1), (6, 33)])
def test_pool_rows_cover_the_edge_challenges_and_the_zeta_one_row(log_n, npub):
    """zeta and kzg gamma of the pool's rows take 0, 1, omega, R - 1 and a random value each; every row's quotients satisfy q (X - a) + v = f; the row with
    zeta = 1 -- where the oracle's inv raises -- has lag = 0, the row with zeta = omega as well (zeta^n = 1) and its z is opened at omega^2"""
    n = 1 << log_n
    spr, n_in = qr.forward_circuit(n, npub, 0x51 + log_n)
    pk, _ = pl.plonk_setup(spr, _srs_for(n), fast=True)
    rows = [po.pool_row(pk, n_in, j, 0x90 + log_n) for j in range(po.POOL)]
    omega = pk["d0"].gen
    for k in ("zeta", "kzg_gamma"):
        vals = [r[k] for r in rows]
        assert {0, 1, omega, R - 1} <= set(vals) and len(set(vals)) == 5
    assert [r["violated"] for r in rows] == [0, 0, 1, 0, 0]
    for r in rows:
        assert _mul_x_minus_a(r["zquot"], r["zeta"] * omega % R, r["values"][7]) == r["bz"]
        assert _mul_x_minus_a(r["q"], r["zeta"], r["value"]) == po.fold7(pk, r["fh"], r["lin"], r["bl"], r["br"], r["bo"], r["kzg_gamma"])
        acc = 0
        for v in reversed(r["values"][:7]):
            acc = (acc * r["kzg_gamma"] + v) % R
        assert r["value"] == acc
        for p, v in ((r["fh"], r["values"][0]), (r["lin"], r["values"][1]), (r["bl"], r["values"][2]), (pk["s2"], r["values"][6])):
            assert pl.poly_eval(p, r["zeta"]) == v
    one, om = rows[1], rows[0]
    assert one["zeta"] == 1 and one["lag"] == 0 and om["zeta"] == omega and om["lag"] == 0 and rows[4]["lag"] != 0
    with pytest.raises(Exception):
        ref.inv(0, R)
    # without the lag term the zeta = 1 row's lin is the formula's: recomputed here with lag = 0 written out
    lz, rz, oz, s1z, s2z, zu = one["values"][2:]
    u, (al, be, ga) = pk["d0"].coset, (one[k] for k in ("alpha", "beta", "gamma"))
    c_s3 = (lz + be * s1z + ga) * (rz + be * s2z + ga) * zu * be % R
    c_z = -(lz + be + ga) * (rz + be * u + ga) * (oz + be * u * u + ga) % R
    for i in (0, n - 1, n, n + 2):
        v = one["bz"][i] * c_z * al
        if i < n:
            v += pk["s3"][i] * c_s3 * al + pk["qm"][i] * lz * rz + pk["ql"][i] * lz + pk["qr"][i] * rz + pk["qo"][i] * oz + pk["cqk"][i]
        assert one["lin"][i] == v % R
    f = [3, 1, 4, 1, 5, 9, 2, 6]
    assert po.open_at(f, 10) == (62951413, [6295141, 629514, 62951, 6295, 629, 62, 6]) and po.open_at([7], 5) == (7, [])


# ------------------------------------------------------------------------------------------------- refusals before the library
@pytest.fixture
def no_library(monkeypatch):
    """any call into the library fails the test"""
    def boom():
        raise AssertionError("the library was called")
    monkeypatch.setattr(bn254, "lib", boom)
    monkeypatch.setattr(plonk, "lib", boom)


def _nothing(nbytes, ptr):
    buf = _lib.DeviceBuffer.__new__(_lib.DeviceBuffer)      # a buffer that owns nothing: no device is needed to describe one
    buf.ptr, buf.nbytes = ptr, nbytes
    return buf


def _key(n=8, npub=2):
    return plonk.ProvingKey(0, None, dict(size=n, n_public=npub), 5)


def _bad_arrays(g):
    """(a wrong version of the (rows, width, 4) array g, the exception)"""
    return ((g.astype(np.int64), TypeError), (g.tolist(), TypeError), (np.zeros(g.shape[:2] + (8,), np.uint64)[:, :, ::2], TypeError), (g[:2], ValueError),
            (g[0], ValueError), (np.zeros(g.shape[:2] + (5,), np.uint64), ValueError))


def _bad_challenges(ch):
    return ((ch[:2], ValueError), (ch.reshape(-1), ValueError), (ch.astype(np.int64), TypeError), (ch.tolist(), TypeError))


def test_wrappers_reject_bad_host_arrays_before_the_library(no_library):
    pk = _key()
    w, z, h, ch = np.zeros((3, 10, 4), np.uint64), np.zeros((3, 11, 4), np.uint64), np.zeros((3, 30, 4), np.uint64), np.zeros((3, 4), np.uint64)
    good = dict(l=w, r=w, o=w, z=z, h=h, alpha=ch, beta=ch, gamma=ch, zeta=ch)
    lin = lambda **kw: pk.linearize_batch(**dict(good, **kw))
    for name in ("l", "r", "o", "z", "h"):
        for bad, exc in _bad_arrays(good[name]) + ((np.zeros((3, 9, 4), np.uint64), ValueError), (np.zeros((3, 12, 4), np.uint64), ValueError)):
            with pytest.raises(exc):
                lin(**{name: bad})
    for kw in (dict(z=w), dict(h=z), dict(rows=2), dict(in_stride=12), dict(h_stride=31), dict(out_stride=12), dict(out=[_nothing(64, 0)] * 4)):
        with pytest.raises(ValueError):
            lin(**kw)
    for name in ("alpha", "beta", "gamma", "zeta"):
        for bad, exc in _bad_challenges(ch):
            with pytest.raises(exc):
                lin(**{name: bad})
    good5 = dict(fh=w, lin=z, l=w, r=w, o=w, zeta=ch, kzg_gamma=ch)
    opn = lambda **kw: pk.open_batch(**dict(good5, **kw))
    for name in ("fh", "lin", "l", "r", "o"):
        for bad, exc in _bad_arrays(good5[name]) + ((np.zeros((3, 9, 4), np.uint64), ValueError), (np.zeros((3, 12, 4), np.uint64), ValueError)):
            with pytest.raises(exc):
                opn(**{name: bad})
    for kw in (dict(lin=w), dict(rows=4), dict(in_stride=10), dict(out_stride=11), dict(out=[_nothing(64, 0)] * 2)):
        with pytest.raises(ValueError):
            opn(**kw)
    for name in ("zeta", "kzg_gamma"):
        for bad, exc in _bad_challenges(ch):
            with pytest.raises(exc):
                opn(**{name: bad})
    for bad, exc in _bad_arrays(w) + ((np.zeros((3, 0, 4), np.uint64), ValueError),):
        with pytest.raises(exc):
            plonk.poly_open_rows(bad, ch)
    for bad, exc in _bad_challenges(ch):
        with pytest.raises(exc):
            plonk.poly_open_rows(w, bad)
    for kw in (dict(rows=2), dict(length=9), dict(in_stride=11), dict(q_stride=10), dict(out=_nothing(64, 0)), dict(values=_nothing(64, 0))):
        with pytest.raises(ValueError):
            plonk.poly_open_rows(w, ch, **kw)
    # no rows: answered without the library
    e = lambda *shape: np.zeros(shape, np.uint64)
    out = pk.linearize_batch(e(0, 10, 4), e(0, 10, 4), e(0, 10, 4), e(0, 11, 4), e(0, 30, 4), e(0, 4), e(0, 4), e(0, 4), e(0, 4))
    assert [a.shape for a in out] == [(0, 8, 4), (0, 10, 4), (0, 11, 4), (0, 10, 4)]
    q, value = pk.open_batch(e(0, 10, 4), e(0, 11, 4), e(0, 10, 4), e(0, 10, 4), e(0, 10, 4), e(0, 4), e(0, 4))
    assert q.shape == (0, 10, 4) and value.shape == (0, 4)
    values, q = zk.poly_open_rows(e(0, 6, 4), e(0, 4))
    assert values.shape == (0, 4) and q.shape == (0, 5, 4) and zk.poly_open_rows(e(0, 6, 4), e(0, 4), divide=False)[1] is None
    pk.handle = C.c_uint64(0)


def test_wrappers_reject_bad_device_geometry_before_the_library(no_library):
    pk = _key()
    n, rows, keep, mb = 8, 3, 30, 0x100000
    made = []

    def buf(elems, slot):
        made.append(_nothing(elems * 32, slot * mb))
        return made[-1]
    try:
        l, r, o, z = (buf(rows * (n + 3), k + 1) for k in range(4))
        h = buf(rows * keep, 5)
        alpha, beta, gamma, zeta = (buf(rows, 6 + k) for k in range(4))
        values, zquot, lin, fh = buf(rows * 8, 10), buf(rows * (n + 3), 11), buf(rows * (n + 3), 12), buf(rows * (n + 3), 13)
        good = dict(l=l, r=r, o=o, z=z, h=h, alpha=alpha, beta=beta, gamma=gamma, zeta=zeta, rows=rows, out=(values, zquot, lin, fh))
        call = lambda **kw: pk.linearize_batch(**dict(good, **kw))
        for kw in (dict(rows=None), dict(rows=-1), dict(rows=4), dict(in_stride=n + 2), dict(in_stride=n + 4), dict(h_stride=keep - 1), dict(h_stride=keep + 1),
                   dict(out_stride=n + 2), dict(out_stride=n + 4), dict(out=(l, zquot, lin, fh)), dict(out=(values, z, lin, fh)), dict(out=(values, zquot, h, fh)),
                   dict(out=(values, zquot, lin, zeta)), dict(out=(values, zquot, lin, lin)), dict(out=(values, zquot, lin, zquot.ptr + 32)),
                   dict(out=(values.ptr, values.ptr + 7 * 32, lin, fh)), dict(z=buf(rows * (n + 3) - 1, 4)), dict(h=buf(rows * keep - 1, 5)),
                   dict(zeta=buf(rows - 1, 9)), dict(out=(buf(rows * 8 - 1, 10), zquot, lin, fh)), dict(out=(values, zquot, buf(rows * (n + 3) - 1, 12), fh))):
            with pytest.raises(ValueError):
                call(**kw)
        for kw in (dict(o=np.zeros((rows, n + 2, 4), np.uint64)), dict(h=np.zeros((rows, keep, 4), np.uint64)), dict(zeta=np.zeros((rows, 4), np.uint64)),
                   dict(out=values), dict(out=(values, zquot, lin)), dict(out=(values, zquot, lin, np.zeros((rows, n + 2, 4), np.uint64))), dict(alpha=None)):
            with pytest.raises(TypeError):
                call(**kw)
        q, value, kg = buf((rows - 1) * (n + 2) + n + 2, 14), buf(rows, 15), buf(rows, 16)
        good5 = dict(fh=fh, lin=lin, l=l, r=r, o=o, zeta=zeta, kzg_gamma=kg, rows=rows, out=(q, value))
        call5 = lambda **kw: pk.open_batch(**dict(good5, **kw))
        for kw in (dict(rows=None), dict(rows=-1), dict(rows=4), dict(in_stride=n + 2), dict(in_stride=n + 4), dict(out_stride=n + 1), dict(out_stride=n + 3),
                   dict(out=(fh, value)), dict(out=(q, kg)), dict(out=(q, lin)), dict(out=(q, q.ptr + 32)), dict(out=(o.ptr + 64, value)),
                   dict(lin=buf(rows * (n + 3) - 1, 12)), dict(kzg_gamma=buf(rows - 1, 16)), dict(out=(q, buf(rows - 1, 15)))):
            with pytest.raises(ValueError):
                call5(**kw)
        for kw in (dict(lin=np.zeros((rows, n + 3, 4), np.uint64)), dict(kzg_gamma=np.zeros((rows, 4), np.uint64)), dict(out=q), dict(out=(q,)), dict(zeta=None)):
            with pytest.raises(TypeError):
                call5(**kw)
        f, pts, qq, vals = buf(rows * 12, 20), buf(rows, 21), buf(rows * 12, 22), buf(rows, 23)
        good1 = dict(f=f, points=pts, length=11, rows=rows, in_stride=12, q_stride=12, out=qq, values=vals)
        call1 = lambda **kw: plonk.poly_open_rows(**dict(good1, **kw))
        for kw in (dict(rows=None), dict(rows=-1), dict(rows=4), dict(length=None), dict(length=0), dict(length=13), dict(in_stride=10), dict(q_stride=9),
                   dict(out=f, q_stride=11), dict(out=f.ptr + 32), dict(out=pts), dict(out=vals), dict(values=f), dict(values=pts), dict(values=qq.ptr + 64),
                   dict(divide=False), dict(points=buf(rows - 1, 21)), dict(values=buf(rows - 1, 23)), dict(out=buf(2 * 12 + 9, 22))):
            with pytest.raises(ValueError):
                call1(**kw)
        for kw in (dict(points=np.zeros((rows, 4), np.uint64)), dict(out=np.zeros((rows, 10, 4), np.uint64)), dict(values=np.zeros((rows, 4), np.uint64)), dict(points=None)):
            with pytest.raises(TypeError):
                call1(**kw)
        # no rows: answered without the library, in all three
        assert call(rows=0) == (values, zquot, lin, fh) and call5(rows=0) == (q, value) and call1(rows=0) == (vals, qq) and call1(rows=0, out=f) == (vals, f)
    finally:
        for b in made:
            b.ptr = 0
    pk.handle = C.c_uint64(0)


# ------------------------------------------------------------------------------------------------------- header and exports
DECLS = (
    "int zk_bn254_fr_poly_open_rows_dev(const void *d_f, size_t in_stride, size_t len, size_t rows, const void *d_points, void *d_q, size_t q_stride, "
    "void *d_values, void *stream);",
    "int zk_bn254_plonk_linearize_batch_dev(uint64_t pk_handle, const void *d_l, const void *d_r, const void *d_o, const void *d_z, size_t in_stride, "
    "const void *d_h, size_t h_stride, size_t rows, const void *d_alpha, const void *d_beta, const void *d_gamma, const void *d_zeta, void *d_values, "
    "void *d_zquot, void *d_lin, void *d_fh, size_t out_stride, void *stream);",
    "int zk_bn254_plonk_open_batch_dev(uint64_t pk_handle, const void *d_fh, const void *d_lin, const void *d_l, const void *d_r, const void *d_o, "
    "size_t in_stride, size_t rows, const void *d_zeta, const void *d_kzg_gamma, void *d_q, size_t out_stride, void *d_value, void *stream);")
NAMES = ("zk_bn254_fr_poly_open_rows_dev", "zk_bn254_plonk_linearize_batch_dev", "zk_bn254_plonk_open_batch_dev")


def test_header_declares_the_entries_and_the_library_exports_them():
    hdr = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "zkmi.h")).read())
    for decl in DECLS:
        assert decl in hdr
    for name in NAMES:
        assert name in _lib.SYMBOLS and hasattr(_lib.lib(), name)
    for name in ("linearize_batch", "open_batch", "poly_open_rows"):
        assert name in zk.__all__ and callable(getattr(zk, name))
    assert callable(plonk.ProvingKey.linearize_batch) and callable(plonk.ProvingKey.open_batch)
    hpp = open(os.path.join(ROOT, "include", "zkmi.hpp")).read()
    assert hpp.index("inline Error ComputeQuotientBatch(") < hpp.index("inline Error LinearizeBatch(") < hpp.index("inline Error OpenBatch(") < hpp.index("}  // namespace plonk")
    assert hpp.index("namespace fr {") < hpp.index("inline Error PolyOpenRows(") < hpp.index("}  // namespace fr")


def test_argument_errors_and_empty_batches_need_no_device():
    """ZK_ERR_ARG for a null pointer (and, for the ingredient, a stride too small or a forbidden overlap), ZK_ERR_HANDLE for an unknown key (not
    ZK_ERR_NO_DEVICE) and ZK_OK for rows = 0: all decided before the device is looked for.  (The stride and overlap errors of the two key entries need a key's
    sizes: tests/test_gpu_plonk_open.py.)"""
    lib = _lib.lib()
    x = np.zeros((128, 4), dtype=np.uint64)
    at = lambda k: C.c_void_p(x.ctypes.data + k * 256)
    sz, null = C.c_size_t, C.c_void_p(0)
    ARG, HANDLE, OK = _lib.ZK_ERR_ARG, _lib.ZK_ERR_HANDLE, _lib.ZK_OK

    names = ("l", "r", "o", "z", "h", "alpha", "beta", "gamma", "zeta", "values", "zquot", "lin", "fh")
    good = {k: at(i) for i, k in enumerate(names)}

    def lin(handle=12345, rows=2, **kw):
        a = dict(good, **kw)
        return lib.zk_bn254_plonk_linearize_batch_dev(C.c_uint64(handle), a["l"], a["r"], a["o"], a["z"], sz(11), a["h"], sz(30), sz(rows), a["alpha"], a["beta"],
                                                      a["gamma"], a["zeta"], a["values"], a["zquot"], a["lin"], a["fh"], sz(11), None)
    assert {k: v for k, v in ((k, lin(**{k: null})) for k in names) if v != ARG} == {}
    assert lin() == HANDLE and lin(handle=0) == HANDLE
    assert lin(rows=0) == OK and lin(rows=0, handle=0) == OK and lin(rows=0, lin=good["l"]) == OK

    names5 = ("fh", "lin", "l", "r", "o", "zeta", "kg", "q", "value")
    good5 = {k: at(i) for i, k in enumerate(names5)}

    def opn(handle=12345, rows=2, **kw):
        a = dict(good5, **kw)
        return lib.zk_bn254_plonk_open_batch_dev(C.c_uint64(handle), a["fh"], a["lin"], a["l"], a["r"], a["o"], sz(11), sz(rows), a["zeta"], a["kg"], a["q"], sz(10),
                                                 a["value"], None)
    assert {k: v for k, v in ((k, opn(**{k: null})) for k in names5) if v != ARG} == {}
    assert opn() == HANDLE and opn(handle=0) == HANDLE
    assert opn(rows=0) == OK and opn(rows=0, handle=0) == OK and opn(rows=0, q=good5["l"]) == OK

    f, pts, q, vals = at(0), at(20), at(30), at(50)              # 8 elements apart per index: two rows of 5 at stride 6 fit below index 2

    def one(f=f, in_stride=6, length=5, rows=2, pts=pts, q=q, q_stride=4, vals=vals):
        return lib.zk_bn254_fr_poly_open_rows_dev(f, sz(in_stride), sz(length), sz(rows), pts, q, sz(q_stride), vals, None)
    bad = {"f": one(f=null), "points": one(pts=null), "values": one(vals=null), "len 0": one(length=0), "in_stride": one(in_stride=4), "q_stride": one(q_stride=3),
           "q = f, other stride": one(q=f, q_stride=5), "q inside f": one(q=C.c_void_p(f.value + 32)), "q over points": one(q=pts), "q over values": one(q=vals),
           "values over f": one(vals=f), "values over points": one(vals=pts)}
    assert {k: v for k, v in bad.items() if v != ARG} == {}
    assert one(rows=0) == OK and one(rows=0, q=null) == OK and one(rows=0, q=f, q_stride=6) == OK and one(rows=0, length=0, in_stride=0) == OK
    assert not x.any()


CPP_CHECK = r"""
#include <cstdio>
#include "zkmi.hpp"
using namespace zkmi;
int main() {
    plonk::ProvingKey pk;                    // no key behind it: handle 0
    fr::Element x[64] = {};
    plonk::LinearizeRows in;
    plonk::LinearizedRows out;
    if (plonk::LinearizeBatch(pk, in, 2, out).code != ZK_ERR_ARG) return 1;                        // null rows
    in.l = in.r = in.o = in.z = in.h = in.alpha = in.beta = in.gamma = in.zeta = x;
    in.in_stride = 11; in.h_stride = 30;
    if (plonk::LinearizeBatch(pk, in, 2, out).code != ZK_ERR_ARG) return 2;                        // no outputs
    out.values = out.zquot = out.lin = out.fh = x; out.out_stride = 11;
    if (plonk::LinearizeBatch(pk, in, 2, out).code != ZK_ERR_HANDLE) return 3;                     // unknown key, answered without a device
    if (!plonk::LinearizeBatch(pk, in, 0, out).ok()) return 4;                                     // no rows: nothing to do
    plonk::OpenRows op;
    if (plonk::OpenBatch(pk, op, 2, x, 10, x).code != ZK_ERR_ARG) return 5;
    op.fh = op.lin = op.l = op.r = op.o = op.zeta = op.kzg_gamma = x;
    op.in_stride = 11;
    if (plonk::OpenBatch(pk, op, 2, nullptr, 10, x).code != ZK_ERR_ARG) return 6;
    if (plonk::OpenBatch(pk, op, 2, x, 10, x).code != ZK_ERR_HANDLE) return 7;
    if (!plonk::OpenBatch(pk, op, 0, x, 10, x).ok()) return 8;
    if (fr::PolyOpenRows(nullptr, 6, 5, 2, x, nullptr, 0, x).code != ZK_ERR_ARG) return 9;
    if (fr::PolyOpenRows(x, 4, 5, 2, x + 20, nullptr, 0, x + 30).code != ZK_ERR_ARG) return 10;    // a stride below the length
    if (fr::PolyOpenRows(x, 6, 5, 2, x + 20, x + 1, 6, x + 30).code != ZK_ERR_ARG) return 11;      // q inside f
    if (!fr::PolyOpenRows(x, 6, 5, 0, x + 20, x, 6, x + 30).ok()) return 12;
    std::puts("ok");
    return 0;
}
"""


def test_cpp_mirrors_compile_over_the_c_entries(tmp_path):
    import subprocess
    src, exe = tmp_path / "open_check.cpp", str(tmp_path / "open_check")
    src.write_text(CPP_CHECK)
    libdir = os.path.join(ROOT, "noir_backend_using_gnark_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + libdir, "-lzkmi",
                           "-Wl,-rpath," + libdir, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "ok" in out.stdout, (out.returncode, out.stdout + out.stderr)
