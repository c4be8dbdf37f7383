"""The row-batched quotient (PLONK round 3) without a GPU: the expectation of the device tests (tests/plonk_quotient_ref.py) reproduces the oracle prover's own
h with status 0 and answers a tampered row with status 1; the pool's circuit has many witnesses; ProvingKey.quotient_batch refuses wrong shapes, dtypes,
strides, counts and overlap BEFORE the library is called; include/zkmi.h declares the entry, libzkmi.so exports it, it answers its argument errors (and rows = 0)
before it looks for a device, and plonk::ComputeQuotientBatch compiles over it."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import noir_backend_using_gnark_amd as zk
from noir_backend_using_gnark_amd import _lib, bn254, plonk
from oracle import bn254_ref as ref
from oracle import plonk_ref as pl
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


# ------------------------------------------------------------------------------------------------------- the reference against the oracle
@pytest.mark.parametrize("log_n,family,npub", CASES)
def test_reference_reproduces_the_oracle_provers_quotient(log_n, family, npub):
    """for a circuit of tests/plonk_shapes.circuit the oracle's trace holds bl, br, bo, bz, the challenges and h: quotient() gives that h, zeros above it and
    status 0, with either transform provider; rounds_1_2() gives the trace's four polynomials; one coefficient of bl incremented gives status 1"""
    n = 1 << log_n
    spr, sol = ps.circuit(family, n, npub, "full", 0x3A0 + 7 * log_n + npub)
    assert ps.domain_size(spr) == n
    pk, _ = pl.plonk_setup(spr, _srs_for(n), fast=True)
    blinders = ps.blinders("max" if family == "max" else "random", log_n)
    mine = qr.setup_polys(spr, fast=log_n & 1)
    assert all(mine[k] == pk[k] for k in ("n", "perm", "ql", "qr", "qm", "qo", "cqk", "lqk", "s1", "s2", "s3")) and (mine["d0"].n, mine["d1"].n) == (pk["d0"].n, pk["d1"].n)
    t = {}
    pl.plonk_prove(pk, sol, blinders, fast=True, trace=t)
    N4, keep = pk["d1"].n, 3 * (n + 2)
    assert N4 == (8 if n < 6 else 4) * n and len(t["h"]) == keep and any(t["h"])
    args = (t["bl"], t["br"], t["bo"], t["bz"], sol[:npub], t["alpha"], t["beta"], t["gamma"])
    h, status = qr.quotient(pk, *args)
    assert len(h) == N4 and h[:keep] == t["h"] and h[keep:] == [0] * (N4 - keep) and status == 0
    assert qr.quotient(pk, *args, fast=True) == (h, 0)
    assert qr.rounds_1_2(pk, sol, blinders, t["beta"], t["gamma"]) == (t["bl"], t["br"], t["bo"], t["bz"])
    for k in (0, n + 1):
        bad = list(t["bl"])
        bad[k] = (bad[k] + 1) % R
        hb, sb = qr.quotient(pk, bad, *args[1:])
        assert sb == 1 and any(hb[keep:]) and hb[:keep] != t["h"]


def test_other_public_inputs_violate_the_placeholder_gates():
    n = 16
    spr, sol = ps.circuit("random", n, 1, "full", 0x77)
    pk, _ = pl.plonk_setup(spr, _srs_for(n), fast=True)
    t = {}
    pl.plonk_prove(pk, sol, ps.blinders("random"), fast=True, trace=t)
    args = (t["bl"], t["br"], t["bo"], t["bz"])
    ch = (t["alpha"], t["beta"], t["gamma"])
    assert qr.quotient(pk, *args, sol[:1], *ch)[1] == 0
    assert qr.quotient(pk, *args, [(sol[0] + 1) % R], *ch)[1] == 1


@pytest.mark.parametrize("log_n,npub", [(2, 0), (3, 1), (6, 33)])
def test_pool_rows_are_witnesses_of_one_circuit(log_n, npub):
    """the forward circuit fills its domain, every pool row is a different satisfying solution of it, and the verdicts are 0, 0, 1, 0, 0"""
    n = 1 << log_n
    spr, n_in = qr.forward_circuit(n, npub, 0x51 + log_n)
    assert ps.domain_size(spr) == n and spr.n_public == npub and n_in == npub + 3
    pk, _ = pl.plonk_setup(spr, _srs_for(n), fast=True)
    rows = [qr.pool_row(pk, n_in, j, 0x90 + log_n) for j in range(qr.POOL)]
    assert len({tuple(r["sol"]) for r in rows}) == qr.POOL and all(spr.is_satisfied(r["sol"]) for r in rows)
    assert (rows[0]["alpha"], rows[1]["beta"], rows[4]["gamma"]) == (0, 0, 0) and {rows[2][k] for k in ("alpha", "beta", "gamma")} == {R - 1}
    assert rows[3]["public"] == [(R - 1) * (i & 1) for i in range(npub)] and rows[3]["sol"][npub:n_in] == [R - 1] * 3 and rows[3]["blinders"] == [R - 1] * 9
    status = [qr.quotient(pk, r["bl"], r["br"], r["bo"], r["bz"], r["public"], r["alpha"], r["beta"], r["gamma"])[1] for r in rows]
    assert status == [0, 0, 1, 0, 0] == [r["violated"] for r in rows]
    assert [qr.rows_of(k) for k in (1, 2, 3, 5)] == [[0], [3, 4], [1, 2, 3], [0, 1, 2, 3, 4]]


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


def test_quotient_batch_rejects_bad_host_arrays_before_the_library(no_library):
    pk = _key()
    assert pk.domain_size == 8 and pk.n_public == 2
    w, z, pub, ch = np.zeros((3, 10, 4), np.uint64), np.zeros((3, 11, 4), np.uint64), np.zeros((3, 2, 4), np.uint64), np.zeros((3, 4), np.uint64)
    good = dict(l=w, r=w, o=w, z=z, public=pub, alpha=ch, beta=ch, gamma=ch)
    call = lambda **kw: pk.quotient_batch(**{k: kw.pop(k, v) for k, v in good.items()}, **kw)
    for name in ("l", "r", "o", "z"):
        g = good[name]
        for bad, exc in ((g.astype(np.int64), TypeError), (g.tolist(), TypeError), (np.zeros(g.shape[:2] + (8,), np.uint64)[:, :, ::2], TypeError),
                         (g[:2], ValueError), (g[0], ValueError), (np.zeros(g.shape[:2] + (5,), np.uint64), ValueError),
                         (np.zeros((3, 9, 4), np.uint64), ValueError), (np.zeros((3, 12, 4), np.uint64), ValueError)):
            with pytest.raises(exc):
                call(**{name: bad})
    with pytest.raises(ValueError):
        call(z=w)                                                 # z has n + 3 coefficients
    for bad, exc in ((pub[:2], ValueError), (np.zeros((3, 3, 4), np.uint64), ValueError), (np.zeros((3, 2), np.uint64), ValueError),
                     (pub.astype(np.int64), TypeError), (pub.tolist(), TypeError), (None, TypeError)):
        with pytest.raises(exc):
            call(public=bad)
    for name in ("alpha", "beta", "gamma"):
        for bad, exc in ((ch[:2], ValueError), (ch.reshape(-1), ValueError), (ch.astype(np.int64), TypeError), (ch.tolist(), TypeError)):
            with pytest.raises(exc):
                call(**{name: bad})
    for kw in (dict(rows=2), dict(in_stride=12), dict(pub_stride=3), dict(out_stride=31), dict(out=_nothing(3 * 30 * 32, 0)), dict(status=_nothing(12, 0))):
        with pytest.raises(ValueError):
            call(**kw)
    empty = lambda *shape: np.zeros(shape, np.uint64)                # no rows: answered without the library
    h, status = pk.quotient_batch(empty(0, 10, 4), empty(0, 10, 4), empty(0, 10, 4), empty(0, 11, 4), empty(0, 2, 4), empty(0, 4), empty(0, 4), empty(0, 4))
    assert h.shape == (0, 30, 4) and status.shape == (0,) and status.dtype == np.int32
    pk.handle = C.c_uint64(0)


def test_quotient_batch_rejects_bad_device_geometry_before_the_library(no_library):
    pk = _key()
    n, npub, rows, keep = 8, 2, 3, 30
    mb = 0x100000
    l, r, o, z = (_nothing(rows * (n + 3) * 32, mb * (k + 1)) for k in range(4))
    pub, alpha, beta, gamma = _nothing(rows * npub * 32, 5 * mb), _nothing(rows * 32, 6 * mb), _nothing(rows * 32, 7 * mb), _nothing(rows * 32, 8 * mb)
    out, status = _nothing(rows * keep * 32, 9 * mb), _nothing(rows * 4, 10 * mb)
    bufs = (l, r, o, z, pub, alpha, beta, gamma, out, status)
    good = dict(l=l, r=r, o=o, z=z, public=pub, alpha=alpha, beta=beta, gamma=gamma, rows=rows, out=out, status=status)
    call = lambda **kw: pk.quotient_batch(**dict(good, **kw))
    try:
        for kw in (dict(rows=None), dict(rows=-1), dict(rows=4), dict(in_stride=n + 2), dict(in_stride=n + 4), dict(pub_stride=npub - 1), dict(pub_stride=npub + 1),
                   dict(out_stride=keep - 1), dict(out_stride=keep + 1), dict(out=l), dict(out=z), dict(out=pub), dict(out=beta), dict(out=l.ptr + 32),
                   dict(status=l), dict(status=z), dict(status=pub), dict(status=alpha), dict(status=out), dict(status=out.ptr + 64),
                   dict(z=_nothing(rows * (n + 3) * 32 - 32, 4 * mb)), dict(public=_nothing(rows * npub * 32 - 32, 5 * mb)), dict(gamma=_nothing((rows - 1) * 32, 8 * mb)),
                   dict(status=_nothing(rows * 4 - 4, 10 * mb))):
            with pytest.raises(ValueError):
                call(**kw)
        for kw in (dict(o=np.zeros((rows, n + 2, 4), np.uint64)), dict(z=np.zeros((rows, n + 3, 4), np.uint64)), dict(public=np.zeros((rows, npub, 4), np.uint64)),
                   dict(alpha=np.zeros((rows, 4), np.uint64)), dict(out=np.zeros((rows, keep, 4), np.uint64)), dict(status=np.zeros(rows, np.int32)), dict(public=None)):
            with pytest.raises(TypeError):
                call(**kw)
    finally:
        for b in bufs:
            b.ptr = 0
    pk.handle = C.c_uint64(0)


# ------------------------------------------------------------------------------------------------------- header and exports
def test_header_declares_the_entry_and_the_library_exports_it():
    hdr = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "zkmi.h")).read())
    decl = ("int zk_bn254_plonk_quotient_batch_dev(uint64_t pk_handle, const void *d_l, const void *d_r, const void *d_o, const void *d_z, size_t in_stride, "
            "const void *d_pub, size_t pub_stride, size_t rows, const void *d_alpha, const void *d_beta, const void *d_gamma, void *d_h, size_t out_stride, "
            "void *d_status, void *stream);")
    assert decl in hdr
    assert "zk_bn254_plonk_quotient_batch_dev" in _lib.SYMBOLS and hasattr(_lib.lib(), "zk_bn254_plonk_quotient_batch_dev")
    assert "quotient_batch" in zk.__all__ and callable(zk.quotient_batch) and callable(plonk.ProvingKey.quotient_batch)
    hpp = open(os.path.join(ROOT, "include", "zkmi.hpp")).read()
    assert hpp.index("inline Error Prove(const ProvingKey& pk, const fr::Vector& solution") < hpp.index("inline Error ComputeQuotientBatch(") < hpp.index("}  // namespace plonk")


def test_argument_errors_and_empty_batches_need_no_device():
    """ZK_ERR_ARG for a null pointer, ZK_ERR_HANDLE for an unknown key (not ZK_ERR_NO_DEVICE) and ZK_OK for rows = 0: all decided before the device is looked
    for.  (The stride and overlap errors need a key's sizes: tests/test_gpu_plonk_quotient.py.)"""
    lib = _lib.lib()
    x = np.zeros((64, 4), dtype=np.uint64)
    at = lambda k: C.c_void_p(x.ctypes.data + k * 128)
    names = ("l", "r", "o", "z", "pub", "alpha", "beta", "gamma", "h", "status")
    good = {k: at(i) for i, k in enumerate(names)}
    sz = C.c_size_t

    def call(handle=12345, rows=2, **kw):
        a = dict(good, **kw)
        return lib.zk_bn254_plonk_quotient_batch_dev(C.c_uint64(handle), a["l"], a["r"], a["o"], a["z"], sz(11), a["pub"], sz(2), sz(rows), a["alpha"], a["beta"],
                                                     a["gamma"], a["h"], sz(30), a["status"], None)

    bad = {k: call(**{k: C.c_void_p(0)}) for k in names if k != "pub"}
    assert {k: v for k, v in bad.items() if v != _lib.ZK_ERR_ARG} == {}
    assert call() == _lib.ZK_ERR_HANDLE and call(handle=0) == _lib.ZK_ERR_HANDLE
    assert call(rows=0) == _lib.ZK_OK and call(rows=0, handle=0) == _lib.ZK_OK and call(rows=0, h=good["l"]) == _lib.ZK_OK
    assert not x.any()


CPP_CHECK = r"""
#include <cstdio>
#include "zkmi.hpp"
using namespace zkmi;
int main() {
    plonk::ProvingKey pk;                    // no key behind it: handle 0
    fr::Element x[8] = {};
    int status[2] = {7, 7};
    plonk::QuotientRows in;
    if (plonk::ComputeQuotientBatch(pk, in, 2, x, 30, status).code != ZK_ERR_ARG) return 1;        // null rows
    in.l = in.r = in.o = in.z = in.alpha = in.beta = in.gamma = x;
    in.in_stride = 11;
    if (plonk::ComputeQuotientBatch(pk, in, 2, x, 30, nullptr).code != ZK_ERR_ARG) return 2;       // no status
    if (plonk::ComputeQuotientBatch(pk, in, 2, x, 30, status).code != ZK_ERR_HANDLE) return 3;     // unknown key, answered without a device
    if (!plonk::ComputeQuotientBatch(pk, in, 0, x, 30, status).ok()) return 4;                     // no rows: nothing to do
    if (status[0] != 7 || status[1] != 7) return 5;
    std::puts("ok");
    return 0;
}
"""


def test_cpp_mirror_compiles_over_the_c_entry(tmp_path):
    import subprocess
    src, exe = tmp_path / "quotient_check.cpp", str(tmp_path / "quotient_check")
    src.write_text(CPP_CHECK)
    libdir = os.path.join(ROOT, "noir_backend_using_gnark_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + libdir, "-lzkmi",
                           "-Wl,-rpath," + libdir, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "ok" in out.stdout, (out.returncode, out.stdout + out.stderr)
