"""The batch PLONK prover's C ABI and Python wrappers without a device: the three symbols are exported and declared, every argument error comes back before a
device is looked for (rows = 0 is ZK_OK, a null pointer and a stage outside 0 .. 4 are ZK_ERR_ARG, an unknown key is ZK_ERR_HANDLE), the wrappers refuse ragged
shapes before any C call, and tests/plonk_batch_ref.py -- the transcript the device is held against in tests/test_gpu_plonk_batch.py -- derives the challenges
oracle/plonk_ref.py derives."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from noir_backend_using_gnark_amd import _lib
from noir_backend_using_gnark_amd import plonk as zp
from oracle import plonk_ref as pl
from tests import plonk_batch_ref as br
from tests import plonk_shapes as ps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH = ("zk_bn254_plonk_prove_batch", "zk_bn254_plonk_prove_batch_info", "zk_bn254_plonk_challenges_batch_dev")
BOGUS = C.c_uint64(0x00ffffffffffff)  # no such handle
NV = 6


def _prove(lib, sol, bl, ch, out, st, rows=2, stride=NV):
    return lib.zk_bn254_plonk_prove_batch(BOGUS, sol, C.c_size_t(NV), C.c_size_t(stride), C.c_size_t(rows), 0, bl, ch, C.c_size_t(0), out, st)


def _args(rows=2):
    return (_lib.vp(np.zeros((rows, NV, 4), np.uint64)), _lib.vp(np.zeros((rows, 9, 4), np.uint64)), _lib.vp(np.zeros((rows, 5, 4), np.uint64)),
            (C.c_uint8 * (548 * rows))(), (C.c_int * rows)())


def _challenges(lib, stage, rows, pub, pts, prev, val, out):
    return lib.zk_bn254_plonk_challenges_batch_dev(BOGUS, C.c_int(stage), C.c_size_t(rows), pub, C.c_size_t(1), pts, prev, val, out, None)


def test_symbols_are_exported_and_declared():
    lib = _lib.lib()
    header = open(os.path.join(ROOT, "include", "zkmi.h")).read()
    for s in BATCH:
        assert s in _lib.SYMBOLS and hasattr(lib, s), s
        assert re.search(r"\bint %s\(" % s, header), s
    assert "ProveBatch(const ProvingKey& pk" in open(os.path.join(ROOT, "include", "zkmi.hpp")).read()
    import noir_backend_using_gnark_amd as zk
    assert zk.plonk_prove_batch is zp.prove_batch and zk.plonk_prove_batch_info is zp.prove_batch_info and zk.plonk_challenges_rows is zp.challenges_rows


def test_no_rows_is_ok_and_writes_nothing():
    lib = _lib.lib()
    sol, bl, ch, _, st = _args()
    out = (C.c_uint8 * 548)(*([0xA5] * 548))
    assert _prove(lib, sol, bl, None, out, st, rows=0) == _lib.ZK_OK
    assert bytes(out) == b"\xa5" * 548
    assert _challenges(lib, 0, 0, sol, sol, None, None, sol) == _lib.ZK_OK
    pk = zp.ProvingKey(BOGUS.value, None, dict(size=8, n_public=1), NV)
    assert zp.prove_batch(pk, np.zeros((0, NV, 4), np.uint64), np.zeros((0, 9, 4), np.uint64)) == []


def test_null_pointers_are_argument_errors_before_the_device():
    lib = _lib.lib()
    for hole in range(4):
        sol, bl, ch, out, st = _args()
        ptrs = [sol, bl, out, st]
        ptrs[hole] = None
        assert _prove(lib, ptrs[0], ptrs[1], ch, ptrs[2], ptrs[3]) == _lib.ZK_ERR_ARG, hole
        assert b"null pointer" in lib.zk_last_error()
    buf = _lib.vp(np.zeros((64, 4), np.uint64))
    for stage, holes in ((0, ("pts", "out")), (1, ("prev", "out")), (2, ("pts", "prev", "out")), (3, ("pts", "prev", "out")), (4, ("pts", "prev", "val", "out"))):
        for hole in holes:
            a = dict(pub=buf, pts=buf, prev=buf, val=buf, out=buf)
            a[hole] = None
            assert _challenges(lib, stage, 2, a["pub"], a["pts"], a["prev"], a["val"], a["out"]) == _lib.ZK_ERR_ARG, (stage, hole)
            assert b"null pointer" in lib.zk_last_error()


def test_stage_outside_the_five_is_an_argument_error():
    lib = _lib.lib()
    buf = _lib.vp(np.zeros((64, 4), np.uint64))
    for stage in (-1, 5, 1 << 20):
        assert _challenges(lib, stage, 2, buf, buf, buf, buf, buf) == _lib.ZK_ERR_ARG, stage
        assert b"stage" in lib.zk_last_error()
    with pytest.raises(ValueError):
        zp.challenges_rows(zp.ProvingKey(BOGUS.value, None, dict(size=8, n_public=0), NV), 5)


def test_unknown_key_is_a_handle_error_without_a_device():
    """the table of keys is the host's: the answer does not depend on a device being there, and there is no CPU fallback behind it"""
    lib = _lib.lib()
    sol, bl, ch, out, st = _args()
    for c in (None, ch):
        assert _prove(lib, sol, bl, c, out, st) == _lib.ZK_ERR_HANDLE
        assert b"unknown PLONK proving-key handle" in lib.zk_last_error()
    chunk, batched, lin = C.c_size_t(0), C.c_int(0), C.c_int(0)
    assert lib.zk_bn254_plonk_prove_batch_info(BOGUS, C.byref(chunk), C.byref(batched), C.byref(lin)) == _lib.ZK_ERR_HANDLE
    buf = _lib.vp(np.zeros((64, 4), np.uint64))
    for stage in range(5):
        assert _challenges(lib, stage, 2, buf, buf, buf, buf, _lib.vp(np.zeros((64, 4), np.uint64))) == _lib.ZK_ERR_HANDLE, stage
    pk = zp.ProvingKey(BOGUS.value, None, dict(size=8, n_public=1), NV)
    with pytest.raises(_lib.ZkmiError) as ei:
        zp.prove_batch(pk, np.zeros((2, NV, 4), np.uint64), np.zeros((2, 9, 4), np.uint64))
    assert ei.value.code == _lib.ZK_ERR_HANDLE
    with pytest.raises(_lib.ZkmiError) as ei:
        zp.prove_batch_info(pk)
    assert ei.value.code == _lib.ZK_ERR_HANDLE


def test_wrappers_refuse_ragged_shapes_before_any_c_call():
    pk = zp.ProvingKey(BOGUS.value, None, dict(size=8, n_public=1), NV)
    z = lambda *shape: np.zeros(shape, np.uint64)  # noqa: E731
    sol, bl, ch = z(2, NV, 4), z(2, 9, 4), z(2, 5, 4)
    for bad in ((sol[:1], bl, None),             # one solution for two rows of blinders
                (sol, bl, ch[:1]),               # one row of challenges
                (sol[:, :NV - 1], bl, None),     # not the key's variables
                (sol, bl[:, :8], None),          # eight blinders
                (sol, bl, ch[:, :4]),            # four challenges
                (sol[0], bl[0], None),           # 1-D vectors of limbs are the single prover's arguments
                (sol, bl[0], None),
                (sol, bl, ch[0]),
                (sol[:, :, :3], bl, None)):      # not limbs
        with pytest.raises(ValueError):
            zp.prove_batch(pk, *bad)
    with pytest.raises(ValueError):
        zp.prove_batch(pk, sol, bl, chunk_rows=-1)
    with pytest.raises(TypeError):
        zp.prove_batch(pk, sol, bl, on_device=True)   # host rows are not device rows
    pts, raw = z(2, 3, 8), np.zeros((2, 32), np.uint8)
    for stage, kw in ((0, dict(public=z(2, 1, 4), points=pts[:, :2])),       # two points where gamma binds three
                      (0, dict(public=z(1, 1, 4), points=pts)),              # row counts differ
                      (0, dict(public=z(2, 2, 4), points=pts)),              # not the key's public inputs
                      (0, dict(public=z(2, 1, 4))),                          # no points
                      (1, dict(prev=raw[0])),                                # 1-D
                      (2, dict(prev=raw, points=pts)),                       # alpha binds one point
                      (3, dict(prev=raw[:, :31], points=pts)),
                      (4, dict(prev=z(2, 4), points=z(2, 5, 8), values=z(2, 7, 4))),   # values are the eight of round 4
                      (4, dict(prev=raw, points=z(2, 5, 8), values=z(2, 8, 4)))):      # stage 4 binds zeta, an element
        with pytest.raises(ValueError):
            zp.challenges_rows(pk, stage, **kw)


@pytest.mark.parametrize("family,log_n,npub", [("random", 2, 1), ("zeros+identity_perm", 3, 0)])
def test_reference_transcript_derives_the_oracles_challenges(family, log_n, npub):
    """the five challenges of oracle/plonk_ref.py's prover, re-derived by tests/plonk_batch_ref.py from the proof's digests and values; the second circuit with
    zero blinders has [L], [R], [O] and the quotient's digests at infinity"""
    n = 1 << log_n
    spr, sol = ps.circuit(family, n, npub, "full", 0xF5 + log_n)
    opk, ovk = pl.plonk_setup(spr, pl.kzg_new_srs(n + 3, 0xA1FA0123456789))
    trace = {}
    proof = pl.plonk_prove(opk, sol, ps.blinders("zeros" if "zeros" in family else "random", log_n), trace=trace)
    if "zeros" in family:
        assert proof["lro"] == [None] * 3
    key = [ovk["s"][0], ovk["s"][1], ovk["s"][2], ovk["ql"], ovk["qr"], ovk["qm"], ovk["qo"], ovk["qk"]]
    got = br.five(key, sol[:npub], proof["lro"], proof["z"], proof["h"], trace["folded_h_digest"], trace["lin_digest"], proof["claimed"] + [proof["zu"]])
    assert list(got) == [trace[k] for k in ("gamma", "beta", "alpha", "zeta", "kzg_gamma")]
    fs = pl.Transcript("gamma", "beta", "alpha", "zeta")
    pl._bind_public_data(fs, ovk, sol[:npub])
    assert fs.challenge_fr("gamma", *proof["lro"]) == got[0] and fs.compute("gamma") == br.stage(0, key, public=sol[:npub], points=proof["lro"])[1]
