"""The Groth16 proof tail for many rows in one device launch (-m gpu), bit-exact: zk_bn254_groth16_finalize_batch / _dev and groth16.finalize_batch.
The expectation is never the code under test: for every row it is zk_bn254_groth16_finalize (the unchanged host tail), and on the tagged rows of
tests/groth16_tail_cases.py also the builder's pure-python bytes (gnark's arrangement through oracle/bn254_ref.py)."""
import ctypes as C
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import noir_backend_using_gnark_amd as zk
from noir_backend_using_gnark_amd import _lib, parallel
from noir_backend_using_gnark_amd import groth16 as g16
from noir_backend_using_gnark_amd import verify as zv
from oracle import bn254_ref as ref
from oracle import oracle as orc
from tests import groth16_tail_cases as tc
from tests.helpers import mont_limbs, sha_image

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BLOCK_ROWS = 64  # rows per workgroup of k_groth16_tail (four waves: one per product group, the lane is the row)
FB_TABLE_BYTES = 32 * 255 * (64 + 128)  # the 8-bit window tables of delta and delta2 a key gains at its first device tail


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    _lib.require_device()  # fail loudly: no silent fallback


def _key(which="base"):
    return zk.ProvingKey(**tc.key(which)[0], precompute_tables=False)


def _host_tail(pk, parts, r, s):
    """the unchanged host path, row by row"""
    return [parallel.groth16_finalize(pk, parts[i], r[i], s[i]) for i in range(parts.shape[0])]


def _stack(rows):
    return np.stack([x.partials for x in rows]), np.stack([x.r for x in rows]), np.stack([x.s for x in rows])


def _dev_call(pk, d_parts, n_partials, d_r, d_s, n, d_out, stream=None):
    return _lib.lib().zk_bn254_groth16_finalize_batch_dev(pk.handle if hasattr(pk, "handle") else C.c_uint64(pk), C.c_void_p(d_parts), C.c_size_t(n_partials),
                                                          C.c_void_p(d_r), C.c_void_p(d_s), C.c_size_t(n), C.c_void_p(d_out), stream)


def _proofs(buf, n):
    raw = buf.to_numpy(np.uint8, (128 * n,)).tobytes()
    return [raw[128 * i:128 * i + 128] for i in range(n)]


class _Hip:
    """a caller's stream, through the HIP runtime the library is linked against"""

    def __init__(self):
        _lib.lib()
        with open("/proc/self/maps") as maps:
            path = next((line.split()[-1] for line in maps if "libamdhip64" in line), "libamdhip64.so")
        self.rt = C.CDLL(path)
        self.stream = C.c_void_p()
        assert self.rt.hipStreamCreate(C.byref(self.stream)) == 0

    def sync(self):
        assert self.rt.hipStreamSynchronize(self.stream) == 0

    def close(self):
        assert self.rt.hipStreamDestroy(self.stream) == 0


@pytest.mark.parametrize("n_partials", [1, 3])
def test_all_tagged_cases_in_one_call_host_and_device_forms(n_partials):
    rows = tc.tagged_rows() if n_partials == 1 else tc.tagged_rows_3()
    parts, r, s = _stack(rows)
    n = len(rows)
    pk = _key()
    want = _host_tail(pk, parts, r, s)
    bad = [x.tag for x, w in zip(rows, want) if w != x.expected]
    assert not bad, "host tail against the pure-python bytes: %s" % bad
    got = g16.finalize_batch(pk, parts, r, s)
    bad = [x.tag for x, g, w in zip(rows, got, want) if g != w]
    assert not bad, bad
    dev = [_lib.DeviceBuffer.from_numpy(v) for v in (parts, r, s)]
    before = [sha_image(d.to_numpy(np.uint64, v.shape)) for d, v in zip(dev, (parts, r, s))]
    hip = _Hip()
    for stream in (None, hip.stream):
        d_out = _lib.DeviceBuffer.from_numpy(np.full(128 * n, 0xA5, np.uint8))
        _lib.check(_dev_call(pk, dev[0].ptr, n_partials, dev[1].ptr, dev[2].ptr, n, d_out.ptr, stream))
        if stream is not None:
            hip.sync()
        got = _proofs(d_out, n)
        bad = [x.tag for x, g, w in zip(rows, got, want) if g != w]
        assert not bad, (stream is not None, bad)
        assert [sha_image(d.to_numpy(np.uint64, v.shape)) for d, v in zip(dev, (parts, r, s))] == before
        d_out.free()
    hip.close()
    pk.free()


POSITIONS = [0, 1, BLOCK_ROWS - 2, BLOCK_ROWS - 1, BLOCK_ROWS, BLOCK_ROWS + 1, 127, 128, 254, 255, 256]
_bulk_cache = {}


def _bulk(n_partials):
    """257 rows, tagged rows at the first, last and workgroup-boundary positions of every row count below, and the host tail's bytes for all of them: once"""
    if n_partials not in _bulk_cache:
        tagged = tc.tagged_rows() if n_partials == 1 else tc.tagged_rows_3()
        parts, r, s, placed = tc.assemble(257, n_partials, 0xB0 + n_partials, tagged, POSITIONS)
        pk = _key()
        want = _host_tail(pk, parts, r, s)
        pk.free()
        for pos, row in placed.items():
            assert want[pos] == row.expected, row.tag
        for v in (parts, r, s):
            v.setflags(write=False)
        _bulk_cache[n_partials] = (parts, r, s, want)
    return _bulk_cache[n_partials]


# 1, 2; the workgroup's 64 rows -1, +0, +1 (a row's four product lanes sit in the same workgroup, so 256 lanes -1 / +1 are the same counts); 255, 256, 257
@pytest.mark.parametrize("n_partials", [1, 3])
@pytest.mark.parametrize("n", [1, 2, BLOCK_ROWS - 1, BLOCK_ROWS, BLOCK_ROWS + 1, 255, 256, 257])
def test_row_counts(n, n_partials):
    parts, r, s, want = _bulk(n_partials)
    pk = _key()
    got = g16.finalize_batch(pk, parts[:n], r[:n], s[:n])
    bad = [i for i in range(n) if got[i] != want[i]]
    assert len(got) == n and not bad, bad
    dev = [_lib.DeviceBuffer.from_numpy(v[:n]) for v in (parts, r, s)]
    d_out = _lib.DeviceBuffer.from_numpy(np.full(128 * (n + 1), 0xA5, np.uint8))
    _lib.check(_dev_call(pk, dev[0].ptr, n_partials, dev[1].ptr, dev[2].ptr, n, d_out.ptr))
    raw = d_out.to_numpy(np.uint8, (128 * (n + 1),)).tobytes()
    assert [raw[128 * i:128 * i + 128] for i in range(n)] == want[:n]
    assert raw[128 * n:] == b"\xa5" * 128  # nothing written past the last row
    pk.free()


def test_one_record_per_row_may_come_without_the_middle_axis():
    parts, r, s, want = _bulk(1)
    pk = _key()
    assert g16.finalize_batch(pk, parts[:5, 0, :], r[:5], s[:5]) == want[:5]
    with pytest.raises(ValueError):
        g16.finalize_batch(pk, parts[:5, 0, :95], r[:5], s[:5])
    pk.free()


def _pk_bytes(pk):
    b = C.c_size_t(0)
    _lib.check(_lib.lib().zk_bn254_groth16_pk_bytes(pk.handle, C.byref(b)))
    return int(b.value)


def test_first_and_third_finalize_and_two_keys_with_different_delta_interleaved():
    parts, r, s, want_base = _bulk(1)
    parts, r, s = parts[:9], r[:9], s[:9]
    k1, k2 = _key("base"), _key("other")
    want = {id(k1): want_base[:9], id(k2): _host_tail(k2, parts, r, s)}
    assert want[id(k1)] != want[id(k2)]
    b1 = _pk_bytes(k1)
    for k in (k1, k2, k1, k2, k1):  # k1 at its first (no delta tables yet), second and third tail, k2 in between
        assert g16.finalize_batch(k, parts, r, s) == want[id(k)]
    assert _pk_bytes(k1) == b1 + FB_TABLE_BYTES  # the tables are the key's: counted with it, freed with it
    tagged = tc.tagged_rows("other")
    p2, r2, s2 = _stack(tagged)
    assert g16.finalize_batch(k2, p2, r2, s2) == [x.expected for x in tagged]
    k1.free()
    k2.free()


def test_two_threads_race_the_first_finalize_of_a_fresh_key():
    parts, r, s, want = _bulk(1)
    pk = _key()
    out, errors = [None, None], []
    gate = threading.Barrier(2)

    def worker(k):
        try:
            lo, hi = (0, 130) if k == 0 else (100, 257)
            gate.wait()
            for _ in range(2):
                out[k] = g16.finalize_batch(pk, parts[lo:hi], r[lo:hi], s[lo:hi])
                assert out[k] == want[lo:hi]
        except Exception as ex:  # noqa: BLE001
            errors.append((k, repr(ex)))

    threads = [threading.Thread(target=worker, args=(k,)) for k in (0, 1)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert out[0] == want[0:130] and out[1] == want[100:257]
    pk.free()


def test_a_freed_key_and_an_unknown_handle_are_refused():
    parts, r, s, want = _bulk(1)
    pk = _key()
    assert g16.finalize_batch(pk, parts[:3], r[:3], s[:3]) == want[:3]
    stale = pk.handle.value
    pk.free()
    L = _lib.lib()
    out = (C.c_uint8 * 384)()
    dev = [_lib.DeviceBuffer.from_numpy(v[:3]) for v in (parts, r, s)]
    d_out = _lib.DeviceBuffer(384)
    for h in (stale, 0x00dead0000beef):
        rc = L.zk_bn254_groth16_finalize_batch(C.c_uint64(h), _lib.vp(parts), C.c_size_t(1), _lib.vp(r), _lib.vp(s), C.c_size_t(3), out)
        assert rc == _lib.ZK_ERR_HANDLE, (hex(h), rc)
        assert _dev_call(h, dev[0].ptr, 1, dev[1].ptr, dev[2].ptr, 3, d_out.ptr) == _lib.ZK_ERR_HANDLE, hex(h)


def test_argument_errors():
    parts, r, s, _ = _bulk(3)
    parts, r, s = np.ascontiguousarray(parts[:4]), np.ascontiguousarray(r[:4]), np.ascontiguousarray(s[:4])
    pk = _key()
    L = _lib.lib()
    sentinel = bytes([0x5A]) * 512
    out = (C.c_uint8 * 512).from_buffer_copy(sentinel)
    good = [_lib.vp(parts), _lib.vp(r), _lib.vp(s), out]

    def host(args, n_partials=3, n=4):
        return L.zk_bn254_groth16_finalize_batch(pk.handle, args[0], C.c_size_t(n_partials), args[1], args[2], C.c_size_t(n), args[3])

    for k in range(4):
        args = list(good)
        args[k] = None
        assert host(args) == _lib.ZK_ERR_ARG, k
    assert host(good, n_partials=0) == _lib.ZK_ERR_ARG
    assert host(good, n=0) == _lib.ZK_OK and bytes(out) == sentinel
    dev = [_lib.DeviceBuffer.from_numpy(v) for v in (parts, r, s)]
    d_out = _lib.DeviceBuffer.from_numpy(np.frombuffer(sentinel, np.uint8))
    ptrs = [dev[0].ptr, dev[1].ptr, dev[2].ptr, d_out.ptr]
    for k in range(4):
        p = list(ptrs)
        p[k] = 0
        assert _dev_call(pk, p[0], 3, p[1], p[2], 4, p[3]) == _lib.ZK_ERR_ARG, k
    assert _dev_call(pk, ptrs[0], 0, ptrs[1], ptrs[2], 4, ptrs[3]) == _lib.ZK_ERR_ARG
    assert _dev_call(pk, ptrs[0], 3, ptrs[1], ptrs[2], 0, ptrs[3]) == _lib.ZK_OK
    assert d_out.to_numpy(np.uint8, (512,)).tobytes() == sentinel
    with pytest.raises(ValueError):
        g16.finalize_batch(pk, parts, r[:3], s)
    assert g16.finalize_batch(pk, np.zeros((0, 3, 96), np.uint64), np.zeros((0, 4), np.uint64), np.zeros((0, 4), np.uint64)) == []
    pk.free()


def test_a_key_over_several_device_entries():
    """host form: row by row through the composite key's combine step, the single-entry bytes; _dev form: refused (tests/groth16_tail_worker.py)"""
    out = subprocess.run([sys.executable, os.path.join(HERE, "groth16_tail_worker.py")], capture_output=True, text=True, timeout=600, env=dict(os.environ, PYTHONPATH=ROOT))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert res and all(res.values()), res


def test_end_to_end_prove_batch_msm5_finalize_batch_verify():
    """log_n = 10: prove_batch on 5 rows == the single prover; the five sums of every row (zk_bn254_groth16_msm5_pk) through finalize_batch == prove_batch; the
    batch verifier accepts"""
    from tests.golden.gen_golden import small_r1cs
    n_public, n_cons, n = 3, 1000, 5
    r1, w0 = small_r1cs(0x77, n_public, n_cons)
    cons = [tuple({wi: mont_limbs([cf])[0] for wi, cf in lin.items()} for lin in con) for con in r1.constraints]
    dev = zk.R1CS(r1.n_public, r1.n_wires, cons)
    pk, vk = zk.setup(dev, mont_limbs(ref.rand_felts(0x78, 5)))
    assert pk.info()["log_domain"] == 10 and g16.batch_info(pk)["batched"]
    ws = []
    for i in range(n):  # the same public wires, other free secret wires; every later wire is the product its constraint defines
        w = list(w0[:n_public]) + [ref.rand_felts(0x900 + i, 1)[0] if i else v for v in w0[n_public:n_public + 3]]
        for L, Rr, _ in r1.constraints:
            dot = lambda lin: sum(cf * w[j] for j, cf in lin.items()) % ref.R  # noqa: E731
            w.append(dot(L) * dot(Rr) % ref.R)
        ws.append(mont_limbs(w))
    ws = np.stack(ws)
    abc = [dev.eval_abc(ws[i]) for i in range(n)]
    a, b, c = (np.stack([abc[i][k] for i in range(n)]) for k in range(3))
    r, s = orc.rand_fr(0x91, n), orc.rand_fr(0x92, n)
    batch = g16.prove_batch(pk, a, b, c, ws, r, s)
    assert batch == [zk.prove(pk, a[i], b[i], c[i], ws[i], r[i], s[i]) for i in range(n)]
    recs = []
    for i in range(n):
        h = g16.compute_h(a[i], b[i], c[i], 10)
        d_w, d_h = _lib.DeviceBuffer.from_numpy(ws[i]), _lib.DeviceBuffer.from_numpy(h)
        recs.append(parallel.groth16_msm5_pk(pk, d_w.ptr, d_h.ptr))
        d_w.free()
        d_h.free()
    assert g16.finalize_batch(pk, np.stack(recs), r, s) == batch
    pubs = np.stack([ws[i][1:n_public] for i in range(n)])
    assert zv.groth16_verify_batch(batch, pk.vk_write_to(vk), pubs).tolist() == [True] * n
    pk.free()
    dev.free()
