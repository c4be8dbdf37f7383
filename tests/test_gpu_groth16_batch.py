"""Batch Groth16 proving on the device (-m gpu), bit-exact: every row of zk.prove_batch / zk.prove_r1cs_batch is the 128 bytes the single prover writes for
that row, and the oracle's where it is asked.  The oracle is the yardstick; the single prover is the cross-check."""
import threading

import numpy as np
import pytest

import noir_backend_using_gnark_amd as zk
from noir_backend_using_gnark_amd import _lib
from noir_backend_using_gnark_amd import groth16 as g16
from noir_backend_using_gnark_amd import verify as zv
from oracle import bn254_ref as ref
from oracle import oracle as orc
from tests.helpers import golden_pk, h2i, mont_limbs, sha_image

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    _lib.require_device()  # fail loudly: no silent fallback


def _random_pkd(log_n, seed=0):
    """as test_groth16_prove_vs_oracle_random_pk: random valid bases, points at infinity in A, B and G2.B"""
    N = 1 << log_n
    n_wires, n_public = N - 3, 5
    g1, g2 = orc.g1_gen_points, orc.g2_gen_points
    pkd = dict(log_domain=log_n, n_wires=n_wires, n_public=n_public,
               g1_alpha=g1(seed + 1, 1)[0], g1_beta=g1(seed + 2, 1)[0], g1_delta=g1(seed + 3, 1)[0],
               g1_a=g1(seed + 4, n_wires), g1_b=g1(seed + 5, n_wires), g1_k=g1(seed + 6, n_wires - n_public),
               g1_z=g1(seed + 7, N), g2_beta=g2(seed + 8, 1)[0], g2_delta=g2(seed + 9, 1)[0], g2_b=g2(seed + 10, n_wires))
    pkd["g1_a"][7] = 0
    pkd["g1_b"][11] = 0
    pkd["g2_b"][11] = 0
    return pkd


def _rows(log_n, n, seed=100):
    """n rows of (a, b, c, w, r, s) with n_constraints < N: row 0 uniform, row 1 witness-like, row 2 an all-zero w, row 3 = row 1 again with another
    (r, s), then alternating uniform / witness-like"""
    N = 1 << log_n
    n_cons, n_wires = N - 10, N - 3
    a, b, c = (np.stack([orc.rand_fr(seed + 3 * i + k, n_cons) for i in range(n)]) for k in range(3))
    w = np.stack([orc.rand_fr(seed + 1000 + i, n_wires, witness_like=bool(i & 1)) for i in range(n)])
    if n > 2:
        w[2] = 0
    if n > 3:
        a[3], b[3], c[3], w[3] = a[1], b[1], c[1], w[1]
    r, s = orc.rand_fr(seed + 5000, n), orc.rand_fr(seed + 5001, n)
    return a, b, c, w, r, s


def _singles(pk, rows, idx=None):
    a, b, c, w, r, s = rows
    return [zk.prove(pk, a[i], b[i], c[i], w[i], r[i], s[i]) for i in (range(len(w)) if idx is None else idx)]


def test_golden_instances(golden):
    """row 0 is the fixture's (a, b, c, w, r, s) and must be the committed proof; the other rows reuse the witness with other (r, s)"""
    for e in golden["groth16"]:
        pkd = golden_pk(e)
        pk = zk.ProvingKey(pkd["log_domain"], pkd["n_wires"], pkd["n_public"], pkd["g1_alpha"], pkd["g1_beta"], pkd["g1_delta"], pkd["g1_a"],
                           pkd["g1_b"], pkd["g1_k"], pkd["g1_z"], pkd["g2_beta"], pkd["g2_delta"], pkd["g2_b"])
        a, b, c, w = (mont_limbs([h2i(v) for v in e[k]]) for k in ("a", "b", "c", "w"))
        n = 6
        r, s = orc.rand_fr(0x60, n), orc.rand_fr(0x61, n)
        r[0], s[0] = mont_limbs([h2i(e["r"])])[0], mont_limbs([h2i(e["s"])])[0]
        rows = tuple(np.stack([v] * n) for v in (a, b, c, w)) + (r, s)
        got = g16.prove_batch(pk, *rows)
        assert got[0].hex() == e["proof"], e["name"]
        assert got == _singles(pk, rows), e["name"]
        pk.free()


@pytest.mark.parametrize("log_n", [10, 12, 14])
def test_random_keys_every_row_is_the_single_provers(log_n):
    pkd = _random_pkd(log_n)
    pk = zk.ProvingKey(**pkd)
    assert g16.batch_info(pk)["batched"]
    rows = _rows(log_n, 64)
    want = _singles(pk, rows)
    oracle = {}
    for n in (1, 2, 3, 5, 64):
        got = g16.prove_batch(pk, *(v[:n] for v in rows))
        assert len(got) == n
        bad = [i for i in range(n) if got[i] != want[i]]
        assert not bad, (log_n, n, bad)
        for i in (0, n - 1):
            if i not in oracle:
                oracle[i] = orc.groth16_prove(pkd, *(v[i] for v in rows))[0]
            assert got[i] == bytes(oracle[i]), (log_n, n, i)
    pk.free()


def test_more_than_one_chunk_and_not_a_multiple_of_it():
    log_n = 10
    pkd = _random_pkd(log_n, seed=40)
    pk = zk.ProvingKey(**pkd)
    info = g16.batch_info(pk)
    assert info["batched"] and info["chunk_rows"] >= 1
    n = 2 * info["chunk_rows"] + 3
    pool = _rows(log_n, 8, seed=300)
    pick = np.arange(n) % 8
    rows = tuple(v[pick] for v in pool[:4]) + (orc.rand_fr(0x70, n), orc.rand_fr(0x71, n))
    got = g16.prove_batch(pk, *rows)
    want = _singles(pk, rows)
    bad = [i for i in range(n) if got[i] != want[i]]
    assert not bad, (info, bad)
    for i in (0, info["chunk_rows"], n - 1):  # the first row of the first two chunks and the last row of the short one
        assert got[i] == bytes(orc.groth16_prove(pkd, *(v[i] for v in rows))[0]), i
    pk.free()


@pytest.mark.parametrize("full_width", [False, True])
def test_device_pointers_give_the_same_bytes_and_are_only_read(full_width):
    log_n, n = 10, 7
    N = 1 << log_n
    pk = zk.ProvingKey(**_random_pkd(log_n, seed=60))
    a, b, c, w, r, s = _rows(log_n, n, seed=500)
    if full_width:  # n_constraints == N
        a, b, c = (np.concatenate([v, np.stack([orc.rand_fr(900 + k, 10) for _ in range(n)])], axis=1) for k, v in enumerate((a, b, c)))
        assert a.shape[1] == N
    want = g16.prove_batch(pk, a, b, c, w, r, s)
    assert want == _singles(pk, (a, b, c, w, r, s))
    dev = [_lib.DeviceBuffer.from_numpy(v) for v in (a, b, c, w)]
    before = [sha_image(d.to_numpy(np.uint64, v.shape)) for d, v in zip(dev, (a, b, c, w))]
    assert before == [sha_image(v) for v in (a, b, c, w)]
    got = g16.prove_batch(pk, *dev, r, s, on_device=True, n_constraints=a.shape[1])
    assert got == want
    assert [sha_image(d.to_numpy(np.uint64, v.shape)) for d, v in zip(dev, (a, b, c, w))] == before
    pk.free()


@pytest.mark.parametrize("how", ["no_tables", "table_window_bits", "large_domain"])
def test_shapes_the_batched_path_may_not_serve_give_the_same_bytes(how):
    log_n = 17 if how == "large_domain" else 10
    n = 3 if how == "large_domain" else 5
    pkd = _random_pkd(log_n, seed=80)
    kw = dict(precompute_tables=False) if how == "no_tables" else dict(table_window_bits=11) if how == "table_window_bits" else {}
    pk = zk.ProvingKey(**pkd, **kw)
    if how != "table_window_bits":
        assert not g16.batch_info(pk)["batched"]
    rows = _rows(log_n, n, seed=700)
    got = g16.prove_batch(pk, *rows)
    assert got == _singles(pk, rows)
    assert got[n - 1] == bytes(orc.groth16_prove(pkd, *(v[n - 1] for v in rows))[0])
    pk.free()


def test_argument_errors_with_a_key():
    pk = zk.ProvingKey(**_random_pkd(10, seed=90))
    a, b, c, w, r, s = _rows(10, 2, seed=800)
    with pytest.raises(ValueError, match="wires of the proving key"):
        g16.prove_batch(pk, a, b, c, w[:, :-1], r, s)
    wide = np.zeros((2, (1 << 10) + 1, 4), np.uint64)
    with pytest.raises(_lib.ZkmiError, match="exceeds the domain size") as ei:
        g16.prove_batch(pk, wide, wide, wide, w, r, s)
    assert ei.value.code == _lib.ZK_ERR_ARG
    pk.free()


def test_prove_r1cs_batch_on_the_golden_r1cs(golden):
    from tests.golden.gen_golden import small_r1cs
    e = next(x for x in golden["groth16"] if x["name"] == "seq_r1cs_13")
    r1 = small_r1cs(0x51, 3, 13)[0]
    cons = [tuple({wi: mont_limbs([cf])[0] for wi, cf in lin.items()} for lin in con) for con in r1.constraints]
    dev = zk.R1CS(r1.n_public, r1.n_wires, cons)
    pk, vk = zk.setup(dev, mont_limbs(ref.rand_felts(0x70, 5)))
    vkb = pk.vk_write_to(vk)
    w = mont_limbs([h2i(v) for v in e["w"]])
    n = 9
    ws = np.stack([w] * n)
    r, s = orc.rand_fr(0x80, n), orc.rand_fr(0x81, n)
    r[0], s[0] = mont_limbs([h2i(e["r"])])[0], mont_limbs([h2i(e["s"])])[0]
    got = g16.prove_r1cs_batch(dev, pk, ws, r, s)
    assert got[0].hex() == e["proof"]
    assert got == [zk.prove_r1cs(dev, pk, ws[i], r[i], s[i]) for i in range(n)]
    pubs = np.stack([w[1:r1.n_public]] * n)
    assert zv.groth16_verify_batch(got, vkb, pubs).tolist() == [True] * n
    ws[4, -1] = mont_limbs([(h2i(e["w"][-1]) + 1) % ref.R])[0]  # one wire of one row changed: that row's proof no longer verifies
    got = g16.prove_r1cs_batch(dev, pk, ws, r, s)
    assert got == [zk.prove_r1cs(dev, pk, ws[i], r[i], s[i]) for i in range(n)]
    assert zv.groth16_verify_batch(got, vkb, pubs).tolist() == [i != 4 for i in range(n)]
    with pytest.raises(ValueError, match="wires of the constraint system"):
        g16.prove_r1cs_batch(dev, pk, ws[:, :-1], r, s)
    pk.free()
    dev.free()


def test_two_threads_batching_against_one_key():
    """as test_concurrent_callers_are_safe: two host threads, each with its own batch against the same key, get what they get when run one after the other"""
    log_n = 10
    pk = zk.ProvingKey(**_random_pkd(log_n, seed=20))
    jobs = [_rows(log_n, 9, seed=2000), _rows(log_n, 12, seed=3000)]
    serial = [g16.prove_batch(pk, *rows) for rows in jobs]
    assert serial[0] == _singles(pk, jobs[0])
    out, errors = [None, None], []

    def worker(k):
        try:
            for _ in range(3):
                out[k] = g16.prove_batch(pk, *jobs[k])
                assert out[k] == serial[k]
        except Exception as ex:  # noqa: BLE001
            errors.append((k, repr(ex)))

    threads = [threading.Thread(target=worker, args=(k,)) for k in (0, 1)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert out == serial
    pk.free()
