"""The MSM's scalar preparation (csrc/msm.hip msm_prepare: recoding, radix sort, bucket bounds, task length, task plan, task records) stage by stage
against the host model of tests/msm_prep_ref.py, and the same inputs through to the sum (-m gpu).

zk_bn254_msm_prep_inspect runs the production preparation through the wrappers the provers call and copies every intermediate back.  Everything is
compared exactly (integers; no tolerance anywhere):
  digits + sort   without dropping the sort is stable: sorted keys and values equal numpy's stable argsort of the model's pairs element for element; with the
                  zero digits dropped the workgroups land in arrival order: the pair count, the sorted keys and the per-bucket multisets of values
  bounds          start == searchsorted(keys, 0 .. nb)
  task length     Lmin <= ctl[2] <= L (what the device picks in between is its own business)
  task plan       tasks per bucket = ceil(count / ctl[2]), task_off their exclusive prefix sum, multi_list the buckets of more than one task, the giants
  task records    the real tasks partition [0, start[nb]) bucket by bucket, in task_off's order
  task sort       a permutation of [0, max_tasks): real tasks first by non-decreasing quantised length key, padding behind
Every case asserts -- from the plan the run returns and from ctl -- that it reached the branch it is named for (tests/test_msm_prep_ref_cpu.py asserts the
same geometry without a GPU), and a failure names the stage.  Whether the zero digits were dropped is read from the run (`dropped`: the preparation handed out
its device-side pair counter), and every compaction input holds zero digits, so a run that lost the switch fails its pair count as well.
The sums of section 4 go through the entries the provers' callers have (g1_multi_exp, ResidentBases.multi_exp / multi_exp_batch): those prepare WITHOUT
dropping, so the compaction and device-length inputs reach k_accumulate through the non-dropping preparation of the same scalars; the dropped-digit path is
tied to sums by the PLONK and Groth16 prover tests.
One regression this file cannot report by name: a k_bucket_bounds that leaves start[nb] unwritten (`b >= nb` for `b > nb`) hands k_task_fill a negative task
length and k_task_scatter an index outside its arrays -- the run ends in a device fault, not in a failed assertion."""
import functools
import time

import numpy as np
import pytest

import noir_backend_using_gnark_amd as zk
from noir_backend_using_gnark_amd import _lib, bn254
from oracle import oracle as orc
from tests import msm_prep_ref as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    _lib.require_device()  # fail loudly: no silent fallback


def _first_diff(a, b):
    if a.shape != b.shape:
        return "lengths %d / %d" % (a.size, b.size)
    i = int(np.flatnonzero(a != b)[0])
    return "first at %d: device %d, model %d (%d differ)" % (i, int(a[i]), int(b[i]), int((a != b).sum()))


def check_stages(label, out, model_keys, model_vals, nb, drop=False):
    """every stage of one inspected preparation against the model's pairs; returns what the reach checks look at"""
    total, dt, ctl = out["total"], out["device_total"], out["ctl"].astype(np.int64)
    assert nb == out["nb"], (label, "plan: nb", out["nb"], nb)
    sk, sv = M.sort_pairs(model_keys, model_vals)
    # ---- 1-2. digits + sort
    assert out["dropped"] == bool(drop), "%s: stage digits: the run %s the compacting recoding (k_msm_digits_compact)" % (label, "took" if out["dropped"] else "did not take")
    if drop:
        assert dt == sk.size, "%s: stage digits (k_msm_digits_compact): the device counts %d non-zero digits, the recoding has %d" % (label, dt, sk.size)
    else:
        assert dt == total == sk.size, "%s: stage digits: pair count %d / %d / %d" % (label, dt, total, sk.size)
    dk = out["keys"][:dt]
    dv = M.unsigned_sentinels(dk, out["vals"][:dt], nb)
    if drop or not (np.array_equal(dk, sk) and np.array_equal(dv, sv)):
        ck, cv = M.canonical_multiset(dk, dv)
        wk, wv = M.canonical_multiset(sk, sv)
        assert np.array_equal(ck, wk), "%s: stage digits (k_msm_digits*) or sort (k_rs_*): the keys are not the recoding's: %s" % (label, _first_diff(ck, wk))
        assert np.array_equal(cv, wv), "%s: stage digits (k_msm_digits*) or sort (k_rs_*): the values inside a bucket are not the recoding's: %s" % (
            label, _first_diff(cv, wv))
        assert np.array_equal(dk, sk), "%s: stage sort (k_rs_hist / k_rs_scan_rows / k_rs_scatter): right pairs, keys out of order: %s" % (label, _first_diff(dk, sk))
        assert drop, "%s: stage sort (k_rs_scatter): right pairs, sorted keys, but not STABLE: %s" % (label, _first_diff(dv, sv))
    # ---- 3. bounds
    start = out["start"]
    want_start = M.bounds(sk, nb)
    assert np.array_equal(start, want_start), "%s: stage bounds (k_bucket_bounds): %s" % (label, _first_diff(start, want_start))
    # ---- 4. task length
    L, Lmin, Lt = out["L"], out["Lmin"], int(ctl[2])
    assert Lmin <= Lt <= L, "%s: stage task length (k_pick_len / k_bucket_stats_pick): %d outside [%d, %d]" % (label, Lt, Lmin, L)
    counts = np.diff(start)
    # ---- 4. task plan
    nt = (counts.astype(np.int64) + Lt - 1) // Lt
    want_off = np.zeros(nb + 1, np.int64)
    np.cumsum(nt, out=want_off[1:])
    task_off = out["task_off"]
    assert np.array_equal(task_off, want_off), "%s: stage task plan (k_task_plan_scan / k_xs_apply): task_off: %s" % (label, _first_diff(task_off, want_off))
    multi = np.sort(out["multi_list"][:ctl[0]])
    want_multi = np.flatnonzero(nt > 1)
    assert np.array_equal(multi, want_multi), "%s: stage task plan (k_task_plan_scan): multi_list holds %d buckets, %d have more than one task" % (label, multi.size, want_multi.size)
    giants = np.flatnonzero(nt > M.GIANT_T)
    listed = ctl[8:8 + min(int(ctl[4]), M.GIANT_MAX)]
    assert ctl[4] == giants.size, "%s: stage task plan (k_task_plan_scan): %d giant buckets counted, %d have more than GIANT_T tasks" % (label, ctl[4], giants.size)
    assert np.unique(listed).size == listed.size and np.isin(listed, giants).all(), "%s: stage task plan (k_task_plan_scan): the listed giants %s" % (label, listed)
    # ---- 4b. task records and their sort
    T, max_tasks = int(want_off[-1]), out["max_tasks"]
    tids, lk, begin = out["task_ids"], out["len_keys"], out["task_begin"]
    assert T <= max_tasks and tids.size == max_tasks
    assert np.array_equal(np.sort(tids), np.arange(max_tasks, dtype=np.uint32)), "%s: stage task sort (k_task_scatter): the task ids are no permutation of [0, %d)" % (label, max_tasks)
    assert (lk[:T] != M.PAD).all() and (lk[T:] == M.PAD).all() and (tids[:T] < T).all(), "%s: stage task sort (k_task_scatter): real tasks first, padding behind" % label
    bshift = M.geometry(out)["bshift"]
    assert (np.diff((lk[:T] >> bshift).astype(np.int64)) >= 0).all(), "%s: stage task sort (k_task_bins / k_task_scatter): length keys not in order" % label
    length = np.zeros(T, np.int64)
    length[tids[:T]] = L - lk[:T].astype(np.int64)
    b = begin[:T].astype(np.int64)
    stage = "%s: stage task records (k_task_fill): " % label
    assert ((length >= 1) & (length <= Lt)).all(), stage + "a task of %d points (task length %d)" % (int(length.min(initial=0)), Lt)
    bucket = np.searchsorted(task_off[1:], np.arange(T), "right")   # the bucket whose task range holds task t
    assert (b >= start[bucket]).all() and (b + length <= start[bucket + 1]).all(), stage + "a task outside its bucket"
    order = np.argsort(b, kind="stable")
    bs, ls = b[order], length[order]
    nnz = int(start[nb])
    assert (T == 0 and nnz == 0) or (bs[0] == 0 and (bs[1:] == bs[:-1] + ls[:-1]).all() and bs[-1] + ls[-1] == nnz), stage + "the tasks do not partition [0, %d)" % nnz
    return dict(counts=counts, nt=nt, Lt=Lt, T=T, ctl=ctl, length=length, bucket=bucket)


def model_pairs(vectors, out, req):
    table = bool(req.get("table_c"))
    n = req.get("n") or vectors[0].shape[0]
    return M.pairs(vectors, n, out["c"], table=table, stride=req.get("stride") or n, row_first=req.get("row_first", 0), row_step=req.get("row_step", 1),
                   drop=M.geometry(out, req.get("drop_zero_digits", False))["compacts"])


def inspect(vectors, req, **kw):
    if req.get("rows"):
        return bn254.msm_prep_inspect(vectors[0], **dict(req, **kw))
    return bn254.msm_prep_inspect(vectors if len(vectors) > 1 else vectors[0], **dict(req, **kw))


def row_vectors(mat, req):
    return [mat[v * req["row_stride"]:v * req["row_stride"] + req["n"]] for v in range(req["rows"])]


# ------------------------------------------------------------------------------------------------------------ 3a digits
@pytest.mark.parametrize("mode,c", [("plain", c) for c in range(2, 23)] + [("table", c) for c in range(8, 25)])
def test_digits_every_width_on_edge_scalars(mode, c):
    """n = 300 (a full workgroup and a partial one): the edge scalars of width c, canonical and as Montgomery images; the stable sort makes the sorted
    pairs a function of the recoding alone"""
    can = M.digit_vector(c, 300, 0xD16 + c)
    req = dict(table_c=c) if mode == "table" else dict(window_bits=c)
    for mont, vec in ((False, can), (True, M.to_mont(can))):
        out = inspect([vec], req, scalars_mont=mont, arrays=("keys", "vals"))
        assert out["c"] == c and out["Wd"] == M.windows(c) and out["total"] == 300 * M.windows(c)
        mk, mv, nb = model_pairs([can], out, req)
        sk, sv = M.sort_pairs(mk, mv)
        label = "%s c=%d mont=%d" % (mode, c, mont)
        assert np.array_equal(out["keys"], sk), "%s: stage digits (k_msm_digits): keys: %s" % (label, _first_diff(out["keys"], sk))
        dv = M.unsigned_sentinels(out["keys"], out["vals"], nb)
        assert np.array_equal(dv, sv), "%s: stage digits (k_msm_digits): values: %s" % (label, _first_diff(dv, sv))
        if c >= 8 and mode == "table":   # the compacting kernel recodes with code of its own
            dr = inspect([vec], dict(req, drop_zero_digits=True), scalars_mont=mont, arrays=("keys", "vals"))
            live = sk != nb
            assert dr["dropped"] and not out["dropped"], "%s: stage digits: drop_zero_digits did not select the compacting recoding" % label
            assert dr["device_total"] == live.sum(), "%s: stage digits (k_msm_digits_compact): pair count" % label
            ck, cv = M.canonical_multiset(dr["keys"][:dr["device_total"]], dr["vals"][:dr["device_total"]])
            wk, wv = M.canonical_multiset(sk[live], sv[live])
            assert np.array_equal(ck, wk) and np.array_equal(cv, wv), "%s: stage digits (k_msm_digits_compact): pairs" % label


TABLE_SHAPES = [("stride_above_n", dict(table_c=13, stride=333))] + \
    [("shard_%d_of_%d" % (f, s), dict(table_c=13, stride=307, row_first=f, row_step=s)) for s in (2, 3) for f in range(s)] + \
    [("shard_first_row_at_Wd", dict(table_c=13, stride=300, row_first=20, row_step=2)), ("shard_first_row_above_Wd", dict(table_c=13, stride=300, row_first=23, row_step=3))]


@pytest.mark.parametrize("name,req", TABLE_SHAPES, ids=[t[0] for t in TABLE_SHAPES])
@pytest.mark.parametrize("drop", [False, True], ids=["keep", "drop"])
def test_table_strides_and_window_shards(name, req, drop):
    """table c = 13 (20 windows): rows further apart than the vector is long; every shard of a two- and three-way window sharding (the carry runs through the
    windows a shard does not own); a shard that owns no window is the empty plan: total 0, nothing touched"""
    can = M.digit_vector(13, 300, 0xD17)
    req = dict(req, drop_zero_digits=drop)
    out = inspect([can], req)
    if req.get("row_first", 0) >= 20:
        assert out["total"] == 0 and out["nb"] == 0 and out["keys"].size == 0 and not out["ctl"].any()
        return
    assert out["Wrows"] == len(M.table_rows(13, req.get("row_first", 0), req.get("row_step", 1))) and out["total"] == 300 * out["Wrows"]
    mk, mv, nb = model_pairs([can], out, req)
    check_stages(name, out, mk, mv, nb, drop)


@pytest.mark.parametrize("drop", [False, True], ids=["keep", "drop"])
def test_batches_by_pointers_and_by_rows(drop):
    """two and three vectors through pointers (two of them the same vector), five as the rows of a matrix whose rows are further apart than they are long"""
    a, b = M.digit_vector(14, 300, 0xD18), orc.rand_fr(0xD19, 300, mont=False, witness_like=True)
    for vecs in ([a, a], [a, b, a], [b, a, a]):
        req = dict(table_c=14, drop_zero_digits=drop)
        out = inspect(vecs, req)
        assert out["W"] == len(vecs) and out["nb"] == len(vecs) << 13
        mk, mv, nb = model_pairs(vecs, out, req)
        check_stages("%d sets by pointers" % len(vecs), out, mk, mv, nb, drop)
    mat = np.concatenate([M.digit_vector(14, 300, 0xD1A), orc.rand_fr(0xD1B, 5 * 311 - 300, mont=False)])
    req = dict(table_c=14, rows=5, n=300, row_stride=311, stride=305, drop_zero_digits=drop)
    out = inspect([mat], req)
    assert out["W"] == 5
    mk, mv, nb = model_pairs(row_vectors(mat, req), out, req)
    check_stages("5 sets by rows", out, mk, mv, nb, drop)


# ------------------------------------------------------------------------------------------------------------ 3b - 3d: the case table
@functools.lru_cache(maxsize=None)   # (a few megabytes at most: the stage test and the sum test of a case share one build)
def _vectors(name):
    return M.CASE[name].build()


def _reach(case, out, geo, st):
    """the branch the case is named for, from the plan the run returned and from what the run left in ctl / the arrays"""
    said = []
    for k, want in case.expect.items():
        assert geo[k] == want, "%s did not reach its branch: %s is %s, not %s" % (case.name, k, geo[k], want)
        said.append("%s=%s" % (k, want))
    r, counts, nt, ctl = case.reach, st["counts"], st["nt"], st["ctl"]
    if "device_total" in r:
        assert out["device_total"] == r["device_total"] < out["total"], (case.name, out["device_total"])
        assert (out["device_total"] + 8191) // 8192 == r.get("tiles_filled", 0) <= geo["sort_tiles"]   # the launch is sized for total, the device's length fills less
        said.append("device_total=%d of %d" % (out["device_total"], out["total"]))
    if geo["compacts"]:
        assert out["dropped"] and out["device_total"] < out["total"], "%s did not reach its branch: dropped=%s, %d of %d pairs" % (
            case.name, out["dropped"], out["device_total"], out["total"])
        said.append("dropped: %d of %d pairs" % (out["device_total"], out["total"]))
    elif case.req.get("drop_zero_digits"):
        assert not out["dropped"] and out["device_total"] == out["total"], "%s did not reach its branch: the fallback dropped digits" % case.name
        said.append("fell back to the non-dropping recoding")
    if "tasks" in r:
        assert st["T"] == r["tasks"] and not out["start"].any()
    if "largest" in r:
        assert counts.max() == r["largest"] and (counts > 0).sum() == 1
    if "bucket" in r:
        bkt, cnt, tasks = r["bucket"]
        assert (counts[bkt], nt[bkt], st["Lt"]) == (cnt, tasks, 32), "%s did not reach its branch: bucket %d holds %d points in %d tasks of %d" % (
            case.name, bkt, counts[bkt], nt[bkt], st["Lt"])
        said.append("bucket %d: %d points, %d tasks" % (bkt, cnt, tasks))
        if tasks > 64 * 64:
            assert ((tasks + 63) // 64 + 63) // 64 * 64 == 128   # giant_seg
    if "giants" in r:
        assert ctl[4] == r["giants"], "%s did not reach its branch: %d giants" % (case.name, ctl[4])
        want_listed = r.get("listed", r["giants"])
        assert min(int(ctl[4]), M.GIANT_MAX) == want_listed
        said.append("giants=%d listed=%d" % (ctl[4], want_listed))
    if "last_task_len" in r:
        bkt = r["bucket"][0]
        last = int(out["task_off"][bkt + 1]) - 1
        assert st["length"][last] == r["last_task_len"] and st["bucket"][last] == bkt
    if geo["stats_pick"]:
        assert ctl[1] > 0 or out["device_total"] == 0   # k_bucket_stats_pick left its statistics
        said.append("stats_pick: largest=%d picked L=%d in [%d, %d]" % (ctl[1], st["Lt"], out["Lmin"], out["L"]))
    print("%s reached: %s" % (case.name, ", ".join(said)))


@pytest.mark.parametrize("case", M.CASES, ids=lambda c: c.name)
def test_stages(case):
    t0 = time.time()
    vectors = _vectors(case.name)
    out = inspect(vectors, case.req)
    geo = M.geometry(out, case.req.get("drop_zero_digits", False))
    vecs = row_vectors(vectors[0], case.req) if case.req.get("rows") else vectors
    mk, mv, nb = model_pairs(vecs, out, case.req)
    st = check_stages(case.name, out, mk, mv, nb, geo["compacts"])
    _reach(case, out, geo, st)
    if case.name == "compact_c7_falls_back":   # the documented fallback: the result is the non-dropping one
        keep = inspect(vectors, dict(case.req, drop_zero_digits=False))
        assert out["device_total"] == out["total"] and all(np.array_equal(out[k], keep[k]) for k in ("keys", "vals", "start", "task_off"))
    print("%s: stages in %.2f s" % (case.name, time.time() - t0))


# ------------------------------------------------------------------------------------------------------------ 4: the same inputs through to the sum
@functools.lru_cache(maxsize=None)
def _points(n, g2):
    return (orc.g2_gen_points if g2 else orc.g1_gen_points)(0x900 + n, n)


def _sum(case, vectors, g2):
    n = vectors[0].shape[0]
    pts, msm = _points(n, g2), (orc.g2_msm if g2 else orc.g1_msm)
    want = [msm(pts, v, scalars_mont=False) for v in vectors]
    c = case.req.get("table_c")
    if not c:
        cfg = zk.MultiExpConfig(window_bits=case.req["window_bits"])
        got = [(zk.g2_multi_exp if g2 else zk.g1_multi_exp)(pts, vectors[0], config=cfg)]
    else:
        rb = bn254.ResidentBases(pts, is_g2=g2, table_window_bits=c)
        try:
            got = list(rb.multi_exp_batch(vectors)) if len(vectors) > 1 else [rb.multi_exp(vectors[0])]
        finally:
            rb.free()
    for v, (g, w) in enumerate(zip(got, want)):
        assert (g == w).all(), "%s: the %s sum of vector %d differs from the oracle's" % (case.name, "G2" if g2 else "G1", v)


@pytest.mark.parametrize("case", [c for c in M.CASES if c.groups], ids=lambda c: c.name)
def test_same_inputs_through_to_the_sum(case):
    """k_accumulate, k_fold_giant, k_fold_multi and the reduce levels behind every boundary shape: G1 (the two giant shapes in G2 too) against the oracle.
    These entries prepare without dropping zero digits, whatever the case's request says (module docstring)."""
    t0 = time.time()
    vectors = _vectors(case.name)
    _sum(case, vectors, False)
    if case.groups == "g1g2":
        _sum(case, vectors, True)
    print("%s: sums in %.2f s" % (case.name, time.time() - t0))
