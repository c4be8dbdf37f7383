"""The MSM's base-side half (csrc/msm.hip: k_build_table, k_accumulate, k_fold_giant, k_fold_multi, k_reduce_l1, k_reduce_l2, k_reduce_wave in both lane
layouts, msm_finish, k_msm_sets_affine) stage by stage against the discrete-log model of tests/msm_tail_ref.py (-m gpu).

zk_bn254_msm_tail_inspect runs the production table build, preparation, accumulate, folds, reduce levels and finishers with a trace attached to the job and
returns every intermediate array as affine points.  Every base is [k_i] G, so the model's value of any entry is an integer x mod r and the point the device
must hold there is [x] G from the oracle -- one oracle call per stage, over the stage's distinct integers.  Everything is compared EXACTLY (no tolerance
anywhere), entry by entry:
  table        every entry (rows of an infinity base and the entries [n, stride) of a row are (0, 0))
  accumulate   every real task's partial sum (the slots of padding tasks are never written and never compared)
  fold         every bucket that has tasks, at its head slot task_off[b] (the other slots of a split bucket are scratch)
  levels       every A and every S of every level, all W * n_out of them
  finish       every set's value, the total in plain mode; with keep_final the affine points and their 32-byte encodings from k_msm_sets_affine
A failure names the stage, the kernel and the first differing entry with its set, chunk and expected integer.  Every case asserts the branch it reached from
the run's own level descriptors and control block and prints it; the degenerate families also assert, from the model's walker replayed on the RUN's task
plan, that equal / opposite / infinite operands met at the stages they are there for (tests/test_msm_tail_ref_cpu.py pins model and walker without a GPU)."""
import functools
import time

import numpy as np
import pytest

from noir_backend_using_gnark_amd import _lib, bn254
from oracle import oracle as orc
from tests import msm_prep_ref as P
from tests import msm_tail_ref as M

pytestmark = pytest.mark.gpu
TABLE_COMPARE_MAX = 40000   # distinct table entries a test asks the oracle for (above: the giant fold inputs with random bases; every geometry case is below)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    _lib.require_device()  # fail loudly: no silent fallback


@functools.lru_cache(maxsize=4)
def _built(name):
    return M.CASE[name].build()


def expected_points(vals, g2: bool) -> np.ndarray:
    """[x] G for every integer of a stage: one oracle call over the distinct non-zero ones; 0 -> (0, 0)"""
    vals = [int(v) for v in vals]
    uniq = sorted(set(vals) - {0})
    out = np.zeros((len(vals), 16 if g2 else 8), np.uint64)
    if uniq:
        pts = (orc.g2_mul_gen_many if g2 else orc.g1_mul_gen_many)(P.limbs(uniq), scalars_mont=False)
        at = {v: i for i, v in enumerate(uniq)}
        sel = np.array([at.get(v, -1) for v in vals], np.int64)
        out[sel >= 0] = pts[sel[sel >= 0]]
    return out


@functools.lru_cache(maxsize=4)
def _bases(name, g2):
    k, vectors = _built(name)
    return expected_points(k, g2)


def compare(label, stage, dev, want_ints, g2, where):
    """dev: (count, width) affine points; want_ints: the model's integers; where(i) names entry i"""
    kernel = M.KERNEL.get(stage.split()[0], stage)
    assert dev.shape[0] == len(want_ints), "%s: stage %s (%s): %d entries, the model has %d" % (label, stage, kernel, dev.shape[0], len(want_ints))
    want = expected_points(want_ints, g2)
    bad = np.flatnonzero((dev != want).any(axis=1))
    if bad.size:
        i = int(bad[0])
        raise AssertionError("%s: stage %s (%s): entry %d (%s) is not [x] G for the model's x = %d%s: device %s; %d of %d entries differ" % (
            label, stage, kernel, i, where(i), want_ints[i], " (the point at infinity)" if want_ints[i] == 0 else "",
            "(0, 0)" if not dev[i].any() else "x = 0x%016x.." % int(dev[i][3]), bad.size, len(want_ints)))
    return int((~dev.any(axis=1)).sum())


def run_case(case):
    t0 = time.time()
    k, vectors = _built(case.name)
    req = M.request(case, vectors)
    g2, table, skip = bool(req.get("is_g2")), bool(req.get("table_c")), req.get("skip_below", 0)
    n = req.get("n") or vectors[0].shape[0]
    arg = vectors[0] if (len(vectors) == 1 or req.get("rows")) else vectors
    out = bn254.msm_tail_inspect(_bases(case.name, g2), arg, **req)
    label, W, B, c = case.name, out["W"], out["B"], out["c"]
    # ---- the branch the run reached: its own descriptors against the model's restatement and against what the case is named for
    lv = out["levels"]
    want_lv, n_final, sh_final = M.levels(out, W, req.get("l2_m", 0), req.get("quad_tail", False))
    got_lv = [{f: d[f] for f in _lib.MSM_TAIL_LEVEL} for d in lv]
    assert got_lv == want_lv and (out["n_final"], out["sh_final"]) == (n_final, sh_final), "%s: the run's levels %s, n_final %d, sh_final %d; msm_accumulate_batch restated: %s, %d, %d" % (
        label, got_lv, out["n_final"], out["sh_final"], want_lv, n_final, sh_final)
    if case.expect:
        e = case.expect
        assert (M.path(lv), n_final, sh_final, W) == (e["path"], e["n_final"], e["sh_final"], e["W"]), "%s did not reach its branch: %s, n_final %d, sh_final %d, W %d" % (
            label, M.path(lv), n_final, sh_final, W)
    # ---- table
    stride = req.get("stride") or n
    said = ["path %s -> finisher at %d entries, sh %d" % (" -> ".join("%s %d" % p for p in M.path(lv)), n_final, sh_final)]
    if table:
        d = M.table_logs(k, n, c, stride, req.get("row_first", 0), req.get("row_step", 1))
        if len(set(d)) <= TABLE_COMPARE_MAX:
            inf = compare(label, "table", out["table"], d, g2, lambda i: "row %d, point %d" % divmod(i, stride))
            said.append("table %d entries (%d at infinity)" % (len(d), inf))
        else:
            said.append("table of %d distinct entries not compared" % len(set(d)))
    else:
        d = list(k[:n])
    # ---- accumulate, fold
    prep = M.prep_from_run(out)
    assert out["tasks"] == prep["T"]
    e = M.task_sums(d, prep, skip)
    off = prep["task_off"]
    bucket_of = np.searchsorted(off[1:], np.arange(prep["T"]), "right")
    inf = compare(label, "accumulate", out["partial_acc"][:prep["T"]], e, g2, lambda t: "task %d of bucket %d (set %d), %d points" % (
        t, bucket_of[t], bucket_of[t] // B, prep["length"][t]))
    x = M.bucket_sums(e, prep)
    heads = sorted(x)
    compare(label, "fold", out["partial_fold"][[int(off[b]) for b in heads]], [x[b] for b in heads], g2, lambda i: "bucket %d (set %d, bucket %d of it), %d tasks at slot %d" % (
        heads[i], heads[i] // B, heads[i] % B, off[heads[i] + 1] - off[heads[i]], off[heads[i]]))
    said.append("%d tasks of length <= %d (%d partial sums at infinity), %d split buckets, %d giants" % (prep["T"], prep["Lt"], inf, out["ctl"][0], out["ctl"][4]))
    # ---- levels
    per_level = M.run_levels(x, W, B, lv)
    for dsc, (A, S) in zip(lv, per_level):
        N = dsc["n_out"]
        for nm, dev, mod in (("A", dsc["A"], A), ("S", dsc["S"], S)):
            compare(label, "%s %s (level %d -> %d, sh %d -> %d)" % (dsc["kind"], nm, dsc["n_in"], N, dsc["sh_in"], dsc["sh_out"]), dev.reshape(W * N, -1),
                    [v for row in mod for v in row], g2, lambda i: "set %d, chunk %d" % divmod(i, N))
    # ---- finish
    V = [M.set_value(per_level[-1][0][w], per_level[-1][1][w], sh_final) for w in range(W)]
    want = M.expected_values(k, M.case_vectors(case, vectors), n, c, table, req.get("row_first", 0), req.get("row_step", 1), skip)
    assert (V if table else [M.total_plain(V, c)]) == want, "%s: the model on the run's task plan does not end in sum s_i k_i" % label
    if req.get("keep_final"):
        compare(label, "sets_affine", out["final_affine"], V, False, lambda w: "set %d" % w)
        wantp = expected_points(V, False)
        for w in range(W):
            assert bytes(out["final_bytes"][w]) == orc.g1_compress(wantp[w]), "%s: stage sets_affine (k_msm_sets_affine): the encoding of set %d (model x = %d)" % (label, w, V[w])
        said.append("device finish over N = %d" % n_final)
    else:
        compare(label, "finish", out["set_values"], V, g2, lambda w: "set %d" % w)
        if not table:
            compare(label, "finish total", out["total"], [M.total_plain(V, c)], g2, lambda i: "the sum over the windows")
    # ---- reach of the degenerate inputs, on the task plan the device chose
    if case.reach or "sparse" in case.flags:
        wk, _ = M.walk_all(d, prep, W, B, want_lv, sh_final, skip)
        for stage, kind in case.reach:
            cnt = wk.count("finish" if stage in ("finish", "sets_affine") else stage, kind)
            assert cnt > 0, "%s did not reach its operands: no %s pair at %s" % (label, kind, stage)
            said.append("%s: %d %s pairs" % (stage, cnt, kind))
    if "sparse" in case.flags:
        hit = [t for t in range(prep["T"]) if prep["length"][t] >= 3 and e[t] == 0 and bucket_of[t] == M.SPARSE_BUCKET]
        assert hit and not out["partial_acc"][hit[0]].any(), "%s did not reach its branch: no task of infinity bases only" % label
        said.append("task %d holds infinity bases only" % hit[0])
    if "all_zero" in case.flags:
        assert out["dropped"] and out["device_total"] == 0 and prep["T"] == 0 and not out["final_affine"].any()
        said.append("all digits dropped: no task")
    if "zero_row_3" in case.flags:
        assert V[3] == 0 and not out["final_affine"][3].any() and all(V[w] for w in (0, 1, 2, 4))
    if "fold_counts" in case.flags:
        nt = np.diff(off)
        assert {b: int(nt[b]) for b in M.FOLD_TASKS} == M.FOLD_TASKS, "%s did not reach its branch: tasks per bucket %s" % (label, {b: int(nt[b]) for b in M.FOLD_TASKS})
        said.append("buckets of %s tasks" % sorted(M.FOLD_TASKS.values()))
    for f in case.flags:
        if f.startswith("prep:"):
            r = P.CASE[f[5:]].reach
            assert out["ctl"][4] == r["giants"] and len(prep["listed"]) == r.get("listed", r["giants"]), "%s did not reach its branch: %d giants" % (label, out["ctl"][4])
            if "bucket" in r:
                bkt, cnt, tasks = r["bucket"]
                assert (off[bkt + 1] - off[bkt], prep["Lt"]) == (tasks, 32), "%s did not reach its branch: bucket %d in %d tasks" % (label, bkt, off[bkt + 1] - off[bkt])
    print("%s reached: %s (%.2f s)" % (label, "; ".join(said), time.time() - t0))
    return out


GEOMETRY = [c for c in M.CASES if not c.flags & {"fold", "family"}]
FOLDS = [c for c in M.CASES if "fold" in c.flags]
FAMILY = [c for c in M.CASES if "family" in c.flags]


@pytest.mark.parametrize("case", GEOMETRY, ids=lambda c: c.name)
def test_geometry(case):
    """random bases [k_i] G, random scalars, n = 300: the smallest shapes that reach every branch of msm_accumulate_batch's level sequence"""
    run_case(case)


@pytest.mark.parametrize("case", FOLDS, ids=lambda c: c.name)
def test_folds(case):
    """k_fold_giant and k_fold_multi: the giant shapes of the preparation's case table and buckets of 2, 3, 4, 5, 64 and 65 tasks, with random bases and with
    every base the generator (every butterfly step of equal full tasks is a doubling)"""
    run_case(case)


@pytest.mark.parametrize("case", FAMILY, ids=lambda c: c.name)
def test_degenerate_families(case):
    """equal, opposite and infinite operands above level 1: the same point in every bucket; alternating signs (S is infinity throughout); the upper half of a wave
    chunk the negative of the lower (opposite operands in the scan and in the butterfly); a third of the bases at infinity"""
    run_case(case)


def test_device_finish_of_an_empty_job():
    """a table shard that owns no window is the empty job: k_msm_sets_affine runs with N = 0 and writes the point at infinity and its encoding for every row"""
    mat = P._rand(3 * 20, 0x7E0)
    out = bn254.msm_tail_inspect(np.zeros((20, 8), np.uint64), mat, table_c=16, row_first=16, rows=3, n=20, row_stride=20, keep_final=True)
    assert out["total"] == 0 and out["levels"] == [] and out["n_final"] == 0
    assert out["final_affine"].shape == (3, 8) and not out["final_affine"].any()
    assert all(bytes(b) == orc.g1_compress(np.zeros(8, np.uint64)) for b in out["final_bytes"])
    print("empty job reached: k_msm_sets_affine with N = 0 over 3 rows")
