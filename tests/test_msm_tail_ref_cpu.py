"""The discrete-log model of the MSM's base-side half (tests/msm_tail_ref.py) and its case table, pinned without a GPU.  For every case the model builds
its OWN preparation (pairs, stable sort, bounds, a task plan) at the shortest and at the longest task length the device may pick, and asserts
  the invariant  sum_j A_j + 2^sh sum_j j S_j = sum_k (k + 1) x[w, k]  at every level and set,
  the end        the sets' values, and in plain mode the total, equal what the MSM is for (sum_i s_i k_i mod r), whatever the task length,
  the walker     its replay of the kernels' additions gives the closed formulas' values at every stage,
  the geometry   the production planner (zk_bn254_msm_tail_inspect's plan-only form: host work) states the level sequence the case is named for, and the
                 model's restatement of msm_accumulate_batch agrees with it,
  the reach      the walker counts equal / opposite / infinite operand pairs at the stages a degenerate case is there for.
A handful of tiny cases tie the integers to points: [model] G equals oracle.bn254_ref.msm_naive over the points [k_i] G."""
import functools

import numpy as np
import pytest

from noir_backend_using_gnark_amd import _lib, bn254
from oracle import bn254_ref as ref
from tests import msm_prep_ref as P
from tests import msm_tail_ref as M


@functools.lru_cache(maxsize=4)
def built(name):
    return M.CASE[name].build()


def plan_of(case, vectors):
    req = M.request(case, vectors)
    n = req.get("n") or vectors[0].shape[0]
    pts = np.zeros((n, 16 if req.get("is_g2") else 8), np.uint64)   # (plan only: never read)
    arg = vectors[0] if (len(vectors) == 1 or req.get("rows")) else vectors
    return req, n, bn254.msm_tail_inspect(pts, arg, plan_only=True, **req)


def model_of(case, k, vectors, plan, req, n, Lt):
    table, c = bool(req.get("table_c")), plan["c"]
    stride = req.get("stride") or n
    vecs = M.case_vectors(case, vectors)
    prep = M.own_prep(vecs, n, c, Lt, table=table, stride=stride, row_first=req.get("row_first", 0), row_step=req.get("row_step", 1))
    d = M.table_logs(k, n, c, stride, req.get("row_first", 0), req.get("row_step", 1)) if table else list(k[:n])
    return prep, d, vecs


# the fold cases have a G2 twin with the same integers: once is enough here
CPU_CASES = [c for c in M.CASES if not ("fold" in c.flags and c.req.get("is_g2"))]


@pytest.mark.parametrize("case", CPU_CASES, ids=lambda c: c.name)
def test_model_invariant_end_value_walker_geometry_and_reach(case):
    k, vectors = built(case.name)
    req, n, plan = plan_of(case, vectors)
    W, B, c = plan["W"], plan["B"], plan["c"]
    table, skip = bool(req.get("table_c")), req.get("skip_below", 0)
    # ---- geometry: the planner's level sequence is the one the case is named for, and the model restates it
    lv, n_final, sh_final = M.levels(plan, W, req.get("l2_m", 0), req.get("quad_tail", False))
    strip = lambda ds: [{f: d[f] for f in _lib.MSM_TAIL_LEVEL} for d in ds]   # noqa: E731
    assert strip(plan["levels"]) == strip(lv) and (plan["n_final"], plan["sh_final"]) == (n_final, sh_final), (case.name, plan["levels"], lv)
    if case.expect:
        e = case.expect
        assert (M.path(lv), n_final, sh_final, W) == (e["path"], e["n_final"], e["sh_final"], e["W"]), (case.name, M.path(lv), n_final, sh_final, W)
    want = M.expected_values(k, M.case_vectors(case, vectors), n, c, table, req.get("row_first", 0), req.get("row_step", 1), skip)
    for Lt in sorted({plan["Lmin"], plan["L"]}):
        prep, d, vecs = model_of(case, k, vectors, plan, req, n, Lt)
        e = M.task_sums(d, prep, skip)
        x = M.bucket_sums(e, prep)
        per_level = M.run_levels(x, W, B, lv)
        for dsc, (A, S) in zip(lv, per_level):
            assert len(A) == W and len(A[0]) == dsc["n_out"]
            for w in range(W):
                assert M.set_value(A[w], S[w], dsc["sh_out"]) == M.bucket_value(x, w, B), "%s: invariant at %s, set %d, task length %d" % (case.name, dsc["kind"], w, Lt)
        V = [M.set_value(per_level[-1][0][w], per_level[-1][1][w], sh_final) for w in range(W)]
        assert (V if table else [M.total_plain(V, c)]) == want, "%s: the end value at task length %d" % (case.name, Lt)
        # ---- the walker computes the same values addition by addition
        wk, got = M.walk_all(d, prep, W, B, lv, sh_final, skip)
        assert got["tasks"] == e and got["heads"] == x and got["values"] == V
        assert [(a, s) for a, s in got["levels"]] == [(a, s) for a, s in per_level], "%s: the walker's levels at task length %d" % (case.name, Lt)
        for stage, kind in case.reach:
            fin = stage in ("finish", "sets_affine")
            assert wk.count("finish" if fin else stage, kind) > 0, "%s at task length %d: no %s operands at %s: %s" % (
                case.name, Lt, kind, stage, {s: dict(n) for s, n in wk.n.items()})
        if "sparse" in case.flags:
            hit = [t for t in range(prep["T"]) if all(d[v >> 1] == 0 for v in prep["vals"][prep["begin"][t]:prep["begin"][t] + prep["length"][t]].tolist() if (v >> 1) >= skip)]
            assert hit and any(prep["length"][t] >= 3 for t in hit), "%s: no task made of infinity bases only" % case.name
        if "fold_counts" in case.flags:
            nt = np.diff(prep["task_off"])
            assert {b: int(nt[b]) for b in M.FOLD_TASKS} == M.FOLD_TASKS and Lt == 32


def test_families_hold_what_they_are_named_for():
    """same point: every A and every S of a level is one value; alternating sign: S is infinity throughout; cancelling halves: the upper half of a wave chunk's
    S is the negative of the lower"""
    for name, check in (("same_point_table_c15_l16_l2", "same"), ("alternating_sign_table_c15_l16_l2", "alt"), ("cancelling_halves_table_c11", "cancel"),
                        ("cancelling_halves_quad_table_c11", "cancel")):
        case = M.CASE[name]
        k, vectors = built(name)
        req, n, plan = plan_of(case, vectors)
        lv, n_final, sh_final = M.levels(plan, plan["W"], req.get("l2_m", 0), req.get("quad_tail", False))
        prep, d, _ = model_of(case, k, vectors, plan, req, n, plan["L"])
        per_level = M.run_levels(M.bucket_sums(M.task_sums(d, prep), prep), plan["W"], plan["B"], lv)
        for dsc, (A, S) in zip(lv, per_level):
            if check == "same":
                assert len(set(A[0])) == 1 and len(set(S[0])) == 1 and A[0][0] and S[0][0], (name, dsc["kind"])
            if check == "alt":
                assert not any(S[0]) and all(A[0]), (name, dsc["kind"])
        if check == "cancel":
            S1, fan = per_level[0][1][0], lv[1]["m"]
            for q in range(len(S1) // fan):
                lo, hi = S1[q * fan:q * fan + fan // 2], S1[q * fan + fan // 2:(q + 1) * fan]
                assert all(a and (a + b) % M.R == 0 for a, b in zip(lo, hi)), (name, q)


@pytest.mark.parametrize("mode,c", [("plain", 3), ("plain", 5), ("table", 8)])
def test_model_integers_are_the_points_of_the_naive_msm(mode, c):
    """n = 6 points [k_i] G, one of them the point at infinity: [the model's end value] G is the naive sum of s_i P_i"""
    n = 6
    k = M.rand_k(n, 0x6A0 + c)
    k[2] = 0
    vec = P.digit_vector(c, 11, 0x6A1)[[2, 3, 6, 7, 8, 9]]   # r - 1, r - 2 and the all-B / carry scalars of this width
    table = mode == "table"
    B = 1 << (c - 1)
    plan = dict(B=B, m1=min(8, B), N1=B // min(8, B))
    W = 1 if table else P.windows(c)
    lv, n_final, sh_final = M.levels(plan, W)
    prep = M.own_prep([vec], n, c, 32, table=table, stride=n)
    d = M.table_logs(k, n, c, n) if table else k
    per_level = M.run_levels(M.bucket_sums(M.task_sums(d, prep), prep), W, B, lv)
    V = [M.set_value(per_level[-1][0][w], per_level[-1][1][w], sh_final) for w in range(W)]
    got = V[0] if table else M.total_plain(V, c)
    pts = [ref.g1_mul(ref.G1_GEN, x) if x else None for x in k]
    assert ref.g1_mul(ref.G1_GEN, got) == ref.msm_naive(ref.FP, pts, P.ints(vec))
    if table:   # a table entry is the point the doubling chain reaches
        assert ref.g1_mul(ref.G1_GEN, d[3 * n + 1]) == ref.g1_mul(pts[1], 1 << (3 * c))


def test_walker_classifies_operand_pairs():
    wk = M.Walk()
    assert wk.add("s", 5, 5) == 10 and wk.add("s", 5, M.R - 5) == 0 and wk.add("s", 0, 7) == 7 and wk.add("s", 7, 0) == 7 and wk.add("s", 0, 0) == 0
    assert wk.add("s", 3, 4) == 7
    assert dict(wk.n["s"]) == dict(equal=1, opposite=1, inf_a=1, inf_b=1, inf_ab=1, generic=1)


def test_tail_inspection_arguments_and_export():
    a, pts = P.digit_vector(11, 20, 1), np.zeros((20, 8), np.uint64)
    assert "zk_bn254_msm_tail_inspect" in _lib.SYMBOLS and hasattr(_lib.lib(), "zk_bn254_msm_tail_inspect")
    for bad in (dict(table_c=11, skip_below=3), dict(window_bits=11, l1_m=16), dict(window_bits=11, keep_final=True), dict(table_c=11, is_g2=True, quad_tail=True),
                dict(table_c=11, is_g2=True, keep_final=True, rows=1)):
        with pytest.raises(_lib.ZkmiError):
            bn254.msm_tail_inspect(np.zeros((20, 16), np.uint64) if bad.get("is_g2") else pts, a, plan_only=True, **bad)
    p = bn254.msm_tail_inspect(pts, a, table_c=16, row_first=16)   # a shard that owns no window: the empty plan runs without a device
    assert p["total"] == 0 and p["levels"] == [] and p["n_final"] == 0
    p = bn254.msm_tail_inspect(pts, a, table_c=13, row_first=1, row_step=2, stride=23, plan_only=True)
    assert p["table_entries"] == 10 * 23 and p["level_entries"] == sum(d["n_out"] for d in p["levels"])
