"""The host model of the MSM's scalar preparation (tests/msm_prep_ref.py) and its case table, pinned without a GPU: the model's recoding against its
definition and against the oracle's Pippenger recoding, its pairs against a direct enumeration, and every case's geometry -- the production planner run
through zk_bn254_msm_prep_inspect's plan-only form, the launch geometry by the host formulas -- against what the case is named for."""
import ctypes as C

import numpy as np
import pytest

from noir_backend_using_gnark_amd import _lib, bn254
from oracle import bn254_ref as ref
from tests import msm_prep_ref as M

ALL_C = range(2, 25)


def inspect_case(case, vectors, **kw):
    arg = vectors[0] if (len(vectors) == 1 or case.req.get("rows")) else vectors
    return bn254.msm_prep_inspect(arg, **dict(case.req, **kw))


@pytest.mark.parametrize("c", ALL_C)
def test_recoding_sums_to_the_scalar_and_stays_in_range(c):
    edge = M.edge_scalars(c)
    assert all(0 <= s < M.R for s in edge) and len(edge) <= 300
    assert M.repeated_digit(1 << (c - 1), c) > 0
    d = M.recode(M.limbs(edge), c)
    B = 1 << (c - 1)
    assert d.shape == (len(edge), M.windows(c)) and d.min() >= -B and d.max() <= B
    for s, row in zip(edge, d):
        assert sum(int(x) << (c * w) for w, x in enumerate(row)) == s, (c, hex(s))
        want = ref.pippenger_digits(s, c)
        assert want[-1] == 0 and list(row) == want[:-1], (c, hex(s))   # (the oracle recodes one window more: always zero below r)
    # the named edges do what they are named for
    rows = {s: list(r) for s, r in zip(edge, d)}
    allB = rows[M.repeated_digit(B, c)]
    assert allB[0] == B and all(x in (0, B) for x in allB) and allB.count(B) >= M.windows(c) - 1
    if c > 2:
        neg = rows[M.repeated_digit(B + 1, c)]
        assert neg[0] == -(B - 1) and neg[1] == -(B - 2)             # B + 1 - 2^c, then the carry on top of it
    ones = rows[M.repeated_digit((1 << c) - 1, c)]
    assert ones[0] == -1 and all(x == 0 for x in ones[1:M.windows(c) - 2])   # the carry runs through every full window
    assert rows[(B + 1) | ((B - 1) << c)][:2] == [-(B - 1), B]
    assert rows[((B + 1) | (B << c)) % M.R][1] == -(B - 1)


def test_random_scalars_agree_with_the_oracle_recoding():
    rng = np.random.default_rng(7)
    xs = [int.from_bytes(rng.bytes(32), "little") % M.R for _ in range(64)]
    for c in ALL_C:
        d = M.recode(M.limbs(xs), c)
        for s, row in zip(xs, d):
            assert list(row) == ref.pippenger_digits(s, c)[:-1]


def test_montgomery_images_round_trip():
    xs = M.edge_scalars(13)[:40]
    assert M.ints(M.to_mont(M.limbs(xs))) == [ref.to_mont(x, M.R) for x in xs]


@pytest.mark.parametrize("table,kw", [(False, {}), (True, dict(stride=11)), (True, dict(stride=9, row_first=1, row_step=3)), (True, dict(stride=9, row_first=40, row_step=2))])
def test_pairs_against_a_direct_enumeration(table, kw):
    c, n = 9, 7
    vecs = [M.digit_vector(c, 12, 1)[3:], M.digit_vector(c, 12, 2)[2:]][:2 if table else 1]
    keys, vals, nb = M.pairs(vecs, n, c, table=table, **kw)
    B, Wd = 1 << (c - 1), M.windows(c)
    want = []
    for v, vec in enumerate(vecs):
        digs = [ref.pippenger_digits(s, c) for s in M.ints(vec[:n])]
        rows = list(range(kw.get("row_first", 0), Wd, kw.get("row_step", 1))) if table else list(range(Wd))
        for k, w in enumerate(rows):
            for i in range(n):
                d = digs[i][w]
                key = nb if d == 0 else (v if table else w) * B + abs(d) - 1
                want.append((key, (((k * kw["stride"] + i) if table else i) << 1) | (d < 0)))
    assert nb == (len(vecs) if table else Wd) * B
    assert list(zip(keys.tolist(), vals.tolist())) == want
    if kw.get("row_first", 0) >= Wd:
        assert keys.size == 0
    sk, sv = M.sort_pairs(keys, vals)
    assert list(zip(sk.tolist(), sv.tolist())) == sorted(want, key=lambda p: p[0])   # (sorted() is stable)
    st = M.bounds(sk, nb)
    assert st[0] == 0 and all(st[b] == sum(1 for k, _ in want if k < b) for b in range(0, nb + 1, 37)) and st[nb] == sum(1 for k, _ in want if k != nb)
    dk, dv, _ = M.pairs(vecs, n, c, table=table, drop=True, **kw)
    assert sorted(zip(dk.tolist(), dv.tolist())) == sorted(p for p in want if p[0] != nb)


def test_a_zero_digit_has_no_sign():
    """all ones plus a carry: digit 0, carry out -- the model gives such a pair sign 0, and the comparison clears whatever the device left there"""
    c = 6
    s = 0b111111_111111_100001   # window 0 negative with a carry, windows 1 and 2 all ones: zeros that pass the carry on
    assert list(M.recode(M.limbs([s]), c)[0][:4]) == [-31, 0, 0, 1]
    keys, vals, nb = M.pairs([M.limbs([s])], 1, c)
    assert (vals[keys == nb] == 0).all() and (keys == nb).sum() == M.windows(c) - 2
    dirty = np.where(keys == nb, vals | 1, vals).astype(np.uint32)
    assert np.array_equal(M.unsigned_sentinels(keys, dirty, nb), vals) and np.array_equal(M.unsigned_sentinels(keys, vals, nb), vals)


def test_sort_plan_formula():
    assert M.rs_plan(1, 19) == dict(npass=3, bits=[7, 6, 6], ntiles=1)
    assert M.rs_plan(8192, 8)["ntiles"] == 1 and M.rs_plan(8193, 8)["ntiles"] == 2
    assert [M.rs_plan(1, b)["npass"] for b in (1, 8, 9, 16, 17, 24, 25, 30)] == [1, 1, 2, 2, 3, 3, 4, 4]


@pytest.mark.parametrize("case", M.CASES, ids=lambda c: c.name)
def test_every_case_plans_to_the_geometry_it_is_named_for(case):
    """the production planner (plan-only inspection: host work) + the host launch formulas, for every shape of the device test"""
    vectors = case.build()
    plan = inspect_case(case, vectors, plan_only=True)
    geo = M.geometry(plan, case.req.get("drop_zero_digits", False))
    for k, want in case.expect.items():
        assert geo[k] == want, (case.name, k, geo[k], want)
    assert plan["total"] == plan["Wrows"] * (case.req.get("n") or vectors[0].shape[0]) * (plan["W"] if case.req.get("table_c") else 1)
    assert plan["max_tasks"] == plan["nb"] + plan["total"] // plan["Lmin"] + 1 and 32 <= plan["Lmin"] <= plan["L"]
    assert (1 << plan["key_bits"]) > plan["nb"] >= (1 << (plan["key_bits"] - 1))   # the sentinel key nb fits the sorted bits, with none to spare
    if "bucket" in case.reach or "giants" in case.reach:   # the GIANT_T boundary cases rest on tasks of exactly 32 points
        assert plan["L"] == plan["Lmin"] == 32 and M.GIANT_POINTS == M.GIANT_T * 32


def test_the_table_covers_what_the_issue_lists():
    geo = {}
    for case in M.CASES:
        geo[case.name] = M.geometry(inspect_case(case, case.build(), plan_only=True), case.req.get("drop_zero_digits", False))
    assert {g["npass"] for g in geo.values()} == {1, 2, 3, 4}
    assert {1, 2, 257} <= {g["scan_tiles"] for g in geo.values()} and 257 in {g["sort_tiles"] for g in geo.values()}
    assert {0, 1} == {g["bshift"] for g in geo.values()} and {True, False} == {g["stats_pick"] for g in geo.values()}
    assert len({c.name for c in M.CASES}) == len(M.CASES)


def test_plan_only_inspection_needs_no_device_and_rejects_bad_requests():
    a = M.digit_vector(16, 300, 3)
    p = bn254.msm_prep_inspect(a, table_c=16, row_first=16, plan_only=True)      # a shard that owns no window: the empty plan
    assert p["total"] == 0 and p["nb"] == 0
    p = bn254.msm_prep_inspect(a, table_c=16, row_first=16)                       # ... which also RUNS without a device: nothing to do
    assert p["total"] == 0 and p["keys"].size == 0
    p = bn254.msm_prep_inspect(a, plan_only=True)                                 # the planner's own window
    wb, dg = np.zeros(1, np.uint32), np.zeros(1, np.uint32)
    _lib.check(_lib.lib().zk_bn254_msm_plan_info(C.c_size_t(300), C.c_int(0), _lib.vp(wb), _lib.vp(dg)))
    assert (p["c"], p["Wd"]) == (int(wb[0]), int(dg[0]))
    for bad in (dict(window_bits=23), dict(table_c=25), dict(table_c=16, stride=299), dict(rows=2, row_stride=150, n=150),
                dict(table_c=16, rows=2, n=200, row_stride=100)):
        with pytest.raises((_lib.ZkmiError, ValueError)):
            bn254.msm_prep_inspect(a, plan_only=True, **bad)
    with pytest.raises(_lib.ZkmiError):
        bn254.msm_prep_inspect([a, a, a, a], table_c=16, plan_only=True)


def test_entry_is_exported():
    assert "zk_bn254_msm_prep_inspect" in _lib.SYMBOLS and hasattr(_lib.lib(), "zk_bn254_msm_prep_inspect")


def test_every_compaction_case_holds_zero_digits():
    """the device test reads `dropped` from the run AND wants device_total < total: the inputs must make the difference visible"""
    for case in M.CASES:
        if case.req.get("drop_zero_digits"):
            v = case.build()
            c = case.req["table_c"]
            keys, _, nb = M.pairs(v, v[0].shape[0], c, table=True, stride=v[0].shape[0])
            assert (keys == nb).any(), case.name
