"""Discrete-log model of the MSM's base-side half (csrc/msm.hip: k_build_table, k_accumulate, k_fold_giant, k_fold_multi, k_reduce_l1, k_reduce_l2,
k_reduce_wave in both lane layouts, msm_finish, k_msm_sets_affine) and the table of inputs its tests share.

Every base is a known multiple of the generator, P_i = [k_i] G, so every table entry, task sum, bucket sum, level entry and window value is an INTEGER mod r
and the point the device must hold there is one oracle call ([x] G).  Equal, opposite and infinite operands (x == y, x == -y, x == 0) can then be placed at
any level on purpose.  The scalar side (limbs, recoding, pairs, the case builders) is tests/msm_prep_ref.py.

Two things live here:
  the model    closed formulas per stage (table_logs, task_sums, bucket_sums, level1, level_next, set_value) and `levels`, which restates the level
               sequence msm_accumulate_batch runs for a plan
  the walker   a replay, in integers, of the operand pairs of every addition the kernels make, in the kernels' own order (the run / acc loops, the suffix
               scan `if (lane + d < FAN)`, the xor butterfly, the fold butterflies with their `first` rule).  It is used for REACH COUNTS only: how many
               additions of a stage had equal, opposite or infinite operands.  Its values are compared with the closed formulas on the CPU
               (tests/test_msm_tail_ref_cpu.py), so the two halves of this file check each other.
A preparation (`prep`) is what either the device returned (prep_from_run) or the model planned itself at a given task length (own_prep)."""
from collections import Counter, namedtuple

import numpy as np

from tests import msm_prep_ref as P

R = P.R
GIANT_T, GIANT_MAX = P.GIANT_T, P.GIANT_MAX
KERNEL = dict(table="k_build_table", accumulate="k_accumulate / acc_task", fold="k_fold_giant / k_fold_multi", l1="k_reduce_l1", l2="k_reduce_l2",
              wave="k_reduce_wave", wave_quad="k_reduce_wave<TailPtQ>", finish="msm_finish", sets_affine="k_msm_sets_affine")


def log2(m: int) -> int:
    assert m > 0 and m & (m - 1) == 0
    return m.bit_length() - 1


# ------------------------------------------------------------------------------------------------------------ geometry
def levels(plan: dict, W: int, l2_m: int = 0, quad: bool = False):
    """(descriptors, n_final, sh_final): the level sequence of msm_accumulate_batch for a plan (B, m1, N1), W bucket sets, a second serial level over l2_m
    entries and the lane layout of the wave levels"""
    N, sh = plan["N1"], log2(plan["m1"])
    assert N * plan["m1"] == plan["B"]
    out = [dict(kind="l1", n_in=plan["B"], n_out=N, sh_in=0, sh_out=sh, m=plan["m1"])]
    if l2_m > 1 and N > 64 * l2_m:
        Nout = (N + l2_m - 1) // l2_m
        out.append(dict(kind="l2", n_in=N, n_out=Nout, sh_in=sh, sh_out=sh + log2(l2_m), m=l2_m))
        N, sh = Nout, sh + log2(l2_m)
    fan = 16 if quad else 64
    host_n = 64 if W == 1 else 1   # one bucket set: its last <= 64 entries are the finisher's
    while N > host_n:
        Nout = (N + fan - 1) // fan
        out.append(dict(kind="wave_quad" if quad else "wave", n_in=N, n_out=Nout, sh_in=sh, sh_out=sh + log2(fan), m=fan))
        N, sh = Nout, sh + log2(fan)
    return out, N, sh


def path(lv) -> list:
    return [(d["kind"], d["n_out"]) for d in lv]


# ------------------------------------------------------------------------------------------------------------ preparations
def giant_seg(cnt: int) -> int:
    return max(64, ((cnt + 63) // 64 + 63) // 64 * 64)


def prep_from_run(out: dict) -> dict:
    """the task records of an inspected run, per task id"""
    nb, task_off = out["nb"], out["task_off"].astype(np.int64)
    T = int(task_off[nb])
    length = np.zeros(T, np.int64)
    length[out["task_ids"][:T]] = out["L"] - out["len_keys"][:T].astype(np.int64)
    ctl = out["ctl"].astype(np.int64)
    return dict(nb=nb, T=T, vals=out["vals"], task_off=task_off, begin=out["task_begin"][:T].astype(np.int64), length=length,
                listed=[int(b) for b in ctl[8:8 + min(int(ctl[4]), GIANT_MAX)]], Lt=int(ctl[2]))


def own_prep(vectors, n: int, c: int, Lt: int, table: bool = False, stride: int = 0, row_first: int = 0, row_step: int = 1) -> dict:
    """the model's own preparation at task length Lt: pairs, stable sort, bounds, tasks of at most Lt points bucket by bucket, the first GIANT_MAX giants listed"""
    keys, vals, nb = P.pairs(vectors, n, c, table=table, stride=stride, row_first=row_first, row_step=row_step)
    sk, sv = P.sort_pairs(keys, vals)
    start = P.bounds(sk, nb).astype(np.int64)
    nt = (np.diff(start) + Lt - 1) // Lt
    task_off = np.zeros(nb + 1, np.int64)
    np.cumsum(nt, out=task_off[1:])
    T = int(task_off[nb])
    bucket = np.repeat(np.arange(nb), nt)
    j = np.arange(T) - task_off[bucket]
    begin = start[bucket] + j * Lt
    length = np.minimum(Lt, start[bucket + 1] - begin)
    return dict(nb=nb, T=T, vals=sv, task_off=task_off, begin=begin, length=length, listed=[int(b) for b in np.flatnonzero(nt > GIANT_T)[:GIANT_MAX]], Lt=Lt)


# ------------------------------------------------------------------------------------------------------------ the model
def table_logs(k, n: int, c: int, stride: int, row_first: int = 0, row_step: int = 1) -> list:
    """d[j * stride + i] = 2^(c * (row_first + j * row_step)) * k_i; entries [n, stride) of a row and the rows of an infinity base (k_i == 0) are infinity (0)"""
    rows = P.table_rows(c, row_first, row_step)
    d = [0] * (len(rows) * stride)
    for j, w in enumerate(rows):
        f = pow(2, c * w, R)
        d[j * stride:j * stride + n] = [f * x % R for x in k[:n]]
    return d


def task_sums(d, prep: dict, skip_below: int = 0) -> list:
    """e_t = sum of +-d[v >> 1] over the task's values; entries below skip_below contribute nothing"""
    vals, e = prep["vals"], []
    for b, ln in zip(prep["begin"].tolist(), prep["length"].tolist()):
        s = 0
        for v in vals[b:b + ln].tolist():
            if (v >> 1) >= skip_below:
                s += -d[v >> 1] if v & 1 else d[v >> 1]
        e.append(s % R)
    return e


def bucket_sums(e, prep: dict) -> dict:
    """bucket -> x_b for the buckets that have tasks (x_b sits at slot task_off[b] after the fold); every other bucket is infinity"""
    off = prep["task_off"]
    return {int(b): sum(e[off[b]:off[b + 1]]) % R for b in np.flatnonzero(np.diff(off) > 0)}


def level1(x: dict, W: int, B: int, m: int):
    """A[w][q] = sum_l (l + 1) x[w B + q m + l], S[w][q] = sum_l x[...]"""
    N = B // m
    A, S = [[0] * N for _ in range(W)], [[0] * N for _ in range(W)]
    for b, v in x.items():
        w, k = divmod(b, B)
        q, l = divmod(k, m)
        S[w][q] = (S[w][q] + v) % R
        A[w][q] = (A[w][q] + (l + 1) * v) % R
    return A, S


def level_next(A, S, m: int, sh: int):
    """S'[q] = sum_l S[q m + l]; A'[q] = sum_l A[q m + l] + 2^sh sum_l l S[q m + l]; entries at or past N are absent"""
    N = len(A[0])
    Nout = (N + m - 1) // m
    A2, S2 = [[0] * Nout for _ in A], [[0] * Nout for _ in A]
    for w in range(len(A)):
        for q in range(Nout):
            js = range(q * m, min(q * m + m, N))
            S2[w][q] = sum(S[w][j] for j in js) % R
            A2[w][q] = (sum(A[w][j] for j in js) + (1 << sh) * sum((j - q * m) * S[w][j] for j in js)) % R
    return A2, S2


def run_levels(x: dict, W: int, B: int, lv: list) -> list:
    """[(A, S)] per level descriptor"""
    out = []
    for d in lv:
        if d["kind"] == "l1":
            out.append(level1(x, W, B, d["m"]))
        else:
            assert d["n_in"] == len(out[-1][0][0])
            out.append(level_next(out[-1][0], out[-1][1], d["m"], d["sh_in"]))
    return out


def set_value(A_w, S_w, sh: int) -> int:
    return (sum(A_w) + (1 << sh) * sum(j * s for j, s in enumerate(S_w))) % R


def bucket_value(x: dict, w: int, B: int) -> int:
    return sum((b - w * B + 1) * v for b, v in x.items() if w * B <= b < (w + 1) * B) % R


def total_plain(V, c: int) -> int:
    return sum(pow(2, c * w, R) * v for w, v in enumerate(V)) % R


def expected_values(k, vectors, n: int, c: int, table: bool, row_first: int = 0, row_step: int = 1, skip_below: int = 0) -> list:
    """what the MSM is FOR, without buckets: table mode: per vector sum_i k_i sum_(owned w) digit_(i, w) 2^(c w); plain: [sum_i s_i k_i] over i >= skip_below"""
    if not table:
        return [sum(s * x for s, x in zip(P.ints(vectors[0][:n])[skip_below:], k[skip_below:n])) % R]
    out = []
    for vec in vectors:
        d = P.recode(np.ascontiguousarray(vec)[:n], c)
        tot = 0
        for w in P.table_rows(c, row_first, row_step):
            tot += pow(2, c * w, R) * sum(int(dg) * x for dg, x in zip(d[:, w].tolist(), k))
        out.append(tot % R)
    return out


# ------------------------------------------------------------------------------------------------------------ the walker
class Walk:
    """counts, per stage, the additions whose operands are equal, opposite, infinite on the left (the accumulator), on the right (the addend) or on both sides"""

    def __init__(self):
        self.n = {}

    def add(self, stage: str, a: int, b: int) -> int:
        c = self.n.setdefault(stage, Counter())
        if a == 0 or b == 0:
            c["inf_ab" if a == b else ("inf_a" if a == 0 else "inf_b")] += 1
        elif a == b:
            c["equal"] += 1
        elif a + b == R:
            c["opposite"] += 1
        else:
            c["generic"] += 1
        return (a + b) % R

    def count(self, stage: str, kind: str) -> int:
        return self.n.get(stage, Counter())[kind]


def walk_accumulate(wk: Walk, d, prep: dict, skip_below: int = 0) -> list:
    vals, e = prep["vals"], []
    for b, ln in zip(prep["begin"].tolist(), prep["length"].tolist()):
        acc = 0
        for v in vals[b:b + ln].tolist():
            if (v >> 1) < skip_below:
                continue
            acc = wk.add("accumulate", acc, (R - d[v >> 1]) % R if v & 1 else d[v >> 1])
        e.append(acc)
    return e


def _butterfly(wk: Walk, stage: str, acc: list, cnt: int) -> int:
    first = 32
    while first >= cnt and first > 0:
        first >>= 1   # the largest power of two below cnt
    d = first
    while d > 0:
        o = [acc[l + d] if l + d < 64 else acc[l] for l in range(64)]   # shfl_down
        for l in range(d):
            acc[l] = wk.add(stage, acc[l], o[l])
        d >>= 1
    return acc[0]


def walk_fold(wk: Walk, e, prep: dict) -> list:
    """the task array after k_fold_giant and k_fold_multi"""
    part, off = list(e), prep["task_off"]
    for b in prep["listed"]:
        t0, t1 = int(off[b]), int(off[b + 1])
        S = giant_seg(t1 - t0)
        for seg in range(64):
            lo = t0 + seg * S
            hi = min(lo + S, t1)
            if lo >= t1 or hi - lo < 2:
                continue
            acc = [0] * 64
            for lane in range(64):
                for t in range(lo + lane, hi, 64):
                    acc[lane] = wk.add("fold_giant", acc[lane], part[t])
            part[lo] = _butterfly(wk, "fold_giant", acc, min(hi - lo, 64))
    for b in np.flatnonzero(np.diff(off) > 1).tolist():
        t0, t1 = int(off[b]), int(off[b + 1])
        nheld, acc = t1 - t0, [0] * 64
        if nheld > GIANT_T and b in prep["listed"]:
            S = giant_seg(nheld)
            nheld = (nheld + S - 1) // S
            for lane in range(nheld):
                acc[lane] = part[t0 + lane * S]
        else:
            for lane in range(64):
                for t in range(t0 + lane, t1, 64):
                    acc[lane] = wk.add("fold_multi", acc[lane], part[t])
        part[t0] = _butterfly(wk, "fold_multi", acc, min(nheld, 64))
    return part


def walk_l1(wk: Walk, heads: dict, W: int, B: int, m: int):
    """heads: bucket -> the point at its first task's slot.  Chunks without a task are skipped (every addition there has two infinite sides)"""
    N = B // m
    A, S = [[0] * N for _ in range(W)], [[0] * N for _ in range(W)]
    for g in sorted({b // m for b in heads}):
        run = acc = 0
        for l in range(m - 1, -1, -1):
            if g * m + l in heads:
                run = wk.add("l1", run, heads[g * m + l])
            acc = wk.add("l1", acc, run)
        A[g // N][g % N], S[g // N][g % N] = acc, run
    return A, S


def walk_l2(wk: Walk, A, S, m: int, sh: int):
    N = len(A[0])
    Nout = (N + m - 1) // m
    A2, S2 = [[0] * Nout for _ in A], [[0] * Nout for _ in A]
    for w in range(len(A)):
        for q in range(Nout):
            if not any(A[w][q * m:q * m + m]) and not any(S[w][q * m:q * m + m]):
                continue
            run = t = asum = 0
            for l in range(m - 1, -1, -1):
                j = q * m + l
                if j >= N:
                    continue
                asum = wk.add("l2", asum, A[w][j])
                run = wk.add("l2", run, S[w][j])
                if l >= 1:
                    t = wk.add("l2", t, run)
            A2[w][q], S2[w][q] = wk.add("l2", asum, (t << sh) % R), run
    return A2, S2


def walk_wave(wk: Walk, A, S, fan: int, sh: int, stage: str = "wave"):
    """lane = entry of the chunk (a quad's four lanes carry one point: fan = 16); all-infinity chunks are skipped"""
    N = len(A[0])
    Nout = (N + fan - 1) // fan
    A2, S2 = [[0] * Nout for _ in A], [[0] * Nout for _ in A]
    for w in range(len(A)):
        for q in range(Nout):
            s = [S[w][q * fan + l] if q * fan + l < N else 0 for l in range(fan)]
            a = [A[w][q * fan + l] if q * fan + l < N else 0 for l in range(fan)]
            if not any(s) and not any(a):
                continue
            d = 1
            while d < fan:   # inclusive suffix sums
                t = [s[l + d] if l + d < fan else s[l] for l in range(fan)]
                for l in range(fan - d):
                    s[l] = wk.add(stage + "_scan", s[l], t[l])
                d <<= 1
            y = [0] + [(v << sh) % R for v in s[1:]]
            y = [wk.add(stage + "_sum", y[l], a[l]) for l in range(fan)]
            d = fan // 2
            while d > 0:
                y = [wk.add(stage + "_butterfly", y[l], y[l ^ d]) for l in range(fan)]
                d >>= 1
            A2[w][q], S2[w][q] = y[0], s[0]
    return A2, S2


def walk_finish(wk: Walk, A_w, S_w, sh: int, stage: str = "finish") -> int:
    """msm_finish's and k_msm_sets_affine's loop over one set's last-level entries"""
    N, val = len(A_w), A_w[0]
    if N > 1:
        run = acc = 0
        for j in range(N - 1, 0, -1):
            run = wk.add(stage, run, S_w[j])
            acc = wk.add(stage, acc, run)
            val = wk.add(stage, val, A_w[j])
        val = wk.add(stage, val, (acc << sh) % R)
    return val


def walk_all(d, prep: dict, W: int, B: int, lv: list, sh_final: int, skip_below: int = 0):
    """the whole replay: (walk, values per stage as the model's functions return them)"""
    wk = Walk()
    e = walk_accumulate(wk, d, prep, skip_below)
    part = walk_fold(wk, e, prep)
    off = prep["task_off"]
    heads = {int(b): part[off[b]] for b in np.flatnonzero(np.diff(off) > 0)}
    out = []
    for dsc in lv:
        if dsc["kind"] == "l1":
            out.append(walk_l1(wk, heads, W, B, dsc["m"]))
        elif dsc["kind"] == "l2":
            out.append(walk_l2(wk, out[-1][0], out[-1][1], dsc["m"], dsc["sh_in"]))
        else:
            out.append(walk_wave(wk, out[-1][0], out[-1][1], dsc["m"], dsc["sh_in"], dsc["kind"]))
    V = [walk_finish(wk, out[-1][0][w], out[-1][1][w], sh_final) for w in range(W)]
    return wk, dict(tasks=e, heads=heads, levels=out, values=V)


# ------------------------------------------------------------------------------------------------------------ the case table
# A case: `req` = keyword arguments of bn254.msm_tail_inspect (without points and vectors), `build()` -> (k, vectors): the bases' discrete logs (python ints mod r,
# 0 = the point at infinity) and the canonical scalar vectors (one matrix for rows=...), `expect` = the geometry it is named for (path: [(kind, n_out)],
# n_final, sh_final, W), `reach` = [(stage, kind)] walker counts that must be non-zero, `flags` = what else its tests look at
Case = namedtuple("Case", "name req build expect reach flags")


def rand_k(n: int, seed: int) -> list:
    rng = np.random.default_rng(seed)
    return [int.from_bytes(rng.bytes(32), "little") % (R - 1) + 1 for _ in range(n)]


def _geo(seed, n=300, sets=1, same=()):
    """random logs, random scalars; `same`: pairs (v, u) of vectors that are the same array object"""
    def build():
        vecs = [P._rand(n, seed + 1 + v) for v in range(sets)]
        for v, u in same:
            vecs[v] = vecs[u]
        return rand_k(n, seed), vecs
    return build


def _rows_matrix(seed, n, rows, row_stride, zero_rows=(), all_zero=False):
    def build():
        mat = P._zeros(rows * row_stride) if all_zero else P._rand(rows * row_stride, seed + 1)
        for v in zero_rows:
            mat[v * row_stride:v * row_stride + n] = 0
        return rand_k(n, seed), [mat]
    return build


def request(case, vectors) -> dict:
    """the keyword arguments of bn254.msm_tail_inspect for a case (a one-row matrix is as long as its vector)"""
    req = dict(case.req)
    if req.get("rows") and "n" not in req:
        req.update(n=vectors[0].shape[0], row_stride=vectors[0].shape[0])
    return req


def case_vectors(case, vectors):
    """the scalar vectors of a case as the model sees them (the rows of a matrix taken apart)"""
    req = request(case, vectors)
    if req.get("rows"):
        n, rs = req["n"], req["row_stride"]
        return [vectors[0][v * rs:v * rs + n] for v in range(req["rows"])]
    return vectors


def _with_logs(prep_case_name, k_of_n):
    """a builder of tests/msm_prep_ref.CASES with bases k_of_n(n)"""
    def build():
        vecs = P.CASE[prep_case_name].build()
        return k_of_n(vecs[0].shape[0]), vecs
    return build


def _fold_counts(k_of_n):
    """table c = 16, task length 32: buckets of 2, 3, 4, 5, 64 and 65 tasks (the last task of the odd ones short): the `first` rule and the strided load"""
    def build():
        vec = P._bucket_fill(16, [(3, 4), (5, 5), (7, 8), (9, 9), (11, 128), (13, 129)], singles=[5, 9, 13])
        return k_of_n(vec.shape[0]), [vec]
    return build


FOLD_TASKS = {2: 2, 4: 3, 6: 4, 8: 5, 10: 64, 12: 65}   # bucket -> tasks of _fold_counts at task length 32


def _units(c, table, l1_m=8, l2_m=0, quad=False, keep_final=False):
    """buckets per entry of the first level that folds across lanes (a wave level, or the finisher where there is none) and that level's fan-in"""
    B = 1 << (c - 1)
    plan = dict(B=B, m1=min(l1_m, B), N1=B // min(l1_m, B))
    lv, n_final, _ = levels(plan, 1 if table else P.windows(c), l2_m, quad)
    unit = plan["m1"] * (l2_m if len(lv) > 1 and lv[1]["kind"] == "l2" else 1)
    waves = [d for d in lv if d["kind"].startswith("wave")]
    return B, unit, (waves[0]["m"] if waves else n_final)


def _one_per_bucket(c, table):
    B = 1 << (c - 1)
    return P.limbs([d if table else P.repeated_digit(d, c) for d in range(1, B + 1)])


def _family(family, c, table, seed, **shape):
    """the degenerate inputs: one point in every bucket of every set (scalar d -> bucket d - 1), the logs chosen per family"""
    def build():
        B, unit, fan = _units(c, table, shape.get("l1_m", 0) or 8, shape.get("l2_m", 0), shape.get("quad_tail", False))
        if family == "same_point":
            return [1] * B, [_one_per_bucket(c, table)]
        if family == "alternating_sign":
            return [1 if i % 2 == 0 else R - 1 for i in range(B)], [_one_per_bucket(c, table)]
        if family == "cancelling_halves":   # bucket b -> entry b // unit -> lane (entry % fan): the upper half of the lanes holds the negatives of the lower
            rho, k, h = rand_k(B, seed), [], max(fan // 2, 1)
            for b in range(B):
                entry = b // unit
                lane, chunk = entry % fan, entry // fan
                x = rho[chunk * fan + lane % h]
                k.append(x if lane < h or fan == 1 else R - x)
            # the scan now meets opposite suffix sums.  For the butterfly, lane 5 + h of every chunk gets the A that makes its y the negative of lane 5's
            # (y_l = 2^sh * suffix_l + A_l): delta moved from the entry's first bucket (weight 1) to its second (weight 2) changes A by delta and leaves S alone
            if shape.get("wave_level", c >= 11) and fan >= 16:
                sh, l0 = log2(unit), 5
                for chunk in range(B // (unit * fan)):
                    ent = [k[(chunk * fan + l) * unit:(chunk * fan + l + 1) * unit] for l in range(fan)]
                    S = [sum(e) % R for e in ent]
                    A = [sum((p + 1) * x for p, x in enumerate(e)) % R for e in ent]
                    suf = [sum(S[l:]) % R for l in range(fan)]
                    y0 = ((suf[l0] << sh) + A[l0]) % R
                    delta = (-y0 - (suf[l0 + h] << sh) - A[l0 + h]) % R
                    b0 = (chunk * fan + l0 + h) * unit
                    k[b0], k[b0 + 1] = (k[b0] - delta) % R, (k[b0 + 1] + delta) % R
            return k, [_one_per_bucket(c, table)]
        assert family == "sparse"
        n, beta = 300, 6
        vec = P._rand(n, seed + 1)
        vec[100:103] = P.limbs([beta + 1] * 3)            # three points whose only non-zero digit puts them into bucket beta of the first set
        dg = np.abs(P.recode(vec, c))
        hits = (dg == beta + 1).any(axis=1) if table else dg[:, 0] == beta + 1
        k = [0 if (i % 3 == 0 or hits[i]) else x for i, x in enumerate(rand_k(n, seed))]
        return k, [vec]
    return build


FAMILIES = ("same_point", "alternating_sign", "cancelling_halves", "sparse")
SPARSE_BUCKET = 6


def _cases():
    out = []
    add = lambda name, req, build, expect=None, reach=(), flags=(): out.append(Case(name, req, build, expect or {}, list(reach), set(flags)))  # noqa: E731
    T = lambda c, **kw: dict(table_c=c, **kw)       # noqa: E731
    Pl = lambda c, **kw: dict(window_bits=c, **kw)  # noqa: E731
    E = lambda path, n_final, sh_final, W=1: dict(path=path, n_final=n_final, sh_final=sh_final, W=W)  # noqa: E731
    # ---- geometry: random logs, random scalars, n = 300: the smallest shapes that reach each branch of the level sequence
    add("plain_c2_no_wave", Pl(2), _geo(0x700), E([("l1", 1)], 1, 1, 128))
    add("plain_c5_wave_of_2_lanes", Pl(5), _geo(0x701), E([("l1", 2), ("wave", 1)], 1, 9, 51))
    add("plain_c10_one_full_wave", Pl(10), _geo(0x702), E([("l1", 64), ("wave", 1)], 1, 9, 26))
    add("plain_c11_two_waves", Pl(11), _geo(0x703), E([("l1", 128), ("wave", 2), ("wave", 1)], 1, 15, 24))
    add("plain_c13_wave_of_8_lanes", Pl(13), _geo(0x704), E([("l1", 512), ("wave", 8), ("wave", 1)], 1, 15, 20))
    add("table_c8_host_finish_at_16", T(8), _geo(0x705), E([("l1", 16)], 16, 3))
    add("table_c10_host_finish_at_64", T(10), _geo(0x706), E([("l1", 64)], 64, 3))
    add("table_c11_host_finish_at_2", T(11), _geo(0x707), E([("l1", 128), ("wave", 2)], 2, 9))
    add("table_c14_l16_l2_not_run", T(14, l1_m=16, l2_m=8), _geo(0x708), E([("l1", 512), ("wave", 8)], 8, 10))
    add("table_c15_l16_l2_runs", T(15, l1_m=16, l2_m=8), _geo(0x709), E([("l1", 1024), ("l2", 128), ("wave", 2)], 2, 13))
    add("table_c17_2_sets_three_waves", T(17), _geo(0x70A, sets=2), E([("l1", 8192), ("wave", 128), ("wave", 2), ("wave", 1)], 1, 21, 2))
    add("table_c12_3_sets_two_the_same", T(12), _geo(0x70B, sets=3, same=[(2, 0)]), E([("l1", 256), ("wave", 4), ("wave", 1)], 1, 15, 3))
    add("table_c13_sharded_rows_stride_above_n", T(13, row_first=1, row_step=2, stride=333), _geo(0x70C), E([("l1", 512), ("wave", 8)], 8, 9))
    add("quad_table_c11", T(11, quad_tail=True), _geo(0x70D), E([("l1", 128), ("wave_quad", 8)], 8, 7))
    add("quad_plain_c9", Pl(9, quad_tail=True), _geo(0x70E), E([("l1", 32), ("wave_quad", 2), ("wave_quad", 1)], 1, 11, 29))
    add("rows_keep_final_5_rows_c9_one_zero_row", T(9, rows=5, n=300, row_stride=307, keep_final=True), _rows_matrix(0x70F, 300, 5, 307, zero_rows=[3]),
        E([("l1", 32), ("wave", 1)], 1, 9, 5), flags=["zero_row_3"])
    for c, nf, pth, sh in ((8, 16, [("l1", 16)], 3), (10, 64, [("l1", 64)], 3), (11, 2, [("l1", 128), ("wave", 2)], 9)):
        add("rows_keep_final_1_row_c%d" % c, T(c, rows=1, n=300, row_stride=300, keep_final=True), _rows_matrix(0x710 + c, 300, 1, 300), E(pth, nf, sh))
    add("rows_keep_final_all_zero_dropped", T(9, rows=5, n=300, row_stride=300, keep_final=True, drop_zero_digits=True),
        _rows_matrix(0x720, 300, 5, 300, all_zero=True), E([("l1", 32), ("wave", 1)], 1, 9, 5), flags=["all_zero"])
    add("g2_plain_c5", Pl(5, is_g2=True), _geo(0x721), E([("l1", 2), ("wave", 1)], 1, 9, 51))
    add("g2_plain_c11", Pl(11, is_g2=True), _geo(0x722), E([("l1", 128), ("wave", 2), ("wave", 1)], 1, 15, 24))
    add("g2_table_c11", T(11, is_g2=True), _geo(0x723), E([("l1", 128), ("wave", 2)], 2, 9))
    add("g2_table_c15_l16_l2_runs", T(15, is_g2=True, l1_m=16, l2_m=8), _geo(0x724), E([("l1", 1024), ("l2", 128), ("wave", 2)], 2, 13))
    # ---- folds: the giant shapes of the preparation's case table and the small task counts, with random logs and with every base the generator
    folds = [("giant_t_exactly_256_tasks", 16, False), ("giant_t_257_tasks", 16, False), ("giant_more_than_64x64_tasks", 16, True), ("giant_more_than_listed", 22, True)]
    for name, c, g2 in folds:
        for grp in ("g1", "g2")[:2 if g2 else 1]:
            for kind, k_of_n in (("random", lambda n, name=name: rand_k(n, 0x730 + len(name))), ("all_one", lambda n: [1] * n)):
                hit = "generic" if kind == "random" else "equal"   # (all bases the generator: the full tasks of a table row are one point, a butterfly step doubles)
                want = [("fold_multi", hit)] if name == "giant_t_exactly_256_tasks" else [("fold_giant", hit if c == 16 else "generic"), ("fold_multi", "generic")]   # (a listed giant's heads differ; c = 22: 683 points per row, no two tasks alike)
                add("fold_%s_%s_%s" % (name, grp, kind), T(c, is_g2=grp == "g2"), _with_logs(name, k_of_n), reach=want, flags=["fold", "prep:" + name])
    for kind, k_of_n in (("random", lambda n: rand_k(n, 0x740)), ("all_one", lambda n: [1] * n)):
        add("fold_2_3_4_5_64_65_tasks_%s" % kind, T(16), _fold_counts(k_of_n),
            reach=[("fold_multi", "generic" if kind == "random" else "equal"), ("fold_multi", "inf_b")], flags=["fold", "fold_counts"])
    # ---- degenerate families: the group law's special cases above level 1
    shapes = [("table_c11", 11, True, {}), ("table_c15_l16_l2", 15, True, dict(l1_m=16, l2_m=8)), ("plain_c11", 11, False, {}),
              ("quad_table_c11", 11, True, dict(quad_tail=True)), ("keep_final_c8", 8, True, dict(keep_final=True)), ("keep_final_c10", 10, True, dict(keep_final=True)),
              ("keep_final_c11", 11, True, dict(keep_final=True)), ("g2_table_c11", 11, True, dict(is_g2=True))]
    for sname, c, table, kw in shapes:
        wave = "wave_quad" if kw.get("quad_tail") else "wave"
        fin = "sets_affine" if kw.get("keep_final") else "finish"
        has_wave, has_l2 = c >= 11, "l2_m" in kw
        for fam in FAMILIES:
            req = dict(T(c) if table else Pl(c), **kw)
            if fam == "sparse" and not table:
                req["skip_below"] = 100
            if kw.get("keep_final"):
                req.update(rows=1)   # (n and row_stride: the vector's length, filled in by the test)
            reach = []
            if fam == "same_point":
                reach = [("l1", "equal")] + ([("l2", "equal")] if has_l2 else []) + ([(wave + "_scan", "equal")] if has_wave else []) + ([(fin, "equal")] if table else [])
            elif fam == "alternating_sign":
                reach = [("l1", "opposite")] + ([("l2", "inf_ab")] if has_l2 else []) + ([(wave + "_scan", "inf_ab")] if has_wave else [])
            elif fam == "cancelling_halves":
                reach = [(wave + "_scan", "opposite"), (wave + "_butterfly", "opposite")] if has_wave else [(fin, "opposite")]
            else:
                reach = [("accumulate", "inf_b"), ("accumulate", "inf_ab")]
            add("%s_%s" % (fam, sname), req, _family(fam, c, table, 0x800 + 16 * len(out), **kw), reach=reach, flags=["family", fam])
    return out


CASES = _cases()
CASE = {c.name: c for c in CASES}
