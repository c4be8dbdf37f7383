"""Host model of the MSM's scalar preparation (csrc/msm.hip msm_prepare, csrc/radix.hpp) and the table of inputs its tests share.

The model is integers in numpy: gnark-crypto's partitionScalars recoding read off the BITS of a scalar (np.unpackbits: no limb arithmetic, so the
kernels' straddling loads are checked against something that has none), the (key, value) pair every digit becomes, numpy's stable argsort for the
sorted order and searchsorted for the bucket bounds.  What the device chooses freely (the task length inside [Lmin, L], the order of equal task-length
bins, where the workgroups of a compaction land) has no model: tests/test_gpu_msm_prep.py checks invariants there.

The plan itself comes from the library (bn254.msm_prep_inspect(plan_only=True): host work, no device); `geometry` adds the launch geometry that follows
from it by the formulas of radix.hpp / msm_prepare.  `CASES` names, for every input, the geometry it is there for: tests/test_msm_prep_ref_cpu.py
asserts it on the CPU and the device test asserts it again on the plan the run returns."""
from collections import namedtuple

import numpy as np

from oracle import bn254_ref as ref

R = ref.R
RS_TILE, RS_MAX_BITS, XS_TILE, TS_BINS = 8192, 8, 2048, 2048   # radix.hpp / msm.hip
GIANT_T, GIANT_MAX, GIANT_POINTS = 256, 48, 8192
PAD = 0xFFFFFFFF


# ------------------------------------------------------------------------------------------------------------ scalars
def limbs(xs) -> np.ndarray:
    """python ints (canonical, < 2^256) -> (n, 4) uint64 little-endian limbs"""
    if len(xs) == 0:
        return np.zeros((0, 4), np.uint64)
    return np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in xs), dtype="<u8").reshape(-1, 4).copy()


def ints(a) -> list:
    a = np.ascontiguousarray(a, dtype="<u8").reshape(-1, 4)
    raw = a.tobytes()
    return [int.from_bytes(raw[32 * i:32 * i + 32], "little") for i in range(a.shape[0])]


def to_mont(a) -> np.ndarray:
    return limbs([x * ref.MONT_R % R for x in ints(a)])


def windows(c: int) -> int:
    return (255 + c - 1) // c


def repeated_digit(d: int, c: int) -> int:
    """d in every c-bit window that keeps the value below r (d * sum_w 2^(c w), the top windows left out where they would overflow)"""
    s = 0
    for w in range(windows(c)):
        if s + (d << (c * w)) < R:
            s += d << (c * w)
    return s


def edge_scalars(c: int) -> list:
    """the scalars section 3a of the issue lists for window width c (python ints, all < r)"""
    B, Wd = 1 << (c - 1), windows(c)
    shift = c * (Wd - 1)
    top = (R - 1) >> shift
    out = [0, 1, R - 1, R - 2, (1 << 253) % R, ((1 << 254) - 1) % R,
           repeated_digit(B, c),                 # every window B: stays positive
           repeated_digit(B + 1, c),             # every window B + 1: negative, and a carry into the next
           repeated_digit((1 << c) - 1, c),      # every window all ones: a carry through every window
           (B + 1) | ((B - 1) << c),             # B - 1 with a carry into it: becomes B, stays positive
           ((B + 1) | (B << c)) % R]             # B with a carry into it: B + 1, negative
    # the largest scalar whose top-window digit takes a carry: r - 1 if the windows below its top one carry, else all ones below the next smaller top digit
    d = recode(limbs([R - 1]), c)[0]
    below = sum(int(d[w]) << (c * w) for w in range(Wd - 1))
    out.append(R - 1 if below < 0 else (top << shift) - 1)
    out += [1 << b for b in range(254) if (1 << b) < R]   # every limb straddle of off + c > 32 and the last limb's edge
    return out


def digit_vector(c: int, n: int, seed: int) -> np.ndarray:
    """(n, 4) canonical scalars: the edge scalars of width c, then random fill"""
    rng = np.random.default_rng(seed)
    e = edge_scalars(c)[:n]
    fill = [int.from_bytes(rng.bytes(32), "little") % R for _ in range(n - len(e))]
    return limbs(e + fill)


# ------------------------------------------------------------------------------------------------------------ recoding
def recode(scalars, c: int) -> np.ndarray:
    """(n, Wd) signed digits of gnark-crypto's partitionScalars: digit_w = bits [c w, c (w + 1)) + carry; above 2^(c-1) it becomes digit - 2^c and carries"""
    a = np.ascontiguousarray(scalars, dtype="<u8").reshape(-1, 4)
    n, Wd, B = a.shape[0], windows(c), 1 << (c - 1)
    out = np.zeros((n, Wd), np.int32)
    pow2 = (np.uint32(1) << np.arange(c, dtype=np.uint32)).astype(np.int64)
    for lo in range(0, n, 1 << 16):
        bits = np.unpackbits(a[lo:lo + (1 << 16)].view(np.uint8).reshape(-1, 32), axis=1, bitorder="little")
        carry = np.zeros(bits.shape[0], np.int64)
        for w in range(Wd):
            b0, b1 = c * w, min(c * (w + 1), 256)
            d = bits[:, b0:b1].astype(np.int64) @ pow2[:b1 - b0] + carry
            neg = d > B
            d = np.where(neg, d - (1 << c), d)
            carry = neg.astype(np.int64)
            out[lo:lo + bits.shape[0], w] = d
        assert not carry.any(), "a scalar at or above 2^(c Wd - 1): not canonical"
    return out


def table_rows(c: int, row_first: int, row_step: int) -> list:
    return list(range(row_first, windows(c), row_step))


def pairs(vectors, n: int, c: int, table: bool = False, stride: int = 0, row_first: int = 0, row_step: int = 1, drop: bool = False):
    """(keys, vals, nb) in the order k_msm_digits writes them: plain: window-major; table: (vector, owned row)-major.  drop: the zero digits are absent
    (their order on the device is the workgroups' arrival order: compare as multisets)."""
    B = 1 << (c - 1)
    sets = len(vectors)
    assert table or sets == 1
    nb = (sets if table else windows(c)) * B
    ks, vs = [], []
    i = np.arange(n, dtype=np.int64)
    for v, sc in enumerate(vectors):
        d = recode(np.ascontiguousarray(sc)[:n], c).astype(np.int64)   # every window is recoded: the carry runs through those a shard does not own
        rows = table_rows(c, row_first, row_step) if table else list(range(windows(c)))
        for k, w in enumerate(rows):
            mag, neg = np.abs(d[:, w]), (d[:, w] < 0).astype(np.int64)
            assert mag.max(initial=0) <= B
            key = np.where(mag > 0, (v if table else w) * B + mag - 1, nb)
            val = (((k * stride + i) if table else i) << 1) | neg
            ks.append(key)
            vs.append(val)
    keys = np.concatenate(ks).astype(np.uint32) if ks else np.zeros(0, np.uint32)
    vals = np.concatenate(vs).astype(np.uint32) if vs else np.zeros(0, np.uint32)
    if drop:
        live = keys != nb
        keys, vals = keys[live], vals[live]
    return keys, vals, nb


def unsigned_sentinels(keys, vals, nb: int):
    """the values with the sign bit of the zero digits' pairs cleared.  A zero digit has no sign: all ones plus a carry recodes to 0 with a carry OUT, and the
    device leaves that carry in the sign bit of a pair nothing reads (key nb lies behind start[nb]).  Index and order of those pairs are still compared."""
    return np.where(keys == nb, vals & np.uint32(0xFFFFFFFE), vals)


def sort_pairs(keys, vals):
    order = np.argsort(keys, kind="stable")
    return keys[order], vals[order]


def bounds(sorted_keys, nb: int) -> np.ndarray:
    return np.searchsorted(sorted_keys, np.arange(nb + 1, dtype=np.uint32), "left").astype(np.uint32)


def canonical_multiset(keys, vals):
    """pairs ordered by (key, value): equal for two arrays that hold the same pairs bucket by bucket"""
    order = np.lexsort((vals, keys))
    return keys[order], vals[order]


# ------------------------------------------------------------------------------------------------------------ launch geometry
def rs_plan(total: int, key_bits: int) -> dict:
    key_bits = max(key_bits, 1)
    npass = (key_bits + RS_MAX_BITS - 1) // RS_MAX_BITS
    bits, at = [], 0
    for p in range(npass):
        bits.append((key_bits - at + npass - p - 1) // (npass - p))
        at += bits[-1]
    return dict(npass=npass, bits=bits, ntiles=(total + RS_TILE - 1) // RS_TILE)


def geometry(plan: dict, drop: bool = False) -> dict:
    """what follows from a plan by the host-side formulas: sort passes and tiles, scan tiles, bin quantisation, which kernel picks the task length, whether
    the zero digits can be dropped (a workgroup's digits must fit its 64 KiB stage)"""
    rs = rs_plan(plan["total"], plan["key_bits"])
    bshift = 0
    while (plan["L"] >> bshift) >= TS_BINS:
        bshift += 1
    return dict(npass=rs["npass"], pass_bits=rs["bits"], sort_tiles=rs["ntiles"], scan_tiles=(plan["nb"] + 1 + XS_TILE - 1) // XS_TILE, bshift=bshift,
                stats_pick=plan["Lmin"] < plan["L"], compacts=bool(drop) and 256 * plan["Wd"] * 8 <= 65536, key_bits=plan["key_bits"], L=plan["L"],
                Lmin=plan["Lmin"])


# ------------------------------------------------------------------------------------------------------------ the case table
# A case: the request (keyword arguments of bn254.msm_prep_inspect without the vectors), a builder of its canonical scalar vectors, the geometry it is
# named for (`expect`: key -> value, compared with geometry(plan)), what the RUN must show (`reach`: checked by the device test on ctl / the arrays) and the
# groups its whole MSM is also run in ("" = stage test only).
Case = namedtuple("Case", "name req build expect reach groups")


def _rand(n, seed):
    from oracle import oracle as orc
    return orc.rand_fr(seed, n, mont=False)


def _witness(n, seed):
    from oracle import oracle as orc
    return orc.rand_fr(seed, n, mont=False, witness_like=True)


def _zeros(n):
    return np.zeros((n, 4), np.uint64)


def _rows_of(values, counts) -> np.ndarray:
    """(sum counts, 4): values[k] repeated counts[k] times (numpy: the large structured inputs)"""
    return np.repeat(limbs(values), counts, axis=0)


def _with_zeros(a, at):
    a[list(at)] = 0
    return a


def _one_nonzero_last(n, seed):
    a = _zeros(n)
    a[n - 1] = _rand(1, seed)[0]
    return a


def _zero_workgroup_between(seed):
    a = _rand(768, seed)
    a[256:512] = 0
    return a


def _bits01(n, seed):
    a = _zeros(n)
    a[:, 0] = np.random.default_rng(seed).integers(0, 2, n).astype(np.uint64)
    return a


def _bucket_fill(c, loads, singles=()):
    """table mode: `loads` = [(digit d, scalars)]: each scalar d * sum_w 2^(c w) puts one point per window into bucket d - 1; singles = digits d that get ONE
    more point (the scalar d itself: window 0 only)"""
    vals = [repeated_digit(d, c) for d, _ in loads] + [int(d) for d in singles]
    cnts = [k for _, k in loads] + [1] * len(singles)
    return _rows_of(vals, cnts)


def _cases():
    T = lambda c, **kw: dict(table_c=c, **kw)   # noqa: E731
    out = []
    add = lambda name, req, build, expect=None, reach=None, groups="g1": out.append(Case(name, req, build, expect or {}, reach or {}, groups))  # noqa: E731
    # ---- 3b compaction: table c = 8 (the narrowest width whose workgroup fits the stage) and c = 16
    for c in (8, 16):
        D = T(c, drop_zero_digits=True)
        e = dict(compacts=True)
        add("compact_c%d_all_zero" % c, D, lambda: [_zeros(300)], e, dict(device_total=0, tasks=0))
        add("compact_c%d_one_nonzero_in_last_partial_workgroup" % c, D, lambda c=c: [_one_nonzero_last(300, 0x3B0 + c)], e)
        add("compact_c%d_zero_workgroup_between_two" % c, D, lambda c=c: [_zero_workgroup_between(0x3B1 + c)], e)
        add("compact_c%d_witness_like" % c, D, lambda c=c: [_witness(1000, 0x3B2 + c)], e)
        for n in (255, 256, 257):   # (random digits of 16 bits are never zero: two zero scalars make the dropping visible in the pair count)
            add("compact_c%d_n%d" % (c, n), D, lambda c=c, n=n: [_with_zeros(_rand(n, 0x3B3 + c + n), (7, n - 1))], e)
    add("compact_c7_falls_back", T(7, drop_zero_digits=True), lambda: [_witness(300, 0x3B7)], dict(compacts=False), groups="")  # (no product entry builds a table narrower than 8)
    # ---- 3c sort geometry
    add("sort_1_pass_table_c8", T(8), lambda: [_rand(300, 0x3C0)], dict(npass=1, key_bits=8))
    add("sort_2_passes_table_c16", T(16), lambda: [_rand(300, 0x3C1)], dict(npass=2, key_bits=16))
    add("sort_3_passes_table_c17", T(17), lambda: [_rand(300, 0x3C2)], dict(npass=3, key_bits=17))
    add("sort_3_passes_table_c24", T(24), lambda: [_rand(300, 0x3C3)], dict(npass=3, key_bits=24))
    add("sort_4_passes_plain_c22", dict(window_bits=22), lambda: [_rand(200, 0x3C4)], dict(npass=4, key_bits=25))
    add("sort_4_passes_rows_512_sets_c16", T(16, rows=512, n=40, row_stride=41), lambda: [_rand(512 * 41, 0x3C5)], dict(npass=4, key_bits=25),
        groups="")  # (512 rows: no bases-level product entry takes more than three vectors; the Groth16 batch tests run the rows path to its sums)
    for n in (511, 512, 513):
        add("sort_tile_edge_n%d" % n, T(16), lambda n=n: [_rand(n, 0x3C6 + n)], dict(sort_tiles=(n * 16 + 8191) // 8192))
    add("sort_257_tiles", T(16), lambda: [_rand(131073, 0x3C7)], dict(sort_tiles=257))
    full = repeated_digit(1, 16)   # sixteen non-zero digits
    add("sort_device_length_one_tile", T(16, drop_zero_digits=True), lambda: [np.concatenate([_rows_of([full], [512]), _zeros(88)])],
        dict(sort_tiles=2, compacts=True), dict(device_total=8192, tiles_filled=1))
    add("sort_device_length_one_past_a_tile", T(16, drop_zero_digits=True), lambda: [np.concatenate([_rows_of([full, 5], [512, 1]), _zeros(87)])],
        dict(sort_tiles=2, compacts=True), dict(device_total=8193, tiles_filled=2))
    add("sort_all_pairs_in_one_key", T(16), lambda: [_rows_of([repeated_digit(77, 16)], [1000])], dict(npass=2), dict(largest=16000))
    # ---- 3d plan geometry
    add("plan_1_scan_tile_table_c11", T(11), lambda: [_rand(300, 0x3D0)], dict(scan_tiles=1))
    add("plan_2_scan_tiles_table_c12", T(12), lambda: [_rand(300, 0x3D1)], dict(scan_tiles=2))
    add("plan_257_scan_tiles_plain_c16", dict(window_bits=16), lambda: [_rand(300, 0x3D2)], dict(scan_tiles=257))
    add("plan_quantised_bins_plain_c2", dict(window_bits=2), lambda: [_rand(2048, 0x3D3)], dict(bshift=1, L=2050))
    add("plan_pick_len_alone", T(16), lambda: [_rand(300, 0x3D4)], dict(stats_pick=False, L=32, Lmin=32))
    add("plan_stats_pick_uniform", T(8), lambda: [_rand(300, 0x3D5)], dict(stats_pick=True, L=166, Lmin=32))
    add("plan_stats_pick_bits", T(8), lambda: [_bits01(300, 0x3D6)], dict(stats_pick=True, L=166, Lmin=32))
    flat = dict(stats_pick=False, L=32, Lmin=32)
    add("giant_t_exactly_256_tasks", T(16), lambda: [_bucket_fill(16, [(9, 512)], singles=range(100, 188))], flat, dict(bucket=(8, 8192, 256), giants=0))
    add("giant_t_257_tasks", T(16), lambda: [_bucket_fill(16, [(9, 512)], singles=[9] + list(range(100, 187)))], flat,
        dict(bucket=(8, 8193, 257), giants=1, last_task_len=1))
    add("giant_more_than_64x64_tasks", T(16), lambda: [_bucket_fill(16, [(9, 8193)])], flat, dict(bucket=(8, 131088, 4097), giants=1), groups="g1g2")
    add("giant_more_than_listed", T(22), lambda: [_bucket_fill(22, [(d, 683) for d in range(1, 50)])], flat, dict(giants=49, listed=48), groups="g1g2")
    # ---- batches (3a's table shapes, here with the whole pipeline behind them)
    add("batch_2_sets_same_pointer", T(16), lambda: (lambda a: [a, a])(_rand(300, 0x3E0)), dict(npass=3, key_bits=17))
    add("batch_3_sets_two_equal", T(12), lambda: (lambda a, b: [a, b, a])(_rand(300, 0x3E1), _witness(300, 0x3E2)), dict(scan_tiles=4))
    return out


CASES = _cases()
CASE = {c.name: c for c in CASES}
