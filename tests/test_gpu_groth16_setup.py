"""GPU suite (-m gpu): groth16.Setup and the solver step on the device (r1cs.hip, util.hip's fixed-base multiplication) against the fast reference of
tests/groth16_setup_ref.py, byte for byte, at the shapes that drive each code path: a hot ONE column and columns either side of SPMV_LONG (k_spmv3_long,
the ballot path of k_csc_count / k_csc_fill), more long columns than SPMV_LONG_MAX holds (the overflow path of k_spmv3), n_wires either side of
k_csc_scan's split and domains of 1 to 2^13 points, the public-wire extremes (nk = 0), and solver rows of 0 to 10^5 entries.

For every system: ProvingKey.WriteTo and VerifyingKey.WriteTo of the device key equal the reference's images, the vk arrays equal the reference's
points, eval_abc equals the reference's a, b, c, and a proof made with the device key equals the oracle's proof with the reference key (same r, s)."""
import time

import numpy as np
import pytest

import noir_backend_using_gnark_amd as zk
from noir_backend_using_gnark_amd import _lib
from oracle import bn254_ref as ref
from oracle import oracle as orc
from tests import groth16_setup_ref as gs

pytestmark = pytest.mark.gpu
R = ref.R


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    _lib.require_device()  # fail loudly: no silent fallback


def _first_diff(got: bytes, want: bytes, what: str) -> str:
    n = min(len(got), len(want))
    k = next((i for i in range(n) if got[i] != want[i]), n)
    return "%s: %d bytes vs %d expected, first difference at byte %d" % (what, len(got), len(want), k)


def _same(got: bytes, want: bytes, what: str):
    if got != want:  # (not a plain assert: a diff of megabytes of key is no help)
        pytest.fail(_first_diff(got, want, what))


def _witness(n_wires: int, seed: int):
    """[1, random...] with every 7th value 0 and every 11th r - 1"""
    w = [1] + ref.rand_felts(seed, n_wires - 1)
    for i in range(1, n_wires):
        if i % 7 == 0:
            w[i] = 0
        elif i % 11 == 0:
            w[i] = R - 1
    return w


def check_system(name: str, sy: gs.System, seed: int, tables: bool):
    tox = tuple(ref.rand_felts(seed, 5))
    w = _witness(sy.n_wires, seed + 1)
    t0 = time.perf_counter()
    want = gs.setup(sy, tox)
    abc = sy.eval_abc(w)
    t_ref = time.perf_counter() - t0
    wm = gs.mont_limbs(w)
    dev = sy.load(seed)
    try:
        t0 = time.perf_counter()
        got = dev.eval_abc(wm)
        for m in range(3):
            exp = gs.mont_limbs(abc[m]).reshape(-1, 4)
            bad = np.flatnonzero((got[m] != exp).any(axis=1))
            assert bad.size == 0, "%s: eval_abc matrix %d differs in %d rows, first %s" % (name, m, bad.size, bad[:8].tolist())
        pk, vk = zk.setup(dev, gs.mont_limbs(tox), precompute_tables=tables)
        try:
            _same(pk.write_to(), want["pk_bytes"], name + " ProvingKey.WriteTo")
            _same(pk.vk_write_to(vk), want["vk_bytes"], name + " VerifyingKey.WriteTo")
            for k in ("g1_alpha", "g1_k", "g2_beta", "g2_gamma", "g2_delta"):
                assert np.array_equal(np.asarray(vk[k], np.uint64).reshape(want["vk"][k].shape), want["vk"][k]), (name, k)
            r, s = gs.mont_limbs(ref.rand_felts(seed + 2, 2))
            exp, _ = orc.groth16_prove(want["key"], *(gs.mont_limbs(v) for v in abc), wm, r, s)
            assert zk.prove_r1cs(dev, pk, wm, r, s) == exp, name + ": proof with the device key"
        finally:
            pk.free()
        print("%s: n_constraints %d, n_wires %d, n_public %d, nnz %s: reference %.2f s CPU, device %.2f s"
              % (name, sy.n_constraints, sy.n_wires, sy.n_public, [int(sy.csr_nnz(m)) for m in range(3)], t_ref, time.perf_counter() - t0))
    finally:
        dev.free()


def _random_sparse(rng, nc, pool, lo_hi, n_coef):
    """lo..hi entries per row drawn from the wires in `pool`, coefficient indices below n_coef"""
    lo, hi = lo_hi
    cnt = rng.integers(lo, hi + 1, size=nc)
    rows = np.repeat(np.arange(nc), cnt)
    return rows, np.asarray(pool)[rng.integers(0, len(pool), size=rows.size)], rng.integers(0, n_coef, size=rows.size)


# ------------------------------------------------------------------------------------------------ the systems
def hot_column_system() -> gs.System:
    """2^14 + 3 constraints (N = 2^15): ONE in every row of L, R and O; 40 columns of 1023, 1024, 1025, 1500 and 4000 entries (no other entry in
    them); 50 wires in no matrix, 50 in O only; the last 300 rows of R hold ONE alone; everything else 1 to 3 entries per column."""
    rng = np.random.default_rng(0x4C)
    nc, nw = (1 << 14) + 3, 12000
    coef = [0, 1, R - 1] + ref.rand_felts(0x4C, 61)
    hot = [100 + 7 * t for t in range(40)]
    nowhere, o_only = range(11000, 11050), range(11050, 11100)
    skip = set(hot) | set(nowhere) | set(o_only) | {0}
    ordinary = [i for i in range(nw) if i not in skip]
    ranges = [[(0, 0, nc, m)] for m in range(3)]
    for t, (wire, size) in enumerate(zip(hot, [1023, 1024, 1025, 1500, 4000] * 8)):
        b = int(rng.integers(0, nc - size + 1 - (300 if t % 3 == 1 else 0)))
        ranges[t % 3].append((wire, b, b + size, 3 + t % 4))
    sparse = [_random_sparse(rng, nc, ordinary, (1, 3), len(coef)), _random_sparse(rng, nc, ordinary, (0, 2), len(coef)),
              _random_sparse(rng, nc, ordinary + list(o_only), (1, 1), len(coef))]
    keep = sparse[1][0] < nc - 300  # the last 300 rows of R name ONE and nothing else: whole waves of the ballot path
    sparse[1] = tuple(a[keep] for a in sparse[1])
    return gs.System(nc, nw, 4, coef, sparse, ranges, cr=ref.rand_felts(0x4D, 6) + [R - 1], g=ref.rand_felts(0x4E, 13))


def overflow_system() -> gs.System:
    """1100 constraints; wires 1 .. 1450 hold a column of 1025 to 1100 contiguous rows in each of L, R and O: 4350 long columns (+ ONE's in L) where
    SPMV_LONG_MAX = 4096 fit the list, and solver rows of ~1450 entries; 1.5 M non-zeros per matrix"""
    rng = np.random.default_rng(0x0F)
    nc, nw = 1100, 1500
    coef = [1, R - 1] + ref.rand_felts(0x0F, 30)
    ranges = [[], [], []]
    for m in range(3):
        for wire in range(1, 1451):
            size = int(rng.integers(1025, nc + 1))
            b = int(rng.integers(0, nc - size + 1))
            ranges[m].append((wire, b, b + size, int(rng.integers(0, 5))))
    tail = list(range(1451, nw))
    sparse = [(np.arange(nc), np.zeros(nc, np.int64), rng.integers(0, len(coef), size=nc)),
              _random_sparse(rng, nc, tail, (1, 1), len(coef)), _random_sparse(rng, nc, tail, (0, 2), len(coef))]
    return gs.System(nc, nw, 4, coef, sparse, ranges, cr=ref.rand_felts(0x10, 5), g=ref.rand_felts(0x11, 17))


def random_system(nc: int, nw: int, npub: int, seed: int) -> gs.System:
    rng = np.random.default_rng(seed)
    coef = [0, 1, R - 1] + ref.rand_felts(seed, 29)
    pool = list(range(nw))
    return gs.System(nc, nw, npub, coef, [_random_sparse(rng, nc, pool, lh, len(coef)) for lh in ((1, 3), (0, 2), (1, 1))])


def eval_rows_system() -> gs.System:
    """solver rows of 0, 1, 1023, 1024, 1025 and 10^5 entries, duplicate wires in a row, coefficients 0, 1, r - 1 on wires whose value is 0 / r - 1"""
    rng = np.random.default_rng(0xE7)
    nc, nw = 9, 2000
    coef = [0, 1, R - 1] + ref.rand_felts(0xE7, 13)
    sizes = [0, 1, 1023, 1024, 1025, 100000, 5, 6, 0]
    sparse = []
    for m in range(3):
        sz = sizes if m == 0 else sizes[::-1] if m == 1 else [1 if j % 2 else 0 for j in range(nc)]
        rows = np.repeat(np.arange(nc), sz)
        wires = rng.integers(0, nw, size=rows.size)
        vids = rng.integers(0, len(coef), size=rows.size)
        if m < 2:
            j6 = np.flatnonzero(rows == (6 if m == 0 else 2))
            wires[j6] = [5, 5, 5, 9, 9][:len(j6)] + [5] * max(0, len(j6) - 5)   # duplicates in one row
            j7 = np.flatnonzero(rows == (7 if m == 0 else 1))
            wires[j7] = [7, 11, 14, 7, 11, 14][:len(j7)]                        # _witness: w_7 = w_14 = 0, w_11 = r - 1
            vids[j7] = [0, 1, 2, 2, 1, 0][:len(j7)]                             # coef[0 .. 2] = 0, 1, r - 1
        sparse.append((rows, wires, vids))
    return gs.System(nc, nw, 2, coef, sparse)


# ------------------------------------------------------------------------------------------------ the tests
def test_setup_with_a_hot_one_column_and_columns_around_spmv_long():
    check_system("hot_column", hot_column_system(), 0x101, tables=True)


def test_setup_with_more_long_columns_than_the_list_holds():
    check_system("overflow", overflow_system(), 0x102, tables=False)


@pytest.mark.parametrize("nw,nc", [(2, 1), (1023, 2), (1024, 3), (1025, 4096), (3 * 1024 + 7, 4097), (2 ** 16 + 1, 4096), (2 ** 16 + 1, 1), (2, 4097)])
def test_setup_geometry_sweep(nw, nc):
    check_system("geometry_%d_wires_%d_constraints" % (nw, nc), random_system(nc, nw, min(nw, 3), 0x200 + nw + nc), 0x103 + nc, tables=bool(nc % 2))


@pytest.mark.parametrize("npub", [1, 30])
def test_setup_public_wire_extremes(npub):
    """n_public = 1: the vk holds one K point; n_public = n_wires: the key's K array is empty"""
    check_system("public_%d_of_30" % npub, random_system(20, 30, npub, 0x300 + npub), 0x104 + npub, tables=npub == 1)


def test_setup_and_solver_rows_at_their_edges():
    check_system("eval_rows", eval_rows_system(), 0x105, tables=True)


def test_setup_rejects_bad_toxic_waste_and_the_handle_still_works():
    """a zero toxic-waste element and a tau with tau^N = 1 are refused; after each refusal a Setup on the same handle gives the reference's bytes"""
    sy = gs.skewed_small()
    tox = ref.rand_felts(0x106, 5)
    want = gs.setup(sy, tox)
    dev = sy.load()
    try:
        def good():
            pk, vk = zk.setup(dev, gs.mont_limbs(tox))
            _same(pk.write_to(), want["pk_bytes"], "ProvingKey.WriteTo after a refusal")
            _same(pk.vk_write_to(vk), want["vk_bytes"], "VerifyingKey.WriteTo after a refusal")
            pk.free()
        for i in range(5):
            bad = list(tox)
            bad[i] = 0
            with pytest.raises(_lib.ZkmiError, match="zero"):
                zk.setup(dev, gs.mont_limbs(bad))
            good()
        gen = ref.Domain(sy.n_constraints).gen
        for tau in (gen, pow(gen, 5, R), 1, R - 1):
            with pytest.raises(_lib.ZkmiError, match="root of unity"):
                zk.setup(dev, gs.mont_limbs([tau] + tox[1:]))
            good()
    finally:
        dev.free()
