"""Shapes for the Groth16 prover sweep (tests/test_gpu_groth16_shapes.py): every small domain, every wire split, every constraint count, the witness and
(a, b, c) kinds at which the orchestration in csrc/groth16.hip and csrc/groth16_batch.hip takes another branch.  No device, no pytest: the C oracle's
generators and numpy only.  tests/test_groth16_shapes_cpu.py holds the table (both references agree on it, it reaches every branch it names, and it can catch
an error).

A case is a key geometry (log_domain, n_wires, n_public) with an infinity pattern, and one proof's data: n_constraints, a witness kind, an (a, b, c) kind and
an (r, s) kind.  Its name is "<key part>__<data part>"; the key's seed comes from the key part and the data's from the whole name, so cases with the same
geometry and infinity pattern share ONE key and become rows of one zk.prove_batch call (batch_groups; one call per n_constraints, since the rows of a batch
have one width).  A key with a single wire has a single public wire where the sweep otherwise asks for two.

The table is a sparse design.  The witness kinds sit at log_domain 2 and 5 on a Latin square over n_public in {1, 3}: every kind meets both domains and both
splits, in two cases instead of four; the (a, b, c) kinds rotate over those cases and the (r, s) kinds over the whole table.

Witness kinds   uniform, witness_like (orc.rand_fr(..., witness_like=True)), zero, e0 = (1, 0, ..., 0), ones, max (all r_mod - 1), pub_zero (public part zero,
                private part uniform), priv_zero (private part zero: K's sum is the point at infinity while A's is not)
(a, b, c) kinds sat (c = a b), zero (h = 0), c_random (c is not a b: the prover does not check, both references define h regardless), a_tail_zero (the second
                half of a -- and so of c = a b -- is zero while b is not: what a caller that padded a itself hands over)
(r, s) kinds    zero (0, 0), r_one (1, 0), s_one (0, 1), max (r_mod - 1 twice), random
Infinity        none; a_all (every point of A: gnark's compact array is empty, NbInfinityA = n_wires); b_all (every point of B and G2.B); wire0, pub_last
                (wire n_public - 1), priv_first (wire n_public), last: that wire's point in A, B and G2.B"""
import hashlib
from typing import NamedTuple

import numpy as np

from oracle import bn254_ref as ref
from oracle import oracle as orc
from tests.helpers import mont_limbs

R = ref.R
BATCH_MAX_LOG_DOMAIN = 16   # csrc/groth16_batch.hip
W_KINDS = ("uniform", "witness_like", "zero", "e0", "ones", "max", "pub_zero", "priv_zero")
ABC_KINDS = ("sat", "zero", "c_random", "a_tail_zero")
RS_KINDS = ("zero", "r_one", "s_one", "max", "random")
INF_KINDS = ("none", "a_all", "b_all", "wire0", "pub_last", "priv_first", "last")
PREDICATES = ("direct", "host_order", "share_k", "nk == 0", "tables_possible", "batched_possible", "w_has_no_pairs", "h_is_zero")


class Case(NamedTuple):
    name: str
    log_domain: int
    n_wires: int
    n_public: int
    n_constraints: int
    w: str
    abc: str
    rs: str
    inf: str

    @property
    def N(self):
        return 1 << self.log_domain

    @property
    def key_part(self):
        return self.name.split("__")[0]


def _name(ld, nw, npub, inf, nc, w, abc, rs, tag=""):
    return "ld%d_w%d_p%d_%s__%snc%d_%s_%s_%s" % (ld, nw, npub, inf, tag, nc, w, abc, rs)


def make_case(ld, nw, npub, nc, w, abc, rs, inf, tag=""):
    assert 1 <= npub <= nw and 0 <= nc <= (1 << ld), (ld, nw, npub, nc)
    assert w in W_KINDS and abc in ABC_KINDS and rs in RS_KINDS and inf in INF_KINDS
    assert inf != "priv_first" or npub < nw
    return Case(_name(ld, nw, npub, inf, nc, w, abc, rs, tag), ld, nw, npub, nc, w, abc, rs, inf)


def predicates(case) -> dict:
    """the branches of csrc/groth16.hip this case is meant to reach, from its shape alone.  `direct` is taken by the device-inputs door and `host_order` by the
    host-inputs door; the test sends every case through both."""
    N, nk = case.N, case.n_wires - case.n_public
    tables = case.n_wires >= 1 and N > 1
    return {
        "direct": case.n_constraints == N and N > 1,                  # on_device && n_constraints == N && N > 1
        "host_order": case.n_wires > 0 and N > 1,                     # !on_device && nw > 0 && N > 1
        "share_k": nk > 0 and case.n_wires > 0,                       # k_shares_w: K's scalars are w[n_public:]
        "nk == 0": nk == 0,
        "tables_possible": tables,                                    # pk_build_tables returns early for n_wires == 0 || N <= 1
        "batched_possible": tables and case.log_domain <= BATCH_MAX_LOG_DOMAIN,
        "w_has_no_pairs": case.w == "zero",                           # msm5_prepare_w drops every digit
        "h_is_zero": case.abc == "zero" or case.n_constraints == 0,
    }


def _build_cases():
    cases, seen = [], set()

    def add(ld, nw, npub, nc=None, w="uniform", abc="sat", rs=None, inf="none"):
        nc = (1 << ld) if nc is None else nc
        shape = (ld, nw, npub, nc, w, abc, inf)
        if shape in seen:
            return
        seen.add(shape)
        cases.append(make_case(ld, nw, npub, nc, w, abc, rs or RS_KINDS[len(cases) % len(RS_KINDS)], inf))

    # every domain: n_wires around N, two public wires (one where the key has a single wire)
    for ld in range(9):
        N = 1 << ld
        for nw in (N - 1, N, N + 1):
            if nw >= 1:
                add(ld, nw, min(2, nw))
    # wire split
    for ld in (1, 3, 6):
        N = 1 << ld
        for nw in (1, 2, 3 * N):
            for npub in (1, 2, nw - 1, nw):
                if 1 <= npub <= nw:
                    add(ld, nw, npub)
    # constraint count
    for ld in (1, 4, 7):
        N = 1 << ld
        for nc in (0, 1, N - 1, N):
            add(ld, N, 2, nc=nc)
    # witness kinds on a Latin square over (log_domain, n_public); the (a, b, c) kinds rotate; n_constraints < N at log_domain 5 except where the caller padded
    for i, w in enumerate(W_KINDS):
        add(2, 5, (1, 3)[i & 1], nc=4, w=w, abc=ABC_KINDS[i % 4])
        abc = ABC_KINDS[(i + 1) % 4]
        add(5, 31, (3, 1)[i & 1], nc=32 if abc == "a_tail_zero" else 29, w=w, abc=abc)
    # the (a, b, c) kinds once more where the padding is the caller's business
    add(3, 8, 2, nc=7, abc="c_random")
    add(4, 17, 3, nc=16, abc="a_tail_zero")
    # points at infinity in the key
    for ld in (3, 5):
        N = 1 << ld
        for inf in INF_KINDS[1:]:
            add(ld, N + 1, 3, inf=inf, w="uniform" if ld == 3 else "max")
    # N = 1: no tables, no batched path, computeH of one point, Z's multi-exp empty
    add(0, 2, 1)
    add(0, 2, 2, w="zero")
    add(0, 2, 1, nc=0)
    add(0, 3, 1, abc="zero", w="e0")
    # skew: the two table geometries (tab_w by n_wires, tab_h by N - 1) far apart
    add(1, 5000, 3)
    add(12, 2, 1)
    add(12, 2, 2)
    return tuple(cases)


CASES = _build_cases()


def seed_of(text: str) -> int:
    return int.from_bytes(hashlib.sha256(text.encode()).digest()[:6], "big")


def infinity_bitmaps(case):
    """gnark's InfinityA / InfinityB: one bool per wire"""
    ia, ib = np.zeros(case.n_wires, bool), np.zeros(case.n_wires, bool)
    if case.inf == "a_all":
        ia[:] = True
    elif case.inf == "b_all":
        ib[:] = True
    elif case.inf != "none":
        i = {"wire0": 0, "pub_last": case.n_public - 1, "priv_first": case.n_public, "last": case.n_wires - 1}[case.inf]
        ia[i] = ib[i] = True
    return ia, ib


def key_dict(case, with_infinity=True) -> dict:
    """the dict zk.ProvingKey(**pkd) and orc.groth16_prove both take: wire-indexed arrays, (0, 0) for a point at infinity.  with_infinity=False: the same key
    with a real point in every place (what a prover that does not skip those wires sums)"""
    k, N, nw = seed_of(case.key_part), case.N, case.n_wires
    g1, g2 = orc.g1_gen_points, orc.g2_gen_points
    pkd = dict(log_domain=case.log_domain, n_wires=nw, n_public=case.n_public, g1_alpha=g1(k + 1, 1)[0], g1_beta=g1(k + 2, 1)[0], g1_delta=g1(k + 3, 1)[0],
               g1_a=g1(k + 4, nw), g1_b=g1(k + 5, nw), g1_k=g1(k + 6, nw - case.n_public), g1_z=g1(k + 7, N), g2_beta=g2(k + 8, 1)[0], g2_delta=g2(k + 9, 1)[0],
               g2_b=g2(k + 10, nw))
    if with_infinity:
        ia, ib = infinity_bitmaps(case)
        pkd["g1_a"][ia] = 0
        pkd["g1_b"][ib] = 0
        pkd["g2_b"][ib] = 0
    return pkd


def compact_key(case, pkd) -> dict:
    """gnark's own layout of the same key: A / B / G2.B without their points at infinity, plus the bitmaps"""
    ia, ib = infinity_bitmaps(case)
    return dict(pkd, g1_a=pkd["g1_a"][~ia], g1_b=pkd["g1_b"][~ib], g2_b=pkd["g2_b"][~ib], infinity_a=ia, infinity_b=ib)


ONE, MAX = mont_limbs([1])[0], mont_limbs([R - 1])[0]


def _mul(a, b):
    return np.stack([orc.fe_op("mul", 0, a[i], b[i]) for i in range(len(a))]) if len(a) else np.zeros((0, 4), np.uint64)


def inputs(case):
    """-> (a, b, c, w, r, s) as Montgomery limb arrays: a, b, c (n_constraints, 4), w (n_wires, 4), r, s (4,)"""
    d, nw, npub, nc = seed_of(case.name), case.n_wires, case.n_public, case.n_constraints
    w = orc.rand_fr(d + 1, nw, witness_like=case.w == "witness_like")
    if case.w == "zero":
        w[:] = 0
    elif case.w == "e0":
        w[:] = 0
        w[0] = ONE
    elif case.w == "ones":
        w[:] = ONE
    elif case.w == "max":
        w[:] = MAX
    elif case.w == "pub_zero":
        w[:npub] = 0
    elif case.w == "priv_zero":
        w[npub:] = 0
    a, b = orc.rand_fr(d + 2, nc), orc.rand_fr(d + 3, nc)
    if case.abc == "a_tail_zero":
        a[nc // 2:] = 0
    c = orc.rand_fr(d + 4, nc) if case.abc == "c_random" else _mul(a, b)
    if case.abc == "zero":
        a[:], b[:], c[:] = 0, 0, 0
    zero = np.zeros(4, np.uint64)
    rnd = orc.rand_fr(d + 5, 2)
    r, s = {"zero": (zero, zero), "r_one": (ONE, zero), "s_one": (zero, ONE), "max": (MAX, MAX), "random": (rnd[0], rnd[1])}[case.rs]
    return a, b, c, w, r.copy(), s.copy()


def batch_groups():
    """-> [(group name, [Case, ...])]: the cases of one key and one n_constraints as the rows of one batch.  A group that would have one row gets a second,
    uniform one, and every row with an all-zero witness sits between two rows whose witness is not zero (further uniform rows where the group has too few), so
    that a preparation shared by the rows cannot hide it.  The added rows are cases of their own (tag "extra") outside CASES."""
    by_key = {}
    for c in CASES:
        by_key.setdefault((c.key_part, c.n_constraints), []).append(c)
    groups = []
    for (key_part, nc), rows in by_key.items():
        first = rows[0]
        plain = [c for c in rows if c.w != "zero"]
        zeros = [c for c in rows if c.w == "zero"]
        extra = iter(make_case(first.log_domain, first.n_wires, first.n_public, nc, "uniform", "sat", "random", first.inf, tag="extra%d_" % k) for k in range(len(rows) + 2))
        while len(plain) < max(len(zeros) + 1, 2 - len(zeros)):
            plain.append(next(extra))
        ordered = []
        for i, c in enumerate(plain):
            ordered.append(c)
            if i < len(zeros):
                ordered.append(zeros[i])
        groups.append(("%s__nc%d" % (key_part, nc), ordered))
    return groups


def differing_parts(got: bytes, want: bytes) -> str:
    """which of Ar | Bs | Krs differ (bytes 0-32, 32-96, 96-128)"""
    return " ".join(n for n, lo, hi in (("Ar", 0, 32), ("Bs", 32, 96), ("Krs", 96, 128)) if got[lo:hi] != want[lo:hi]) or "none"
