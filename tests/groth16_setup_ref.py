"""Test infrastructure: groth16.Setup (oracle/bn254_ref.groth16_setup) and the solver step a, b, c = L w, R w, O w restated over a constraint
system held as numpy arrays, fast enough for 2^16 wires and millions of non-zeros -- the reference the device Setup (r1cs.hip) is compared with.

A `System` keeps each matrix (L, R, O) in two parts:
  * sparse entries: (row, wire, coefficient index) triples, the coefficient being `coef[index]` -- any shape, duplicates in a row included;
  * range columns (wire, b, e, k): the wire's column holds rows b .. e-1 with coefficient cr[k] * g[j % len(g)] in row j.
A range column's transposed product is then cr[k] * (P[e] - P[b]) with P the prefix sums of g[j % len(g)] * lag_j, and its part of the row sums
comes from a difference array: both O(n_constraints + n_wires) big-integer work however many entries the ranges hold.

The key's points come from the C oracle's batched fixed-base multiplication (orc_g1_mul_gen_many / orc_g2_mul_gen_many); the byte images from
oracle/plonk_ref.groth16_pk_bytes / groth16_vk_bytes.  Values are canonical Python ints mod r except where limbs are named."""
from __future__ import annotations

import numpy as np

from oracle import bn254_ref as ref
from oracle import oracle as orc
from oracle import plonk_ref as pl

R, Q = ref.R, ref.Q
_RINV_Q = pow(ref.MONT_R, -1, Q)


def canon_limbs(xs) -> np.ndarray:
    """ints < 2^256 -> (n, 4) little-endian uint64 limbs"""
    return np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in xs), dtype="<u8").reshape(-1, 4).astype(np.uint64)


def limbs_int(a) -> int:
    return int.from_bytes(np.ascontiguousarray(a, np.uint64).tobytes(), "little")


def mont_limbs(xs) -> np.ndarray:
    return canon_limbs([x % R * ref.MONT_R % R for x in xs])


def batch_inv(xs):
    """Montgomery's trick: every x non-zero"""
    pre, run = [], 1
    for x in xs:
        pre.append(run)
        run = run * x % R
    inv = pow(run, -1, R)
    out = [0] * len(xs)
    for i in range(len(xs) - 1, -1, -1):
        out[i] = inv * pre[i] % R
        inv = inv * xs[i] % R
    return out


class System:
    def __init__(self, n_constraints: int, n_wires: int, n_public: int, coef, sparse, ranges=((), (), ()), cr=(), g=(1,)):
        """coef: list of ints; sparse: three (rows, wires, coefficient indices) triples of int arrays; ranges: three lists of (wire, b, e, k)."""
        assert 1 <= n_public <= n_wires
        self.n_constraints, self.n_wires, self.n_public = n_constraints, n_wires, n_public
        self.coef = [c % R for c in coef]
        self.sparse = [tuple(np.asarray(a, dtype=np.int64) for a in s) for s in sparse]
        self.ranges = [list(r) for r in ranges]
        self.cr, self.g = [c % R for c in cr], [x % R for x in g]
        for rows, wires, vids in self.sparse:
            assert rows.size == wires.size == vids.size
            assert rows.size == 0 or (rows.min() >= 0 and rows.max() < n_constraints and wires.min() >= 0 and wires.max() < n_wires)
        for rg in self.ranges:
            for wire, b, e, k in rg:
                assert 0 <= wire < n_wires and 0 <= b <= e <= n_constraints and 0 <= k < len(self.cr)

    @classmethod
    def from_ref(cls, r1: ref.R1CS):
        """an oracle/bn254_ref R1CS (dicts wire -> coefficient) as a System"""
        coef, sparse = [], []
        for m in range(3):
            rows, wires, vids = [], [], []
            for j, con in enumerate(r1.constraints):
                for wire, cf in con[m].items():
                    rows.append(j); wires.append(wire); vids.append(len(coef)); coef.append(cf)
            sparse.append((rows, wires, vids))
        return cls(len(r1.constraints), r1.n_wires, r1.n_public, coef, sparse)

    def to_ref(self) -> ref.R1CS:
        """the same system as dicts (duplicates in a row summed: the products are linear in the entries) -- small systems only"""
        cons = [({}, {}, {}) for _ in range(self.n_constraints)]
        for m in range(3):
            for j, i, v in self._entries(m):
                cons[j][m][i] = (cons[j][m].get(i, 0) + v) % R
        return ref.R1CS(self.n_public, self.n_wires - self.n_public, cons)

    def _entries(self, m):
        rows, wires, vids = self.sparse[m]
        out = [(j, i, self.coef[v]) for j, i, v in zip(rows.tolist(), wires.tolist(), vids.tolist())]
        for wire, b, e, k in self.ranges[m]:
            out += [(j, wire, self.cr[k] * self.g[j % len(self.g)] % R) for j in range(b, e)]
        return out

    # ---------------------------------------------------------------------------------------------------- the device's CSR form
    def csr(self, m: int, seed: int = 0):
        """(ptr, idx, Montgomery val) of matrix m by constraint; the entries of a row in a seeded random order"""
        rows, wires, vids = (list(a) for a in self.sparse[m])
        ng = len(self.g)
        base = len(self.coef)
        for wire, b, e, k in self.ranges[m]:
            j = np.arange(b, e, dtype=np.int64)
            rows.append(j)
            wires.append(np.full(e - b, wire, np.int64))
            vids.append(base + k * ng + j % ng)
        rows, wires, vids = (np.concatenate([np.asarray(a, np.int64).reshape(-1) for a in x]) if x else np.zeros(0, np.int64) for x in (rows, wires, vids))
        perm = np.random.default_rng(seed).permutation(rows.size)
        order = perm[np.argsort(rows[perm], kind="stable")]
        table = mont_limbs(self.coef + [c * x for c in self.cr for x in self.g])
        ptr = np.zeros(self.n_constraints + 1, np.uint32)
        ptr[1:] = np.cumsum(np.bincount(rows, minlength=self.n_constraints))
        val = np.ascontiguousarray(table[vids[order]]) if order.size else np.zeros((0, 4), np.uint64)
        return ptr, np.ascontiguousarray(wires[order].astype(np.uint32)), val

    def csr_nnz(self, m: int) -> int:
        return int(self.sparse[m][0].size) + sum(e - b for _, b, e, _ in self.ranges[m])

    def load(self, seed: int = 0):
        """zk_bn254_r1cs_load of the CSR form -> a noir_backend_using_gnark_amd.groth16.R1CS"""
        import ctypes as C

        from noir_backend_using_gnark_amd import _lib
        from noir_backend_using_gnark_amd.groth16 import R1CS
        mats = [self.csr(m, seed + m) for m in range(3)]
        ptrs = []
        for ptr, idx, val in mats:
            ptrs += [ptr.ctypes.data, (idx if idx.size else np.zeros(1, np.uint32)).ctypes.data, (val if val.size else np.zeros((1, 4), np.uint64)).ctypes.data]
        raw = _lib.R1CS(self.n_constraints, self.n_wires, self.n_public, *ptrs)
        h = C.c_uint64(0)
        _lib.check(_lib.lib().zk_bn254_r1cs_load(C.byref(raw), C.byref(h)))
        return R1CS.from_handle(h.value, self.n_public, self.n_wires, self.n_constraints)

    # ---------------------------------------------------------------------------------------------------- the reference
    def eval_abc(self, w):
        """a, b, c = L w, R w, O w (lists of ints)"""
        nc, ng = self.n_constraints, len(self.g)
        out = []
        for m in range(3):
            acc = [0] * nc
            rows, wires, vids = self.sparse[m]
            for j, i, v in zip(rows.tolist(), wires.tolist(), vids.tolist()):
                acc[j] += self.coef[v] * w[i]
            diff = [0] * (nc + 1)
            for wire, b, e, k in self.ranges[m]:
                t = self.cr[k] * w[wire]
                diff[b] += t
                diff[e] -= t
            run = 0
            for j in range(nc):
                run = (run + diff[j]) % R
                acc[j] = (acc[j] + self.g[j % ng] * run) % R
            out.append(acc)
        return tuple(out)

    def column_sums(self, lag):
        """A_i, B_i, C_i = sum_j M[j][i] lag_j (the transposed products)"""
        nc, ng = self.n_constraints, len(self.g)
        P = [0] * (nc + 1)
        for j in range(nc):
            P[j + 1] = (P[j] + self.g[j % ng] * lag[j]) % R
        out = []
        for m in range(3):
            acc = [0] * self.n_wires
            rows, wires, vids = self.sparse[m]
            for j, i, v in zip(rows.tolist(), wires.tolist(), vids.tolist()):
                acc[i] += self.coef[v] * lag[j]
            for wire, b, e, k in self.ranges[m]:
                acc[wire] += self.cr[k] * (P[e] - P[b])
            out.append([x % R for x in acc])
        return tuple(out)


def lagrange_at(tau: int, n: int):
    """L_j(tau) = (tau^n - 1) / n * w^j / (tau - w^j) over the size-n domain: w^j built incrementally, one batch inversion"""
    gen = ref.Domain(n).gen
    ws = [1] * n
    for j in range(1, n):
        ws[j] = ws[j - 1] * gen % R
    zt = (pow(tau, n, R) - 1) % R
    assert zt, "tau is a root of unity of the domain"
    scale = zt * pow(n, -1, R) % R
    return [scale * w % R * d % R for w, d in zip(ws, batch_inv([(tau - w) % R for w in ws]))]


def _g1_tuples(a):
    raw = np.ascontiguousarray(a, np.uint64).tobytes()
    out = []
    for o in range(0, len(raw), 64):
        x, y = int.from_bytes(raw[o:o + 32], "little"), int.from_bytes(raw[o + 32:o + 64], "little")
        out.append(None if x == 0 and y == 0 else (x * _RINV_Q % Q, y * _RINV_Q % Q))
    return out


def _g2_tuples(a):
    raw = np.ascontiguousarray(a, np.uint64).tobytes()
    out = []
    for o in range(0, len(raw), 128):
        v = [int.from_bytes(raw[o + 32 * t:o + 32 * t + 32], "little") for t in range(4)]
        out.append(None if not any(v) else tuple((v[2 * t] * _RINV_Q % Q, v[2 * t + 1] * _RINV_Q % Q) for t in range(2)))
    return out


def setup(sys_: System, toxic, nthreads: int = 0) -> dict:
    """groth16.Setup(sys_) with toxic = (tau, alpha, beta, gamma, delta) ints.  Returns
    key: the oracle's key dict (oracle.groth16_prove takes it as is), vk: the device's vk dict layout (g1_alpha, g1_k = the n_public points K_i / gamma,
    g2_beta, g2_gamma, g2_delta), pk_bytes / vk_bytes: the ProvingKey.WriteTo / VerifyingKey.WriteTo images."""
    tau, alpha, beta, gamma, delta = (t % R for t in toxic)
    dom = ref.Domain(max(sys_.n_constraints, 1))
    n, logn = dom.n, dom.logn
    lag = lagrange_at(tau, n)
    A, B, Cc = sys_.column_sums(lag)
    gi, di = pow(gamma, -1, R), pow(delta, -1, R)
    npub = sys_.n_public
    K = [(beta * a + alpha * b + c) % R for a, b, c in zip(A, B, Cc)]
    zt_d = (pow(tau, n, R) - 1) * di % R
    z = [0] * n
    p = zt_d
    for i in range(n):
        z[ref.bitrev(i, logn)] = p
        p = p * tau % R
    g1 = lambda xs: orc.g1_mul_gen_many(canon_limbs(xs), scalars_mont=False, nthreads=nthreads) if len(xs) else np.zeros((0, 8), np.uint64)
    g2 = lambda xs: orc.g2_mul_gen_many(canon_limbs(xs), scalars_mont=False, nthreads=nthreads)
    s1 = g1([alpha, beta, delta])
    s2 = g2([beta, gamma, delta])
    key = dict(log_domain=logn, n_wires=sys_.n_wires, n_public=npub, g1_alpha=s1[0], g1_beta=s1[1], g1_delta=s1[2],
               g1_a=g1(A), g1_b=g1(B), g1_k=g1([k * di % R for k in K[npub:]]), g1_z=g1(z), g2_beta=s2[0], g2_delta=s2[2], g2_b=g2(B))
    vk = dict(g1_alpha=s1[0], g1_k=g1([k * gi % R for k in K[:npub]]), g2_beta=s2[0], g2_gamma=s2[1], g2_delta=s2[2])
    t1 = {k: _g1_tuples(key[k]) for k in ("g1_alpha", "g1_beta", "g1_delta", "g1_a", "g1_b", "g1_k", "g1_z")}
    t2 = {k: _g2_tuples(key[k]) for k in ("g2_beta", "g2_delta", "g2_b")}
    pk_t = dict(domain=dom, g1_alpha=t1["g1_alpha"][0], g1_beta=t1["g1_beta"][0], g1_delta=t1["g1_delta"][0], g1_a=t1["g1_a"], g1_b=t1["g1_b"],
                g1_k=t1["g1_k"], g1_z=t1["g1_z"], g2_beta=t2["g2_beta"][0], g2_delta=t2["g2_delta"][0], g2_b=t2["g2_b"])
    vk_t = dict(g1_alpha=pk_t["g1_alpha"], g1_beta=pk_t["g1_beta"], g1_delta=pk_t["g1_delta"], g2_beta=pk_t["g2_beta"], g2_delta=pk_t["g2_delta"],
                g2_gamma=_g2_tuples(s2[1])[0], g1_ic=_g1_tuples(vk["g1_k"]))
    return dict(key=key, vk=vk, pk_bytes=pl.groth16_pk_bytes(pk_t), vk_bytes=pl.groth16_vk_bytes(vk_t))


def skewed_small(seed: int = 0x64) -> System:
    """64 constraints over 24 wires (3 public): the ONE wire in every row of L, R and O; wire 23 in no matrix; wire 22 in O only; a duplicate wire
    in row 5 of L; coefficients 0, 1 and r - 1 among random ones; one range column in each matrix."""
    rng = np.random.default_rng(seed)
    nc, nw = 64, 24
    coef = [0, 1, R - 1] + ref.rand_felts(seed, 29)
    sparse = []
    for m in range(3):
        rows, wires = list(range(nc)), [0] * nc
        for j in range(nc):
            for _ in range(int(rng.integers(0 if m else 1, 3))):
                rows.append(j)
                wires.append(int(rng.integers(1, 22)))
        if m == 0:
            rows += [5, 5]
            wires += [7, 7]
        if m == 2:
            rows += [9, 40]
            wires += [22, 22]
        sparse.append((rows, wires, rng.integers(0, len(coef), size=len(rows))))
    ranges = ([(11, 3, 40, 0)], [(12, 0, 64, 1)], [(13, 20, 21, 2)])
    return System(nc, nw, 3, coef, sparse, ranges, cr=ref.rand_felts(seed + 1, 3), g=ref.rand_felts(seed + 2, 5))
