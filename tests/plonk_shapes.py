"""Circuits, solutions and blinders for the PLONK prover sweeps (tests/test_gpu_plonk_shapes.py) and the constants both test modules share.  Pure Python,
no device.  tests/test_plonk_shapes_cpu.py checks every builder (satisfied, the requested domain, the permutation it claims) and that the two oracles
give the same bytes on all of them, so a device mismatch points at the device.

A family is a '+'-joined set of traits.  Value traits: `zeros`, `max` (default: random values with a planted 0 and 1).  Wiring traits: `identity_perm`,
`one_cycle` (default: random wiring).  Selector trait: `empty_rows`.  `random` names the defaults.  FAMILIES lists the six single ones;
"zeros+identity_perm" is the one combination the tests use."""
from oracle import bn254_ref as ref
from oracle import plonk_ref as pl

R = ref.R

SWEEP_LOG_N = range(2, 17)
NPUB_CASES = (0, 1, 31, 32, 33, 64)
PI_DIRECT_MAX = 32          # csrc/plonk.hip PLONK_PI_DIRECT_MAX: up to here k_qk_coset adds the public inputs' share point by point; above, qk is transformed
WINDOW_TABLE_MIN = 4096     # csrc/plonk.hip: with the Lagrange-form SRS, l, r, o are committed from the wire values (plonk_blind_tail) iff n + 2 >= 4096
FAMILIES = ("random", "zeros", "max", "identity_perm", "one_cycle", "empty_rows")
BLINDER_FAMILIES = ("random", "zeros", "max")
FILLS = ("full", "half", "one_short")
DEGENERATE = ("zeros", "zeros+identity_perm")   # with zero blinders: l = r = o = 0, commitments that are the point at infinity


def scan_plan(length):
    """(K, nb) of csrc/scan.hpp scan_plan(): K consecutive elements per lane, nb workgroups of 256 lanes"""
    K = max(8, (length + 256 * 1024 - 1) // (256 * 1024))
    lanes = (length + K - 1) // K
    return K, (lanes + 255) // 256


def scan_lengths(n):
    """the lengths the prover scans at domain size n: z's prefix product (n), l / r / o (n + 2), z's division (n + 3), the quotient's three parts
    (3(n + 2)) -- and n + 8, the length scan_bufs() is called with: ONE plan serves all of them"""
    return (n, n + 2, n + 3, 3 * (n + 2), n + 8)


def domain_size(spr):
    """fft.NewDomain(nbConstraints + nbPublic).Cardinality"""
    n = 1
    while n < len(spr.constraints) + spr.n_public:
        n <<= 1
    return n


def rows_of(n, fill):
    """nc + npub for a domain of n rows: "full" = n, "half" = n // 2 + 1 (the fewest rows that still select this domain), "one_short" = n - 1, or an
    integer in (n / 2, n]"""
    rows = {"full": n, "half": n // 2 + 1, "one_short": n - 1}[fill] if isinstance(fill, str) else int(fill)
    assert n >= 2 and n & (n - 1) == 0 and n // 2 < rows <= n, (n, fill)
    return rows


def with_solution(spr, sol):
    """the same gates with qk re-derived so that `sol` satisfies them"""
    gates = []
    for ql, qr, qo, qm, _, xa, xb, xc in spr.constraints:
        qk = (-(ql * sol[xa] + qr * sol[xb] + qo * sol[xc] + qm * sol[xa] * sol[xb])) % R
        gates.append((ql, qr, qo, qm, qk, xa, xb, xc))
    return pl.SparseR1CS(spr.n_public, spr.n_secret, gates)


def circuit(family, n, npub, fill, seed):
    """-> (SparseR1CS, solution): satisfiable, nc + npub == rows_of(n, fill), hence a domain of exactly n rows.

    random         random wiring over nvars ~ rows / 3 variables (long copy cycles), random selectors, every 7th gate without qm, every 11th without ql, qr
                   (tests/test_gpu_plonk.py _random_circuit); solution[1] = 0, solution[2] = 1
    zeros          every variable 0, hence every qk = 0
    max            every secret variable r - 1, the public ones alternate 0, r - 1; qk derived
    identity_perm  nvars = 3 (nc + npub); gate i names the variables npub + 3 i, + 1, + 2 and nothing else names them.  The slots no gate fills -- R and O of
                   the npub placeholder rows, all three of the n - rows padding rows -- name variable 0 as gnark's lro array does (zero-initialised), and so
                   does L of the first placeholder row (npub > 0) or of the first gate (npub == 0).  The permutation is therefore the identity everywhere
                   except on ONE cycle through those slots, in increasing slot order; with npub == 0 and fill "full" that cycle has length 1 and the
                   permutation IS the identity (z = 1).  expected_identity_perm() restates this.
    one_cycle      every slot of every gate names the first secret variable (variable npub); with npub == 0 that is variable 0, which the padding rows
                   name too: one cycle through all 3 n slots
    empty_rows     every second gate (the odd ones) has ql = qr = qo = qm = qk = 0
    """
    traits = set(family.split("+"))
    assert traits <= {"random", "zeros", "max", "identity_perm", "one_cycle", "empty_rows"}, family
    rows = rows_of(n, fill)
    nc = rows - npub
    assert nc >= 1 and npub >= 0, (n, npub, fill)
    g = ref.SplitMix64(seed)
    if "identity_perm" in traits:
        nvars = 3 * rows
        wires = [(npub + 3 * i, npub + 3 * i + 1, npub + 3 * i + 2) for i in range(nc)]
    elif "one_cycle" in traits:
        nvars = npub + 1
        wires = [(npub, npub, npub)] * nc
    else:
        nvars = max(npub + 3, rows // 3 + 3)
        wires = [tuple(int(g.next() % nvars) for _ in range(3)) for _ in range(nc)]
    if "zeros" in traits:
        sol = [0] * nvars
    elif "max" in traits:
        sol = [(R - 1) * (i & 1) for i in range(npub)] + [R - 1] * (nvars - npub)
    else:
        sol = [g.felt() for _ in range(nvars)]
        if nvars > 2 and "one_cycle" not in traits:
            sol[1], sol[2] = 0, 1
    gates = []
    for i, (xa, xb, xc) in enumerate(wires):
        ql, qr, qo, qm = (g.felt() for _ in range(4))
        if i % 7 == 0: qm = 0
        if i % 11 == 0: ql = qr = 0
        if "empty_rows" in traits and i & 1: ql = qr = qo = qm = 0
        gates.append((ql, qr, qo, qm, 0, xa, xb, xc))
    spr = with_solution(pl.SparseR1CS(npub, nvars - npub, gates), sol)
    return spr, sol


def expected_identity_perm(n, npub, rows):
    """the permutation of an identity_perm circuit, from its docstring alone"""
    zero_slots = [0]
    for j in (1, 2):
        zero_slots += [j * n + i for i in range(npub)]
    for j in (0, 1, 2):
        zero_slots += [j * n + i for i in range(rows, n)]
    zero_slots = sorted(set(zero_slots))
    perm = list(range(3 * n))
    for k, s in enumerate(zero_slots):
        perm[s] = zero_slots[k - 1]     # buildPermutation: every slot points at the previous slot of its variable, the first at the last
    return perm


def blinders(family, seed=0):
    """the nine blinding scalars (l: 2, r: 2, o: 2, z: 3)"""
    return {"random": lambda: ref.rand_felts(0xB11D + seed, 9), "zeros": lambda: [0] * 9, "max": lambda: [R - 1] * 9}[family]()


def edge_public_values(spr, sol):
    """the same circuit with public inputs r - 1, 0, random, r - 1, 0, ... (qk re-derived)"""
    sol = list(sol)
    for i in range(spr.n_public):
        if i % 3 != 2:
            sol[i] = (R - 1, 0)[i % 3]
    return with_solution(spr, sol), sol


VIOLATIONS = ("last_gate", "first_gate", "public_input")


def violation_circuit(n, npub, seed):
    """-> (spr, sol, {where: variable}): a random circuit that fills its domain (the last gate is row n - 1) with one fresh secret variable that only the last
    gate names (its O slot), one that only the first gate names (its O slot), and public variable 0 named by the second gate's L slot; the three selectors
    in front of them are non-zero, so changing any of the three values violates that gate."""
    spr, sol = circuit("random", n, npub, "full", seed)
    assert npub >= 1 and len(spr.constraints) >= 3
    gates, sol = [list(c) for c in spr.constraints], list(sol)
    v_first, v_last = len(sol), len(sol) + 1
    g = ref.SplitMix64(seed ^ 0xBAD)
    sol += [g.felt(), g.felt()]
    gates[0][7], gates[-1][7], gates[1][5] = v_first, v_last, 0
    for row, col in ((0, 2), (-1, 2), (1, 0)):
        if gates[row][col] == 0: gates[row][col] = 1 + g.felt() % (R - 1)
    gates[1][3] = 0   # no product term on the public input's gate: its change cannot be cancelled by the other factor being zero
    out = with_solution(pl.SparseR1CS(npub, len(sol) - npub, gates), sol)
    return out, sol, dict(last_gate=v_last, first_gate=v_first, public_input=0)


def c_key(orc, spr, srs_np, nthreads=0):
    """the C oracle's key (orc.PlonkKeyC) for a SparseR1CS"""
    M = pl.ints_to_mont_np
    g = spr.constraints
    return orc.PlonkKeyC(spr.n_public, spr.n_vars, *[M([c[k] for c in g]) for k in (0, 1, 3, 2, 4)], *[[c[k] for c in g] for k in (5, 6, 7)], srs_np, nthreads=nthreads)


def decode_proof(proof, decompress):
    """Proof.WriteTo bytes -> the dict oracle/plonk_ref.plonk_verify takes"""
    assert len(proof) == 548 and proof[256:260] == b"\x00\x00\x00\x07"
    pts = [decompress(proof[32 * i:32 * i + 32]) for i in range(7)]
    return dict(lro=pts[0:3], z=pts[3], h=pts[4:7], batch_h=decompress(proof[224:256]),
                claimed=[int.from_bytes(proof[260 + 32 * i:292 + 32 * i], "big") for i in range(7)],
                z_open_h=decompress(proof[484:516]), zu=int.from_bytes(proof[516:548], "big"))
