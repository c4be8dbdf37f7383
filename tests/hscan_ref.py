"""Host model of the stages of the Horner suffix scan (csrc/scan.hpp), in Python integers and from the definition -- not from the kernels.

The scan over a row f of `n` coefficients at a point a is S_i = f_i + a S_(i+1) with S_n = 0.  The device cuts the row into workgroups of 256 lanes of K
consecutive coefficients: workgroup b spans [256 K b, 256 K (b + 1)), lane t of it starts at 256 K b + t K.  Write S^(b) for the same recurrence over the
coefficients of workgroup b ALONE (zero from the workgroup's end, or the row's end, on).  Then what the three passes leave behind is

    btot after pass 1   btot_local[b] = S^(b) at the workgroup's first index
    tcarry[b][t]        S^(b) at the first index of lane t + 1; zero for lane 255 and for lanes past the row's end
    btot after pass 2   btot[b] = S at the first index of workgroup b + 1
    total               S_0 = f(a)
    q                   q_i = S_(i+1) for i < n, so q_(n-1) = 0: the coefficients of (f - f(a)) / (X - a), and one zero

and a workgroup wholly above the row's end holds zeros at every stage.  tests/test_hscan_ref_cpu.py holds this against oracle/plonk_ref.py's poly_eval and
divide_by_x_minus_a; tests/test_gpu_hscan_stages.py holds zk_bn254_hscan_inspect against it."""
from oracle import bn254_ref as ref

R = ref.R
LANES = 256


def suffix(f, a):
    """[S_0 .. S_n] of S_i = f_i + a S_(i+1), S_n = 0"""
    S = [0] * (len(f) + 1)
    acc = 0
    for i in range(len(f) - 1, -1, -1):
        acc = (f[i] + a * acc) % R
        S[i] = acc
    return S


def scan_blocks(n, K):
    """workgroups a row of n coefficients needs at K coefficients per lane (csrc/scan.hpp scan_blocks)"""
    return ((n + K - 1) // K + LANES - 1) // LANES


def stages(f, a, K, nb=0):
    """every stage of the scan of f at a with K coefficients per lane over nb workgroups (0: what the row needs)"""
    n, W = len(f), LANES * K
    nb = nb or scan_blocks(n, K)
    assert n >= 1 and K >= 1 and nb * W >= n, (n, K, nb)
    S = suffix(f, a)
    btot_local, btot, tcarry = [0] * nb, [0] * nb, [[0] * LANES for _ in range(nb)]
    for b in range(nb):
        lo, hi = W * b, min(n, W * (b + 1))
        if lo >= n:
            continue  # wholly above the row's end: zeros
        Sb = suffix(f[lo:hi], a)  # Sb[i - lo] = S^(b)_i; zero from hi on
        btot_local[b] = Sb[0]
        for t in range(LANES - 1):
            i = lo + (t + 1) * K
            tcarry[b][t] = Sb[i - lo] if i < hi else 0
        btot[b] = S[hi] if hi == W * (b + 1) else 0
    return dict(K=K, nb=nb, btot_local=btot_local, tcarry=tcarry, btot=btot, total=S[0], q=S[1:])


def poly_with_root(rng, n, root):
    """(X - root) times a random polynomial of n - 1 coefficients"""
    g = [rng.randrange(R) for _ in range(n - 1)]
    p = [0] * n
    for i, c in enumerate(g):
        p[i] = (p[i] - root * c) % R
        p[i + 1] = (p[i + 1] + c) % R
    return p


def element_of_order(m):
    """an element of multiplicative order exactly m in Fr (m a power of a prime that divides r - 1), or None where r - 1 has no such factor"""
    if (R - 1) % m:
        return None
    p = next(d for d in range(2, m + 1) if m % d == 0)  # m = p^e
    for base in range(2, 64):
        w = pow(base, (R - 1) // m, R)
        if pow(w, m // p, R) != 1:
            return w
    raise AssertionError("no element of order %d among the small bases" % m)


def lengths_for(K):
    """the boundary lengths of the stage tests at K coefficients per lane: a row shorter than a lane, one lane, a tail lane of one coefficient, a top workgroup
    of 1, 2 and 256 live lanes"""
    W = LANES * K
    out = []
    for n in (1, K - 1, K, K + 1, W - 1, W, W + 1, 2 * W, 2 * W + 1, 2 * W + K + 1):
        if n >= 1 and n not in out:
            out.append(n)
    return out
