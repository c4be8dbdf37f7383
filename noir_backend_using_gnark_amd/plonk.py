"""Host-side mirror of gnark v0.8.0's PLONK backend for the hot path (pinned at /root/reference/gnark_backend_ffi/go.mod:23):
    plonk.Setup(spr, srs)          reached at /root/reference/gnark_backend_ffi/backend/plonk/plonk.go:21   -> setup(circuit, srs)
    plonk.Prove(spr, pk, witness)  reached at backend/plonk/plonk.go:67 (PlonkProveWithPK, main.go:24-37)  -> prove(pk, solution, blinders)
The constraint system is the reference's: one gate qL*xa + qR*xb + qO*xc + qM*xa*xb + qK = 0 per ACIR arithmetic opcode
(backend/plonk/sparse_r1cs.go:44-107).  `prove` starts where gnark's prover is after `spr.Solve`: the values of all variables.
The blinding scalars (upstream: fr.SetRandom) are explicit inputs; the challenges follow upstream's SHA-256 transcript unless pinned.
Everything dispatches to libzkmi.so; nothing is computed on the host here."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, lib, vp
from .bn254 import ResidentBases

PROOF_BYTES = _lib.PLONK_PROOF_BYTES


class Circuit:
    """cs.SparseR1CS in the shape the reference builds it: n_public public + (n_vars - n_public) secret variables, gates as arrays.
    Coefficients: (n_constraints, 4) uint64 Montgomery images (numpy) or DeviceBuffers; wire ids: uint32 numpy arrays."""

    def __init__(self, n_public: int, n_vars: int, ql, qr, qo, qm, qk, xa, xb, xc):
        self.n_public, self.n_vars = n_public, n_vars
        self.xa, self.xb, self.xc = (np.ascontiguousarray(v, dtype=np.uint32) for v in (xa, xb, xc))
        self.n_constraints = int(self.xa.shape[0])
        self.on_device = isinstance(ql, _lib.DeviceBuffer)
        self.coeffs = [ql, qr, qo, qm, qk] if self.on_device else [np.ascontiguousarray(v, dtype=np.uint64).reshape(-1, 4) for v in (ql, qr, qo, qm, qk)]


class ProvingKey:
    """plonk.ProvingKey resident in HBM (canonical selectors / permutation polynomials, their Lagrange-coset forms on the big domain,
    the per-proof workspace) plus the verifying key's digests."""

    def __init__(self, handle: int, srs: ResidentBases, vk: dict | None, n_vars: int):
        self.handle, self.srs, self.vk, self.n_vars = C.c_uint64(handle), srs, vk, n_vars

    def export(self, which: int, n: int) -> np.ndarray:
        out = np.zeros((n, 4), dtype=np.uint64)
        check(lib().zk_bn254_plonk_pk_export(self.handle, C.c_int(which), vp(out), C.c_size_t(n)))
        return out

    def write(self, as_hex: bool = False) -> bytes:
        """plonk.ProvingKey.WriteTo (as_hex: the text SerializeProvingKey hands to Rust, internal/backend/helpers.go:82-87)"""
        n = C.c_size_t(0)
        lib().zk_bn254_plonk_pk_write(self.handle, C.c_int(int(as_hex)), C.create_string_buffer(1), C.c_size_t(0), C.byref(n))  # size query
        buf = C.create_string_buffer(n.value)
        check(lib().zk_bn254_plonk_pk_write(self.handle, C.c_int(int(as_hex)), buf, C.c_size_t(n.value), C.byref(n)))
        return buf.raw[:n.value]

    def lagrange_srs(self) -> None:
        """Build the SRS's Lagrange form over this key's domain (zk_bn254_plonk_pk_lagrange_srs): later proofs commit l, r, o from the wire values."""
        check(lib().zk_bn254_plonk_pk_lagrange_srs(self.handle))

    @property
    def domain_size(self) -> int:
        """Domain[0].Cardinality"""
        if self.vk is not None:
            return int(self.vk["size"])
        n = C.c_size_t(0)
        check(lib().zk_bn254_plonk_pk_info(self.handle, C.byref(n), None, None, None))
        return int(n.value)

    def ratio_batch(self, l, r, o, beta, gamma, *, rows: int | None = None, in_stride: int | None = None, out_stride: int | None = None, out=None):
        """ratio_copy_batch with this key's permutation, domain and twiddles (zk_bn254_plonk_ratio_batch_dev): round 2 of `rows` proofs against one key.
        Host arrays ((rows, n, 4); beta, gamma (rows, 4)) go to the device and Z comes back as a new array; device buffers / pointers are used where they are
        and `out` (made here when None) is returned.  Every shape / dtype / stride / count error is raised before the library is called."""
        return _pk_ratio_batch(self, l, r, o, beta, gamma, rows=rows, in_stride=in_stride, out_stride=out_stride, out=out)

    @property
    def n_public(self) -> int:
        """NbPublicVariables"""
        if self.vk is not None:
            return int(self.vk["n_public"])
        k = C.c_size_t(0)
        check(lib().zk_bn254_plonk_pk_info(self.handle, None, C.byref(k), None, None))
        return int(k.value)

    def quotient_batch(self, l, r, o, z, public, alpha, beta, gamma, *, rows: int | None = None, in_stride: int | None = None, pub_stride: int | None = None,
                       out_stride: int | None = None, out=None, status=None):
        """Round 3 of `rows` proofs against this key (zk_bn254_plonk_quotient_batch_dev; include/zkmi.h says the rest): from the blinded canonical l, r, o (n + 2
        coefficients), z (n + 3), the public inputs and alpha, beta, gamma of each row to the 3 (n + 2) coefficients of its quotient and a verdict per row
        (int32: 0, or 1 where the quotient is not a polynomial -- which fails neither the call nor the other rows).  Two forms, every shape / dtype / stride /
        count / overlap error raised before the library is called:
          host    l, r, o: (rows, n + 2, 4) uint64 arrays, z: (rows, n + 3, 4), public: (rows, n_public, 4), alpha, beta, gamma: (rows, 4)
                  -> (h, status), new arrays of (rows, 3 (n + 2), 4) uint64 and (rows,) int32
          device  device buffers / pointers; rows is required; row v of l, r, o, z at element v * in_stride (default n + 3), of the public inputs at v * pub_stride
                  (default n_public), of h at v * out_stride (default 3 (n + 2)) of `out`; `out` and `status` must overlap nothing else (made here when None)
                  -> (out, status)"""
        return quotient_batch(self, l, r, o, z, public, alpha, beta, gamma, rows=rows, in_stride=in_stride, pub_stride=pub_stride, out_stride=out_stride, out=out,
                              status=status)

    def linearize_batch(self, l, r, o, z, h, alpha, beta, gamma, zeta, *, rows: int | None = None, in_stride: int | None = None, h_stride: int | None = None,
                        out_stride: int | None = None, out=None):
        """Round 4 of `rows` proofs against this key (zk_bn254_plonk_linearize_batch_dev; include/zkmi.h says the rest): from the rows of round 3 -- the blinded
        canonical l, r, o (n + 2 coefficients), z (n + 3), the quotient h (3 (n + 2)) -- and alpha, beta, gamma, zeta of each row to the proof's eight values
        (foldedH, lin, l, r, o, s1, s2 at zeta, z at omega zeta), the quotient of z at omega zeta (n + 2), the linearised polynomial (n + 3) and the folded
        quotient (n + 2).  Two forms, every shape / dtype / stride / count / overlap error raised before the library is called:
          host    l, r, o: (rows, n + 2, 4) uint64 arrays, z: (rows, n + 3, 4), h: (rows, 3 (n + 2), 4), alpha, beta, gamma, zeta: (rows, 4)
                  -> (values (rows, 8, 4), zquot (rows, n + 2, 4), lin (rows, n + 3, 4), fh (rows, n + 2, 4)), new arrays
          device  device buffers / pointers; rows is required; row v of l, r, o, z at element v * in_stride (default n + 3), of h at v * h_stride (default
                  3 (n + 2)); out: the four buffers (values, zquot, lin, fh), values 8 elements per row and the others v * out_stride apart (default n + 3),
                  overlapping nothing (made here when None) -> out"""
        return linearize_batch(self, l, r, o, z, h, alpha, beta, gamma, zeta, rows=rows, in_stride=in_stride, h_stride=h_stride, out_stride=out_stride, out=out)

    def open_batch(self, fh, lin, l, r, o, zeta, kzg_gamma, *, rows: int | None = None, in_stride: int | None = None, out_stride: int | None = None, out=None):
        """Round 5's polynomial of `rows` proofs against this key (zk_bn254_plonk_open_batch_dev): kzg.BatchOpenSinglePoint's fold of (fh, lin, l, r, o, s1, s2)
        under the challenge kzg_gamma of each row, divided by X - zeta.  Two forms, errors raised before the library is called:
          host    fh, l, r, o: (rows, n + 2, 4) uint64 arrays, lin: (rows, n + 3, 4), zeta, kzg_gamma: (rows, 4) -> (q (rows, n + 2, 4), value (rows, 4))
          device  device buffers / pointers; rows is required; row v of the five polynomials at element v * in_stride (default n + 3); out: the two buffers
                  (q, value), row v of q at v * out_stride (default n + 2), overlapping nothing (made here when None) -> out"""
        return open_batch(self, fh, lin, l, r, o, zeta, kzg_gamma, rows=rows, in_stride=in_stride, out_stride=out_stride, out=out)

    def commit_rows(self, rows_data, *, from_values: bool = False, length: int | None = None, rows: int | None = None, row_stride: int | None = None, out=None,
                    compressed=False, points: bool = True):
        """The digests a round ends in, for the rows of the batch entries above (zk_bn254_plonk_commit_batch_dev): every row of a matrix of Montgomery images
        committed against this key's SRS -- coefficients: l, r, o, Z, the thirds of h, the opening quotients -- or, with from_values, against its Lagrange form
        (lagrange_srs() first): a row is then the n wire values followed by the two blinders b0, b1.  A (rows, length, 4) uint64 array, or device rows with
        length, rows and row_stride; bn254.rows_digests says what the two forms take and return."""
        return commit_rows(self, rows_data, from_values=from_values, length=length, rows=rows, row_stride=row_stride, out=out, compressed=compressed, points=points)

    def free(self):
        if self.handle.value:
            check(lib().zk_bn254_plonk_pk_free(self.handle))
            self.handle = C.c_uint64(0)


def _vk_dict(v: _lib.PlonkVK) -> dict:
    a = lambda x: np.array(list(x), dtype=np.uint64)
    return dict(size=int(v.size), n_public=int(v.n_public), size_inv=a(v.size_inv), generator=a(v.generator), coset_shift=a(v.coset_shift),
                s=a(v.s).reshape(3, 8), ql=a(v.ql), qr=a(v.qr), qm=a(v.qm), qo=a(v.qo), qk=a(v.qk))


def setup(circuit: Circuit, srs: ResidentBases) -> ProvingKey:
    """plonk.Setup: selectors and permutation polynomials in canonical form, their commitments (the verifying key), the cached
    Lagrange-coset forms.  `srs` = kzg SRS.G1 registered with ResidentBases (>= domain size + 3 points)."""
    ptr = (lambda b: b.ptr) if circuit.on_device else (lambda a: a.ctypes.data)
    c = _lib.PlonkCircuit(circuit.n_public, circuit.n_constraints, circuit.n_vars, *[ptr(v) for v in circuit.coeffs],
                          circuit.xa.ctypes.data, circuit.xb.ctypes.data, circuit.xc.ctypes.data, 1 if circuit.on_device else 0, 0)
    h, vk = C.c_uint64(0), _lib.PlonkVK()
    check(lib().zk_bn254_plonk_setup(C.byref(c), srs.handle, C.byref(h), C.byref(vk)))
    return ProvingKey(h.value, srs, _vk_dict(vk), circuit.n_vars)


def load_proving_key(log_n: int, n_public: int, n_vars: int, polys: dict, permutation, xa, xb, xc, vk: dict, srs: ResidentBases) -> ProvingKey:
    """gnark's own ProvingKey fields (as plonk.Setup / ReadFrom leave them): polys = canonical ql, qr, qm, qo, cqk, s1, s2, s3 and lqk."""
    keep = {k: np.ascontiguousarray(polys[k], dtype=np.uint64) for k in ("ql", "qr", "qm", "qo", "cqk", "lqk", "s1", "s2", "s3")}
    perm = np.ascontiguousarray(permutation, dtype=np.int64)
    w = [np.ascontiguousarray(v, dtype=np.uint32) for v in (xa, xb, xc)]
    vs = np.ascontiguousarray(vk["s"], dtype=np.uint64)
    vq = {k: np.ascontiguousarray(vk[k], dtype=np.uint64) for k in ("ql", "qr", "qm", "qo", "qk")}
    k = _lib.PlonkPK(log_n, n_public, int(w[0].shape[0]), n_vars, *[keep[x].ctypes.data for x in ("ql", "qr", "qm", "qo", "cqk", "lqk", "s1", "s2", "s3")],
                     perm.ctypes.data, w[0].ctypes.data, w[1].ctypes.data, w[2].ctypes.data, vs.ctypes.data, *[vq[x].ctypes.data for x in ("ql", "qr", "qm", "qo", "qk")])
    h = C.c_uint64(0)
    check(lib().zk_bn254_plonk_pk_load(C.byref(k), srs.handle, C.byref(h)))
    return ProvingKey(h.value, srs, vk, n_vars)


def read_proving_key(data, n_vars: int, xa, xb, xc, srs, is_hex: bool = False) -> ProvingKey:
    """plonk.ProvingKey.ReadFrom on gnark's bytes (or the hex text DeserializeProvingKey receives, helpers.go:49-60); the wire ids are the
    rebuilt spr's (plonk.go:54).  The vectors are decoded on the device straight into the resident key."""
    raw = data.encode("ascii") if isinstance(data, str) else bytes(data)
    w = [np.ascontiguousarray(v, dtype=np.uint32) for v in (xa, xb, xc)]
    h = C.c_uint64(0)
    rc = lib().zk_bn254_plonk_pk_read(C.c_char_p(raw), C.c_size_t(len(raw)), C.c_int(int(is_hex)), C.c_size_t(n_vars), C.c_size_t(int(w[0].shape[0])),
                                      w[0].ctypes.data_as(C.c_void_p), w[1].ctypes.data_as(C.c_void_p), w[2].ctypes.data_as(C.c_void_p), srs.handle, C.byref(h))
    if rc in (_lib.ZK_ERR_LEN, _lib.ZK_ERR_ARG):
        raise ValueError((lib().zk_last_error() or b"").decode())
    check(rc)
    return ProvingKey(h.value, srs, None, n_vars)


def prove(pk: ProvingKey, solution, blinders, challenges=None) -> bytes:
    """plonk.Prove after the solver -> Proof.WriteTo bytes (548).  solution: (n_vars, 4) Montgomery values of all variables (numpy) or a
    DeviceBuffer; blinders: (9, 4); challenges: None (Fiat-Shamir as upstream) or (5, 4) = gamma, beta, alpha, zeta, kzg gamma."""
    on_dev = isinstance(solution, _lib.DeviceBuffer)
    if on_dev:
        ptr, n = C.c_void_p(solution.ptr), pk.n_vars
    else:
        sol = np.ascontiguousarray(solution, dtype=np.uint64).reshape(-1, 4)
        ptr, n = vp(sol), sol.shape[0]
    bl = np.ascontiguousarray(blinders, dtype=np.uint64).reshape(9, 4)
    ch = None if challenges is None else np.ascontiguousarray(challenges, dtype=np.uint64).reshape(5, 4)
    out = (C.c_uint8 * PROOF_BYTES)()
    rc = lib().zk_bn254_plonk_prove(pk.handle, ptr, C.c_size_t(n), C.c_int(int(on_dev)), vp(bl), vp(ch) if ch is not None else None, out)
    if rc == _lib.ZK_ERR_LEN:
        raise ValueError((lib().zk_last_error() or b"").decode())
    check(rc)
    return bytes(out)


# ---- many witnesses against one key in one call, the proofs assembled on the device (zk_bn254_plonk_prove_batch; include/zkmi.h says the rest)
def _batch_rows(name, a, width):
    """a (rows, width, 4) uint64 array of Montgomery images, or ValueError"""
    a = np.ascontiguousarray(a, dtype=np.uint64)
    if a.ndim != 3 or a.shape[1:] != (width, 4):
        raise ValueError("%s has shape %s, not (rows, %d, 4)" % (name, a.shape, width))
    return a


def prove_batch(pk: ProvingKey, solutions, blinders, challenges=None, *, on_device: bool = False, chunk_rows: int = 0) -> list:
    """plonk.Prove for every row of `solutions` against one key in one device call -> a list of Proof.WriteTo bytes (548 each), None where the row's solution
    does not satisfy the circuit (which fails neither the call nor the other rows).  Row v is byte for byte prove(pk, solutions[v], blinders[v], challenges[v]).
    solutions: (rows, n_vars, 4) Montgomery values, public inputs first -- a numpy array, or with on_device a DeviceBuffer / device pointer of rows * n_vars
    contiguous elements; blinders: (rows, 9, 4); challenges: None (Fiat-Shamir as upstream) or (rows, 5, 4) = gamma, beta, alpha, zeta, kzg gamma of each row;
    chunk_rows: 0, or a cap on the rows per chunk (it never changes a byte).  Shapes are checked before the library is called."""
    bl = _batch_rows("blinders", blinders, 9)
    rows = bl.shape[0]
    ch = None if challenges is None else _batch_rows("challenges", challenges, 5)
    if ch is not None and ch.shape[0] != rows:
        raise ValueError("challenges has %d rows, blinders %d" % (ch.shape[0], rows))
    if int(chunk_rows) < 0:
        raise ValueError("chunk_rows must not be negative")
    if on_device:
        if not isinstance(solutions, _DEV):
            raise TypeError("with on_device, solutions is a device buffer or a device pointer")
        if isinstance(solutions, _lib.DeviceBuffer) and rows * pk.n_vars * 32 > solutions.nbytes:
            raise ValueError("solutions: %d rows of %d variables do not fit the device buffer (%d bytes)" % (rows, pk.n_vars, solutions.nbytes))
        ptr = C.c_void_p(_ptr(solutions))
    else:
        sol = _batch_rows("solutions", solutions, pk.n_vars)
        if sol.shape[0] != rows:
            raise ValueError("solutions has %d rows, blinders %d" % (sol.shape[0], rows))
        ptr = vp(sol)
    if rows == 0:
        return []
    out = np.zeros((rows, PROOF_BYTES), dtype=np.uint8)
    status = np.zeros(rows, dtype=np.int32)
    rc = lib().zk_bn254_plonk_prove_batch(pk.handle, ptr, C.c_size_t(pk.n_vars), C.c_size_t(pk.n_vars), C.c_size_t(rows), C.c_int(int(bool(on_device))), vp(bl),
                                          vp(ch) if ch is not None else None, C.c_size_t(int(chunk_rows)), vp(out), vp(status))
    if rc == _lib.ZK_ERR_LEN:
        raise ValueError((lib().zk_last_error() or b"").decode())
    check(rc)
    return [None if status[v] else out[v].tobytes() for v in range(rows)]


def prove_batch_info(pk: ProvingKey) -> dict:
    """zk_bn254_plonk_prove_batch_info: {"chunk_rows": rows per chunk of prove_batch with device-resident solutions, "commits_batched": whether the row MSM's
    batched path serves the key's SRS, "lin_by_linearity": whether the linearised polynomial's digest is taken from the key's digests instead of an MSM}"""
    chunk, batched, lin = C.c_size_t(0), C.c_int(0), C.c_int(0)
    check(lib().zk_bn254_plonk_prove_batch_info(pk.handle, C.byref(chunk), C.byref(batched), C.byref(lin)))
    return {"chunk_rows": int(chunk.value), "commits_batched": bool(batched.value), "lin_by_linearity": int(lin.value)}


_STAGE_POINTS = (3, 0, 1, 3, 5)


def challenges_rows(pk: ProvingKey, stage: int, *, public=None, points=None, prev=None, values=None):
    """One challenge of the prover's transcript for every row, on the device (zk_bn254_plonk_challenges_batch_dev) -> (challenges (rows, 4) uint64 Montgomery,
    raw (rows, 32) uint8: the digests the next stage binds as `prev`).  stage 0 gamma: public (rows, n_public, 4), points (rows, 3, 8) = [L], [R], [O] as affine
    Montgomery images, (0, 0) = infinity; 1 beta: prev; 2 alpha: prev, points (rows, 1, 8) = [Z]; 3 zeta: prev, points (rows, 3, 8) = [H0], [H1], [H2];
    4 kzg's folding gamma: prev = zeta (rows, 4), points (rows, 5, 8) = [foldedH], [lin], [L], [R], [O], values (rows, 8, 4) of which the first seven are bound.
    Every shape is checked before the library is called."""
    stage = int(stage)
    if stage not in range(5):
        raise ValueError("stage %d is not one of the five challenges 0 .. 4" % stage)
    arrays, rows = [], None

    def take(name, a, dtype, shape):
        nonlocal rows
        if a is None:
            raise ValueError("stage %d needs %s" % (stage, name))
        a = np.ascontiguousarray(a, dtype=dtype)
        if a.ndim != len(shape) + 1 or a.shape[1:] != shape:
            raise ValueError("%s has shape %s, not (rows,%s)" % (name, a.shape, "".join(" %d," % k for k in shape)))
        if rows is not None and a.shape[0] != rows:
            raise ValueError("%s has %d rows, not %d" % (name, a.shape[0], rows))
        rows = a.shape[0]
        arrays.append(a)
        return a

    npub = pk.n_public
    pub = take("public", public, np.uint64, (npub, 4)) if stage == 0 and npub else None  # a key without public inputs binds none
    pts = take("points", points, np.uint64, (_STAGE_POINTS[stage], 8)) if stage != 1 else None
    prv = None
    if stage in (1, 2, 3):
        prv = take("prev", prev, np.uint8, (32,))
    elif stage == 4:
        prv = take("prev", prev, np.uint64, (4,))
    val = take("values", values, np.uint64, (8, 4)) if stage == 4 else None
    if rows == 0:
        return np.zeros((0, 4), np.uint64), np.zeros((0, 32), np.uint8)
    bufs = {k: _lib.DeviceBuffer.from_numpy(a) for k, a in (("pub", pub), ("pts", pts), ("prev", prv), ("val", val)) if a is not None}
    out = _lib.DeviceBuffer(2 * rows * 32)
    p = lambda k: C.c_void_p(bufs[k].ptr if k in bufs else 0)
    try:
        check(lib().zk_bn254_plonk_challenges_batch_dev(pk.handle, C.c_int(stage), C.c_size_t(rows), p("pub"), C.c_size_t(npub), p("pts"), p("prev"), p("val"),
                                                        C.c_void_p(out.ptr), C.c_void_p(0)))
        both = out.to_numpy(np.uint8, (2 * rows, 32))
        return np.ascontiguousarray(both[:rows]).view(np.uint64).reshape(rows, 4), np.ascontiguousarray(both[rows:])
    finally:
        out.free()
        for b in bufs.values():
            b.free()


# ---- round 2 for many witnesses: iop.BuildRatioCopyConstraint with the row as a grid dimension (zk_bn254_iop_ratio_copy_batch[_dev], zk_bn254_plonk_ratio_batch_dev)
_DEV = (int, _lib.DeviceBuffer)


def _ptr(a) -> int:
    return a if isinstance(a, int) else a.ptr


def _host_rows(name, a, n=None):
    """a C-contiguous (rows, n, 4) uint64 array, or TypeError / ValueError"""
    if not (isinstance(a, np.ndarray) and a.dtype == np.uint64 and a.flags["C_CONTIGUOUS"]):
        raise TypeError("%s must be a C-contiguous uint64 numpy array (or a device buffer)" % name)
    if a.ndim != 3 or a.shape[2] != 4 or (n is not None and a.shape[1] != n):
        raise ValueError("%s has shape %s, not (rows, %s, 4)" % (name, a.shape, "n" if n is None else n))
    return a


def _host_challenges(name, a, rows):
    if not (isinstance(a, np.ndarray) and a.dtype == np.uint64 and a.flags["C_CONTIGUOUS"]):
        raise TypeError("%s must be a C-contiguous uint64 numpy array" % name)
    if a.shape != (rows, 4):
        raise ValueError("%s has shape %s, not (%d, 4): one challenge per row" % (name, a.shape, rows))
    return a


def _power_of_two(n):
    n = int(n)
    if n < 1 or n & (n - 1) or n > 1 << 28:
        raise ValueError("the domain size %d is not a power of two up to 2^28" % n)
    return n


def _host_perm(perm, n):
    if not isinstance(perm, np.ndarray) or perm.dtype.kind not in "iu":
        raise TypeError("perm must be an integer numpy array of 3 n positions")
    if perm.shape != (3 * n,):
        raise ValueError("perm has shape %s, not (%d,)" % (perm.shape, 3 * n))
    if perm.size and (int(perm.min()) < 0 or int(perm.max()) >= 3 * n):
        raise ValueError("perm holds a position outside [0, %d)" % (3 * n))
    return np.ascontiguousarray(perm, dtype=np.uint32)


def _dev_geometry(bufs, n, rows, in_stride, out_stride, out, extra=(), out_width=None):
    """the checks of a call on device rows, before the library: bufs = (name, buffer) of the rows read, n elements each (the smallest in_stride); extra = (name,
    buffer, bytes) of what else is read; out_width: elements per row of `out` (the smallest out_stride) where that is not n"""
    if rows is None:
        raise ValueError("rows is required with device-resident data")
    rows = int(rows)
    wide = n if out_width is None else out_width
    in_stride, out_stride = int(n if in_stride is None else in_stride), int(wide if out_stride is None else out_stride)
    if rows < 0:
        raise ValueError("rows must not be negative")
    if out_width is None and (in_stride < n or out_stride < n):
        raise ValueError("in_stride = %d / out_stride = %d is below the domain size %d" % (in_stride, out_stride, n))
    if in_stride < n or out_stride < wide:
        raise ValueError("in_stride = %d / out_stride = %d is below the %d / %d elements of a row" % (in_stride, out_stride, n, wide))
    span = lambda stride, width=n: ((rows - 1) * stride + width) * 32 if rows else 0
    reads = [(name, b, span(in_stride)) for name, b in bufs] + list(extra)
    for name, b, nbytes in reads + ([("out", out, span(out_stride, wide))] if out is not None else []):
        if not isinstance(b, _DEV):
            raise TypeError("%s must be a device buffer or a device pointer, like l" % name)
        if isinstance(b, _lib.DeviceBuffer) and nbytes > b.nbytes:
            raise ValueError("%s: %d bytes do not fit the device buffer (%d bytes)" % (name, nbytes, b.nbytes))
    if out is not None:
        lo, hi = _ptr(out), _ptr(out) + span(out_stride, wide)
        for name, b, nbytes in reads:
            if nbytes and _ptr(b) < hi and lo < _ptr(b) + nbytes:
                raise ValueError("out overlaps %s" % name)
    return rows, in_stride, out_stride


def permutation_sigma(perm, n: int | None = None):
    """3 n positions (gnark's pk.Permutation, L | R | O) -> a DeviceBuffer of the 3 n elements S1 | S2 | S3 in Lagrange form (zk_bn254_iop_sigma_dev): what
    ratio_copy_batch takes as `perm` next to device rows.  perm: an integer numpy array, or a device buffer / pointer of uint32 together with n."""
    if isinstance(perm, _DEV):
        if n is None:
            raise ValueError("n is required with a device-resident permutation")
        n = _power_of_two(n)
        if isinstance(perm, _lib.DeviceBuffer) and 3 * n * 4 > perm.nbytes:
            raise ValueError("3 * %d positions do not fit the device buffer (%d bytes)" % (n, perm.nbytes))
        src, keep = perm, None
    else:
        if not isinstance(perm, np.ndarray) or perm.ndim != 1 or perm.size % 3:
            raise ValueError("perm must be a flat integer numpy array of 3 n positions")
        n = _power_of_two(perm.size // 3)
        src = keep = _lib.DeviceBuffer.from_numpy(_host_perm(perm, n))
    out = _lib.DeviceBuffer(3 * n * 32)
    try:
        rc = lib().zk_bn254_iop_sigma_dev(C.c_void_p(_ptr(src)), C.c_uint32(n.bit_length() - 1), C.c_void_p(out.ptr), C.c_void_p(0))
        if rc == _lib.ZK_ERR_ARG:
            raise ValueError((lib().zk_last_error() or b"").decode())
        check(rc)
    except Exception:
        out.free()
        raise
    finally:
        if keep is not None:
            keep.free()
    return out


def ratio_copy_batch(l, r, o, perm, beta, gamma, *, rows: int | None = None, in_stride: int | None = None, out_stride: int | None = None, n: int | None = None, out=None):
    """iop.BuildRatioCopyConstraint for `rows` witnesses of one domain and one permutation, each row with its own beta and gamma: Z per row, Lagrange form,
    regular order (include/zkmi.h says the rest).  Two forms, every shape / dtype / stride / count error raised before the library is called:
      host    l, r, o: (rows, n, 4) uint64 arrays; perm: 3 n integer positions; beta, gamma: (rows, 4) -> a new (rows, n, 4) array
      device  l, r, o, beta, gamma: device buffers / pointers; perm: S1 | S2 | S3 as permutation_sigma leaves it; rows and n are required, row v of the wires at
              element v * in_stride, of Z at v * out_stride (both default n) of `out`, a device buffer that must not overlap an input (made here when None) -> out"""
    if isinstance(l, _DEV):
        if n is None:
            raise ValueError("n is required with device-resident data")
        n = _power_of_two(n)
        cnt = 0 if rows is None else max(int(rows), 0)
        rows, in_stride, out_stride = _dev_geometry((("l", l), ("r", r), ("o", o)), n, rows, in_stride, out_stride, out,
                                                    (("perm", perm, 3 * n * 32), ("beta", beta, cnt * 32), ("gamma", gamma, cnt * 32)))
        if out is None:
            out = _lib.DeviceBuffer(max(((rows - 1) * out_stride + n) * 32 if rows else 0, 32))
        check(lib().zk_bn254_iop_ratio_copy_batch_dev(C.c_void_p(_ptr(l)), C.c_void_p(_ptr(r)), C.c_void_p(_ptr(o)), C.c_size_t(in_stride), C.c_uint32(n.bit_length() - 1),
                                                      C.c_size_t(rows), C.c_void_p(_ptr(perm)), C.c_void_p(_ptr(beta)), C.c_void_p(_ptr(gamma)), C.c_void_p(_ptr(out)),
                                                      C.c_size_t(out_stride), C.c_void_p(0)))
        return out
    l = _host_rows("l", l)
    cnt, size = l.shape[0], _power_of_two(l.shape[1])
    if n is not None and int(n) != size:
        raise ValueError("n = %d != %d elements per row" % (n, size))
    r, o = _host_rows("r", r, size), _host_rows("o", o, size)
    if r.shape[0] != cnt or o.shape[0] != cnt:
        raise ValueError("l, r and o have %d, %d and %d rows" % (cnt, r.shape[0], o.shape[0]))
    if rows is not None and int(rows) != cnt:
        raise ValueError("rows = %d != %d rows of the arrays" % (rows, cnt))
    for name, v in (("in_stride", in_stride), ("out_stride", out_stride)):
        if v is not None and int(v) != size:
            raise ValueError("the rows of a host array are contiguous: %s must be %d" % (name, size))
    if out is not None:
        raise ValueError("out belongs to the device form: the host form returns a new array")
    p = _host_perm(perm, size)
    beta, gamma = _host_challenges("beta", beta, cnt), _host_challenges("gamma", gamma, cnt)
    z = np.zeros((cnt, size, 4), dtype=np.uint64)
    check(lib().zk_bn254_iop_ratio_copy_batch(vp(l), vp(r), vp(o), C.c_uint32(size.bit_length() - 1), C.c_size_t(cnt), vp(p), vp(beta), vp(gamma), vp(z)))
    return z


def _pk_ratio_batch(self, l, r, o, beta, gamma, *, rows: int | None = None, in_stride: int | None = None, out_stride: int | None = None, out=None):
    """ProvingKey.ratio_batch"""
    n = self.domain_size
    bufs = []
    if isinstance(l, _DEV):
        cnt = 0 if rows is None else max(int(rows), 0)
        rows, in_stride, out_stride = _dev_geometry((("l", l), ("r", r), ("o", o)), n, rows, in_stride, out_stride, out, (("beta", beta, cnt * 32), ("gamma", gamma, cnt * 32)))
        if out is None:
            out = _lib.DeviceBuffer(max(((rows - 1) * out_stride + n) * 32 if rows else 0, 32))
        host = None
    else:
        l, r, o = _host_rows("l", l, n), _host_rows("r", r, n), _host_rows("o", o, n)
        cnt = l.shape[0]
        if r.shape[0] != cnt or o.shape[0] != cnt:
            raise ValueError("l, r and o have %d, %d and %d rows" % (cnt, r.shape[0], o.shape[0]))
        if rows is not None and int(rows) != cnt:
            raise ValueError("rows = %d != %d rows of the arrays" % (rows, cnt))
        for name, v in (("in_stride", in_stride), ("out_stride", out_stride)):
            if v is not None and int(v) != n:
                raise ValueError("the rows of a host array are contiguous: %s must be %d" % (name, n))
        if out is not None:
            raise ValueError("out belongs to the device form: the host form returns a new array")
        beta, gamma = _host_challenges("beta", beta, cnt), _host_challenges("gamma", gamma, cnt)
        host = np.zeros((cnt, n, 4), dtype=np.uint64)
        if cnt == 0:
            return host
        rows, in_stride, out_stride = cnt, n, n
        bufs = [_lib.DeviceBuffer.from_numpy(v) for v in (l, r, o, beta, gamma)]
        l, r, o, beta, gamma = bufs
        out = _lib.DeviceBuffer(host.nbytes)
        bufs.append(out)
    try:
        check(lib().zk_bn254_plonk_ratio_batch_dev(self.handle, C.c_void_p(_ptr(l)), C.c_void_p(_ptr(r)), C.c_void_p(_ptr(o)), C.c_size_t(in_stride), C.c_size_t(rows),
                                                   C.c_void_p(_ptr(beta)), C.c_void_p(_ptr(gamma)), C.c_void_p(_ptr(out)), C.c_size_t(out_stride), C.c_void_p(0)))
        return out if host is None else out.to_numpy(np.uint64, host.shape)
    finally:
        for b in bufs:
            b.free()



# ---- round 3 for many witnesses: the quotient with the row as a grid dimension (zk_bn254_plonk_quotient_batch_dev)
def _host_rows_of(name, a, widths):
    """_host_rows for a row of one of `widths` elements"""
    a = _host_rows(name, a)
    if a.shape[1] not in widths:
        raise ValueError("%s has shape %s, not (rows, %s, 4)" % (name, a.shape, " or ".join(str(w) for w in widths)))
    return a


def quotient_batch(pk: ProvingKey, l, r, o, z, public, alpha, beta, gamma, *, rows: int | None = None, in_stride: int | None = None, pub_stride: int | None = None,
                   out_stride: int | None = None, out=None, status=None):
    """ProvingKey.quotient_batch"""
    n, npub = pk.domain_size, pk.n_public
    keep = 3 * (n + 2)
    bufs = []
    if isinstance(l, _DEV):
        cnt = 0 if rows is None else max(int(rows), 0)
        pub_stride = int(npub if pub_stride is None else pub_stride)
        if pub_stride < npub:
            raise ValueError("pub_stride = %d is below the %d public inputs" % (pub_stride, npub))
        if npub == 0 and public is None:
            public = 0
        extra = [("z", z, ((cnt - 1) * int(n + 3 if in_stride is None else in_stride) + n + 3) * 32 if cnt else 0),
                 ("public", public, ((cnt - 1) * pub_stride + npub) * 32 if cnt and npub else 0),
                 ("alpha", alpha, cnt * 32), ("beta", beta, cnt * 32), ("gamma", gamma, cnt * 32)]
        if in_stride is not None and int(in_stride) < n + 3:
            raise ValueError("in_stride = %d is below n + 3 = %d" % (in_stride, n + 3))
        rows, in_stride, out_stride = _dev_geometry((("l", l), ("r", r), ("o", o)), n + 2, rows, n + 3 if in_stride is None else in_stride, out_stride, out, extra,
                                                    out_width=keep)
        if status is not None:
            if not isinstance(status, _DEV):
                raise TypeError("status must be a device buffer or a device pointer, like l")
            if isinstance(status, _lib.DeviceBuffer) and rows * 4 > status.nbytes:
                raise ValueError("status: %d bytes do not fit the device buffer (%d bytes)" % (rows * 4, status.nbytes))
            lo, hi = _ptr(status), _ptr(status) + rows * 4
            span = ((rows - 1) * in_stride + n + 2) * 32 if rows else 0
            for name, b, nbytes in [(k, v, span) for k, v in (("l", l), ("r", r), ("o", o))] + extra + \
                                   ([("out", out, ((rows - 1) * out_stride + keep) * 32 if rows else 0)] if out is not None else []):
                if rows and nbytes and _ptr(b) < hi and lo < _ptr(b) + nbytes:
                    raise ValueError("status overlaps %s" % name)
        made = []
        if out is None:
            out = _lib.DeviceBuffer(max(((rows - 1) * out_stride + keep) * 32 if rows else 0, 32))
            made.append(out)
        if status is None:
            status = _lib.DeviceBuffer(max(rows * 4, 32))
            made.append(status)
        host = None
    else:
        l, r, o = (_host_rows_of(k, v, (n + 2, n + 3)) for k, v in (("l", l), ("r", r), ("o", o)))
        z = _host_rows_of("z", z, (n + 3,))
        cnt = l.shape[0]
        if not (r.shape[0] == o.shape[0] == z.shape[0] == cnt):
            raise ValueError("l, r, o and z have %d, %d, %d and %d rows" % (cnt, r.shape[0], o.shape[0], z.shape[0]))
        if rows is not None and int(rows) != cnt:
            raise ValueError("rows = %d != %d rows of the arrays" % (rows, cnt))
        if not (isinstance(public, np.ndarray) and public.dtype == np.uint64 and public.flags["C_CONTIGUOUS"]):
            raise TypeError("public must be a C-contiguous uint64 numpy array")
        if public.shape != (cnt, npub, 4):
            raise ValueError("public has shape %s, not (%d, %d, 4)" % (public.shape, cnt, npub))
        for name, v, want in (("in_stride", in_stride, n + 3), ("pub_stride", pub_stride, npub), ("out_stride", out_stride, keep)):
            if v is not None and int(v) != want:
                raise ValueError("the rows of a host array are contiguous: %s must be %d" % (name, want))
        if out is not None or status is not None:
            raise ValueError("out and status belong to the device form: the host form returns new arrays")
        alpha, beta, gamma = _host_challenges("alpha", alpha, cnt), _host_challenges("beta", beta, cnt), _host_challenges("gamma", gamma, cnt)
        host = np.zeros((cnt, keep, 4), dtype=np.uint64)
        if cnt == 0:
            return host, np.zeros((0,), dtype=np.int32)
        rows, in_stride, pub_stride, out_stride = cnt, n + 3, npub, keep

        def padded(a):
            if a.shape[1] == n + 3:
                return a
            w = np.zeros((cnt, n + 3, 4), dtype=np.uint64)
            w[:, :n + 2] = a
            return w
        bufs = [_lib.DeviceBuffer.from_numpy(v) for v in (padded(l), padded(r), padded(o), z, public, alpha, beta, gamma)]
        l, r, o, z, public, alpha, beta, gamma = bufs
        out, status = _lib.DeviceBuffer(host.nbytes), _lib.DeviceBuffer(max(cnt * 4, 32))
        bufs += [out, status]
        made = []
    try:
        p = lambda b: C.c_void_p(_ptr(b))
        check(lib().zk_bn254_plonk_quotient_batch_dev(pk.handle, p(l), p(r), p(o), p(z), C.c_size_t(in_stride), p(public), C.c_size_t(pub_stride), C.c_size_t(rows),
                                                      p(alpha), p(beta), p(gamma), p(out), C.c_size_t(out_stride), p(status), C.c_void_p(0)))
        if host is None:
            return out, status
        return out.to_numpy(np.uint64, host.shape), status.to_numpy(np.int32, (rows,))
    except Exception:
        for b in made:
            b.free()
        raise
    finally:
        for b in bufs:
            b.free()


# ---- rounds 4 and 5 for many witnesses: the openings with the row as a grid dimension (zk_bn254_fr_poly_open_rows_dev, zk_bn254_plonk_linearize_batch_dev,
# zk_bn254_plonk_open_batch_dev)
def _dev_spans(rows, reads, writes, same=()):
    """the checks of a call on device rows, before the library: reads / writes = (name, buffer, stride, width) in elements (row v at v * stride, width elements).
    Every buffer is a device buffer or pointer and holds its rows; a write overlaps no read and no other write, but for the pairs of names in `same`."""
    span = lambda stride, width: ((rows - 1) * stride + width) * 32 if rows and width else 0
    for name, b, stride, width in list(reads) + list(writes):
        if not isinstance(b, _DEV):
            raise TypeError("%s must be a device buffer or a device pointer" % name)
        if stride < width:
            raise ValueError("%s: a stride of %d is below the %d elements of a row" % (name, stride, width))
        if isinstance(b, _lib.DeviceBuffer) and span(stride, width) > b.nbytes:
            raise ValueError("%s: %d bytes do not fit the device buffer (%d bytes)" % (name, span(stride, width), b.nbytes))
    for k, (name, b, stride, width) in enumerate(writes):
        lo, hi = _ptr(b), _ptr(b) + span(stride, width)
        for other, c, s2, w2 in list(reads) + list(writes[k + 1:]):
            if (name, other) not in same and lo < hi and span(s2, w2) and _ptr(c) < hi and lo < _ptr(c) + span(s2, w2):
                raise ValueError("%s overlaps %s" % (name, other))


def _rows_count(rows):
    if rows is None:
        raise ValueError("rows is required with device-resident data")
    if int(rows) < 0:
        raise ValueError("rows must not be negative")
    return int(rows)


def _host_strides(given):
    for name, v, want in given:
        if v is not None and int(v) != want:
            raise ValueError("the rows of a host array are contiguous: %s must be %d" % (name, want))


def _padded(a, width):
    if a.shape[1] == width:
        return a
    w = np.zeros((a.shape[0], width, 4), dtype=np.uint64)
    w[:, :a.shape[1]] = a
    return w


def _run(call, bufs, made, result):
    """call() into the library; the buffers of `bufs` are freed afterwards, those of `made` only if it fails"""
    try:
        check(call())
        return result()
    except Exception:
        for b in made:
            b.free()
        raise
    finally:
        for b in bufs:
            b.free()


def poly_open_rows(f, points, *, length: int | None = None, rows: int | None = None, in_stride: int | None = None, q_stride: int | None = None, divide: bool = True,
                   out=None, values=None):
    """Rows of polynomials, each opened at its own point (zk_bn254_fr_poly_open_rows_dev): values[v] = f_v(points[v]) and, with divide, the length - 1 coefficients
    of (f_v - f_v(a_v)) / (X - a_v) (kzg.dividePolyByXminusA).  Every shape / dtype / stride / count / overlap error is raised before the library is called.
      host    f: (rows, length, 4) uint64, points: (rows, 4) -> (values (rows, 4), q (rows, length - 1, 4) or None without divide)
      device  device buffers / pointers; rows and length are required; row v of f at element v * in_stride (default length); with divide, q goes to `out` at
              v * q_stride: a buffer that overlaps nothing else (default stride length - 1; made here when None), or f itself with q_stride = in_stride (in
              place: element length - 1 of each row stays); `values` (rows elements) is made here when None -> (values, out or None)"""
    if isinstance(f, _DEV):
        rows = _rows_count(rows)
        if length is None or int(length) < 1:
            raise ValueError("length (>= 1 coefficients per row) is required with device-resident data")
        length = int(length)
        in_stride = int(length if in_stride is None else in_stride)
        in_place = divide and out is not None and isinstance(out, _DEV) and _ptr(out) == _ptr(f)
        q_stride = int((in_stride if in_place else length - 1) if q_stride is None else q_stride)
        if not divide and out is not None:
            raise ValueError("out takes the quotients: there are none without divide")
        if in_place and q_stride != in_stride:
            raise ValueError("in place the quotient's stride is in_stride = %d, not %d" % (in_stride, q_stride))
        reads = [("f", f, in_stride, length), ("points", points, 1, 1)]
        writes = ([("out", out, q_stride, length - 1)] if out is not None else []) + ([("values", values, 1, 1)] if values is not None else [])
        _dev_spans(rows, reads, writes, same={("out", "f")} if in_place else ())
        made = []
        if divide and out is None:
            out = _lib.DeviceBuffer(max(((rows - 1) * q_stride + length - 1) * 32 if rows else 0, 32))
            made.append(out)
        if values is None:
            values = _lib.DeviceBuffer(max(rows * 32, 32))
            made.append(values)
        if rows == 0:
            return values, out
        return _run(lambda: lib().zk_bn254_fr_poly_open_rows_dev(C.c_void_p(_ptr(f)), C.c_size_t(in_stride), C.c_size_t(length), C.c_size_t(rows), C.c_void_p(_ptr(points)),
                                                                 C.c_void_p(_ptr(out) if divide else 0), C.c_size_t(q_stride), C.c_void_p(_ptr(values)), C.c_void_p(0)),
                    [], made, lambda: (values, out))
    f = _host_rows("f", f)
    cnt, width = f.shape[0], f.shape[1]
    if width < 1:
        raise ValueError("a polynomial has at least one coefficient")
    if rows is not None and int(rows) != cnt:
        raise ValueError("rows = %d != %d rows of the array" % (rows, cnt))
    if length is not None and int(length) != width:
        raise ValueError("length = %d != the %d coefficients of a row" % (length, width))
    _host_strides((("in_stride", in_stride, width), ("q_stride", q_stride, width - 1)))
    if out is not None or values is not None:
        raise ValueError("out and values belong to the device form: the host form returns new arrays")
    points = _host_challenges("points", points, cnt)
    if cnt == 0:
        return np.zeros((0, 4), np.uint64), (np.zeros((0, width - 1, 4), np.uint64) if divide else None)
    bufs = [_lib.DeviceBuffer.from_numpy(f), _lib.DeviceBuffer.from_numpy(points), _lib.DeviceBuffer(cnt * 32), _lib.DeviceBuffer(max(cnt * (width - 1) * 32, 32))]
    df, dp, dv, dq = bufs
    return _run(lambda: lib().zk_bn254_fr_poly_open_rows_dev(C.c_void_p(df.ptr), C.c_size_t(width), C.c_size_t(width), C.c_size_t(cnt), C.c_void_p(dp.ptr),
                                                             C.c_void_p(dq.ptr if divide else 0), C.c_size_t(width - 1), C.c_void_p(dv.ptr), C.c_void_p(0)),
                bufs, [], lambda: (dv.to_numpy(np.uint64, (cnt, 4)), dq.to_numpy(np.uint64, (cnt, width - 1, 4)) if divide else None))


def _same_rows(named):
    cnt = named[0][1].shape[0]
    if any(a.shape[0] != cnt for _, a in named):
        raise ValueError("%s have %s rows" % (", ".join(k for k, _ in named), ", ".join(str(a.shape[0]) for _, a in named)))
    return cnt


def linearize_batch(pk: ProvingKey, l, r, o, z, h, alpha, beta, gamma, zeta, *, rows: int | None = None, in_stride: int | None = None, h_stride: int | None = None,
                    out_stride: int | None = None, out=None):
    """ProvingKey.linearize_batch"""
    n = pk.domain_size
    keep = 3 * (n + 2)
    if isinstance(l, _DEV):
        rows = _rows_count(rows)
        in_stride, h_stride, out_stride = int(n + 3 if in_stride is None else in_stride), int(keep if h_stride is None else h_stride), int(n + 3 if out_stride is None else out_stride)
        if in_stride < n + 3 or h_stride < keep or out_stride < n + 3:
            raise ValueError("in_stride = %d / h_stride = %d / out_stride = %d is below n + 3 = %d / 3 (n + 2) = %d / n + 3" % (in_stride, h_stride, out_stride, n + 3, keep))
        if out is not None and not (isinstance(out, (tuple, list)) and len(out) == 4):
            raise TypeError("out is the four device buffers (values, zquot, lin, fh)")
        reads = [("l", l, in_stride, n + 2), ("r", r, in_stride, n + 2), ("o", o, in_stride, n + 2), ("z", z, in_stride, n + 3), ("h", h, h_stride, keep),
                 ("alpha", alpha, 1, 1), ("beta", beta, 1, 1), ("gamma", gamma, 1, 1), ("zeta", zeta, 1, 1)]
        shapes = (("values", 8, 8), ("zquot", out_stride, n + 2), ("lin", out_stride, n + 3), ("fh", out_stride, n + 2))
        _dev_spans(rows, reads, [(k, b, s, w) for (k, s, w), b in zip(shapes, out)] if out is not None else [])
        made = []
        if out is None:
            out = made = [_lib.DeviceBuffer(max(((rows - 1) * s + w) * 32 if rows else 0, 32)) for _, s, w in shapes]
        out = tuple(out)
        if rows == 0:
            return out
        p = lambda b: C.c_void_p(_ptr(b))
        return _run(lambda: lib().zk_bn254_plonk_linearize_batch_dev(pk.handle, p(l), p(r), p(o), p(z), C.c_size_t(in_stride), p(h), C.c_size_t(h_stride), C.c_size_t(rows),
                                                                     p(alpha), p(beta), p(gamma), p(zeta), p(out[0]), p(out[1]), p(out[2]), p(out[3]),
                                                                     C.c_size_t(out_stride), C.c_void_p(0)), [], made, lambda: out)
    l, r, o = (_host_rows_of(k, v, (n + 2, n + 3)) for k, v in (("l", l), ("r", r), ("o", o)))
    z, h = _host_rows_of("z", z, (n + 3,)), _host_rows_of("h", h, (keep,))
    cnt = _same_rows((("l", l), ("r", r), ("o", o), ("z", z), ("h", h)))
    if rows is not None and int(rows) != cnt:
        raise ValueError("rows = %d != %d rows of the arrays" % (rows, cnt))
    _host_strides((("in_stride", in_stride, n + 3), ("h_stride", h_stride, keep), ("out_stride", out_stride, n + 3)))
    if out is not None:
        raise ValueError("out belongs to the device form: the host form returns new arrays")
    ch = [_host_challenges(k, v, cnt) for k, v in (("alpha", alpha), ("beta", beta), ("gamma", gamma), ("zeta", zeta))]
    shapes = ((cnt, 8, 4), (cnt, n + 2, 4), (cnt, n + 3, 4), (cnt, n + 2, 4))
    if cnt == 0:
        return tuple(np.zeros(s, np.uint64) for s in shapes)
    bufs = [_lib.DeviceBuffer.from_numpy(v) for v in [_padded(l, n + 3), _padded(r, n + 3), _padded(o, n + 3), z, h] + ch]
    outs = [_lib.DeviceBuffer(cnt * 8 * 32)] + [_lib.DeviceBuffer(cnt * (n + 3) * 32) for _ in range(3)]
    bufs += outs
    p = lambda b: C.c_void_p(b.ptr)
    return _run(lambda: lib().zk_bn254_plonk_linearize_batch_dev(pk.handle, *(p(b) for b in bufs[:4]), C.c_size_t(n + 3), p(bufs[4]), C.c_size_t(keep), C.c_size_t(cnt),
                                                                 *(p(b) for b in bufs[5:9]), *(p(b) for b in outs), C.c_size_t(n + 3), C.c_void_p(0)),
                bufs, [], lambda: (outs[0].to_numpy(np.uint64, shapes[0]),) + tuple(np.ascontiguousarray(b.to_numpy(np.uint64, (cnt, n + 3, 4))[:, :s[1]])
                                                                                     for b, s in zip(outs[1:], shapes[1:])))


def open_batch(pk: ProvingKey, fh, lin, l, r, o, zeta, kzg_gamma, *, rows: int | None = None, in_stride: int | None = None, out_stride: int | None = None, out=None):
    """ProvingKey.open_batch"""
    n = pk.domain_size
    if isinstance(fh, _DEV):
        rows = _rows_count(rows)
        in_stride, out_stride = int(n + 3 if in_stride is None else in_stride), int(n + 2 if out_stride is None else out_stride)
        if in_stride < n + 3 or out_stride < n + 2:
            raise ValueError("in_stride = %d / out_stride = %d is below n + 3 = %d / n + 2 = %d" % (in_stride, out_stride, n + 3, n + 2))
        if out is not None and not (isinstance(out, (tuple, list)) and len(out) == 2):
            raise TypeError("out is the two device buffers (q, value)")
        reads = [("fh", fh, in_stride, n + 2), ("lin", lin, in_stride, n + 3), ("l", l, in_stride, n + 2), ("r", r, in_stride, n + 2), ("o", o, in_stride, n + 2),
                 ("zeta", zeta, 1, 1), ("kzg_gamma", kzg_gamma, 1, 1)]
        shapes = (("q", out_stride, n + 2), ("value", 1, 1))
        _dev_spans(rows, reads, [(k, b, s, w) for (k, s, w), b in zip(shapes, out)] if out is not None else [])
        made = []
        if out is None:
            out = made = [_lib.DeviceBuffer(max(((rows - 1) * s + w) * 32 if rows else 0, 32)) for _, s, w in shapes]
        out = tuple(out)
        if rows == 0:
            return out
        p = lambda b: C.c_void_p(_ptr(b))
        return _run(lambda: lib().zk_bn254_plonk_open_batch_dev(pk.handle, p(fh), p(lin), p(l), p(r), p(o), C.c_size_t(in_stride), C.c_size_t(rows), p(zeta), p(kzg_gamma),
                                                                p(out[0]), C.c_size_t(out_stride), p(out[1]), C.c_void_p(0)), [], made, lambda: out)
    fh, l, r, o = (_host_rows_of(k, v, (n + 2, n + 3)) for k, v in (("fh", fh), ("l", l), ("r", r), ("o", o)))
    lin = _host_rows_of("lin", lin, (n + 3,))
    cnt = _same_rows((("fh", fh), ("lin", lin), ("l", l), ("r", r), ("o", o)))
    if rows is not None and int(rows) != cnt:
        raise ValueError("rows = %d != %d rows of the arrays" % (rows, cnt))
    _host_strides((("in_stride", in_stride, n + 3), ("out_stride", out_stride, n + 2)))
    if out is not None:
        raise ValueError("out belongs to the device form: the host form returns new arrays")
    ch = [_host_challenges(k, v, cnt) for k, v in (("zeta", zeta), ("kzg_gamma", kzg_gamma))]
    if cnt == 0:
        return np.zeros((0, n + 2, 4), np.uint64), np.zeros((0, 4), np.uint64)
    bufs = [_lib.DeviceBuffer.from_numpy(v) for v in [_padded(fh, n + 3), lin, _padded(l, n + 3), _padded(r, n + 3), _padded(o, n + 3)] + ch]
    dq, dv = _lib.DeviceBuffer(cnt * (n + 2) * 32), _lib.DeviceBuffer(cnt * 32)
    bufs += [dq, dv]
    p = lambda b: C.c_void_p(b.ptr)
    return _run(lambda: lib().zk_bn254_plonk_open_batch_dev(pk.handle, *(p(b) for b in bufs[:5]), C.c_size_t(n + 3), C.c_size_t(cnt), p(bufs[5]), p(bufs[6]), p(dq),
                                                            C.c_size_t(n + 2), p(dv), C.c_void_p(0)),
                bufs, [], lambda: (dq.to_numpy(np.uint64, (cnt, n + 2, 4)), dv.to_numpy(np.uint64, (cnt, 4))))


# ---- the digests every round ends in, for the rows of the batch entries above (zk_bn254_plonk_commit_batch_dev)
def commit_rows(pk: ProvingKey, rows_data, *, from_values: bool = False, length: int | None = None, rows: int | None = None, row_stride: int | None = None, out=None,
                compressed=False, points: bool = True):
    """ProvingKey.commit_rows"""
    from .bn254 import rows_digests

    def dev(ptr, stride, n_, rows_, o, c):
        return lib().zk_bn254_plonk_commit_batch_dev(pk.handle, C.c_void_p(ptr), C.c_size_t(stride), C.c_size_t(n_), C.c_size_t(rows_), C.c_int(int(bool(from_values))),
                                                     C.c_void_p(o), C.c_void_p(c))

    if from_values:
        width = length if isinstance(rows_data, _DEV) else (rows_data.shape[1] if isinstance(rows_data, np.ndarray) and rows_data.ndim == 3 else None)
        if width is not None and int(width) != pk.domain_size + 2:
            raise ValueError("a row of values is the n = %d wire values and two blinders, not %d elements" % (pk.domain_size, width))
    return rows_digests(dev, None, rows_data, length, rows, row_stride, out, compressed, points)
