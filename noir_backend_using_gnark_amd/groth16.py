"""Host-side mirror of gnark v0.8.0 groth16 prove for the hot path (pinned at /root/reference/gnark_backend_ffi/go.mod:23;
the reference's live call is groth16.Prove at /root/reference/gnark_backend_ffi/main.go:131; the FFI it intended is the
commented-out ProveWithPK at backend/groth16/r1cs.go:107-143).  `prove` takes what gnark's prover has after
`r1cs.Solve`: the evaluation vectors a, b, c and the wire values w -- plus the randomness (r, s) as explicit inputs."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import Groth16PK, check, lib, vp


class ProvingKey:
    """groth16.ProvingKey{G1{Alpha,Beta,Delta,A,B,K,Z}, G2{Beta,Delta,B}} resident in HBM.

    Arrays are gnark memory images (numpy uint64) or, with bases_on_device=True, raw device pointers for the five
    base arrays (used by the benchmark, whose bases are generated on the device).

    gnark's own layout: pass infinity_a / infinity_b (the []bool InfinityA / InfinityB, one entry per wire); g1_a then holds the
    n_wires - NbInfinityA points gnark stores, g1_b / g2_b the n_wires - NbInfinityB ones (setup.go).  Without the bitmaps the
    arrays are wire-indexed with (0,0) for a point at infinity.

    window_shard=(rank, count): the WINDOW-sharded key of one rank -- the whole key, but only the table rows (digit windows) w = rank + k * count;
    msm5 against it yields the partial sums over those windows of the full wire / h vectors.

    device_mask: several GPUs in ONE process (zk_init_devices): bit i = device entry i holds a range slice of the key (2, 4 or 8 entries);
    prove() on such a key runs computeH block-sharded over the entries and the five MSMs per slice -- same bytes.

    A rank of a range-sharded proof loads ITS slice as a key of its own (n_wires / n_public / log_domain describe the
    slice; shard_full_z=True on every rank but the last, whose Z slice ends with the unused N-th entry)."""

    def __init__(self, log_domain: int, n_wires: int, n_public: int, g1_alpha, g1_beta, g1_delta, g1_a, g1_b, g1_k, g1_z,
                 g2_beta, g2_delta, g2_b, bases_on_device: bool = False, precompute_tables: bool = True, shard_full_z: bool = False,
                 infinity_a=None, infinity_b=None, table_window_bits: int = 0, window_shard: tuple | None = None, device_mask: int = 0):
        self.log_domain, self.n_wires, self.n_public = log_domain, n_wires, n_public
        self._keep = []
        inf_a = inf_b = 0
        nb_a = nb_b = 0
        if (infinity_a is None) != (infinity_b is None):
            raise ValueError("InfinityA and InfinityB come together")
        if infinity_a is not None:
            ia = np.ascontiguousarray(np.asarray(infinity_a).astype(np.uint8))
            ib = np.ascontiguousarray(np.asarray(infinity_b).astype(np.uint8))
            if ia.size != n_wires or ib.size != n_wires:
                raise ValueError("InfinityA / InfinityB need one entry per wire")
            self._keep += [ia, ib]
            inf_a, inf_b = ia.ctypes.data, ib.ctypes.data
            nb_a, nb_b = int(np.count_nonzero(ia)), int(np.count_nonzero(ib))

        def host(a):
            a = np.ascontiguousarray(a, dtype=np.uint64)
            self._keep.append(a)
            return a.ctypes.data

        def base(a):
            if bases_on_device:
                return int(a.ptr if isinstance(a, _lib.DeviceBuffer) else a)
            return host(a) if np.asarray(a).size else 0

        pk = Groth16PK(log_domain, n_wires, n_public, host(g1_alpha), host(g1_beta), host(g1_delta), base(g1_a), base(g1_b),
                       base(g1_k), base(g1_z), host(g2_beta), host(g2_delta), base(g2_b), 1 if bases_on_device else 0,
                       (0 if precompute_tables else 1) | (2 if shard_full_z else 0) | (4 if window_shard else 0), inf_a, inf_b, nb_a, nb_b, table_window_bits, device_mask,
                       *(window_shard or (0, 0)))
        if bases_on_device:
            self._keep += [g1_a, g1_b, g1_k, g1_z, g2_b]  # keep DeviceBuffers alive
        self.handle = C.c_uint64(0)
        check(lib().zk_bn254_groth16_pk_load(C.byref(pk), C.byref(self.handle)))

    @classmethod
    def from_handle(cls, handle: int, log_domain: int, n_wires: int, n_public: int):
        """wraps a key that already lives in the library (groth16.Setup on the device)"""
        pk = cls.__new__(cls)
        pk.log_domain, pk.n_wires, pk.n_public, pk._keep, pk.handle = log_domain, n_wires, n_public, [], C.c_uint64(handle)
        return pk

    @classmethod
    def read_from(cls, data, is_hex: bool | None = None, precompute_tables: bool = True, table_window_bits: int = 0):
        """groth16.ProvingKey.ReadFrom on the bytes of ProvingKey.WriteTo (or their hex text, the form the reference's ProveWithPK receives:
        backend/groth16/r1cs.go:107-128): points are decompressed on the device."""
        raw = data.encode("ascii") if isinstance(data, str) else bytes(data)
        if is_hex is None:
            is_hex = isinstance(data, str)
        h = C.c_uint64(0)
        rc = lib().zk_bn254_groth16_pk_read(C.c_char_p(raw), C.c_size_t(len(raw)), C.c_int(int(is_hex)), C.c_int(0 if precompute_tables else 1),
                                            C.c_int(table_window_bits), C.byref(h))
        if rc in (_lib.ZK_ERR_LEN, _lib.ZK_ERR_ARG):
            raise ValueError((lib().zk_last_error() or b"").decode())
        check(rc)
        pk = cls.from_handle(h.value, 0, 0, 0)
        i = pk.info()
        pk.log_domain, pk.n_wires, pk.n_public = i["log_domain"], i["n_wires"], i["n_public"]
        return pk

    def write_to(self, as_hex: bool = False):
        """groth16.ProvingKey.WriteTo (compressed points; A / B / G2.B without their points at infinity + InfinityA / InfinityB) -> bytes, or hex str"""
        n = C.c_size_t(0)
        check(lib().zk_bn254_groth16_pk_write(self.handle, C.c_int(int(as_hex)), None, C.c_size_t(0), C.byref(n)))
        buf = C.create_string_buffer(n.value)
        check(lib().zk_bn254_groth16_pk_write(self.handle, C.c_int(int(as_hex)), buf, C.c_size_t(n.value), C.byref(n)))
        return buf.raw[:n.value].decode() if as_hex else buf.raw[:n.value]

    def vk_write_to(self, vk: dict, as_hex: bool = False):
        """groth16.VerifyingKey.WriteTo from setup()'s vk dict (this key supplies [beta]1 and [delta]1)"""
        g1 = np.ascontiguousarray(np.concatenate([np.asarray(vk["g1_alpha"], np.uint64).reshape(1, 8), np.asarray(vk["g1_k"], np.uint64).reshape(-1, 8)]))
        g2 = np.ascontiguousarray(np.stack([np.asarray(vk[k], np.uint64).reshape(16) for k in ("g2_beta", "g2_gamma", "g2_delta")]))
        n = C.c_size_t(0)
        cap = 2 * (292 + 32 * (g1.shape[0] - 1))
        buf = C.create_string_buffer(cap)
        rc = lib().zk_bn254_groth16_vk_write(self.handle, vp(g1), C.c_size_t(g1.shape[0] - 1), vp(g2), C.c_int(int(as_hex)), buf, C.c_size_t(cap), C.byref(n))
        if rc == _lib.ZK_ERR_LEN:
            raise ValueError((lib().zk_last_error() or b"").decode())
        check(rc)
        return buf.raw[:n.value].decode() if as_hex else buf.raw[:n.value]

    def info(self) -> dict:
        nw, npub, ld, tab = C.c_size_t(0), C.c_size_t(0), C.c_uint32(0), C.c_int(0)
        check(lib().zk_bn254_groth16_pk_info(self.handle, C.byref(nw), C.byref(npub), C.byref(ld), C.byref(tab)))
        return dict(n_wires=int(nw.value), n_public=int(npub.value), log_domain=int(ld.value), tables=bool(tab.value))

    def free(self):
        if self.handle.value:
            check(lib().zk_bn254_groth16_pk_free(self.handle))
            self.handle = C.c_uint64(0)


def _ptr(x):
    if isinstance(x, _lib.DeviceBuffer):
        return C.c_void_p(x.ptr)
    if isinstance(x, int):
        return C.c_void_p(x)
    return vp(np.ascontiguousarray(x, dtype=np.uint64))


def prove(pk: ProvingKey, a, b, c, w, r, s, n_constraints: int | None = None, on_device: bool = False, n_wires: int | None = None) -> bytes:
    """groth16.Prove from the solver output: returns Proof.WriteTo bytes (Ar | Bs | Krs compressed, 128 B).
    len(w) != the key's wire count is the library's error (ZK_ERR_LEN -> ValueError), like a mismatched MultiExp upstream."""
    if not on_device:
        a, b, c, w = (np.ascontiguousarray(v, dtype=np.uint64).reshape(-1, 4) for v in (a, b, c, w))
        if not (a.shape == b.shape == c.shape):
            raise ValueError("a, b, c must have the same length")
        n_constraints = a.shape[0]
        n_wires = w.shape[0]
    elif n_wires is None:
        n_wires = pk.n_wires  # device pointers carry no length: the caller vouches for n_wires elements
    r = np.ascontiguousarray(r, dtype=np.uint64).reshape(4)
    s = np.ascontiguousarray(s, dtype=np.uint64).reshape(4)
    proof = (C.c_uint8 * 128)()
    rc = lib().zk_bn254_groth16_prove(pk.handle, _ptr(a), _ptr(b), _ptr(c), C.c_size_t(n_constraints), _ptr(w), C.c_size_t(n_wires), vp(r), vp(s),
                                      C.c_int(int(on_device)), proof)
    if rc == _lib.ZK_ERR_LEN:
        raise ValueError((lib().zk_last_error() or b"").decode())
    check(rc)
    return bytes(proof)


def compute_h(a, b, c, log_domain: int) -> np.ndarray:
    """gnark's computeH(a, b, c, domain): (N, 4) coefficients of h in the (bit-reversed) order upstream leaves them."""
    a, b, c = (np.ascontiguousarray(v, dtype=np.uint64).reshape(-1, 4) for v in (a, b, c))
    if not (a.shape == b.shape == c.shape):
        raise ValueError("a, b, c must have the same length")
    h = np.zeros((1 << log_domain, 4), dtype=np.uint64)
    check(lib().zk_bn254_groth16_compute_h(vp(a), vp(b), vp(c), C.c_size_t(a.shape[0]), C.c_uint32(log_domain), vp(h)))
    return h


def compute_h_batch(a, b, c, log_domain: int) -> np.ndarray:
    """computeH of every row of the (rows, n, 4) arrays a, b, c in the launches of one (zk_bn254_groth16_compute_h_batch): (rows, N, 4), row i what compute_h gives
    for a[i], b[i], c[i].  Shape and dtype errors are raised before the library is called."""
    for v in (a, b, c):
        if not (isinstance(v, np.ndarray) and v.dtype == np.uint64):
            raise TypeError("a, b, c must be uint64 numpy arrays")
        if v.ndim != 3 or v.shape[2] != 4:
            raise ValueError("a, b, c must have shape (rows, n, 4), not %s" % (v.shape,))
    if not (a.shape == b.shape == c.shape):
        raise ValueError("a, b, c must have the same shape")
    if not 0 <= int(log_domain) <= 28:
        raise ValueError("log_domain must be in 0 .. 28")
    rows, n = a.shape[0], a.shape[1]
    if n > (1 << log_domain):
        raise ValueError("n = %d exceeds the domain size %d" % (n, 1 << log_domain))
    a, b, c = (np.ascontiguousarray(v) for v in (a, b, c))
    h = np.zeros((rows, 1 << log_domain, 4), dtype=np.uint64)
    check(lib().zk_bn254_groth16_compute_h_batch(vp(a), vp(b), vp(c), C.c_size_t(n), C.c_uint32(log_domain), C.c_size_t(rows), vp(h)))
    return h


class R1CS:
    """cs.R1CS resident in HBM: constraints (L w) o (R w) = (O w) over the wires [ONE, public..., secret..., internal...]; n_public counts the
    ONE wire (gnark's GetNbPublicVariables).  `constraints`: list of (L, R, O), each a dict wire -> Montgomery coefficient (4 limbs)."""

    def __init__(self, n_public: int, n_wires: int, constraints):
        self.n_public, self.n_wires, self.n_constraints = n_public, n_wires, len(constraints)
        mats = []
        for m in range(3):
            ptr, idx, val = [0], [], []
            for con in constraints:
                for wire, coeff in con[m].items():
                    idx.append(wire)
                    val.append(np.asarray(coeff, dtype=np.uint64).reshape(4))
                ptr.append(len(idx))
            mats.append((np.asarray(ptr, dtype=np.uint32), np.asarray(idx, dtype=np.uint32), np.ascontiguousarray(np.stack(val)) if val else np.zeros((0, 4), np.uint64)))
        self._keep = mats
        raw = _lib.R1CS(self.n_constraints, n_wires, n_public, *[a.ctypes.data for mat in mats for a in mat])
        self.handle = C.c_uint64(0)
        check(lib().zk_bn254_r1cs_load(C.byref(raw), C.byref(self.handle)))

    @classmethod
    def from_handle(cls, handle: int, n_public: int, n_wires: int, n_constraints: int):
        r = cls.__new__(cls)
        r.n_public, r.n_wires, r.n_constraints, r._keep, r.handle = n_public, n_wires, n_constraints, [], C.c_uint64(handle)
        return r

    def eval_abc(self, w) -> tuple:
        """a, b, c = L w, R w, O w on the device (the solver's output for a system without hints) -> numpy"""
        w = np.ascontiguousarray(w, dtype=np.uint64).reshape(-1, 4)
        dw = _lib.DeviceBuffer.from_numpy(w)
        out = [_lib.DeviceBuffer(max(self.n_constraints, 1) * 32) for _ in range(3)]
        rc = lib().zk_bn254_r1cs_eval_abc_dev(self.handle, C.c_void_p(dw.ptr), C.c_size_t(w.shape[0]), *[C.c_void_p(o.ptr) for o in out], None)
        if rc == _lib.ZK_ERR_LEN:
            raise ValueError((lib().zk_last_error() or b"").decode())
        check(rc)
        return tuple(o.to_numpy(np.uint64, (self.n_constraints, 4)) for o in out)

    def eval_abc_rows(self, w, on_device: bool = False, rows: int | None = None, out=None) -> tuple:
        """eval_abc of every row of w (rows, n_wires, 4) in ONE launch -- the launch prove_r1cs_batch makes (zk_bn254_r1cs_eval_abc_rows_dev) -> a, b, c, each
        (rows, n_constraints, 4) numpy.  on_device=True: w is a DeviceBuffer of `rows` rows of this system's n_wires elements, only read.  out: three
        DeviceBuffers of at least rows x n_constraints elements to write into (theirs otherwise); the arrays returned are read back from them."""
        if on_device:
            if not isinstance(w, _lib.DeviceBuffer):
                raise TypeError("on_device=True takes a DeviceBuffer of rows")
            if rows is None:
                raise ValueError("a device buffer carries no shape: rows is needed")
            n, n_wires, dw = int(rows), self.n_wires, w
            if n < 0 or n * n_wires * 32 > w.nbytes:
                raise ValueError("%d rows of %d wires do not fit the buffer's %d bytes" % (n, n_wires, w.nbytes))
        else:
            w = _rows(w, "w")
            n, n_wires = w.shape[0], w.shape[1]
            if rows is not None and rows != n:
                raise ValueError("rows = %d, w has %d" % (rows, n))
            dw = _lib.DeviceBuffer.from_numpy(w)
        need = n * self.n_constraints * 32
        if out is None:
            out = [_lib.DeviceBuffer(max(need, 32)) for _ in range(3)]
        elif len(out) != 3 or not all(isinstance(o, _lib.DeviceBuffer) and o.nbytes >= need for o in out):
            raise ValueError("out must be three DeviceBuffers of at least %d bytes" % need)
        rc = lib().zk_bn254_r1cs_eval_abc_rows_dev(self.handle, C.c_void_p(dw.ptr), C.c_size_t(n_wires), C.c_size_t(n), *[C.c_void_p(o.ptr) for o in out], None)
        if rc == _lib.ZK_ERR_LEN:
            raise ValueError((lib().zk_last_error() or b"").decode())
        check(rc)
        return tuple(o.to_numpy(np.uint64, (n, self.n_constraints, 4)) for o in out)

    def free(self):
        if self.handle.value:
            check(lib().zk_bn254_r1cs_free(self.handle))
            self.handle = C.c_uint64(0)


def setup(r1cs: R1CS, toxic, precompute_tables: bool = True):
    """groth16.Setup(r1cs) with the toxic waste (tau, alpha, beta, gamma, delta; (5, 4) Montgomery) as input -> (ProvingKey, vk dict)."""
    tx = np.ascontiguousarray(toxic, dtype=np.uint64).reshape(5, 4)
    h = C.c_uint64(0)
    vk1 = np.zeros((1 + r1cs.n_public, 8), np.uint64)
    vk2 = np.zeros((3, 16), np.uint64)
    check(lib().zk_bn254_groth16_setup(r1cs.handle, vp(tx), C.c_int(0 if precompute_tables else 1), C.byref(h), vp(vk1), vp(vk2)))
    log_n = max(r1cs.n_constraints - 1, 0).bit_length()
    pk = ProvingKey.from_handle(h.value, log_n, r1cs.n_wires, r1cs.n_public)
    return pk, dict(g1_alpha=vk1[0], g1_k=vk1[1:], g2_beta=vk2[0], g2_gamma=vk2[1], g2_delta=vk2[2])


def prove_r1cs(r1cs: R1CS, pk: ProvingKey, w, r, s) -> bytes:
    """groth16.Prove(r1cs, pk, witness): the full wire vector in (numpy, or a DeviceBuffer already in HBM), a / b / c on the device, 128 bytes out."""
    on_dev = isinstance(w, _lib.DeviceBuffer)
    if on_dev:
        wp, nw = C.c_void_p(w.ptr), r1cs.n_wires
    else:
        w = np.ascontiguousarray(w, dtype=np.uint64).reshape(-1, 4)
        wp, nw = vp(w), w.shape[0]
    r = np.ascontiguousarray(r, dtype=np.uint64).reshape(4)
    s = np.ascontiguousarray(s, dtype=np.uint64).reshape(4)
    proof = (C.c_uint8 * 128)()
    rc = lib().zk_bn254_groth16_prove_r1cs(r1cs.handle, pk.handle, wp, C.c_size_t(nw), vp(r), vp(s), C.c_int(int(on_dev)), proof)
    if rc == _lib.ZK_ERR_LEN:
        raise ValueError((lib().zk_last_error() or b"").decode())
    check(rc)
    return bytes(proof)


def _rs_rows(r, s, n: int):
    r = np.ascontiguousarray(r, dtype=np.uint64).reshape(-1, 4)
    s = np.ascontiguousarray(s, dtype=np.uint64).reshape(-1, 4)
    if r.shape[0] != n or s.shape[0] != n:
        raise ValueError("r and s need one element per row of w (%d): got %d and %d" % (n, r.shape[0], s.shape[0]))
    return r, s


def _rows(v, what: str) -> np.ndarray:
    v = np.ascontiguousarray(v, dtype=np.uint64)
    if v.ndim == 2 and v.shape[1] == 4:
        raise ValueError("%s must be a matrix of limbs (rows, elements, 4), one row per proof" % what)
    if v.ndim != 3 or v.shape[2] != 4:
        raise ValueError("%s must have the shape (rows, elements, 4)" % what)
    return v


def batch_info(pk: ProvingKey) -> dict:
    """rows per chunk of the batched path for this key, and whether the batched path serves it (else prove_batch runs the rows through prove)"""
    rows, batched = C.c_size_t(0), C.c_int(0)
    check(lib().zk_bn254_groth16_batch_info(pk.handle, C.byref(rows), C.byref(batched)))
    return dict(chunk_rows=int(rows.value), batched=bool(batched.value))


def prove_batch(pk: ProvingKey, a, b, c, w, r, s, on_device: bool = False, n_constraints: int | None = None) -> list:
    """groth16.Prove for many witnesses against one key in one call: a, b, c (rows, n_constraints, 4), w (rows, n_wires, 4), r, s (rows, 4) -> one 128-byte
    proof per row, each byte for byte what prove() returns for that row.  on_device=True: a, b, c, w are DeviceBuffers / device pointers of row-major
    matrices (n_constraints says how wide a, b, c are; w is the key's wire count wide) and the row count comes from r."""
    if on_device:
        r = np.ascontiguousarray(r, dtype=np.uint64).reshape(-1, 4)
        r, s = _rs_rows(r, s, r.shape[0])
        if n_constraints is None:
            raise ValueError("device matrices carry no shape: n_constraints is needed")
        n, n_wires = r.shape[0], pk.n_wires
    else:
        a, b, c, w = _rows(a, "a"), _rows(b, "b"), _rows(c, "c"), _rows(w, "w")
        n, n_wires = w.shape[0], w.shape[1]
        if not (a.shape == b.shape == c.shape):
            raise ValueError("a, b, c must have the same shape")
        if a.shape[0] != n:
            raise ValueError("a, b, c have %d rows, w has %d" % (a.shape[0], n))
        r, s = _rs_rows(r, s, n)
        n_constraints = a.shape[1]
    proofs = (C.c_uint8 * (128 * max(n, 1)))()
    rc = lib().zk_bn254_groth16_prove_batch(pk.handle, _ptr(a), _ptr(b), _ptr(c), C.c_size_t(n_constraints), _ptr(w), C.c_size_t(n_wires), vp(r), vp(s),
                                            C.c_size_t(n), C.c_int(int(on_device)), proofs)
    if rc == _lib.ZK_ERR_LEN:
        raise ValueError((lib().zk_last_error() or b"").decode())
    check(rc)
    raw = bytes(proofs)
    return [raw[128 * i:128 * i + 128] for i in range(n)]


def finalize_batch(pk: ProvingKey, partials, r, s) -> list:
    """The second half of prove() for many rows in one device launch (zk_bn254_groth16_finalize_batch): partials (n_proofs, n_partials, 96) -- or (n_proofs, 96)
    for one record per row -- of uint64 limbs as zk_bn254_groth16_msm5_* writes them (A, B1, K, Z as G1 XYZZ, then G2.B), r, s (n_proofs, 4) -> one 128-byte
    proof per row, each byte for byte what parallel.groth16_finalize returns for that row."""
    partials = np.ascontiguousarray(partials, dtype=np.uint64)
    if partials.ndim == 2:
        partials = partials.reshape(partials.shape[0], 1, partials.shape[1])
    if partials.ndim != 3 or partials.shape[2] != 96:
        raise ValueError("partials must have the shape (n_proofs, n_partials, 96) or (n_proofs, 96)")
    n, n_partials = partials.shape[0], partials.shape[1]
    if n and n_partials == 0:
        raise ValueError("a row needs at least one record")
    r, s = _rs_rows(r, s, n)
    proofs = (C.c_uint8 * (128 * max(n, 1)))()
    check(lib().zk_bn254_groth16_finalize_batch(pk.handle, vp(partials), C.c_size_t(n_partials), vp(r), vp(s), C.c_size_t(n), proofs))
    raw = bytes(proofs)
    return [raw[128 * i:128 * i + 128] for i in range(n)]


def prove_r1cs_batch(r1cs: R1CS, pk: ProvingKey, w, r, s, on_device: bool = False) -> list:
    """groth16.Prove(r1cs, pk, witness) for many witnesses: w (rows, n_wires, 4) -> one proof per row, each what prove_r1cs() returns for it.
    on_device=True: w is a DeviceBuffer of row-major rows already in HBM, the constraint system's wire count wide and only read; the row count comes from r."""
    if on_device:
        if not isinstance(w, _lib.DeviceBuffer):
            raise TypeError("on_device=True takes a DeviceBuffer of rows")
        r = np.ascontiguousarray(r, dtype=np.uint64).reshape(-1, 4)
        r, s = _rs_rows(r, s, r.shape[0])
        n, n_wires, wp = r.shape[0], r1cs.n_wires, C.c_void_p(w.ptr)
        if n * n_wires * 32 > w.nbytes:
            raise ValueError("%d rows of %d wires do not fit the buffer's %d bytes" % (n, n_wires, w.nbytes))
    else:
        if isinstance(w, _lib.DeviceBuffer):
            raise TypeError("a DeviceBuffer of rows needs on_device=True")
        w = _rows(w, "w")
        r, s = _rs_rows(r, s, w.shape[0])
        n, n_wires, wp = w.shape[0], w.shape[1], vp(w)
    proofs = (C.c_uint8 * (128 * max(n, 1)))()
    rc = lib().zk_bn254_groth16_prove_r1cs_batch(r1cs.handle, pk.handle, wp, C.c_size_t(n_wires), vp(r), vp(s), C.c_size_t(n), C.c_int(int(on_device)), proofs)
    if rc == _lib.ZK_ERR_LEN:
        raise ValueError((lib().zk_last_error() or b"").decode())
    check(rc)
    raw = bytes(proofs)
    return [raw[128 * i:128 * i + 128] for i in range(n)]
