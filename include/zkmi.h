/* zkmi.h -- C ABI of libzkmi.so: the MI355X (gfx950) BN254 proving hot path.
 *
 * This is the drop-in boundary for the ONE path this repository replaces inside
 * lambdaclass/noir_backend_using_gnark: the gnark-crypto calls that gnark's provers make
 *     (*G1Jac).MultiExp / (*G2Jac).MultiExp      ecc/bn254/multiexp.go          (Pippenger MSM)
 *     (*fft.Domain).FFT / FFTInverse / BitReverse ecc/bn254/fr/fft/fft.go        (radix-2 NTT over Fr)
 *     computeH + the 5 MSMs of groth16.Prove      gnark internal/backend/bn254/groth16/prove.go
 *     kzg.Commit (= one G1 MSM)                   ecc/bn254/fr/kzg/kzg.go
 * The reference pins those modules at /root/reference/gnark_backend_ffi/go.mod:5 (gnark-crypto v0.9.1) and
 * go.mod:23 (gnark v0.8.0) and reaches them ONLY through
 *     groth16.Prove   /root/reference/gnark_backend_ffi/main.go:131
 *     plonk.Prove     /root/reference/gnark_backend_ffi/backend/plonk/plonk.go:67
 *     plonk.Setup     /root/reference/gnark_backend_ffi/backend/plonk/plonk.go:21
 *     kzg.NewSRS      /root/reference/gnark_backend_ffi/backend/common.go:137
 * (there is no direct MultiExp / fft call site in the reference: SURVEY.md §0 fact 2).  INTEGRATION.md shows the
 * cgo stubs that bind each entry point below at those gnark-crypto call sites; the outer Rust->Go FFI
 * (PlonkProveWithPK & co, /root/reference/gnark_backend_ffi/main.go:24-78) is untouched by construction.
 *
 * Conventions
 *  - plain C types only; every pointer is valid for the duration of the call only (cgo rule: C must not retain Go
 *    pointers) unless the function name ends in _dev, in which case the pointer is a HIP device pointer owned by
 *    the caller.
 *  - field elements are gnark-crypto's memory image: uint64_t[4], little-endian limbs, Montgomery form
 *    (x * 2^256 mod p).  G1Affine = {X, Y}; G2Affine = {X.A0, X.A1, Y.A0, Y.A1}; the point at infinity is (0,0).
 *  - results that are points are AFFINE (canonical); the Go shim calls FromAffine to satisfy *G1Jac.
 *  - return value: 0 = ok, negative = zk_status error; zk_last_error() gives a thread-local message.
 *  - thread-safe and re-entrant: gnark issues its MSMs from several goroutines; each call picks a stream slot.
 *  - there is NO CPU fallback: without a usable HIP device every compute entry point returns ZK_ERR_NO_DEVICE.
 */
#ifndef ZKMI_H
#define ZKMI_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct { uint64_t l[4]; } zk_fr;                 /* fr.Element  (go.mod:5 ecc/bn254/fr)  */
typedef struct { uint64_t l[4]; } zk_fp;                 /* fp.Element  (go.mod:5 ecc/bn254/fp)  */
typedef struct { zk_fp x, y; } zk_g1_affine;             /* bn254.G1Affine */
typedef struct { zk_fp x0, x1, y0, y1; } zk_g2_affine;   /* bn254.G2Affine {X E2{A0,A1}, Y E2{A0,A1}} */

typedef enum {
    ZK_OK = 0,
    ZK_ERR_LEN = -1,        /* MultiExp: "len(points) != len(scalars)" */
    ZK_ERR_NB_TASKS = -2,   /* MultiExp: "invalid config: config.NbTasks > 1024" */
    ZK_ERR_NO_DEVICE = -3,  /* no usable gfx950 device / HIP runtime -- never falls back to the CPU */
    ZK_ERR_HIP = -4,        /* a HIP call failed; see zk_last_error() */
    ZK_ERR_ARG = -5,        /* bad argument (null pointer, size not a power of two, log_n > 28, ...) */
    ZK_ERR_HANDLE = -6,     /* unknown or freed handle (or a proving key that live msm5 sessions still use) */
    ZK_ERR_BUSY = -7        /* no stream slot became free within the time limit (ZKMI_SLOT_TIMEOUT_S, default 120 s): a caller
                               that holds an msm5 session (5 of the 8 slots) and asks for more would otherwise wait forever */
} zk_status;

/* mirrors ecc.MultiExpConfig{NbTasks, ScalarsMont} of gnark-crypto v0.9.1, plus device-side knobs */
typedef struct {
    int nb_tasks;      /* accepted for compatibility; > 1024 is rejected like upstream; otherwise ignored      */
    int scalars_mont;  /* 1: scalars are Montgomery fr.Element images; 0: regular (canonical) form -- upstream's zero value
                          (gnark v0.8.0 calls FromMont() on the wire values / h and passes the default config)         */
    int window_bits;   /* 0 = auto (cost model for the GPU), else c in [2, 22]; against registered bases with window
                          tables an explicit value selects the plain (table-less) method                              */
    int device_mask;   /* several GPUs in ONE process (zk_init_devices): bit i = device entry i takes part; 0 = the process default
                          (zk_set_default_devices; every entry once zk_init_devices was called, else the calling thread's entry)  */
} zk_msm_cfg;

enum { ZK_DIT = 0, ZK_DIF = 1 }; /* fft.Decimation (same iota order as gnark-crypto) */

/* ---- lifecycle ------------------------------------------------------------------------------------------------ */
int zk_device_count(void);             /* number of visible HIP devices (0 if none / runtime missing)             */
int zk_init(int device);               /* optional: bind the calling process to `device` (default: 0, lazily)     */
/* Several GPUs in ONE process (the reference is one process: nargo -> Rust -> cgo; gnark_backend_ffi/main.go:24-37).  zk_init_devices gives the process
 * its device list: one ENTRY per listed HIP device, in order (devices == NULL or n == 0: every visible device); a device may be listed several times
 * (each listing is an entry with streams and workspaces of its own: "virtual devices").  From then on the calls that carry a device_mask -- and, through
 * the process default, those that do not (zk_bn254_ntt on host slices, zk_bn254_bases_register*) -- spread over the entries: MSMs by point range, a
 * resident Groth16 key by wire range with computeH block-sharded, transforms by blocks; results are the single-GPU bytes.  Resident objects carry their
 * entry in their handle, so every call on a handle runs on that handle's GPU whatever thread makes it; zk_set_entry picks the entry for the calls of the
 * calling THREAD that take no handle (zk_dev_alloc, zk_bn254_ntt_dev, ...).  Calling zk_init_devices again may only extend the list. */
int zk_init_devices(const int *devices, size_t n);
/* The stream slots a first proof will take, created ahead of time: a HIP stream costs 7-14 ms to create on MI355X / ROCm 7.2 and the first one of a process
 * 40-160 ms (tools/hip_start_bench.hip), so the library creates them when a slot is first used -- or here, for a caller that has host work to do meanwhile (the
 * export shim reads srs.hex).  n slots of the calling thread's device entry (at most all 8). */
int zk_warm_streams(int n);
/* The same for the five slots of a Groth16 proof session INCLUDING their high-priority streams (what zk_bn254_groth16_prove takes at once).  After
 * zk_init_flags(ZK_INIT_LEAN_STREAMS) this is also what ALLOWS those streams: until it is called a lean process runs every chain on the slots' own streams (its
 * first proof creates no stream; the export path calls it when a key's second proof is asked for). */
int zk_warm_session_streams(void);
/* The same from the library's background thread, one slot at a time (each slot is held only while its stream is created): proofs that arrive meanwhile find
 * their five slots and keep running on the slots' own streams until all five high-priority streams exist.  Returns at once. */
int zk_warm_session_streams_background(void);
/* 1 when no background job (window tables of a key or SRS that proves again, zk_warm_session_streams_background) is queued or running; waits up to timeout_ms
 * for that (< 0: as long as it takes), 0 on timeout.  For callers that want the tables in place before they measure or compare; the provers never wait. */
int zk_background_wait(int timeout_ms);
/* Background jobs start when no call is in flight: zk_background_hold(+1) / (-1) brackets a call of several phases (the export shim does it around every
 * export; the library's export entry points do it themselves); a job waits for the count to reach zero and the stream slots to be free, at most
 * zk_background_set_yield_ms (default 250, 0 = start at once; [0, 60000]).  Neither changes a result. */
void zk_background_hold(int delta);
int zk_background_set_yield_ms(int ms);
/* Process-wide start-up choices; call before anything that touches a device.  ZK_INIT_LEAN_STREAMS: a device entry creates only the five streams every caller
 * needs with itself and every other stream on first use (the default also creates the five high-priority streams of a Groth16 proof session up front: 40 ms more
 * start-up, 1 % less per 2^20 proof -- WHICH streams share a hardware queue follows creation order).  For a process that makes one proof and exits. */
#define ZK_INIT_LEAN_STREAMS 1u
int zk_init_flags(uint32_t flags);
int zk_device_entries(int *devices_out, size_t cap); /* number of entries; devices_out[i] = HIP device of entry i */
int zk_set_entry(int entry);
int zk_set_default_devices(uint32_t mask);
uint32_t zk_default_devices(void);
const char *zk_last_error(void);
const char *zk_version(void);

/* ---- MSM: (*G1Jac).MultiExp / (*G2Jac).MultiExp ------------------------------------------------------------------
 * out = sum_i scalars[i] * points[i].  n_points != n_scalars -> ZK_ERR_LEN (upstream error).  Host pointers. */
int zk_bn254_g1_msm(const zk_g1_affine *points, size_t n_points, const zk_fr *scalars, size_t n_scalars,
                    const zk_msm_cfg *cfg, zk_g1_affine *out);
int zk_bn254_g2_msm(const zk_g2_affine *points, size_t n_points, const zk_fr *scalars, size_t n_scalars,
                    const zk_msm_cfg *cfg, zk_g2_affine *out);
/* Same, inputs already resident in HBM (device pointers); `stream` is a hipStream_t or NULL for the library's own. */
int zk_bn254_g1_msm_dev(const void *d_points, const void *d_scalars, size_t n, const zk_msm_cfg *cfg,
                        zk_g1_affine *out_host, void *stream);
int zk_bn254_g2_msm_dev(const void *d_points, const void *d_scalars, size_t n, const zk_msm_cfg *cfg,
                        zk_g2_affine *out_host, void *stream);
/* Partial result for range-sharded multi-GPU MSM: the un-normalised sum as XYZZ (4 coordinates, same limb image);
 * partials from several ranks are combined with zk_bn254_g1_sum_xyzz / zk_bn254_g2_sum_xyzz on any rank. */
int zk_bn254_g1_msm_partial_dev(const void *d_points, const void *d_scalars, size_t n, const zk_msm_cfg *cfg,
                                uint64_t out_xyzz[16], void *stream);
int zk_bn254_g2_msm_partial_dev(const void *d_points, const void *d_scalars, size_t n, const zk_msm_cfg *cfg,
                                uint64_t out_xyzz[32], void *stream);
int zk_bn254_g1_sum_xyzz(const uint64_t *partials, size_t n_partials, zk_g1_affine *out);
int zk_bn254_g2_sum_xyzz(const uint64_t *partials, size_t n_partials, zk_g2_affine *out);

/* Resident bases (Groth16 pk.G1.{A,B,K,Z}, pk.G2.B, kzg SRS.G1): upload once, reuse for every proof. */
int zk_bn254_bases_register(const void *points, size_t n, int is_g2, uint64_t *handle);
int zk_bn254_bases_free(uint64_t handle);
int zk_bn254_msm_bases(uint64_t handle, size_t offset, const zk_fr *scalars, size_t n, const zk_msm_cfg *cfg, void *out);
/* the same with the points (register) / the scalars (msm) already in HBM -- KZG commits of polynomials that the NTTs left on the device.
 * Registration builds precomputed window tables 2^(c*w)*P_i when they fit (>= 4096 bases): every commit then feeds one bucket set. */
int zk_bn254_bases_register_dev(const void *d_points, size_t n, int is_g2, uint64_t *handle);
/* The same with the table geometry chosen by the caller: table_window_bits = 0 auto (tables for >= 4096 bases when they fit),
 * -1 no tables, else c in [8, 24] (tables at any n: how the tests reach the widths the planner picks at 2^22 .. 2^26 points). */
int zk_bn254_bases_register_cfg(const void *points, size_t n, int is_g2, int on_device, int table_window_bits, uint64_t *handle);
/* Window tables for a base array registered without them (table_window_bits as above; 0 = the planner's width, nothing below 4096 bases; a handle that has
 * a table is left alone).  The tables of 1,000,000 G1 points take 17 ms to build and save a 2^19-gate PLONK proof 1.4 ms: a process that makes ONE proof (nargo
 * prove) is better off without them, one that makes many builds them when the second proof is asked for (csrc/goffi.cpp does exactly that). */
int zk_bn254_bases_build_table(uint64_t handle, int table_window_bits);
/* The same on the library's background thread: returns at once; multi-exps against the handle run without the table until it is published.  (What the
 * export shim does when a process's SECOND proving call arrives: that call no longer waits for the build.) */
int zk_bn254_bases_build_table_background(uint64_t handle, int table_window_bits);
int zk_bn254_msm_bases_dev(uint64_t handle, size_t offset, const void *d_scalars, size_t n, const zk_msm_cfg *cfg, void *out);
/* The Lagrange form of a registered G1 base array over the domain of 2^log_n points, as a base array of its own: out[i] = (1/n) sum_j w^(-ij) in[j] for i < n (the
 * inverse transform taken in the exponent: n/2 log2 n + n point-by-scalar multiplications on the device), then in[n] - in[0] and in[n+1] - in[1] (for a KZG SRS:
 * [tau^n - 1], [tau^(n+1) - tau], the points of gnark's blinding).  sum_i e_i out[i] == sum_j c_j in[j] whenever c = FFTInverse(e): a polynomial is committed from its
 * EVALUATIONS -- wire values, small -- instead of its coefficients.  Needs 2^log_n + 2 points on one device entry; free the result with zk_bn254_bases_free. */
int zk_bn254_bases_lagrange(uint64_t handle, uint32_t log_n, uint64_t *out_handle);
/* `count` scalar vectors of n elements each against ONE registered base array: out[k] = MultiExp(bases[offset : offset + n], scalars[k]) -- plonk.Prove's
 * three simultaneous kzg.Commit calls (l, r, o; h1, h2, h3: gnark v0.8.0 backend/plonk/bn254/prove.go, reached from gnark_backend_ffi/backend/plonk/plonk.go:53-73).
 * With a G1 window table and count <= 3 they are ONE multi-scalar multiplication with a bucket set per vector (one recoding, one accumulate launch); otherwise the
 * vectors run one after the other.  out: count affine points of the handle's group; the same points as count calls of zk_bn254_msm_bases. */
int zk_bn254_msm_bases_batch(uint64_t handle, size_t offset, const zk_fr *const *scalars, uint32_t count, size_t n, const zk_msm_cfg *cfg, void *out);
int zk_bn254_msm_bases_batch_dev(uint64_t handle, size_t offset, const void *const *d_scalars, uint32_t count, size_t n, const zk_msm_cfg *cfg, void *out);
/* ROW-BATCHED COMMITMENTS: the digests of `rows` scalar vectors -- row v = the n elements at element v * row_stride of one matrix -- against ONE registered G1
 * base array: gnark-crypto's kzg.Commit for many polynomials at once.  Row v of the output is, byte for byte, the point zk_bn254_msm_bases_dev returns for
 * (handle, offset, d_scalars + v * row_stride, n, cfg); the compressed form is G1Affine.Bytes() of that point.
 *   d_out         rows zk_g1_affine -- gnark's Montgomery image, (0, 0) = infinity --, 16-byte aligned    } device memory in the _dev form, host memory in the
 *   d_compressed  rows x 32 bytes, 4-byte aligned; may be NULL                                             } host form (whose rows are contiguous: stride n)
 *   flags         ZK_MSM_ROWS_SPARSE: the scalars are wire-like (0 / 1 / small), the zero digits never enter the sort -- same digests either way;
 *                 ZK_MSM_ROWS_NO_POINTS: the caller only hashes the digests: d_out may be NULL when d_compressed is given.  Any other bit: ZK_ERR_ARG.
 * BATCHED PATH: a G1 handle on one device entry with its window table (not window-sharded), no explicit cfg->window_bits, rows >= 1: one recoding, one sort,
 * one task plan, ONE accumulate launch and one reduction for all the rows of a chunk, finished on the device (no point comes back to the host); one row is a
 * chunk of one row of the same kernels.  A chunk is the largest row count <= 1024 whose workspace fits 1 GiB and whose sort keys and positions fit their 30 /
 * 31 bits (zk_bn254_msm_rows_info reports it, for a call without an explicit window width, and whether the batched path serves the handle at all: *batched = 0,
 * *chunk_rows = 1 otherwise; the workspace bound is the one that cuts: it holds a chunk below 2^26 positions); more rows run
 * chunk after chunk.  Everything else -- no table, a composite handle, an explicit window width -- runs the rows one after the other through the single
 * multi-exp and delivers the same bytes.  A G2 handle is ZK_ERR_ARG.
 * ERRORS are decided before a device is looked for: null pointers, unknown flag bits, row_stride < n with more than one row (ZK_ERR_ARG), offset + n beyond the
 * registered bases (ZK_ERR_LEN), an unknown handle (ZK_ERR_HANDLE).  The entries synchronise before they return. */
#define ZK_MSM_ROWS_SPARSE 1u
#define ZK_MSM_ROWS_NO_POINTS 2u
int zk_bn254_msm_bases_rows_dev(uint64_t handle, size_t offset, const void *d_scalars, size_t row_stride, size_t n, size_t rows, const zk_msm_cfg *cfg,
                                uint32_t flags, void *d_out, void *d_compressed);
int zk_bn254_msm_bases_rows(uint64_t handle, size_t offset, const zk_fr *scalars, size_t n, size_t rows, const zk_msm_cfg *cfg, uint32_t flags, zk_g1_affine *out,
                            uint8_t *compressed);
int zk_bn254_msm_rows_info(uint64_t handle, size_t n, uint32_t flags, size_t *chunk_rows, int *batched);
/* Scalars kept resident and recoded ONCE for every base array they pair with.  groth16.Prove's five MultiExp calls (gnark v0.8.0 groth16 prove.go, reached
 * from gnark_backend_ffi/main.go:131) pair A, B1, K and G2.B with the SAME wire values: through zk_bn254_msm_bases each call uploads the 32 B x n scalars and
 * recodes them (digits, radix sort, task plan).  zk_bn254_scalars_register uploads once (cfg->scalars_mont says which form they are in);
 * zk_bn254_msm_bases_prepared(bases, bases_offset, scalars, skip, cfg, out) = sum_{i >= skip} scalars[i] * bases[bases_offset + i - skip] shares one recoding
 * among base arrays registered over the same index space (A, B1, G2.B) and makes a second one from the resident copy for K (skip = n_public) -- callable
 * from concurrent threads, like upstream's goroutines.  Same affine result as zk_bn254_msm_bases on the same data. */
int zk_bn254_scalars_register(const zk_fr *scalars, size_t n, const zk_msm_cfg *cfg, uint64_t *handle);
int zk_bn254_scalars_free(uint64_t handle);
int zk_bn254_msm_bases_prepared(uint64_t bases, size_t bases_offset, uint64_t scalars_handle, size_t skip, const zk_msm_cfg *cfg, void *out);

/* ---- NTT: (*fft.Domain).FFT / FFTInverse / fft.BitReverse ------------------------------------------------------
 * In place on a[0 .. 2^log_n).  decimation: ZK_DIF natural in -> bit-reversed out; ZK_DIT bit-reversed in ->
 * natural out.  coset != 0 evaluates on / interpolates from the coset g*H, g = 5 (FrMultiplicativeGen).
 * FFTInverse also scales by 1/N exactly like upstream.
 * INPUT CONTRACT (zk_bn254_ntt, zk_bn254_ntt_devices, zk_bn254_ntt_dev): every element is a CANONICAL fr.Element image, i.e. a Montgomery value REDUCED
 * below r -- what gnark's arithmetic always produces.  The transforms do NOT reduce a 256-bit word mod r first: the butterflies unpack the word as it is and
 * keep lazily reduced 29-bit-limb values whose proven bounds (tools/u29_ntt_model.py, bound_pass) start from an entry below 2.2 r, while a 256-bit word can
 * be as large as 5.29 r.  For an image in [r, 2^256) the result is undefined (e.g. one in [4r, 2^256) handed to the DIT transform without coset meets a
 * subtraction bias of 4 r in the twiddle-free first stage).  tests/test_gpu_ntt_shapes.py sweeps exactly this contract: canonical images up to r - 1. */
int zk_bn254_ntt(zk_fr *a, uint32_t log_n, int inverse, int decimation, int coset);
/* the same over several device entries of this process (bit i of device_mask = entry i; 2, 4 or 8 entries): block k of the array goes to entry k over that
 * GPU's own PCIe link, the transform runs block-sharded with two all-to-all transposes between the GPUs.  zk_bn254_ntt == device_mask 0 (process default). */
int zk_bn254_ntt_devices(zk_fr *a, uint32_t log_n, int inverse, int decimation, int coset, uint32_t device_mask);
int zk_bn254_ntt_dev(void *d_a, uint32_t log_n, int inverse, int decimation, int coset, void *stream);
/* Row batches: the same transform on `rows` vectors of one domain in ONE launch per pass (the row is a grid dimension), instead of one under-filled launch per
 * pass per vector.  Row i is a[i * row_stride .. i * row_stride + 2^log_n), row_stride in elements and >= 2^log_n; elements between the rows are not touched.
 * The input contract is the one above, per row; row i's result is bit for bit zk_bn254_ntt_dev's on that row.  rows == 0 does nothing.
 * zk_bn254_ntt_batch takes contiguous host rows (row_stride = 2^log_n) on one device: it never spreads over device entries.  ZK_ERR_ARG, before the device is
 * touched: null pointer, log_n > 28, bad decimation, row_stride < 2^log_n. */
int zk_bn254_ntt_batch_dev(void *d_a, uint32_t log_n, size_t rows, size_t row_stride, int inverse, int decimation, int coset, void *stream);
int zk_bn254_ntt_batch(zk_fr *a, uint32_t log_n, size_t rows, int inverse, int decimation, int coset);
int zk_bn254_bit_reverse(zk_fr *a, uint32_t log_n);
int zk_bn254_bit_reverse_dev(void *d_a, uint32_t log_n, void *stream);

/* ---- Groth16: computeH and Prove (gnark v0.8.0 internal/backend/bn254/groth16/prove.go) -------------------------
 * computeH: a, b, c hold n <= 2^log_N evaluations each; h_out receives 2^log_N coefficients in the order gnark's
 * computeH leaves them (bit-reversed; the caller uses h[:N-1]).
 * INPUT CONTRACT: as for the NTT entries above -- a, b, c are canonical fr.Element images (< r); the first passes unpack the caller's words as they are, so
 * an image in [r, 2^256) gives an undefined result. */
int zk_bn254_groth16_compute_h(const zk_fr *a, const zk_fr *b, const zk_fr *c, size_t n, uint32_t log_N, zk_fr *h_out);
int zk_bn254_groth16_compute_h_dev(const void *d_a, const void *d_b, const void *d_c, size_t n, uint32_t log_N,
                                   void *d_h_out, void *stream);
/* computeH of `rows` triples in the launches of one (the six transforms with the row as a grid dimension).  Row i of a, b, c holds n <= 2^log_N evaluations at
 * element i * in_stride (in_stride >= n) and is zero-padded to the domain; the inputs are only read.  Row i of the result, 2^log_N coefficients in computeH's order,
 * goes to element i * out_stride (out_stride >= 2^log_N) of d_h_out; elements between the rows are not touched.  d_h_out may be d_a itself when row i of both is
 * the same memory (in_stride == out_stride, or one row); any other overlap of d_h_out with an input is ZK_ERR_ARG.  Same input contract as above; row i's result
 * is bit for bit zk_bn254_groth16_compute_h_dev's on that row.  The host entry takes contiguous rows: a, b, c (rows, n), h_out (rows, 2^log_N).  Scratch comes
 * from the slot's arena, at most 1 GiB at a time: more rows than fit run in chunks.  ZK_ERR_ARG, before the device is touched: null pointer, log_N > 28,
 * n > 2^log_N, in_stride < n, out_stride < 2^log_N.  rows == 0 does nothing. */
int zk_bn254_groth16_compute_h_batch_dev(const void *d_a, const void *d_b, const void *d_c, size_t n, size_t in_stride, uint32_t log_N, size_t rows,
                                         void *d_h_out, size_t out_stride, void *stream);
int zk_bn254_groth16_compute_h_batch(const zk_fr *a, const zk_fr *b, const zk_fr *c, size_t n, uint32_t log_N, size_t rows, zk_fr *h_out);
/* computeH sharded over G = 2^log_g GPUs (one process per GPU; SURVEY.md 8e: the transposes are all-to-all over xGMI,
 * issued by the host between the phases -- the library never communicates).  Rank rho owns the block
 * [rho*M, (rho+1)*M), M = 2^log_D / G, of a, b, c (natural order) and receives the same block of h (gnark's
 * bit-reversed order).  "Transposed" = after an all-to-all of the block viewed as G chunks of M/G elements.
 *   phase 0: a, b, c transposed      -> cross stages of FFTInverse(DIF)                         -> transpose back
 *   phase 1: a, b, c blocks          -> block part of FFTInverse(DIF), *1/D*g^bitrev(i), block part of FFT(DIT, coset) -> transpose
 *   phase 2: a, b, c transposed      -> cross stages of FFT(DIT); a = (a*b - c)/(g^D - 1); cross stages of FFTInverse(DIF) -> transpose a back
 *   phase 3: a block                 -> block part of FFTInverse(DIF, coset): a is this rank's block of h.
 * Phases 0 and 1 act on each array independently and skip null pointers; phase 2 = phase 4 (cross stages of FFT(DIT), per array) followed by
 * phase 5 (the pointwise step and the final cross stages, all three arrays) -- so that the host can pipeline the transposes of b, c under the
 * stages of a (parallel.compute_h_sharded(pipelined=True): async collectives, one array ahead).
 * The six-transform schedule (default of parallel.compute_h_sharded; exact by linearity): c stays in coefficient form --
 *   phase 6: blocks given (c)    -> rest of FFTInverse(DIF) with 1/D: block of the coefficients, bit-reversed order (no further transpose of c)
 *   phase 7: a, b transposed, after phase 4 on each -> a = a*b; cross stages of FFTInverse(DIF) on a            -> transpose a back
 *   phase 8: a block + c block   -> block part of FFTInverse(DIF, coset) on a; a = (a - c)/(g^D - 1): this rank's block of h.
 *   Order: transpose a, b, c; 0 each; transpose each; 1 on a, b and 6 on c; transpose a, b; 4 on a, b; 7; transpose a; 8  -- 9 transposes instead of 10.
 * log_g = 0 degenerates to zk_bn254_groth16_compute_h_dev (no exchange).  In place; asynchronous on `stream` if given. */
int zk_bn254_groth16_h_shard_dev(int phase, void *d_a, void *d_b, void *d_c, uint32_t log_D, uint32_t log_g,
                                 uint32_t rank, void *stream);

/* A standalone (*Domain).FFT / FFTInverse sharded by blocks over G = 2^log_g GPUs (BASELINE configs[4] on several GPUs; the decomposition of the sharded
 * computeH above, for any of the eight mode combinations).  Rank rho holds block rho of the STORED order (natural for DIF input / DIT output, bit-reversed for
 * DIF output / DIT input); the library never communicates -- the host runs the steps with its all-to-all transposes (X) in between:
 *     FFT(DIF):        [2 if coset]  X  0  X  1              FFT(DIT):         1  X  0  X
 *     FFTInverse(DIF):               X  0  X  1              FFTInverse(DIT):  1  X  0  X  [2 if coset]
 *   step 0: the log_g cross stages on TRANSPOSED data;  step 1: the size-M transform of the block, with 1/D and the coset factors that can ride on it;
 *   step 2: the coset factor g^(+-i) on the natural-order block where it cannot (a no-op in the other modes).  log_g <= 3; in place; asynchronous on
 *   `stream` if given.  noir_backend_using_gnark_amd/parallel.py: ntt_sharded. */
int zk_bn254_ntt_shard_dev(int step, void *d_a, uint32_t log_D, uint32_t log_g, uint32_t rank, int inverse, int decimation, int coset,
                           void *stream);

/* ProvingKey image (host pointers; copied to the device by zk_bn254_groth16_pk_load).  Same field names as gnark's
 * groth16.ProvingKey{G1{Alpha,Beta,Delta,A,B,K,Z}, G2{Beta,Delta,B}, InfinityA, InfinityB, NbInfinityA, NbInfinityB}
 * (gnark v0.8.0 internal/backend/bn254/groth16/setup.go; the reference reaches it at gnark_backend_ffi/main.go:121,131 and
 * meant to pass it through backend/groth16/r1cs.go:107-143).
 *   - gnark's layout: infinity_a / infinity_b point at the []bool images (one byte per wire, != 0: that wire's point is the point
 *     at infinity and is NOT stored); g1_a then holds n_wires - nb_infinity_a points, g1_b and g2_b n_wires - nb_infinity_b,
 *     exactly the slices gnark keeps.  pk_load expands them on the device (one scatter kernel) to wire-indexed arrays, so the
 *     prover reads the full wire vector and needs no per-MSM filtering of the scalars.
 *   - dense layout: infinity_a == infinity_b == NULL; g1_a / g1_b / g2_b have n_wires entries, (0,0) = infinity contributes nothing.
 * K has n_wires - n_public entries; Z has 2^log_domain entries in gnark's (bit-reversed) order, N-1 are used. */
typedef struct {
    uint32_t log_domain;
    size_t n_wires, n_public;
    const zk_g1_affine *g1_alpha, *g1_beta, *g1_delta;
    const zk_g1_affine *g1_a, *g1_b, *g1_k, *g1_z;
    const zk_g2_affine *g2_beta, *g2_delta;
    const zk_g2_affine *g2_b;
    int bases_on_device; /* 1: g1_a, g1_b, g1_k, g1_z, g2_b are DEVICE pointers that stay owned by the caller */
    int flags;           /* bit 0: do NOT build the precomputed window tables 2^(c*w)*P_i (they cost ~13x the bases in HBM and
                            are what makes the resident-key MSMs ~20% cheaper; skipped automatically when HBM is short)
                            bit 1: all 2^log_domain entries of Z are used (a non-final slice of a range-sharded key)
                            bit 2: WINDOW-sharded key (BASELINE north_star / configs[2] wording): the key holds ALL wires, but its window
                                   tables only the rows w = shard_rank + k * shard_count of the ceil(255/c) digit windows -- 1/shard_count
                                   of the table memory; zk_bn254_groth16_msm5_pk then returns the partial sums over those windows of
                                   the FULL wire / h vectors, and the records of all ranks finalize as in the range-sharded mode.
                                   Needs the tables (an error when they do not fit). */
    const uint8_t *infinity_a, *infinity_b; /* gnark's InfinityA / InfinityB ([]bool, HOST pointers, n_wires bytes) or NULL */
    size_t nb_infinity_a, nb_infinity_b;    /* gnark's NbInfinityA / NbInfinityB; must equal the number of non-zero bytes */
    int table_window_bits;                  /* 0: planner's choice; else the window width c in [8, 24] of the tables */
    int device_mask;                        /* several GPUs in ONE process: bit i = device entry i holds a range slice of the key (2, 4 or 8 entries);
                                               0 = the process default.  zk_bn254_groth16_prove on such a key runs computeH block-sharded over the
                                               entries and the five MSMs per slice; same proof bytes. */
    uint32_t shard_rank, shard_count;       /* flags bit 2: this rank and the number of ranks (window sharding) */
} zk_groth16_pk;
int zk_bn254_groth16_pk_load(const zk_groth16_pk *pk, uint64_t *handle);
int zk_bn254_groth16_pk_free(uint64_t handle);   /* ZK_ERR_HANDLE while an msm5 session still uses the key */
/* Geometry of a loaded key (any out pointer may be NULL): lets a caller validate len(w) before handing a bare pointer over. */
int zk_bn254_groth16_pk_info(uint64_t handle, size_t *n_wires, size_t *n_public, uint32_t *log_domain, int *has_tables);
/* Window tables for a resident key that was loaded without them (flags bit 0): what a caller does once a key turns out to be used again -- the export path
 * (zk_groth16_prove_with_pk) reads a key text without tables for its first proof and builds them when the second is asked for.  table_window_bits: 0 = the
 * planner's choice, else [8, 24].  A key that has its tables already, or whose tables do not fit, is left as it is: *built (optional) = 1 / 0. */
int zk_bn254_groth16_pk_build_tables(uint64_t handle, int table_window_bits, int *built);
/* HBM held by a resident Groth16 key (the base arrays it owns + its window tables) */
int zk_bn254_groth16_pk_bytes(uint64_t handle, size_t *bytes);
/* Prove with the prover randomness (r, s) as INPUTS (upstream draws them from crypto/rand; pinning them is what
 * makes "bit-exact proof bytes" well defined).  a, b, c: n_constraints evaluations (solver output); w: n_wires wire
 * values; all Montgomery fr.Element.  proof_out = Ar | Bs | Krs in gnark's compressed encoding (32+64+32 bytes),
 * i.e. Proof.WriteTo.  `on_device` != 0: a, b, c, w are device pointers. */
int zk_bn254_groth16_prove(uint64_t pk_handle, const void *a, const void *b, const void *c, size_t n_constraints,
                           const void *w, size_t n_wires, const zk_fr *r, const zk_fr *s, int on_device, uint8_t proof_out[128]);
/* n_wires = len(w): must equal the key's wire count (ZK_ERR_LEN otherwise -- the library reads exactly that many elements). */

/* ---- R1CS on the device: groth16.Setup and the solver's a, b, c (gnark v0.8.0; reference: groth16.Setup at gnark_backend_ffi/main.go:121, the
 * R1CS the reference meant to build from Noir's RawR1CS at backend/groth16/r1cs.go:9-72) ------------------------------------------------------
 * L, R, O: sparse matrices by constraint (CSR: *_ptr has n_constraints + 1 entries starting at 0, *_idx wire ids, *_val Montgomery
 * coefficients); wires = [ONE, public..., secret..., internal...], n_public counts the ONE wire like gnark's GetNbPublicVariables(). */
typedef struct {
    size_t n_constraints, n_wires, n_public;
    const uint32_t *l_ptr, *l_idx; const zk_fr *l_val;
    const uint32_t *r_ptr, *r_idx; const zk_fr *r_val;
    const uint32_t *o_ptr, *o_idx; const zk_fr *o_val;
} zk_r1cs;
int zk_bn254_r1cs_load(const zk_r1cs *r1cs, uint64_t *handle);
int zk_bn254_r1cs_free(uint64_t handle);
/* a = L w, b = R w, c = O w: what r1cs.Solve leaves for a system without hints (one lane per matrix row); device pointers. */
int zk_bn254_r1cs_eval_abc_dev(uint64_t handle, const void *d_w, size_t n_wires, void *d_a, void *d_b, void *d_c, void *stream);
/* The same for `rows` wire vectors in ONE launch -- the launch zk_bn254_groth16_prove_r1cs_batch makes for a step of its rows.  d_w: rows x n_wires elements,
 * row-major (row z at d_w + z * n_wires), only read; d_a, d_b, d_c: rows x n_constraints elements each, row z at offset z * n_constraints, every element
 * written and nothing beyond.  Device pointers, all Montgomery fr.Element.  rows == 0: ZK_OK, nothing touched.  At most 65535 rows per call (the row is a grid
 * dimension): more is ZK_ERR_ARG and nothing is written.  Other errors as above: ZK_ERR_ARG null pointer, ZK_ERR_HANDLE, ZK_ERR_LEN n_wires. */
int zk_bn254_r1cs_eval_abc_rows_dev(uint64_t handle, const void *d_w, size_t n_wires, size_t rows, void *d_a, void *d_b, void *d_c, void *stream);
/* groth16.Setup with the toxic waste (tau, alpha, beta, gamma, delta; Montgomery, non-zero) as INPUT -- upstream draws it; pinning it is what
 * makes a key reproducible.  The key is built in HBM (Lagrange basis at tau, transposed products, fixed-base scalar multiplications) and comes
 * back as a resident proving key; vk_g1 (1 + n_public points: [alpha]G1, then K_i / gamma) and vk_g2 ([beta]G2, [gamma]G2, [delta]G2) on
 * the host.  flags bit 0: no window tables. */
int zk_bn254_groth16_setup(uint64_t r1cs_handle, const zk_fr toxic[5], int flags, uint64_t *pk_handle, zk_g1_affine *vk_g1,
                           zk_g2_affine vk_g2[3]);
/* groth16.Prove from the witness: a, b, c by the device solver step above, then zk_bn254_groth16_prove on resident data. */
int zk_bn254_groth16_prove_r1cs(uint64_t r1cs_handle, uint64_t pk_handle, const void *w, size_t n_wires, const zk_fr *r,
                                const zk_fr *s, int on_device, uint8_t proof_out[128]);
/* Many witnesses against ONE key in one call.  a, b, c: row-major n_proofs x n_constraints; w: row-major n_proofs x n_wires; r, s: n_proofs elements each
 * (all Montgomery fr.Element; on_device != 0: a, b, c, w are device pointers, only read).  proofs_out[128 i .. 128 i + 128) is byte for byte what
 * zk_bn254_groth16_prove / zk_bn254_groth16_prove_r1cs writes for row i with r[i], s[i] -- whichever path the call takes: a single-device key with its window
 * tables and log_domain <= 16 is served by a batched path (the rows of a chunk share one scalar preparation, one accumulate launch per base array and one
 * reduction; csrc/groth16_batch.hip), every other key row by row by the single prover.  n_proofs == 0: ZK_OK, nothing written.  Errors are the single prover's
 * (ZK_ERR_ARG null pointer / n_constraints above the domain, ZK_ERR_LEN len(w), ZK_ERR_HANDLE), checked before the device is touched where they can be; on any
 * error proofs_out is unspecified. */
int zk_bn254_groth16_prove_batch(uint64_t pk_handle, const void *a, const void *b, const void *c, size_t n_constraints, const void *w,
                                 size_t n_wires, const zk_fr *r, const zk_fr *s, size_t n_proofs, int on_device, uint8_t *proofs_out);
int zk_bn254_groth16_prove_r1cs_batch(uint64_t r1cs_handle, uint64_t pk_handle, const void *w, size_t n_wires, const zk_fr *r,
                                      const zk_fr *s, size_t n_proofs, int on_device, uint8_t *proofs_out);
/* Rows per chunk of the batched path for this key (a function of its geometry and the call's 1 GiB workspace), and whether the batched path serves the key at
 * all (*batched = 0: rows go through the single prover, *chunk_rows = 1).  Either out pointer may be NULL. */
int zk_bn254_groth16_batch_info(uint64_t pk_handle, size_t *chunk_rows, int *batched);

/* ---- Groth16 key wire formats (gnark v0.8.0 groth16 marshal.go): what the reference's intended Groth16 FFI moves as hex --
 * ProveWithPK(rawR1CS, encodedProvingKey) -> provingKey.ReadFrom at gnark_backend_ffi/backend/groth16/r1cs.go:107-143; Preprocess -> both keys at
 * r1cs.go:214-266.  ProvingKey.WriteTo (compressed points): Domain 168 B | G1.Alpha, Beta, Delta | G1.A, G1.B, G1.Z, G1.K (u32 count + 32 B each) |
 * G2.Beta, Delta | G2.B (u32 count + 64 B each) | nbWires, NbInfinityA, NbInfinityB (u64) | InfinityA, InfinityB (nbWires bytes each).
 *   pk_read : every point is decompressed ON THE DEVICE (G1: one square root; G2: an Fp2 square root + the r-torsion check gnark-crypto's Decoder
 *             applies), then the key is loaded like zk_bn254_groth16_pk_load's gnark layout.  flags: bit 0 = no window tables.
 *   pk_write: out == NULL only returns the size in *out_len.  A / B / G2.B leave without their points at infinity.
 *   vk_write: VerifyingKey.WriteTo = [alpha]1 [beta]1 [beta]2 [gamma]2 [delta]1 [delta]2 u32 len(K) K, from zk_bn254_groth16_setup's vk_g1 (n_k =
 *             n_public points after [alpha]1) / vk_g2 and the resident key. */
int zk_bn254_groth16_pk_read(const void *data, size_t len, int is_hex, int flags, int table_window_bits, uint64_t *handle);
int zk_bn254_groth16_pk_write(uint64_t handle, int as_hex, void *out, size_t cap, size_t *out_len);
int zk_bn254_groth16_vk_write(uint64_t pk_handle, const zk_g1_affine *vk_g1, size_t n_k, const zk_g2_affine vk_g2[3], int as_hex, void *out,
                              size_t cap, size_t *out_len);

/* ---- Verification on the HOST (SURVEY 8f keeps it last: O(1) next to a proof, no device work, ~10 ms on one core) -- the counterpart of the reference's
 * PlonkVerifyWithVK (gnark_backend_ffi/main.go:44-56 -> backend/plonk/plonk.go:28-51) and of the intended Groth16 VerifyWithVK (backend/groth16/r1cs.go:176-212).
 * Inputs are gnark's wire images (Proof.WriteTo, VerifyingKey.WriteTo as bytes or hex text) and the public witness as Montgomery fr.Elements (Groth16: without
 * the constant wire).  *accepted = 1 / 0 for well-formed inputs; what gnark's ReadFrom rejects is ZK_ERR_ARG / ZK_ERR_LEN.
 *   zk_bn254_groth16_verify : e(Ar, Bs) == e(alpha, beta) e(sum w_i K_i, gamma) e(Krs, delta)
 *   zk_bn254_plonk_verify   : gnark v0.8.0 plonk.Verify -- challenges from the SHA-256 transcript, quotient identity at zeta, two KZG checks against
 *                             srs_g2 = the SRS's ([1]2, [alpha]2) (zk_bn254_kzg_srs_read / _new_srs_dev return them)
 *   zk_bn254_pairing_check  : prod_i e(p_i, q_i) == 1 (optimal ate over the host field types; building block of the two above) */
int zk_bn254_groth16_verify(const uint8_t proof[128], const void *vk, size_t vk_len, int vk_is_hex, const zk_fr *public_inputs, size_t n_public,
                            int *accepted);
int zk_bn254_plonk_verify(const uint8_t proof[548] /* ZK_PLONK_PROOF_BYTES */, const void *vk, size_t vk_len, int vk_is_hex, const zk_g2_affine srs_g2[2],
                          const zk_fr *public_inputs, size_t n_public, int *accepted);
int zk_bn254_pairing_check(const zk_g1_affine *p, const zk_g2_affine *q, size_t n, int *is_one);

/* ---- Pairings and batch Groth16 / PLONK verification on the DEVICE.
 * zk_gt is bn254.GT's memory image: E12 {C0 E6{B0, B1, B2}, C1 E6{...}}, each E2 {A0, A1}, Montgomery (384 bytes) -- gnark's tower Fp6 = Fp2[v]/(v^3 - xi),
 * Fp12 = Fp6[w]/(w^2 - v), xi = 9 + u.
 *   zk_bn254_pair      : prod_i e(p_i, q_i), the reduced optimal ate pairing, exactly f^((q^12 - 1) / r) with f = prod_i of the Miller values of the host
 *                        pairing (csrc/pairing.hpp); computed on the device (one Miller loop per lane, a product tree, one final exponentiation).
 *   zk_bn254_pair_host : the same value on the host (pairing.hpp).  n == 0 gives one; a point at infinity on either side contributes one.  Inputs are
 *                        affine Montgomery images and are not validated (as zk_bn254_pairing_check).  The value is NOT claimed to equal gnark-crypto's
 *                        bn254.Pair: its final exponentiation may compute a fixed power of this one; products tested against one agree either way.
 *   zk_bn254_groth16_verify_batch : groth16.Verify for n_proofs proofs (n_proofs x 128 bytes, Proof.WriteTo) against ONE verifying key (bytes or hex);
 *                        public_inputs: n_proofs x n_public Montgomery fr.Elements, row-major, without the constant wire.  accepted[i] equals what
 *                        zk_bn254_groth16_verify says of proof i, except that a malformed proof encoding (flags, x >= q, no square root, a G2 point outside
 *                        the r-torsion) -- ZK_ERR_ARG there -- is a 0 here and does not affect the other proofs.  *n_accepted = the number of ones.
 *                        A malformed key is ZK_ERR_ARG / ZK_ERR_LEN, n_public + 1 != len(K) is ZK_ERR_LEN, as in the host verifier.
 *                        The valid proofs are first checked together: one random linear combination with r_i = the low 128 bits of
 *                        SHA-256("zkmi-groth16-batch" || SHA-256(vk bytes) || SHA-256(proofs || public inputs) || u64 i little-endian), forced non-zero --
 *                        derived, not random, so results are reproducible; a batch with an invalid proof passes with probability about 2^-128 in the
 *                        random-oracle model.  If that check fails, every valid proof is checked on its own on the device.  Proofs go through in chunks of
 *                        at most 2^16; the device workspace is about 5 KB + 96 (n_public + 1) bytes per proof of a chunk.
 *   zk_bn254_plonk_verify_batch : plonk.Verify for n_proofs proofs (n_proofs x 548 bytes, Proof.WriteTo) against ONE verifying key (368 bytes, bytes or hex)
 *                        and the SRS's srs_g2 = ([1]2, [alpha]2); public_inputs: n_proofs x n_public Montgomery fr.Elements, row-major.  accepted[i] equals
 *                        what zk_bn254_plonk_verify says of proof i, except that a malformed proof (an invalid point encoding, a batched-opening count other
 *                        than 7) -- ZK_ERR_ARG there -- is a 0 here and does not affect the other proofs.  Claimed values are reduced mod r (fr.SetBytes), as
 *                        on the host.  A malformed key, and n_public != NbPublicVariables, are ZK_ERR_ARG / ZK_ERR_LEN with the host verifier's messages.
 *                        Each proof's transcript, quotient identity and folded KZG opening are computed on the device, one lane per proof; a proof that
 *                        fails its quotient identity is rejected there.  The 2 n KZG openings of the remaining n proofs are then checked together:
 *                        e(sum_i rho_i (D_i - e_i G + zeta_i W_i) + rho'_i (Z_i - zu_i G + zeta_i omega W'_i), [1]2) e(-sum_i rho_i W_i + rho'_i W'_i, [alpha]2)
 *                        == 1 -- two Miller loops whatever n is -- with rho_i, rho'_i = the low 128 bits of SHA-256("zkmi-plonk-batch" || SHA-256(vk bytes) ||
 *                        SHA-256(srs_g2) || SHA-256(proofs || public inputs) || u64 i little-endian || 0 / 1), forced non-zero.  If that check fails, every
 *                        remaining proof gets its own two-pairing check on the device.  Chunks of at most 2^16 proofs; the device workspace is about
 *                        8.4 KB + 32 n_public bytes per proof of a chunk.
 * The device entries return ZK_ERR_NO_DEVICE without a GPU, after argument validation; there is no CPU fallback. */
typedef struct { zk_fp c[12]; } zk_gt;
int zk_bn254_pair(const zk_g1_affine *p, const zk_g2_affine *q, size_t n, zk_gt *out);
int zk_bn254_pair_host(const zk_g1_affine *p, const zk_g2_affine *q, size_t n, zk_gt *out);
int zk_bn254_groth16_verify_batch(const uint8_t *proofs, size_t n_proofs, const void *vk, size_t vk_len, int vk_is_hex, const zk_fr *public_inputs,
                                  size_t n_public, uint8_t *accepted, size_t *n_accepted);
int zk_bn254_plonk_verify_batch(const uint8_t *proofs, size_t n_proofs, const void *vk, size_t vk_len, int vk_is_hex,
                                const zk_g2_affine srs_g2[2], const zk_fr *public_inputs, size_t n_public,
                                uint8_t *accepted, size_t *n_accepted);

/* The two batch verifiers for proofs and public inputs that already lie in HBM: nothing of them comes down but 32 bytes per row.
 *   d_proofs           device: row v's 128 (548) bytes at d_proofs + v * proof_stride bytes; any stride >= the row (the gap is not read), any alignment.
 *   d_public_inputs    device: row v's n_public Montgomery fr.Elements at element v * pub_stride (pub_stride >= n_public; 4-byte aligned); may be NULL when
 *                      n_public == 0.
 *   vk, srs_g2, accepted, n_accepted   host, as in the entries above.
 * accepted[i] equals what zk_bn254_groth16_verify_batch / zk_bn254_plonk_verify_batch says for the same bytes: a malformed proof encoding is a 0 and does not
 * touch its neighbours; a malformed key and a wrong n_public give the same codes and messages, decided before a device is looked for, as are a null pointer and
 * a stride below its row with more than one row (ZK_ERR_ARG).  The checks, the chunks and the fallback are those of the entries above -- one core serves both
 * forms -- and only the coefficients' derivation differs, because the host never sees the rows:
 *   d_v    = SHA-256(row v's proof bytes || row v's 32 * n_public public-input bytes AS THEY LIE IN MEMORY -- the Montgomery images, little-endian limbs),
 *            one lane per row on the device (zk_bn254_rows_sha256_dev below);
 *   D      = SHA-256(d_0 || d_1 || ... || d_{n-1}) over ALL n_proofs rows of the call (not per chunk), on the host;
 *   r_i    = the low 128 bits of SHA-256("zkmi-groth16-batch-rows" || SHA-256(vk bytes) || D || u64 i little-endian), forced non-zero;
 *   rho_i, rho'_i = the low 128 bits of SHA-256("zkmi-plonk-batch-rows" || SHA-256(vk bytes) || SHA-256(srs_g2) || D || u64 i little-endian || 0 / 1), forced
 *            non-zero -- i counts over the whole call; "low 128 bits": the digest read as a big-endian integer, as above.
 * The host-input entries keep their derivation: the same proofs get other coefficients there and the same verdicts.
 *   zk_bn254_rows_sha256_dev : d_out[32 v ..] = SHA-256(a_v || b_v), a_v the a_len bytes at d_a + v * a_stride, b_v the b_len bytes at d_b + v * b_stride;
 *            either span may be empty (its pointer is then not read and may be NULL).  Everything in HBM, any alignment.  With `stream` the call only
 *            enqueues; stream == NULL runs on a stream of the library's and returns when the launch is complete.  A null pointer of a span that is read, a
 *            stride below its span with more than one row: ZK_ERR_ARG before a device is looked for; rows == 0: ZK_OK, nothing launched. */
int zk_bn254_groth16_verify_batch_dev(const void *d_proofs, size_t proof_stride, size_t n_proofs, const void *vk, size_t vk_len, int vk_is_hex,
                                      const void *d_public_inputs, size_t pub_stride, size_t n_public, uint8_t *accepted, size_t *n_accepted);
int zk_bn254_plonk_verify_batch_dev(const void *d_proofs, size_t proof_stride, size_t n_proofs, const void *vk, size_t vk_len, int vk_is_hex,
                                    const zk_g2_affine srs_g2[2], const void *d_public_inputs, size_t pub_stride, size_t n_public,
                                    uint8_t *accepted, size_t *n_accepted);
int zk_bn254_rows_sha256_dev(const void *d_a, size_t a_len, size_t a_stride, const void *d_b, size_t b_len, size_t b_stride, size_t rows,
                             void *d_out /* rows x 32 */, void *stream);

/* Batch PLONK verification against MANY verifying keys of one SRS in one call (DESIGN 3.10 "Many keys"): row i is a proof for vks[key_of[i]].  All keys made
 * from one SRS share srs_g2 = ([1]2, [alpha]2), so the combined opening check above stays ONE product of two pairings when every lane reads its own key
 * (S1..Qk, n, omega, u, n_public, the transcript's prefix): the two Miller loops and the final exponentiation are paid once per call, not once per key.
 *   vks, vk_lens       host: n_keys keys, each 368 bytes (vk_is_hex == 0) or their hex text (all keys in the same form).  Keys may differ in domain size,
 *                      n_public and every point; a key no row refers to is parsed and otherwise unused; the same key may be given twice.
 *   key_of             HOST memory in both forms: n_proofs indices below n_keys.
 *   public_inputs      row i's inputs are the first n_public(key_of[i]) Montgomery fr.Elements at element i * pub_stride -- host memory, packed with that
 *   / d_public_inputs  stride, in the first form; device memory in the _dev form.  Nothing beyond them is read, neither for the verdict nor for the
 *                      coefficients.  May be NULL when every key has n_public 0.
 *   d_proofs           device: row v's 548 bytes at d_proofs + v * proof_stride, any stride >= 548, any alignment.
 * accepted[i] equals what zk_bn254_plonk_verify says of (proof i, vks[key_of[i]], srs_g2, its public inputs), except that a malformed proof is a 0 and touches
 * no other row, as in zk_bn254_plonk_verify_batch; with n_keys == 1 the verdicts are that entry's for the same rows (the coefficients are not).
 * *n_accepted = the number of ones.
 * Decided before a device is looked for, each leaving *n_accepted = 0: ZK_ERR_ARG for a null pointer that is read, n_keys == 0 with n_proofs > 0, a
 * key_of[i] >= n_keys (the message names the row and the value), proof_stride < 548 with more than one row; ZK_ERR_LEN for pub_stride below the largest
 * n_public among the keys with more than one row; a malformed key j gives the host verifier's code and message with "key j: " in front.  n_proofs == 0 is
 * ZK_OK: the keys are still parsed, nothing is launched.  Without a GPU: ZK_ERR_NO_DEVICE, after the above.
 * The coefficients stay derived: rho_i, rho'_i = the low 128 bits of SHA-256(prefix || u64 i little-endian || 0 / 1), forced non-zero, i counting over the
 * whole call, with
 *   KD     = SHA-256(u64 n_keys little-endian || SHA-256(vk_0 bytes) || ... || SHA-256(vk_{K-1} bytes) || key_of as n_proofs little-endian u32), "vk bytes" the
 *            368-byte image (hex text decoded);
 *   host form    prefix = "zkmi-plonk-batch-keys" || KD || SHA-256(srs_g2) || SHA-256(proofs || row 0's n_public(key_of[0]) public inputs || row 1's || ...)
 *                -- the Montgomery images as they lie, only the used ones (117 bytes);
 *   device form  prefix = "zkmi-plonk-batch-keys-rows" || KD || SHA-256(srs_g2) || D (122 bytes), D = SHA-256(d_0 || ... || d_{n-1}) on the host and
 *                d_v = SHA-256(row v's 548 bytes || its 32 * n_public(key_of[v]) public-input bytes as they lie in memory), one lane per row on the device.
 * Chunks of at most 2^16 proofs; the device workspace is about 8.7 KB per proof of a chunk, the public inputs of a chunk at their stride in the host form,
 * 752 bytes per key and 4 (device form: 36) bytes per row of the call. */
int zk_bn254_plonk_verify_batch_keys(const uint8_t *proofs, size_t n_proofs,
        const void *const *vks, const size_t *vk_lens, size_t n_keys, int vk_is_hex,
        const zk_g2_affine srs_g2[2], const uint32_t *key_of /* host, n_proofs */,
        const zk_fr *public_inputs, size_t pub_stride,
        uint8_t *accepted, size_t *n_accepted);
int zk_bn254_plonk_verify_batch_keys_dev(const void *d_proofs, size_t proof_stride, size_t n_proofs,
        const void *const *vks, const size_t *vk_lens, size_t n_keys, int vk_is_hex,
        const zk_g2_affine srs_g2[2], const uint32_t *key_of /* host */,
        const void *d_public_inputs, size_t pub_stride,
        uint8_t *accepted, size_t *n_accepted);

/* Batch Groth16 verification against MANY verifying keys in one call (DESIGN 3.9 "Many keys"): row i is a proof for vks[key_of[i]].  Groth16 keys share
 * nothing -- each has its own alpha, beta, gamma, delta and K table -- so a chunk's check is
 *   prod_i e(r_i Ar_i, Bs_i)  prod_{k used} e(-c_k0 alpha_k, beta_k) e(-sum_j c_kj K_kj, gamma_k) e(-sum_{i: key_of[i] = k} r_i Krs_i, delta_k) == 1,
 *   c_kj = sum_{i: key_of[i] = k, i valid} r_i w_ij (w_i0 = 1):
 * n + 3 K_used Miller loops, one product tree and ONE final exponentiation per chunk instead of one per key.  The per-key sums and the 3 K_used fixed terms
 * are made on the device; the host only sorts the chunk's lanes by key.  If the check fails, every valid proof gets its own four-pairing check under its key.
 *   vks, vk_lens       host: n_keys keys, VerifyingKey.WriteTo bytes (vk_is_hex == 0) or their hex text (all keys in the same form).  Keys may differ in
 *                      n_public and every point; a key no row refers to is parsed and otherwise unused; the same key may be given twice.
 *   key_of             HOST memory in both forms: n_proofs indices below n_keys.
 *   public_inputs      row i's inputs are the first n_public(key_of[i]) Montgomery fr.Elements at element i * pub_stride -- host memory, packed with that
 *   / d_public_inputs  stride, in the first form; device memory in the _dev form.  Nothing beyond them is read, neither for the verdict nor for the
 *                      coefficients.  May be NULL when every key has n_public 0.
 *   d_proofs           device: row v's 128 bytes at d_proofs + v * proof_stride, any stride >= 128, any alignment.
 * accepted[i] equals what zk_bn254_groth16_verify says of (proof i, vks[key_of[i]], its public inputs), except that a malformed proof encoding is a 0 and
 * touches no other row, as in zk_bn254_groth16_verify_batch; with n_keys == 1 the verdicts are that entry's for the same rows (the coefficients are not).
 * *n_accepted = the number of ones.
 * Decided before a device is looked for, each leaving *n_accepted = 0: ZK_ERR_ARG for a null pointer that is read, n_keys == 0 with n_proofs > 0, a
 * key_of[i] >= n_keys (the message names the row and the value), proof_stride < 128 with more than one row; ZK_ERR_LEN for pub_stride below the largest
 * n_public among the keys with more than one row; a malformed key j gives the host verifier's code and message with "key j: " in front.  n_proofs == 0 is
 * ZK_OK: the keys are still parsed, nothing is launched.  Without a GPU: ZK_ERR_NO_DEVICE, after the above.
 * The coefficients stay derived: r_i = the low 128 bits of SHA-256(prefix || u64 i little-endian), forced non-zero, i counting over the whole call, with
 *   KD     = SHA-256(u64 n_keys little-endian || SHA-256(vk_0 bytes) || ... || SHA-256(vk_{K-1} bytes) || key_of as n_proofs little-endian u32), "vk bytes" the
 *            binary image (hex text decoded);
 *   host form    prefix = "zkmi-groth16-batch-keys" || KD || SHA-256(proofs || row 0's n_public(key_of[0]) public inputs || row 1's || ...) -- the
 *                Montgomery images as they lie, only the used ones;
 *   device form  prefix = "zkmi-groth16-batch-keys-rows" || KD || D, D = SHA-256(d_0 || ... || d_{n-1}) on the host and
 *                d_v = SHA-256(row v's 128 bytes || its 32 * n_public(key_of[v]) public-input bytes as they lie in memory), one lane per row on the device.
 * Chunks of at most 2^16 proofs; the device workspace is about 6 KB per proof of a chunk, the public inputs of a chunk at their stride in the host form,
 * 464 bytes per key, 64 bytes per K point of the keys, about 350 bytes per key used in a chunk and 4 (device form: 36) bytes per row of the call. */
int zk_bn254_groth16_verify_batch_keys(const uint8_t *proofs, size_t n_proofs,
        const void *const *vks, const size_t *vk_lens, size_t n_keys, int vk_is_hex,
        const uint32_t *key_of /* host, n_proofs */,
        const zk_fr *public_inputs, size_t pub_stride,
        uint8_t *accepted, size_t *n_accepted);
int zk_bn254_groth16_verify_batch_keys_dev(const void *d_proofs, size_t proof_stride, size_t n_proofs,
        const void *const *vks, const size_t *vk_lens, size_t n_keys, int vk_is_hex,
        const uint32_t *key_of /* host */,
        const void *d_public_inputs, size_t pub_stride,
        uint8_t *accepted, size_t *n_accepted);

/* The two halves of zk_bn254_groth16_prove, exposed so that one proof can be range-sharded over several GPUs
 * (one process per GPU): every rank runs the five MSMs on ITS slice of the bases / wire values / h, the un-normalised
 * XYZZ sums (4 x G1 = 64 limbs, then G2 = 32 limbs; order A, B1, K, Z, B2) are all-gathered, and any rank finishes.
 *   msm5_dev : d_a, d_b (G1), d_b2 (G2) against d_w[0..nw); d_k against d_wk[0..nk); d_z against d_h[0..nz).
 *   finalize : sums n_partials x 96-limb records, adds alpha/beta/delta terms with (r, s), writes the 128-byte proof. */
int zk_bn254_groth16_msm5_dev(const void *d_a, const void *d_b, const void *d_b2, const void *d_w, size_t nw,
                              const void *d_k, const void *d_wk, size_t nk, const void *d_z, const void *d_h, size_t nz,
                              uint64_t out_xyzz[96], void *stream);
/* msm5 against a loaded key whose base arrays are THIS rank's slices (n_wires / n_public / log_domain describe the
 * slice; flags bit 1 on every rank but the last): uses the key's resident window tables.  d_w: n_wires wire values of
 * the slice, complete before the call (their preparation starts at once); d_h: this rank's block of h, awaited on
 * `stream` (the stream computeH was enqueued on) if given. */
int zk_bn254_groth16_msm5_pk(uint64_t pk_handle, const void *d_w, const void *d_h, uint64_t out_xyzz[96], void *stream);
/* The same in two calls: _begin starts the scalar-side preparation of the wire values at once (it does not need h), so it
 * runs while the host drives the sharded computeH and its exchanges; _end (always call it: it releases the session)
 * enqueues the rest behind `stream` and waits for the record. */
int zk_bn254_groth16_msm5_pk_begin(uint64_t pk_handle, const void *d_w, uint64_t *session);
int zk_bn254_groth16_msm5_pk_end(uint64_t session, const void *d_h, uint64_t out_xyzz[96], void *stream);
/* Gives a session up without finishing it (an exception between _begin and _end): waits for the work already enqueued and
 * releases the five stream slots.  Unknown / already ended sessions return ZK_ERR_HANDLE. */
int zk_bn254_groth16_msm5_pk_abort(uint64_t session);
/* The session's high-priority stream (valid until _end): run the sharded computeH and its exchanges on it -- that is the
 * stream zk_bn254_groth16_prove runs computeH on, and it never shares a hardware queue with the preparation of w. */
int zk_bn254_groth16_msm5_session_stream(uint64_t session, void **stream_out);
int zk_bn254_groth16_finalize(uint64_t pk_handle, const uint64_t *partials, size_t n_partials, const zk_fr *r,
                              const zk_fr *s, uint8_t proof_out[128]);
/* finalize for MANY rows in one device launch (csrc/groth16_tail.hip): one lane group per row sums the row's records, multiplies delta / delta2 through the
 * key's 8-bit window tables in HBM (built at the key's first call, freed with the key, counted by zk_bn254_groth16_pk_bytes), computes s*(A + alpha) and
 * r*(B1 + beta), shares one inversion among the three proof elements and compresses them.
 * n_proofs rows; partials: row-major n_proofs x n_partials x 96 limbs; r, s: n_proofs elements; proofs_out: 128 bytes per row.
 * proofs_out[128 i ..] is byte for byte what zk_bn254_groth16_finalize writes for row i.
 * n_proofs == 0: ZK_OK, nothing written.  A null pointer or n_partials == 0: ZK_ERR_ARG; an unknown key: ZK_ERR_HANDLE.  A key spread over several device
 * entries finalizes row by row on the host from the host form; the _dev form refuses it with ZK_ERR_ARG.  _dev with `stream`: enqueued behind it, returns
 * without a sync; with stream == NULL: on a stream of the library's own, returns when the bytes are there.  Both may be called from concurrent threads. */
int zk_bn254_groth16_finalize_batch(uint64_t pk_handle, const uint64_t *partials, size_t n_partials, const zk_fr *r, const zk_fr *s,
                                    size_t n_proofs, uint8_t *proofs_out);                      /* host pointers */
int zk_bn254_groth16_finalize_batch_dev(uint64_t pk_handle, const void *d_partials, size_t n_partials, const void *d_r, const void *d_s,
                                        size_t n_proofs, void *d_proofs_out, void *stream);      /* device pointers; inputs only read */

/* ---- PLONK: plonk.Setup / plonk.Prove (gnark v0.8.0 internal/backend/bn254/plonk/{setup,prove}.go) ------------------------------
 * The reference's only live prove path: PlonkProveWithPK (gnark_backend_ffi/main.go:24-37) -> plonk.Prove at
 * backend/plonk/plonk.go:67; plonk.Setup at backend/plonk/plonk.go:21; the constraint system is one gate
 *     qL*xa + qR*xb + qO*xc + qM*xa*xb + qK == 0
 * per ACIR arithmetic opcode (backend/plonk/sparse_r1cs.go:44-107).  The commitments are kzg.Commit = one G1 MSM over the SRS
 * registered with zk_bn254_bases_register* (>= domain size + 3 points; kzg.NewSRS at backend/common.go:137); the transforms are the
 * fft.Domain calls above on the small domain n and the big domain 4n (8n below 6 gates).  Everything between the solver's output and
 * the 548 proof bytes runs on the device except the Fiat-Shamir hashes and a few G1 scalar multiplications. */
typedef struct {
    size_t n_public, n_constraints, n_vars; /* spr.NbPublicVariables, len(spr.Constraints), number of variables (public first) */
    const void *ql, *qr, *qo, *qm, *qk;     /* n_constraints fr.Elements each (Montgomery); host pointers unless coeffs_on_device */
    const uint32_t *xa, *xb, *xc;           /* wire ids of every gate (HOST pointers) */
    int coeffs_on_device;
    int reserved;
} zk_plonk_circuit;
/* gnark's ProvingKey as plonk.Setup / ProvingKey.ReadFrom leave it: canonical (regular) Ql, Qr, Qm, Qo, CQk, S1..S3Canonical and LQk of
 * 2^log_n entries each, Permutation of 3 * 2^log_n entries, the verifying key's digests -- plus the gates' wire ids (from the spr). */
typedef struct {
    uint32_t log_n;
    size_t n_public, n_constraints, n_vars;
    const zk_fr *ql, *qr, *qm, *qo, *cqk, *lqk, *s1, *s2, *s3;
    const int64_t *permutation;
    const uint32_t *xa, *xb, *xc;
    const zk_g1_affine *vk_s /* [3] */, *vk_ql, *vk_qr, *vk_qm, *vk_qo, *vk_qk;
} zk_plonk_pk;
typedef struct {                 /* plonk.VerifyingKey (without the SRS) */
    uint64_t size, n_public;     /* Domain[0].Cardinality, NbPublicVariables */
    zk_fr size_inv, generator, coset_shift;
    zk_g1_affine s[3], ql, qr, qm, qo, qk;
} zk_plonk_vk;
int zk_bn254_plonk_setup(const zk_plonk_circuit *circuit, uint64_t srs_handle, uint64_t *pk_handle, zk_plonk_vk *vk_out);
int zk_bn254_plonk_pk_load(const zk_plonk_pk *pk, uint64_t srs_handle, uint64_t *pk_handle);
int zk_bn254_plonk_pk_free(uint64_t pk_handle);
/* The SRS in LAGRANGE form over this key's domain, built once ([L_i(tau)] = the inverse transform of the SRS "in the exponent": n/2 log2 n + n point-by-scalar
 * multiplications -- 0.15 s at 2^19 gates, 1.3 s at 2^22).  From then on zk_bn254_plonk_prove commits l, r, o from the WIRE VALUES: the same three digests
 * (sum_i l_i [L_i(tau)] + b0 [tau^n - 1] + b1 [tau^(n+1) - tau] is kzg.Commit of the blinded coefficients), from scalars that are bits and words in any real circuit
 * instead of uniform field elements -- a quarter to a third of the additions -- and without waiting for the three inverse transforms.  For a prover that keeps its
 * key (a process that makes one proof should not call it); needs the SRS on one device entry.  A key that has it: ZK_OK, untouched. */
int zk_bn254_plonk_pk_lagrange_srs(uint64_t pk_handle);
/* plonk.ProvingKey.ReadFrom / WriteTo on gnark's bytes (is_hex / as_hex: the hex text the reference ships, internal/backend/helpers.go:49-60,
 * 82-87): verifying key | Domain[0] | Domain[1] | Ql Qr Qm Qo CQk LQk S1 S2 S3 (u32 BE length + 32 B BE elements) | Permutation (3n raw BE
 * int64).  The nine vectors are decoded / encoded on the device; the wire ids come from the spr the caller rebuilt (plonk.go:54). */
int zk_bn254_plonk_pk_read(const void *data, size_t len, int is_hex, size_t n_vars, size_t n_constraints, const uint32_t *xa,
                           const uint32_t *xb, const uint32_t *xc, uint64_t srs_handle, uint64_t *pk_handle);
int zk_bn254_plonk_pk_write(uint64_t pk_handle, int as_hex, void *out, size_t cap, size_t *out_len);
/* Shape of a resident key (any out pointer may be NULL): Domain[0].Cardinality, NbPublicVariables, number of gates, number of variables. */
int zk_bn254_plonk_pk_info(uint64_t pk_handle, size_t *domain_size, size_t *n_public, size_t *n_constraints, size_t *n_vars);
/* Canonical polynomials of a resident key, for inspection: which = 0..8 -> Ql, Qr, Qm, Qo, CQk, S1, S2, S3 (canonical), LQk; n entries. */
int zk_bn254_plonk_pk_export(uint64_t pk_handle, int which, zk_fr *out_host, size_t n);
enum { ZK_PLONK_PROOF_BYTES = 548 }; /* Proof.WriteTo: 7 x 32 B digests | 32 B + u32 count + 7 x 32 B | 32 B + 32 B */
/* plonk.Prove after the solver.  solution: n_vars values of all variables (public first; Montgomery; device pointer if on_device).
 * blinders: the 9 scalars upstream draws with fr.SetRandom -- Blind(1) of l, r, o (2 each) and Blind(2) of z (3) -- as INPUTS, which is
 * what makes the proof bytes reproducible.  challenges: NULL = SHA-256 Fiat-Shamir exactly as upstream (transcript "gamma", "beta",
 * "alpha", "zeta" + kzg's folding "gamma"); else 5 pinned values (gamma, beta, alpha, zeta, kzg gamma; Montgomery).
 * ZK_ERR_ARG when the solution does not satisfy the circuit (the quotient is not a polynomial; upstream fails in Solve). */
int zk_bn254_plonk_prove(uint64_t pk_handle, const void *solution, size_t n_vars, int on_device, const zk_fr blinders[9],
                         const zk_fr *challenges, uint8_t proof_out[ZK_PLONK_PROOF_BYTES]);
/* synthetic data (bench / tests): qk[i] = -(ql*a + qr*b + qo*c + qm*a*b) for gate i with a, b, c = solution[xa[i]], ... -- makes any
 * assignment of random coefficients and wires satisfiable.  All pointers are device pointers. */
int zk_bn254_plonk_synth_qk_dev(void *d_qk, const void *d_ql, const void *d_qr, const void *d_qo, const void *d_qm, const void *d_xa,
                                const void *d_xb, const void *d_xc, const void *d_solution, size_t n_constraints, void *stream);

/* ---- iop: the copy-constraint ratio (gnark-crypto ecc/bn254/fr/iop BuildRatioCopyConstraint, round 2 of plonk.Prove) for MANY witnesses of one domain -----
 * For `rows` triples l, r, o in Lagrange form, regular order, over the domain of 2^log_n points, and one permutation of the 3 * 2^log_n wire slots:
 *     num_i = prod_j (w_j(i) + beta u^j omega^i + gamma)        den_i = prod_j (w_j(i) + beta sigma_j(i) + gamma)        z[0] = 1,  z[i+1] = z[i] num_i / den_i
 * with u the domain's multiplicative generator (fft.Domain.FrMultiplicativeGen, as getSupportIdentityPermutation shifts the three copies) and sigma_j(i) =
 * id(perm[j n + i]), id(p) = u^(p / n) omega^(p mod n).  Z comes back in Lagrange form, regular order.  fr.BatchInvert's rule holds: the inverse of 0 is 0, so
 * a zero num_i or den_i makes every later z zero, as upstream's rolling products do.  Every row has its own challenges: beta[v], gamma[v].
 * Row v of l, r, o starts at element v * in_stride (in_stride >= n), row v of Z at element v * out_stride (out_stride >= n); the inputs are only read and
 * elements between the rows are not touched.  The row is a grid dimension: one launch per step for all rows (three launches in all up to n = 2^11, five
 * above), against five small launches per witness.  One row runs the five launches of zk_bn254_plonk_prove's own round 2, and row v of a batch is bit for bit
 * the one-row call on that row.
 * INPUT CONTRACT, each entry below: every field element in and out is a canonical fr.Element image in Montgomery form (< r); another 256-bit word gives an
 * undefined result.
 * ARGUMENT ERRORS, each entry below, decided before a device is looked for: a null pointer, log_n > 28, in_stride or out_stride below n, d_z overlapping an
 * input -> ZK_ERR_ARG; an unknown key -> ZK_ERR_HANDLE; rows == 0 (n == 0 for the inversion) -> ZK_OK, nothing happens.
 * STREAMS: the workspace of these entries is the slot's arena, which the next call reuses, so they synchronise `stream` (NULL: the slot's own) before they
 * return, as zk_bn254_groth16_compute_h_batch_dev does.  At most 1 GiB of workspace at a time: more rows than fit run in chunks.
 *   zk_bn254_iop_sigma_dev             3n uint32 positions (gnark's pk.Permutation, L | R | O) -> the 3n elements S1 | S2 | S3 in Lagrange form: sigma above.
 *                                      ZK_ERR_ARG if an entry is >= 3n (d_sigma is then undefined).
 *   zk_bn254_iop_ratio_copy_batch_dev  device rows; d_sigma as zk_bn254_iop_sigma_dev leaves it; d_beta, d_gamma: `rows` device elements each.
 *   zk_bn254_iop_ratio_copy_batch      host arrays, contiguous rows: l, r, o, z_out (rows, n); perm 3n positions; beta, gamma `rows` elements.
 *   zk_bn254_plonk_ratio_batch_dev     the same through a resident PLONK key: its permutation, its domain and that domain's twiddles (n = the key's domain).
 *   zk_bn254_fr_batch_invert_dev       fr.BatchInvert in place on n device elements: a[i] <- 1 / a[i], zeros stay zeros. */
int zk_bn254_iop_sigma_dev(const void *d_perm, uint32_t log_n, void *d_sigma, void *stream);
int zk_bn254_iop_ratio_copy_batch_dev(const void *d_l, const void *d_r, const void *d_o, size_t in_stride, uint32_t log_n, size_t rows, const void *d_sigma,
                                      const void *d_beta, const void *d_gamma, void *d_z, size_t out_stride, void *stream);
int zk_bn254_iop_ratio_copy_batch(const zk_fr *l, const zk_fr *r, const zk_fr *o, uint32_t log_n, size_t rows, const uint32_t *perm, const zk_fr *beta,
                                  const zk_fr *gamma, zk_fr *z_out);
int zk_bn254_plonk_ratio_batch_dev(uint64_t pk_handle, const void *d_l, const void *d_r, const void *d_o, size_t in_stride, size_t rows, const void *d_beta,
                                   const void *d_gamma, void *d_z, size_t out_stride, void *stream);
int zk_bn254_fr_batch_invert_dev(void *d_a, size_t n, void *stream);

/* ---- plonk: the quotient (round 3 of plonk.Prove: prove.go's evaluation of the constraints on the coset of the big domain, iop.DivideByXMinusOne, the
 * inverse coset transform) for MANY witnesses of one resident key -----
 * For `rows` witnesses of the key `pk_handle` (domain n, big domain N4 = 4n or 8n), each given by its blinded canonical l, r, o (n + 2 coefficients) and z
 * (n + 3), its public inputs and its own challenges alpha[v], beta[v], gamma[v]:
 *     h = [ gate + alpha (z(omega X) prod_j (w_j + beta S_j + gamma) - z prod_j (w_j + beta u^j X + gamma)) + alpha^2 (z - 1) L_1 ] / (X^n - 1)
 * with gate = ql l + qr r + qm l r + qo o + qk and qk completed with the row's public inputs, evaluated on the coset of the big domain and brought back to
 * canonical form, regular order: the 3 (n + 2) coefficients H[0] | H[1] | H[2] that zk_bn254_plonk_prove commits, bit for bit.
 * Row v of l, r, o, z starts at element v * in_stride (in_stride >= n + 3), its n_public public inputs at element v * pub_stride of d_pub (pub_stride >=
 * n_public; an array of solutions with pub_stride = n_vars works; d_pub may be NULL for a key without public inputs), its h at element v * out_stride
 * (out_stride >= 3 (n + 2)).  The inputs are only read; elements between the rows of d_h are not touched.
 * d_status: one int32 per row, written for EVERY row: 0, or 1 where the quotient is not a polynomial (some coefficient of h at or above 3 (n + 2) is non-zero:
 * the witness violates the constraints).  Such a row does not fail the call: the return code is ZK_OK, the row's 3 (n + 2) coefficients are still the
 * transform's, and every other row is unaffected.
 * The row is a grid dimension: one launch per step for all rows (spread, one transform over the 4 * rows polynomials, qk, the quotient kernel, the inverse
 * transform, the tail), whatever their number; one row is rows = 1 of the same launches.  Workspace: 5 * N4 elements per row (plus n where the key has more
 * than 32 public inputs) from the slot's arena, at most 1 GiB at a time: more rows run in chunks.  The key's per-proof workspace is not used, so calls on one
 * key overlap each other and a proof in flight.
 * INPUT CONTRACT: canonical fr.Element images in Montgomery form (< r), as above.
 * ARGUMENT ERRORS, decided before a device is looked for: a null pointer, in_stride < n + 3, pub_stride < n_public, out_stride < 3 (n + 2), d_h or d_status
 * overlapping an input or each other -> ZK_ERR_ARG; an unknown key -> ZK_ERR_HANDLE; rows == 0 -> ZK_OK, nothing happens.
 * STREAMS: synchronises `stream` (NULL: the slot's own) before it returns, like the entries above. */
int zk_bn254_plonk_quotient_batch_dev(uint64_t pk_handle, const void *d_l, const void *d_r, const void *d_o, const void *d_z, size_t in_stride, const void *d_pub,
                                      size_t pub_stride, size_t rows, const void *d_alpha, const void *d_beta, const void *d_gamma, void *d_h, size_t out_stride,
                                      void *d_status, void *stream);

/* ---- plonk: the openings (rounds 4 and 5 of plonk.Prove: the evaluations at zeta and omega zeta, kzg.Open of Z, computeLinearizedPolynomial, the folded
 * quotient, kzg.BatchOpenSinglePoint's fold and its division by X - zeta) for MANY witnesses of one resident key -----
 * The row is a grid dimension and every per-row challenge is read from a device array: the launches of a call do not depend on the number of rows (4, 7 and 5
 * per chunk for the three entries), nothing is copied to the host inside a call, and one row is rows = 1 of the same kernels, so row v of a call is bit for
 * bit the one-row call on that row.  The commitments of the outputs are the caller's.
 *   zk_bn254_fr_poly_open_rows_dev      the ingredient: for each row v, d_values[v] = f_v(a_v) with f_v the `len` coefficients (len >= 1) at d_f + v * in_stride
 *       (in_stride >= len) and a_v = d_points[v]; where d_q is not NULL, q_v = (f_v - f_v(a_v)) / (X - a_v) (kzg.dividePolyByXminusA), len - 1 coefficients
 *       at d_q + v * q_stride (q_stride >= len - 1; nothing when len == 1).  d_q may be NULL (evaluate only), d_f itself with q_stride == in_stride (in place:
 *       element len - 1 of each row stays as it was), or disjoint from d_f.  The Horner suffix scan in three passes on the plan K = max(8, ceil(len / 2^18))
 *       coefficients per lane, 256 lanes per workgroup; the powers a^K and a^(256 K) of a row's point are computed once per row.
 *   zk_bn254_plonk_linearize_batch_dev  round 4.  In, per row v: the blinded canonical l, r, o (n + 2 coefficients) and z (n + 3) at element v * in_stride
 *       (in_stride >= n + 3), the 3 (n + 2) coefficients H[0] | H[1] | H[2] that zk_bn254_plonk_quotient_batch_dev wrote at v * h_stride (h_stride >=
 *       3 (n + 2)), alpha[v], beta[v], gamma[v], zeta[v].  Out, per row v:
 *         d_values + 8 v          foldedH(zeta), lin(zeta), l(zeta), r(zeta), o(zeta), s1(zeta), s2(zeta), z(omega zeta): the proof's order
 *         d_zquot + v out_stride  the n + 2 coefficients of (z - z(omega zeta)) / (X - omega zeta)
 *         d_lin + v out_stride    the n + 3 coefficients of the linearised polynomial
 *                                   (alpha c_z + lag) z + alpha c_s3 s3 + l(zeta) r(zeta) qm + l(zeta) ql + r(zeta) qr + o(zeta) qo + qk, with
 *                                   c_s3 = (l(zeta) + beta s1(zeta) + gamma) (r(zeta) + beta s2(zeta) + gamma) z(omega zeta) beta,
 *                                   c_z = -(l(zeta) + beta zeta + gamma) (r(zeta) + beta u zeta + gamma) (o(zeta) + beta u^2 zeta + gamma),
 *                                   lag = (zeta^n - 1) / (zeta - 1) * alpha^2 / n, where 1 / 0 = 0 as fr.Element.Inverse has it
 *         d_fh + v out_stride     the n + 2 coefficients of h1 + zeta^(n+2) h2 + zeta^(2(n+2)) h3
 *       with out_stride >= n + 3.  These are the values and polynomials of zk_bn254_plonk_prove, bit for bit.
 *   zk_bn254_plonk_open_batch_dev       round 5's polynomial.  In, per row v: fh, l, r, o (n + 2 coefficients) and lin (n + 3) at element v * in_stride
 *       (in_stride >= n + 3), zeta[v] and kzg_gamma[v] = g, the challenge of kzg.BatchOpenSinglePoint (derived by the caller from the digests and values of round
 *       4).  Out: d_q + v * out_stride, the n + 2 coefficients (out_stride >= n + 2) of (folded - folded(zeta)) / (X - zeta) with
 *       folded = fh + g lin + g^2 l + g^3 r + g^4 o + g^5 s1 + g^6 s2; d_value[v] = folded(zeta), which is sum_i g^i claimed_i.
 * Elements between the rows of an output are not touched; the inputs are only read.  Workspace: the slot's arena, at most 1 GiB and 65,535 rows at a time: more
 * rows run in chunks on the same stream.  The key's per-proof workspace is not used, so calls on one key overlap each other and a proof in flight.
 * INPUT CONTRACT: canonical fr.Element images in Montgomery form (< r), as above.
 * ARGUMENT ERRORS, decided before a device is looked for: a null pointer (but for the d_q of the ingredient), len == 0, a stride below what is said above, an
 * output overlapping an input or another output (but for the in-place form of the ingredient) -> ZK_ERR_ARG; an unknown key -> ZK_ERR_HANDLE; rows == 0 ->
 * ZK_OK, nothing happens.
 * STREAMS: each synchronises `stream` (NULL: the slot's own) before it returns, like the entries above. */
int zk_bn254_fr_poly_open_rows_dev(const void *d_f, size_t in_stride, size_t len, size_t rows, const void *d_points, void *d_q, size_t q_stride, void *d_values,
                                   void *stream);
int zk_bn254_plonk_linearize_batch_dev(uint64_t pk_handle, const void *d_l, const void *d_r, const void *d_o, const void *d_z, size_t in_stride, const void *d_h,
                                       size_t h_stride, size_t rows, const void *d_alpha, const void *d_beta, const void *d_gamma, const void *d_zeta, void *d_values,
                                       void *d_zquot, void *d_lin, void *d_fh, size_t out_stride, void *stream);
int zk_bn254_plonk_open_batch_dev(uint64_t pk_handle, const void *d_fh, const void *d_lin, const void *d_l, const void *d_r, const void *d_o, size_t in_stride,
                                  size_t rows, const void *d_zeta, const void *d_kzg_gamma, void *d_q, size_t out_stride, void *d_value, void *stream);
/* The digests every round ends in, for the rows of the entries above: row v = the `len` Montgomery images at element v * row_stride of d_rows, committed through
 * zk_bn254_msm_bases_rows_dev (its contract, chunks and outputs: d_out rows zk_g1_affine, d_compressed rows x 32 bytes, either -- not both -- may be NULL).
 *   from_values = 0   coefficients against the key's SRS, len <= its size (l, r, o, Z, the thirds of h, the opening quotients)
 *   from_values = 1   len = n + 2: the n wire VALUES of a row followed by its two blinders b0, b1, against the key's Lagrange form (zk_bn254_plonk_pk_lagrange_srs;
 *                     ZK_ERR_ARG if the key has none) -- the digest of the blinded l / r / o without their inverse transforms, the zero digits dropped
 * It holds the key as the entries above do (shared: calls overlap each other and a proof in flight) and synchronises before it returns. */
int zk_bn254_plonk_commit_batch_dev(uint64_t pk_handle, const void *d_rows, size_t row_stride, size_t len, size_t rows, int from_values, void *d_out,
                                    void *d_compressed);

/* BATCH PLONK PROVING: the proofs of `rows` witnesses against ONE resident key in one call, assembled on the device from the row entries above -- round 1's
 * gather, blinding and canonical forms, the row forms of rounds 2 to 5, the row-batched commitments, the Fiat-Shamir transcript (one lane per row) and
 * Proof.WriteTo.  Row v's ZK_PLONK_PROOF_BYTES are, byte for byte, what zk_bn254_plonk_prove writes for that solution, those blinders and those challenges.
 * Nothing but the finished proofs and the verdicts crosses to the host, and no host work grows with the number of rows.
 *   zk_bn254_plonk_prove_batch
 *     solutions    row v = the n_vars Montgomery images at element v * sol_stride (public inputs first): host memory, or device memory when on_device != 0
 *     blinders     rows x 9, host: the nine blinding scalars of each row (l: 2, r: 2, o: 2, z: 3)
 *     challenges   NULL: gnark's SHA-256 transcript, exactly as zk_bn254_plonk_prove derives it; otherwise rows x 5 pinned values, host, in the single prover's
 *                  order (gamma, beta, alpha, zeta, kzg's folding gamma): a copy takes the place of every transcript launch, the path is otherwise the same
 *     chunk_rows   0, or a cap on the automatic chunk (so that several chunks can be had at a small size); it never changes a byte
 *     proofs_out   rows x 548 bytes, host;  status_out: rows int, host: 0 = a proof; 1 = the row's solution does not satisfy the circuit (the verdict of
 *                  zk_bn254_plonk_quotient_batch_dev): its 548 bytes are zero, and neither the call nor the other rows fail
 *     The digest of the folded quotient is always taken by linearity from the row's own [H0], [H1], [H2]; the digest of the linearised polynomial by linearity from
 *     [Z] and the key's digests once the key's digests are known to be consistent (Setup's key; a key read from its wire image after a single proof has checked
 *     it), through the row MSM otherwise -- the same bytes.  The batch itself never marks a key consistent.
 *     CHUNKS: the rows run in chunks, the largest row count whose workspace -- per row: the solution (host form), l, r, o as values and as coefficients, z, the
 *     quotient's workspace, h, the linearised polynomial, the folded quotient, the two opening quotients, the openings' workspace, the digests -- fits 1 GiB of the
 *     slot's arena, capped at a third of the row MSM's own chunk (zk_bn254_msm_rows_info) and by chunk_rows.  Per chunk the host synchronises a fixed number of
 *     times (in front of every row MSM) and makes one copy of proofs and verdicts.
 *     The key's `live` lock is held shared; neither its per-proof mutex nor its per-proof workspace is touched: calls overlap each other and a single proof in
 *     flight.  A key whose bases are not on one device entry runs its rows through zk_bn254_plonk_prove one after the other.
 *   zk_bn254_plonk_prove_batch_info   *chunk_rows: the automatic chunk for device-resident solutions (1 for a key that runs row by row); *commits_batched: whether
 *     the row MSM's batched path serves the key's SRS; *lin_by_linearity: whether the next batch takes the linearised polynomial's digest by linearity.  Any of the
 *     three may be NULL.
 *   zk_bn254_plonk_challenges_batch_dev   the transcript alone: challenge `stage` of `rows` proofs, one lane per row, everything in device memory.
 *     stage 0  gamma: binds the key's eight digests, the row's public inputs (npub Montgomery images at d_pub + v * pub_stride), then [L], [R], [O]
 *     stage 1  beta:  binds gamma's raw digest            stage 2  alpha: beta's raw digest, then [Z]          stage 3  zeta: alpha's raw digest, then [H0], [H1], [H2]
 *     stage 4  kzg's folding gamma, a transcript of its own: binds zeta, [foldedH], [lin], [L], [R], [O], the key's [S1], [S2], and the seven claimed values
 *     d_points   the stage's points of row v, zk_g1_affine each ((0, 0) = infinity, bound as 0x40 and 63 zero bytes), at d_points + (3, -, 1, 3, 5 for stages
 *                0 .. 4) * v in the order above; unused (may be NULL) at stage 1
 *     d_prev     stages 1 to 3: the previous stage's raw digests, 32 bytes per row, as that stage wrote them; stage 4: zeta[v], one Montgomery image per row;
 *                unused (may be NULL) at stage 0
 *     d_values   stage 4: eight elements per row as zk_bn254_plonk_linearize_batch_dev writes them, of which the first seven are bound; unused otherwise
 *     d_out      2 * rows * 32 bytes: the challenge of row v, reduced as fr.SetBytes, Montgomery, at element v; behind the rows challenges the raw 32-byte digests,
 *                row v at byte 32 * (rows + v): the next stage's d_prev
 *     The part of gamma's message that is the same for every row ("gamma" and the key's digests) is hashed once per call on the host.
 * ARGUMENT ERRORS, decided before a device is looked for: a null pointer, a stage outside 0 .. 4, sol_stride < n_vars or pub_stride < npub with more than one
 * row, an output overlapping an input or the other output -> ZK_ERR_ARG; n_vars not the key's -> ZK_ERR_LEN; an unknown key -> ZK_ERR_HANDLE; rows == 0 ->
 * ZK_OK, nothing happens.  zk_bn254_plonk_prove_batch returns ZK_OK whenever its arguments were sound.  The challenges entry synchronises `stream` (NULL: the
 * slot's own) before it returns. */
int zk_bn254_plonk_prove_batch(uint64_t pk_handle, const void *solutions, size_t n_vars, size_t sol_stride, size_t rows, int on_device,
                               const zk_fr *blinders /* rows x 9 */, const zk_fr *challenges /* NULL or rows x 5 */, size_t chunk_rows /* 0 = automatic */,
                               uint8_t *proofs_out /* rows x 548, host */, int *status_out /* rows, host */);
int zk_bn254_plonk_prove_batch_info(uint64_t pk_handle, size_t *chunk_rows, int *commits_batched, int *lin_by_linearity);
int zk_bn254_plonk_challenges_batch_dev(uint64_t pk_handle, int stage, size_t rows, const void *d_pub, size_t pub_stride, const void *d_points,
                                        const void *d_prev, const void *d_values, void *d_out, void *stream);

/* ---- the callers either side of the PLONK path: the reference's exported entry points, restated over the device path -----------------------
 * PlonkPreprocess (gnark_backend_ffi/main.go:58-78) and PlonkProveWithPK (main.go:24-37) take the ACIR as JSON (acir/acir.go:17-75), the witness
 * values as the hex felt vector (internal/backend/helpers.go:24-33) and the key as hex of ProvingKey.WriteTo (helpers.go:49-60, 82-87); the
 * lowering is BuildSparseR1CS / HandleValues (backend/plonk/sparse_r1cs.go:18-107, backend/common.go:45-76).  Differences: the SRS is a
 * resident handle instead of srs.hex re-read per call; errors are codes instead of log.Fatal; outputs go to caller buffers (no terminator);
 * the blinding scalars can be pinned (NULL = /dev/urandom).
 * layout: how witnesses become constraint-system variables --
 *   ZK_ACIR_LAYOUT_REFERENCE             HandleValues exactly as written (backend/common.go:45-76): public variables in witness order, then one
 *                                        SECRET variable per (witness, non-matching public input) when there are public inputs -- so with |P| >= 2
 *                                        public inputs a private witness has |P| variables, a public one |P| - 1 secret copies besides its public
 *                                        variable -- and the gates name the LAST variable added for a witness (indexMap, last write wins); a term
 *                                        that names a witness without a variable gets variable 0 (Go's map zero value).  Keys and proofs made this
 *                                        way are the reference's own; libgnark_backend.so uses it.
 *   ZK_ACIR_LAYOUT_ONE_VAR_PER_WITNESS   public witnesses first, then the others, one variable each; unknown witnesses are an error.  Identical to
 *                                        the reference layout for zero or one public input.
 *   zk_plonk_preprocess: pk_hex_out == NULL only returns the sizes in *pk_len / *vk_len; pk_handle (optional) keeps the key resident.
 *   zk_plonk_prove_with_pk: pk_hex == NULL uses the resident key pk_handle (the reference deserialises the key on every call); ZK_ERR_ARG when the
 *                           key's public / variable / gate counts are not the circuit's. */
enum { ZK_ACIR_LAYOUT_REFERENCE = 0, ZK_ACIR_LAYOUT_ONE_VAR_PER_WITNESS = 1 };
int zk_plonk_preprocess(const char *acir_json, size_t acir_len, const char *values_hex, size_t values_len, int layout,
                        uint64_t srs_handle, char *pk_hex_out, size_t pk_cap, size_t *pk_len, char *vk_hex_out, size_t vk_cap,
                        size_t *vk_len, uint64_t *pk_handle);
int zk_plonk_prove_with_pk(const char *acir_json, size_t acir_len, const char *values_hex, size_t values_len, int layout,
                           const char *pk_hex, size_t pk_len, uint64_t pk_handle, uint64_t srs_handle, const zk_fr *blinders,
                           char proof_hex_out[2 * ZK_PLONK_PROOF_BYTES]);
/* BuildSparseR1CS alone: the gates of an ACIR circuit (Montgomery coefficients, variable ids with the public variables first) and the
 * witness order (variable k holds witness order[k] + 1).  Array pointers may be NULL (first call sizes them through *n_constraints / *n_vars). */
int zk_acir_to_sparse_r1cs(const char *acir_json, size_t acir_len, size_t n_values, int layout, size_t *n_public, size_t *n_vars,
                           size_t *n_constraints, zk_fr *ql, zk_fr *qr, zk_fr *qo, zk_fr *qm, zk_fr *qk, uint32_t *xa, uint32_t *xb,
                           uint32_t *xc, uint32_t *order);
/* What the verifier needs of HandleValues (backend/common.go:45-60; PlonkVerifyWithVK, main.go:44-56): out[k] = 0-based position, in the witness-value
 * vector, of public variable k.  *n_public is set even when cap is too small (ZK_ERR_ARG then). */
int zk_acir_public_witnesses(const char *acir_json, size_t acir_len, size_t n_values, int layout, uint32_t *out, size_t cap, size_t *n_public);
/* What the export path keeps resident between calls.  The reference re-reads everything per call (main.go:24-37 -> backend/plonk/plonk.go:53-73: the ACIR
 * is unmarshalled and lowered, the key hex-decoded and ReadFrom'd); at 2^19 gates that is 0.24 GB of JSON and 0.33 GB of key text in front of a 10 ms
 * prover.  zk_plonk_prove_with_pk / zk_plonk_preprocess / zk_acir_public_witnesses identify both texts by a 128-bit content key and keep the lowered
 * circuit (wiring + variable order in HBM) and the decoded key (with its big-coset forms) resident, least recently used first out, within
 * ZKMI_TABLE_CAP_GB (0 keeps nothing).  A key text is only ever matched together with the circuit text and the SRS it was first seen with. */
int zk_export_cache_info(size_t *n_circuits, size_t *n_keys, size_t *bytes);
int zk_acir_lower_resident(const char *acir_json, size_t acir_len, size_t n_values, int layout, int with_coefficients); /* host only: lower now, keep resident
    (start-up overlap: the export shim runs it beside the SRS load); with_coefficients: the selectors too, kept for the zk_plonk_preprocess that follows */
int zk_export_cache_clear(void);
/* Size (G1 points) of an SRS the export shim creates when srs.hex is missing: 1,000,000 like the reference (backend/common.go:137) unless a TEST set another
 * (4 .. 2^28) before the shim's first call -- a setter instead of an environment variable, so that nothing in a prover's environment can change its SRS. */
int zk_export_set_new_srs_size(size_t n);
size_t zk_export_new_srs_size(void);
/* HBM held by a resident PLONK key */
int zk_bn254_plonk_pk_bytes(uint64_t handle, size_t *bytes);

/* buildR1CS of the reference's intended Groth16 FFI (backend/groth16/r1cs.go:9-72; payload RawR1CS, src/gnark_backend_wrapper/groth16/
 * acir_to_r1cs.rs:18-60) on a JSON RawR1CS: a resident R1CS plus the full wire vector [ONE, public, secret, product variables] in HBM
 * (*d_witness, n_wires Montgomery elements; release with zk_dev_free) -- feed them to zk_bn254_groth16_setup / zk_bn254_groth16_prove_r1cs
 * (on_device = 1).  See frontend.hip for the points where the reference's sketch is made well-defined. */
int zk_groth16_r1cs_from_raw(const char *raw_json, size_t len, uint64_t *r1cs_handle, void **d_witness, size_t *n_wires, size_t *n_public);
/* The exported entry points of that FFI, restated over the device path (errors are codes instead of log.Fatal; outputs go to caller buffers, no
 * terminator; randomness may be pinned, NULL = /dev/urandom as upstream draws it):
 *   zk_groth16_preprocess      Preprocess    (r1cs.go:214-266): groth16.Setup -> hex(ProvingKey.WriteTo), hex(VerifyingKey.WriteTo); toxic = tau, alpha,
 *                              beta, gamma, delta.  pk_hex_out == NULL only returns the sizes; pk_handle (optional) keeps the key resident.
 *   zk_groth16_prove_with_pk   ProveWithPK   (r1cs.go:107-143): hex key (or pk_handle when pk_hex == NULL) -> 256 hex characters of Proof.WriteTo;
 *                              rs = the prover's (r, s).
 *   zk_groth16_prove_with_meta ProveWithMeta (r1cs.go:74-105): Setup + Prove, the key never leaves HBM. */
int zk_groth16_preprocess(const char *raw_json, size_t raw_len, const zk_fr *toxic, char *pk_hex_out, size_t pk_cap, size_t *pk_len,
                          char *vk_hex_out, size_t vk_cap, size_t *vk_len, uint64_t *pk_handle);
int zk_groth16_prove_with_pk(const char *raw_json, size_t raw_len, const char *pk_hex, size_t pk_len, uint64_t pk_handle, const zk_fr *rs,
                             char proof_hex_out[256]);
int zk_groth16_prove_with_meta(const char *raw_json, size_t raw_len, const zk_fr *toxic, const zk_fr *rs, char proof_hex_out[256]);
/* What these three keep resident between calls (the sketch re-reads everything per call, r1cs.go:107-128: json.Unmarshal of the RawR1CS, buildR1CS,
 * hex.DecodeString + ProvingKey.ReadFrom): a RawR1CS text carries the circuit AND this proof's values string, so the circuit is identified by the content
 * keys of the text before and after that string (same offset, same length); the key text by its content key.  Resident: the R1CS in HBM with the witness ->
 * wire order and the operands of every product variable (the wire vector of a later proof is assembled on the device from the values string alone), the
 * decoded key -- without window tables for its first proof, with them from its second on.  Same LRU bound as the PLONK entries (zk_export_cache_info counts both).
 *   zk_groth16_lower_resident  read a RawR1CS text into the cache now; to_device = 0: host only (start-up overlap: the export shim runs it beside the HIP
 *                              runtime's start), 1: also upload the circuit (beside the key's decoding)
 *   zk_groth16_key_resident    decode a key text into the cache now (no window tables)
 *   zk_groth16_public_inputs   buildWitnesses' public part for VerifyWithVK (r1cs.go:176-212): the values of the public wires after ONE, in wire order
 *                              (Montgomery); host only; *n_public is set even when cap is too small (ZK_ERR_ARG then). */
int zk_groth16_lower_resident(const char *raw_json, size_t raw_len, int to_device);
int zk_groth16_key_resident(const char *pk_hex, size_t pk_len);
int zk_groth16_public_inputs(const char *raw_json, size_t raw_len, zk_fr *out, size_t cap, size_t *n_public);

/* MANY WITNESS-VALUE TEXTS OF ONE CIRCUIT PER CALL.  A caller of the export path holds the circuit text and one hex felt vector (encode_felts) per witness;
 * zk_bn254_plonk_prove_batch / zk_bn254_groth16_prove_r1cs_batch take rows that are already lowered.  These entries are the step between: the texts of a chunk go
 * up in one pitched copy, ONE launch decodes them (zk_bn254_felts_decode_hex_rows_dev), one or two assemble the rows -- HandleValues' variable order (duplicated
 * secret variables included) for PLONK; [ONE, public, secret, one product per mul term] for Groth16 -- and the rows go to the batch prover as they lie in HBM.
 *   values_hex     host: row v is the values_len characters at values_hex + v * values_stride.  Every row has the same length: for PLONK values_len = 8 + 64 *
 *                  (the count in row 0's header) -- the n_values the circuit is lowered with, as in zk_plonk_prove_with_pk; for Groth16 the length of the values
 *                  string the RawR1CS text was read with (ZK_ERR_LEN otherwise).
 *   raw_json       the RawR1CS text: its own embedded values string only identifies the circuit (it must be plain hex) and is NOT a row.
 *   status_out     host, one per row (the enum below).  A bad row fails neither the call nor its neighbours; its output row is defined: zeros where a felt was
 *                  rejected (its proof: all '0').  For any status but ZK_ROW_OK the proof characters of the row are all '0'.
 *   zk_plonk_solutions_rows / zk_groth16_wires_rows   the assembly alone: rows x n_vars (n_wires) Montgomery elements in device memory, row v at element
 *                  v * sol_stride (wire_stride); the stride may be anything for one row and must hold a row otherwise (ZK_ERR_ARG).
 *   zk_plonk_prove_batch_with_pk / zk_groth16_prove_batch_with_pk   for a row with status ZK_ROW_OK the 1096 (256) characters at proofs_hex_out + v * 1096 (256)
 *                  are exactly what zk_plonk_prove_with_pk / zk_groth16_prove_with_pk writes for the same circuit, that row's values text, the same key and
 *                  that row's blinders (nine) / (r, s).  blinders / rs == NULL: drawn from /dev/urandom, rows x 9 / rows x 2.  The key as in the single entries:
 *                  a text found or made resident by its content key and pinned for the call, or a resident handle; its shape is checked against the circuit once
 *                  per call.  A cached PLONK key's proof count advances by `rows` (the Lagrange form of its SRS is built before the batch that reaches the
 *                  sixteenth); a cached Groth16 key that proves again gets its window tables in the background, and until it has them its rows run one by one
 *                  inside zk_bn254_groth16_prove_r1cs_batch -- the same bytes.
 *   CHUNKS         assembly, then the prover, per chunk of zk_bn254_plonk_prove_batch_info / zk_bn254_groth16_batch_info rows, capped by chunk_rows (0 = no cap;
 *                  it never changes a byte): the call's staging -- texts, decoded values, rows -- never exceeds one chunk.  The staging is the call's own: the
 *                  resident circuit's per-proof buffers are not touched and its mutex is held only while the circuit and the key are made resident, so a
 *                  call overlaps a single proof on the same circuit.  No stream slot is held while another is acquired.
 *   The PLONK batch is only faster than the loop of single calls where the batch prover is: on an SRS registered without a window table it is not
 *   (zk_bn254_plonk_prove_batch_info's commits_batched = 0), and no table is built here.
 * ARGUMENT ERRORS, decided before a device is looked for: a null pointer, values_stride < values_len with more than one row, neither pk_hex nor pk_handle ->
 * ZK_ERR_ARG; values_len != 8 + 64 * (row 0's count) -> ZK_ERR_LEN; rows == 0 -> ZK_OK, nothing written. */
enum {
    ZK_ROW_OK = 0,            /* decoded (and, from the batch provers, proved) */
    ZK_ROW_UNSATISFIED = 1,   /* the batch prover's verdict: the solution violates the circuit (PLONK only) */
    ZK_ROW_BAD_HEX = 2,       /* invalid hex character in the row's felts */
    ZK_ROW_NOT_CANONICAL = 3, /* a felt >= r */
    ZK_ROW_BAD_COUNT = 4,     /* the row's count header is not n_values */
    ZK_ROW_BAD_PROOF_HEX      /* (the next value: five) the verify-batch entries below: an invalid hex character in the row's proof text */
};
int zk_plonk_solutions_rows(const char *acir_json, size_t acir_len, int layout, const char *values_hex, size_t values_len, size_t values_stride,
                            size_t rows, void *d_solutions /* rows x n_vars, device */, size_t sol_stride, int *status_out /* rows, host */);
int zk_groth16_wires_rows(const char *raw_json, size_t raw_len, const char *values_hex, size_t values_len, size_t values_stride,
                          size_t rows, void *d_wires /* rows x n_wires, device */, size_t wire_stride, int *status_out /* rows, host */);
int zk_plonk_prove_batch_with_pk(const char *acir_json, size_t acir_len, int layout, const char *values_hex, size_t values_len, size_t values_stride,
                                 size_t rows, const char *pk_hex, size_t pk_len, uint64_t pk_handle, uint64_t srs_handle,
                                 const zk_fr *blinders /* NULL or rows x 9 */, size_t chunk_rows /* 0 = automatic */,
                                 char *proofs_hex_out /* rows x 1096 */, int *status_out /* rows */);
int zk_groth16_prove_batch_with_pk(const char *raw_json, size_t raw_len, const char *values_hex, size_t values_len, size_t values_stride, size_t rows,
                                   const char *pk_hex, size_t pk_len, uint64_t pk_handle, const zk_fr *rs /* NULL or rows x 2 */,
                                   size_t chunk_rows, char *proofs_hex_out /* rows x 256 */, int *status_out /* rows */);

/* MANY PROOF TEXTS OF ONE CIRCUIT PER CALL: the verifying counterpart of the two entries above.  What the export shim's PlonkVerifyWithVK / VerifyWithVK do per
 * proof -- hex-decode the proof, find the public values in the values text, convert them to Montgomery form, verify -- for `rows` proofs against ONE verifying
 * key, without a host loop: per chunk the proof texts and the values texts go up in two pitched copies, one launch decodes the proofs
 * (zk_bn254_bytes_decode_hex_rows_dev), one checks the values texts and decodes the public values (zk_bn254_felts_public_hex_rows_dev), and the rows go to
 * zk_bn254_plonk_verify_batch_dev / zk_bn254_groth16_verify_batch_dev where they lie.
 *   proofs_hex     host: row v is the 1096 (256) characters at proofs_hex + v * proofs_stride -- hex of Proof.WriteTo, either letter case.
 *   values_hex     host, as in the entries above: row v's values_len characters at values_hex + v * values_stride.  The circuit is found or made resident by
 *                  content as there (host side only: no circuit buffer goes to the device).  The public positions come from the lowering: for PLONK
 *                  zk_acir_public_witnesses' positions; for Groth16 the public wires after ONE in wire order -- what zk_groth16_public_inputs reads.  The
 *                  RawR1CS text's own embedded values string only identifies the circuit and is NOT a row.
 *   vk_hex         the verifying key's hex text; srs_g2: the SRS's ([1]2, [alpha]2) as in zk_bn254_plonk_verify.
 *   status_out     host, one per row: ZK_ROW_OK, or why the row was not verified -- ZK_ROW_BAD_PROOF_HEX (decided first, as the shim decodes the proof first),
 *                  ZK_ROW_BAD_COUNT, ZK_ROW_BAD_HEX (EVERY character of the values text is checked: hex.DecodeString sees the whole text),
 *                  ZK_ROW_NOT_CANONICAL (a PUBLIC felt >= r; a felt >= r at a position that is not public is not an error, as the shim never decodes it).
 *   accepted       host, one per row.  For any status but ZK_ROW_OK accepted[v] = 0: the row fails neither the call nor its neighbours (it goes through the
 *                  verifier as zeros, which is a rejected lane).  For a row with ZK_ROW_OK accepted[v] is what the shim's sequence -- hex-decode the proof, take
 *                  the public values, zk_bn254_plonk_verify / zk_bn254_groth16_verify -- returns for that row's texts; a proof encoding that call refuses
 *                  with ZK_ERR_ARG is a 0 here.  *n_accepted = the number of ones.
 *   CHUNKS         at most 2^16 - 1 rows at a time and no more than keeps the staging within 256 MiB, capped by chunk_rows (0 = no cap; it never changes a
 *                  verdict: the coefficients are derived over the chunk handed to the verifier, and a verdict does not depend on them).  The staging is the
 *                  call's own and never exceeds one chunk.  No stream slot is held while another is acquired.
 * The number of public values not matching the key is ZK_ERR_LEN for the call, with upstream's message ("invalid witness size").  ARGUMENT ERRORS, decided
 * before a device is looked for: a null pointer, a stride below its row with more than one row -> ZK_ERR_ARG; values_len != 8 + 64 * (row 0's count) ->
 * ZK_ERR_LEN; rows == 0 -> ZK_OK, nothing written.  A malformed key: ZK_ERR_ARG / ZK_ERR_LEN as in the host verifier.  Without a GPU: ZK_ERR_NO_DEVICE after
 * all of these. */
int zk_plonk_verify_batch_with_vk(const char *acir_json, size_t acir_len, int layout, const char *proofs_hex, size_t proofs_stride,
                                  const char *values_hex, size_t values_len, size_t values_stride, size_t rows, const char *vk_hex, size_t vk_len,
                                  const zk_g2_affine srs_g2[2], size_t chunk_rows, uint8_t *accepted /* rows */, int *status_out /* rows */,
                                  size_t *n_accepted);
int zk_groth16_verify_batch_with_vk(const char *raw_json, size_t raw_len, const char *proofs_hex, size_t proofs_stride, const char *values_hex,
                                    size_t values_len, size_t values_stride, size_t rows, const char *vk_hex, size_t vk_len, size_t chunk_rows,
                                    uint8_t *accepted /* rows */, int *status_out /* rows */, size_t *n_accepted);

/* What the MSM planner picks for n points (with / without resident window tables): window width c and the number of c-bit
 * digits per scalar, i.e. mixed additions per scalar multiplication -- used by bench.py to turn launches into work. */
int zk_bn254_msm_plan_info(size_t n, int window_tables, uint32_t *window_bits, uint32_t *digits);

/* The scalar-side half of an MSM alone, for inspection / tests: signed-digit recoding, radix sort, bucket bounds, device-chosen task
 * length, task plan and task records -- the production preparation itself, run through the same wrappers the provers call (plain;
 * against a window table; a batch of up to three pointers; the rows of one matrix), on HOST scalars, with every intermediate copied
 * back.  No bases are involved.  Nothing stays behind: the slot is released and the preparation's event destroyed on every path.
 *   request   n scalars per vector; window_bits (0: the planner's choice; ignored in table mode) and scalars_mont as in zk_msm_cfg;
 *             table != 0: one bucket set per vector against a table of width c whose rows are `stride` entries apart and hold the
 *             windows row_first + k * row_step; `sets` vectors given by vec[0..sets) (by_rows == 0, sets <= 3; equal pointers stay
 *             equal on the device) or as the rows vec[0] + v * row_stride of one matrix (by_rows != 0); drop_zero_digits as in the
 *             provers (silently off where a workgroup's digits do not fit its stage: windows narrower than 8 bits).
 *   result    the plan, `dropped` (1 when the run took the compacting recoding and its device-side pair counter, else 0), the pair count as the
 *             device knows it (that counter when digits were dropped, else total), the
 *             64-word control block ([0] split buckets, [1] largest bucket, [2] task length, [3] buckets above 8192 points, [4] giant
 *             buckets found, [8..56) ids of those listed) and, where the pointer is not NULL, the arrays: keys / vals [total] (the
 *             first device_total entries are meaningful), start / task_off [nb + 1], task_begin / len_keys / task_ids [max_tasks],
 *             multi_list [nb] (the first ctl[0] entries are meaningful).
 * With ALL array pointers NULL only the plan is filled in (host work: no device is needed, the scalars are not read): call once for
 * the sizes, allocate, call again.  An empty plan (n == 0, or a table shard that owns no window) reports total == 0 and touches nothing. */
typedef struct {
    size_t n;
    int window_bits, scalars_mont, table, drop_zero_digits;
    uint32_t c, row_first, row_step, sets;
    size_t stride;
    int by_rows, reserved;
    const zk_fr *vec[3];
    size_t row_stride;
} zk_msm_prep_request;
typedef struct {
    uint32_t c, W, Wd, Wrows, B, nb, key_bits, L, Lmin, m1, N1, dropped;
    uint64_t total, max_tasks, device_total;
    uint32_t ctl[64];
    uint32_t *keys, *vals, *start, *task_off, *task_begin, *len_keys, *task_ids, *multi_list;
} zk_msm_prep_result;
int zk_bn254_msm_prep_inspect(const zk_msm_prep_request *req, zk_msm_prep_result *res);

/* The base-side half of an MSM behind that preparation, for inspection / tests: window table, bucket accumulation, the folds of split
 * buckets, every reduction level and the finishers -- the production calls themselves (msm_build_table_g1 / _g2, the four preparation
 * wrappers, msm_g1_accumulate / msm_g2_accumulate, msm_g?_finish / msm_g?_finish_sets / msm_g1_sets_affine_dev), on HOST scalars and
 * HOST points, with a trace attached to the job: after the accumulate launch, after the two fold launches and after every reduce launch
 * the job's stream is synchronised and the raw device array copied.  No kernel and no launch differs from a prover's.  Nothing stays
 * behind: the slot is released, the preparation's event destroyed and points and table freed on every path.
 *   request   prep: as for zk_bn254_msm_prep_inspect.  points: n affine points (zk_g1_affine, or zk_g2_affine with is_g2; gnark's
 *             Montgomery image, (0, 0) = infinity).  Table mode: the table of prep.c-bit windows is built from them (rows prep.row_first +
 *             k * prep.row_step, prep.stride entries apart, into a zeroed buffer); l1_m / l2_m are the buckets per lane of the first level
 *             and the entries per lane of the second thread-serial level (0: the defaults, 8 and none), as a prover's MsmTable carries them.
 *             quad_tail (G1): the wave levels with four lanes per point.  keep_final (G1, table mode): the last level stays on the device
 *             and msm_g1_sets_affine_dev finishes it.  skip_below (plain method only; an argument error against a table): points with a
 *             smaller index are left out of the sums.
 *   result    prep: everything zk_msm_prep_result holds, from THIS run (the device picks the task length).  m2 (l2_m as planned), tasks
 *             (real tasks: task_off[nb]), n_final / sh_final (entries per bucket set left to the finisher and their shift), n_levels
 *             descriptors: kind (1 = k_reduce_l1, 2 = k_reduce_l2, 3 = k_reduce_wave, 4 = k_reduce_wave with four lanes per point),
 *             entries per set going in (level 1: buckets) and coming out, the shift sh before and after (value of a set = sum_j A_j +
 *             2^sh * sum_j j * S_j), and m: the entries one lane (1, 2) or one wave (3, 4) folds.  table_entries = rows * stride;
 *             level_entries = sum over the levels of W * n_out.
 *             Arrays, where the pointer is not NULL -- all of them AFFINE points (4 words per coordinate: 8 per G1 point, 16 per G2
 *             point; (0, 0) = infinity), converted on the host: table [table_entries]; partial_acc / partial_fold [max_tasks]: the task
 *             array after the accumulate launch and after the two fold launches (the slots of padding tasks, which no kernel writes, come
 *             back as (0, 0); after the fold a split bucket's sum sits in its first task's slot, the others are scratch); level_a /
 *             level_s [level_entries]: the levels one after the other, set w of a level at [w * n_out, (w + 1) * n_out); without
 *             keep_final set_values [W] (plain: the windows' values; table: one sum per vector) and, plain method, total [1]; with
 *             keep_final final_affine [sets] and final_bytes [sets * 32] (the compressed encodings) from the device finish.
 * With ALL array pointers NULL (prep's too) only the plan, the level descriptors and the sizes are filled in (host work, no device):
 * call once for the sizes, allocate, call again; the run's own descriptors are compared with those and a difference is an error.
 * An empty plan touches nothing, except that with keep_final the device finish still runs and writes infinities. */
#define ZK_MSM_TAIL_MAX_LEVELS 12
typedef struct {
    zk_msm_prep_request prep;
    const void *points;
    int is_g2, quad_tail, keep_final, reserved;
    uint32_t l1_m, l2_m, skip_below, reserved2;
} zk_msm_tail_request;
typedef struct {
    uint32_t kind, n_in, n_out, sh_in, sh_out, m;
} zk_msm_tail_level;
typedef struct {
    zk_msm_prep_result prep;
    uint32_t m2, tasks, n_final, sh_final, n_levels, reserved;
    zk_msm_tail_level level[ZK_MSM_TAIL_MAX_LEVELS];
    uint64_t table_entries, level_entries;
    uint64_t *table, *partial_acc, *partial_fold, *level_a, *level_s, *set_values, *total, *final_affine;
    uint8_t *final_bytes;
} zk_msm_tail_result;
int zk_bn254_msm_tail_inspect(const zk_msm_tail_request *req, zk_msm_tail_result *res);

/* The Horner suffix scan under every PLONK proof and every KZG opening (S_i = f_i + a S_(i+1): S_0 = f(a), q_i = S_(i+1)), for inspection / tests: up to
 * ZK_HSCAN_ROWS_MAX HOST rows -- coefficients, length, point -- are uploaded and the production launcher of the argument-point kernels is called once, with the
 * points prepared by the production preparation (a -> a, a^K, a^(256 K)) and a trace attached: after the first launch the stream is synchronised and the
 * workgroup totals copied, since the second launch overwrites them in place.  No kernel and no launch differs from a prover's; the profile names are the single
 * PLONK prover's (plonk_horner_local, plonk_horner_blocks, plonk_divide_apply).  Nothing stays behind: the slot is released on every path.
 *   request   rows in [1, ZK_HSCAN_ROWS_MAX]; K >= 1 coefficients per lane (the caller's, NOT the planner's: any K runs); nb workgroups of 256 lanes per row,
 *             0 = what the longest row needs at this K (((len + K - 1) / K + 255) / 256), a larger value is taken as it is, a smaller one is an error; pad: guard
 *             elements in front of and behind every row.  f[r]: pad + len[r] + pad Montgomery elements, the coefficients in the middle; equal f pointers stay ONE
 *             device array.  q[r]: where row r's quotient goes, a buffer of the same shape -- or f[r] itself: division in place (not with a shared f).  Both are
 *             uploaded whole, guards included, and copied back whole after the run, so the caller sees what was written where.  eval_only: two launches, no lane
 *             carries kept, no quotient (q[r] may be NULL; where given it comes back as it went in).  a[r]: the point (Montgomery).
 *   result    nb as used; the arrays, where the pointer is not NULL, are uploaded from the caller's memory before the run (the caller's poison shows what no
 *             kernel wrote) and copied back after it: tcarry [rows * nb * 256] the lane carries after pass 1 ((row nb + block) 256 + lane; untouched with
 *             eval_only), btot_local [rows * nb] the workgroup totals after pass 1 (the trace), btot [rows * nb] after pass 2, total [rows] = f_r(a_r).
 * Errors, decided before a device is looked for: ZK_ERR_ARG for a null pointer, rows == 0 or above ZK_HSCAN_ROWS_MAX, K == 0, a length of 0, nb below what the
 * longest row needs, rows * nb above 65,536, a missing q[r] without eval_only, in-place division of a shared f, two rows with one q. */
#define ZK_HSCAN_ROWS_MAX 8
typedef struct {
    uint32_t rows, K, nb, pad;
    int eval_only, reserved;
    zk_fr *f[ZK_HSCAN_ROWS_MAX], *q[ZK_HSCAN_ROWS_MAX];
    size_t len[ZK_HSCAN_ROWS_MAX];
    zk_fr a[ZK_HSCAN_ROWS_MAX];
} zk_hscan_request;
typedef struct {
    uint32_t nb, reserved;
    zk_fr *tcarry, *btot_local, *btot, *total;
} zk_hscan_result;
int zk_bn254_hscan_inspect(const zk_hscan_request *req, zk_hscan_result *res);

/* The Lagrange-form transform of a base array (zk_bn254_bases_lagrange: the inverse radix-2 transform taken in the exponent), for inspection / tests: n_points
 * HOST G1 points are uploaded and the production builder is called once with a trace attached: after the scale-in launch, after every stage launch and after the
 * finish the stream is synchronised and the array copied, since every stage overwrites it in place.  No kernel and no launch differs from those of
 * zk_bn254_bases_lagrange; the profile names are its own (lagrange_scale_in, lagrange_dif_stage, lagrange_finish).  Nothing stays behind: the uploaded points and
 * the base array that the builder registers are freed on every path.
 *   request   points: n_points >= 2^log_n + 2 affine points (gnark's Montgomery image, (0, 0) = infinity); log_n <= 27.
 *   result    n = 2^log_n.  stage_points [(log_n + 1) * n * 8 words], stage_inf [(log_n + 1) * n]: array 0 is the work array after the scale-in ((1 / n) P_j),
 *             array k the same array after the k-th stage (butterflies i, i + m with m = n / 2^k), in the device's order -- the last one is the transform in
 *             bit-reversed order.  The device keeps these entries projective (XYZZ); they come back NORMALISED on the host: the affine image of the group element,
 *             whichever representative the kernels left, and stage_inf[i] = 1 where the entry is the point at infinity (its image is then (0, 0)) -- a flag of
 *             its own, read from the projective entry, so that an image of zeros under a flag of 0 is a wrong point and not an infinity.
 *             final_points [(n + 2) * 8 words], final_inf [n + 2]: the n + 2 affine points as the finish wrote them (the registered bases), final_inf[i] = 1
 *             where the device wrote (0, 0).
 * Errors, decided before a device is looked for: ZK_ERR_ARG for a null pointer, log_n above 27 and fewer than 2^log_n + 2 points. */
typedef struct {
    const zk_g1_affine *points;
    size_t n_points;
    uint32_t log_n, reserved;
} zk_lagrange_request;
typedef struct {
    uint64_t *stage_points, *final_points;
    uint8_t *stage_inf, *final_inf;
} zk_lagrange_result;
int zk_bn254_lagrange_inspect(const zk_lagrange_request *req, zk_lagrange_result *res);

/* ---- felt-vector wire codec (the data format in front of the hot path) -------------------------------------------
 * The reference hands witness values to the Go side as hex( u32 BE count || count x 32 B BE canonical felts )
 * [REF src/gnark_backend_wrapper/serialize.rs:33-47,71-106; gnark_backend_ffi/internal/backend/helpers.go:24-33
 * DeserializeFelts = hex.DecodeString + fr.Vector.UnmarshalBinary].  One kernel decodes the hex text, reverses the byte
 * order, rejects non-canonical values like gnark-crypto ("invalid fr.Element encoding": >= r is an error, not reduced) and
 * converts to the Montgomery image, writing the vector straight into HBM -- ready to be the `w` of zk_bn254_groth16_prove
 * (on_device) or the scalars of zk_bn254_msm_bases.  Errors: ZK_ERR_LEN (length does not match the count), ZK_ERR_ARG
 * (bad hex character, non-canonical felt, capacity).
 *   decode_hex      : hex on the host -> d_out (device, capacity `cap` felts); *n_out = count.
 *   decode_hex_dev  : the whole text already in HBM (d_text must sit 8 bytes before a 16-byte boundary; n = its count).
 *   decode_bytes_dev: raw fr.Vector.MarshalBinary bytes in HBM (d_raw 4 bytes before a 16-byte boundary).
 *   encode_hex      : Montgomery vector in HBM -> 8 + 64 n hex characters on the host (encode_felts), no terminator.
 *   decode_hex_rows_dev: `rows` texts of the same count n in ONE launch (the row is a grid dimension), everything in HBM.  d_text points at row 0's count
 *                     header, 8 bytes before a 16-byte boundary; row z's text starts z * pitch bytes further (pitch: a multiple of 16, at least 8 + 64 n -- a
 *                     contiguous host buffer does not give that: stage the rows with one pitched copy, e.g. to pitch 64 n + 16).  Row z's n elements go to
 *                     d_out + z * out_stride (out_stride >= n elements; the gap is not written), its verdict to d_status[z]: 0, 1 = invalid hex character,
 *                     2 = a felt >= r.  A bad row fails neither the call nor its neighbours, and every one of its n elements is still written: zero where the
 *                     felt was rejected.  The count headers are the caller's to check (they are not read).  With `stream` the call only enqueues (the status
 *                     words are cleared on that stream first) and the caller decides when to read them; stream == NULL runs on a stream of the library's and
 *                     returns when the launch is complete.  At most 65,535 rows per call, more is ZK_ERR_ARG, as are a null pointer, a pitch or stride that
 *                     does not hold a row and a misaligned d_text -- all decided before a device is looked for; rows == 0 or n == 0: ZK_OK, nothing launched. */
int zk_bn254_felts_decode_hex(const char *hex, size_t hex_len, void *d_out, size_t cap, size_t *n_out);
int zk_bn254_felts_decode_hex_dev(const void *d_text, size_t text_len, void *d_out, size_t cap, size_t n, int to_mont,
                                  void *stream);
int zk_bn254_felts_decode_bytes_dev(const void *d_raw, size_t raw_len, void *d_out, size_t cap, size_t n, int to_mont,
                                    void *stream);
int zk_bn254_felts_encode_hex(const void *d_in, size_t n, char *hex_out, size_t cap);
int zk_bn254_felts_decode_hex_rows_dev(const void *d_text, size_t pitch, size_t rows, size_t n, void *d_out, size_t out_stride,
                                       int to_mont, int *d_status /* rows */, void *stream);
/* Text rows for the verifiers (zk_plonk_verify_batch_with_vk / zk_groth16_verify_batch_with_vk), everything in HBM, the row a grid dimension (at most 65,535
 * rows per call), any pitch that holds a row and any alignment of d_text:
 *   bytes_decode_hex_rows_dev : 2 * n_bytes hex characters per row (row v at d_text + v * pitch) -> n_bytes bytes per row (at d_out + v * out_stride bytes).
 *                     Both letter cases, as Go's hex.DecodeString.  d_status[v] = ZK_ROW_OK or ZK_ROW_BAD_HEX; a rejected row's bytes are all zero.
 *   felts_public_hex_rows_dev : row v is a felt-vector text of 8 + 64 * n_values characters.  Its count header is compared with n_values, EVERY character
 *                     after it is checked for being hex, and only the felts at d_where[0 .. n_public) (device, 0-based positions < n_values; NULL when
 *                     n_public == 0) are decoded, into Montgomery form, at d_pub + v * pub_stride elements.  d_status[v] = ZK_ROW_OK, ZK_ROW_BAD_COUNT,
 *                     ZK_ROW_BAD_HEX or ZK_ROW_NOT_CANONICAL (a decoded felt >= r), the first of these that applies; a felt >= r at a position that is not
 *                     in d_where is not an error.  A rejected row's n_public elements are zeros.
 * With `stream` the calls only enqueue; stream == NULL runs on a stream of the library's and returns when the launch is complete.  A null pointer, more than
 * 65,535 rows, a pitch or stride that does not hold a row: ZK_ERR_ARG before a device is looked for; rows == 0: ZK_OK, nothing launched. */
int zk_bn254_bytes_decode_hex_rows_dev(const void *d_text, size_t pitch, size_t rows, size_t n_bytes, void *d_out, size_t out_stride,
                                       int *d_status /* rows */, void *stream);
int zk_bn254_felts_public_hex_rows_dev(const void *d_text, size_t pitch, size_t rows, size_t n_values, const uint32_t *d_where, size_t n_public,
                                       void *d_pub, size_t pub_stride, int *d_status /* rows */, void *stream);

/* ---- synthetic data on the device (bench / tests; deterministic SplitMix64 streams) -------------- */
int zk_bn254_fr_random_dev(void *d_out, size_t n, uint64_t seed, int mont, int witness_like, void *stream);
int zk_bn254_g1_generate_dev(void *d_out, size_t n, uint64_t seed, void *stream); /* P_i = k_i * G1 */
int zk_bn254_g2_generate_dev(void *d_out, size_t n, uint64_t seed, void *stream); /* P_i = k_i * G2 */
int zk_bn254_fr_mul_dev(void *d_out, const void *d_a, const void *d_b, size_t n, void *stream); /* out = a*b (Montgomery) */

/* ---- kzg.NewSRS(size, alpha) (gnark-crypto ecc/bn254/fr/kzg; the reference: backend/common.go:137 with size 1_000_000, main.go:176):
 * d_g1_out[i] = alpha^i * G1 for i < size, on the device (register it with zk_bn254_bases_register_dev); g2_out = [G2, alpha * G2] on the
 * host.  alpha: Montgomery fr.Element (toxic waste: the caller's business, exactly as upstream's test-only constructor). */
int zk_bn254_kzg_new_srs_dev(void *d_g1_out, size_t size, const zk_fr *alpha, zk_g2_affine g2_out[2], void *stream);
/* kzg.SRS.ReadFrom / WriteTo (what LoadSRS / SaveSRS move through srs.hex: backend/common.go:86-125, re-read on every call at
 * backend/plonk/plonk.go:16,34,58): G2[0] | G2[1] (64 B compressed) | u32 BE count | count x 32 B compressed G1, as bytes or hex text.
 * _read decompresses the G1 points on the device (one square root each) straight into a registered base array (window tables per
 * table_window_bits as in zk_bn254_bases_register_cfg) and returns the two G2 points; _write is the inverse.  Errors: ZK_ERR_LEN (size
 * does not match the count), ZK_ERR_ARG (bad hex, bad flags, x >= q, no square root, G2 point outside the r-torsion). */
int zk_bn254_kzg_srs_read(const void *data, size_t len, int is_hex, int table_window_bits, uint64_t *handle, size_t *n_g1,
                          zk_g2_affine g2_out[2]);
int zk_bn254_kzg_srs_write(uint64_t handle, const zk_g2_affine g2[2], int as_hex, void *out, size_t cap, size_t *out_len);
/* The two G2 points of an SRS image, on the HOST: all that plonk.Verify needs of the SRS (backend/plonk/plonk.go:28-51 re-reads the whole file for it).  No
 * device work: a process that only verifies never starts the HIP runtime.  Header and length are checked as in _read; the G1 points are not looked at. */
int zk_bn254_kzg_srs_g2(const void *data, size_t len, int is_hex, zk_g2_affine g2_out[2]);

/* ---- KZG openings: the rest of gnark-crypto v0.9.1's kzg package (ecc/bn254/fr/kzg/kzg.go: Open, BatchOpenSinglePoint, FoldProof, Verify,
 * BatchVerifySinglePoint, BatchVerifyMultiPoints) [UPSTREAM-RECALL].  plonk.Prove's last round is BatchOpenSinglePoint of seven polynomials at zeta and Open of
 * Z at omega zeta (gnark v0.8.0 backend/plonk/bn254/prove.go, reached from gnark_backend_ffi/backend/plonk/plonk.go:67); plonk.Verify ends in
 * BatchVerifySinglePoint and Verify.  zk_kzg_opening is kzg.OpeningProof{H, ClaimedValue}; a kzg.BatchOpeningProof{H, ClaimedValues} travels as h + claimed[count].
 * The hash of deriveGamma (the folding challenge: a one-challenge fiatshamir transcript "gamma" over the point, the digests' RawBytes and the claimed values) is
 * SHA-256 ONLY -- what gnark's PLONK passes; upstream takes any hash.Hash.
 * Proving side, on the DEVICE.  srs: a registered G1 base array (zk_bn254_bases_register*, zk_bn254_kzg_srs_read), on ONE device entry: a handle spread over
 * several entries (device_mask) is refused with ZK_ERR_ARG.  polys[k]: lens[k] Montgomery coefficients, host pointers, or device pointers if on_device.
 *   zk_bn254_kzg_open : `count` >= 1 independent openings, polynomial k at points[k]: out[k].claimed_value = p_k(z_k), out[k].h = Commit((p_k - p_k(z_k)) / (X - z_k)).
 *                       count == 1 is kzg.Open.  All rows share one set of scan launches (polynomial, length and point are indexed per row) and up to three
 *                       quotients one multi-scalar multiplication when the SRS has a window table; eight rows are in flight at a time.
 *   zk_bn254_kzg_batch_open_single_point : kzg.BatchOpenSinglePoint -- out_claimed[k] = p_k(point); gamma = deriveGamma(point, digests, out_claimed);
 *                       *out_h = Commit((sum_k gamma^k p_k - sum_k gamma^k p_k(point)) / (X - point)).  Any count; lengths may differ.
 *   Errors: count == 0 or a null array ZK_ERR_ARG; an unknown handle ZK_ERR_HANDLE; a length of 0 or above the SRS's size ZK_ERR_LEN ("kzg: invalid polynomial
 *   size (larger than SRS or == 0)", ErrInvalidPolynomialSize).  A constant polynomial (length 1) has an empty quotient: h = infinity, no error -- what upstream
 *   does with it is unpinned.  Without a GPU: ZK_ERR_NO_DEVICE after the checks that need no handle; there is no CPU fallback.
 * Verifying side.  Points are affine Montgomery images and are not validated (as zk_bn254_pairing_check); srs_g2 = ([1]2, [alpha]2).
 *   zk_bn254_kzg_verify (HOST, never starts the HIP runtime) : kzg.Verify -- e(C - v G + z H, [1]2) e(-H, [alpha]2) == 1; *accepted = 1 / 0.
 *   zk_bn254_kzg_fold_proof (HOST) : kzg.FoldProof -- out_opening = {h, sum_k gamma^k claimed[k]}, out_digest = sum_k gamma^k digests[k].
 *   zk_bn254_kzg_batch_verify_single_point (HOST) : kzg.BatchVerifySinglePoint = fold, then verify.
 *   zk_bn254_kzg_verify_batch (DEVICE) : kzg.BatchVerifyMultiPoints with a verdict per opening: accepted[i] equals what zk_bn254_kzg_verify says of (digests[i],
 *                       openings[i], points[i]).  The openings are first checked together, e(sum_i lambda_i (C_i - v_i G + z_i H_i), [1]2)
 *                       e(-sum_i lambda_i H_i, [alpha]2) == 1 -- two Miller loops whatever n is -- with lambda_i = the low 128 bits of SHA-256("zkmi-kzg-batch" ||
 *                       SHA-256(srs_g2) || SHA-256(digests || openings || points) || u64 i little-endian), forced non-zero: derived, not random (upstream draws
 *                       them), so results are reproducible; a batch with a wrong opening passes with probability about 2^-128 in the random-oracle model.  If
 *                       that check fails, every opening gets its own two-pairing check on the device.  Chunks of at most 2^16 openings; about 4.3 KB of
 *                       device workspace per opening of a chunk; one stream slot per call.  ZK_ERR_NO_DEVICE without a GPU, after the null-pointer checks. */
typedef struct { zk_g1_affine h; zk_fr claimed_value; } zk_kzg_opening;
int zk_bn254_kzg_open(uint64_t srs, const void *const *polys, const size_t *lens, const zk_fr *points, size_t count, int on_device, zk_kzg_opening *out);
int zk_bn254_kzg_batch_open_single_point(uint64_t srs, const void *const *polys, const size_t *lens, const zk_g1_affine *digests, size_t count,
                                         const zk_fr *point, int on_device, zk_g1_affine *out_h, zk_fr *out_claimed);
int zk_bn254_kzg_verify(const zk_g1_affine *digest, const zk_kzg_opening *opening, const zk_fr *point, const zk_g2_affine srs_g2[2], int *accepted);
int zk_bn254_kzg_fold_proof(const zk_g1_affine *digests, size_t count, const zk_g1_affine *h, const zk_fr *claimed, const zk_fr *point,
                            zk_kzg_opening *out_opening, zk_g1_affine *out_digest);
int zk_bn254_kzg_batch_verify_single_point(const zk_g1_affine *digests, size_t count, const zk_g1_affine *h, const zk_fr *claimed, const zk_fr *point,
                                           const zk_g2_affine srs_g2[2], int *accepted);
int zk_bn254_kzg_verify_batch(const zk_g1_affine *digests, const zk_kzg_opening *openings, const zk_fr *points, size_t n_openings,
                              const zk_g2_affine srs_g2[2], uint8_t *accepted, size_t *n_accepted);

/* ---- device memory plumbing for hosts without a HIP binding (ctypes tests, the cgo shim) ------------------------ */
int zk_dev_alloc(void **d_ptr, size_t bytes);
int zk_dev_free(void *d_ptr);
int zk_dev_h2d(void *d_dst, const void *h_src, size_t bytes);
int zk_dev_d2h(void *h_dst, const void *d_src, size_t bytes);
int zk_dev_sync(void);

/* ---- per-kernel timing (hipEvent pairs on the stream the kernels run on; feeds bench.py's roofline object) ------- */
int zk_profile_enable(int on);
/* a host-side section of a caller above the C ABI (libgnark_backend.so's SRS handling), accounted beside the library's own; no-op unless profiling is on */
int zk_profile_host(const char *name, double ms);                 /* 1: record an event pair around every kernel launch */
int zk_profile_reset(void);
int zk_profile_count(void);                    /* number of distinct kernel names seen */
int zk_profile_get(int idx, char *name_out, size_t name_cap, uint64_t *launches, double *total_ms);

/* ---- host-only self test (runs WITHOUT a GPU): the shared 32-bit-limb field / XYZZ code vs the 64-bit host code;
 * returns the number of mismatches (0 = ok). */
int zk_selftest_host(void);

#ifdef __cplusplus
}
#endif
#endif /* ZKMI_H */
