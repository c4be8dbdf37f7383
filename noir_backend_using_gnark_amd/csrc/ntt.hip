// Radix-2 NTT over BN254 Fr on gfx950, with the exact in-place semantics of gnark-crypto v0.9.1
// `(*fft.Domain).FFT / FFTInverse` and `fft.BitReverse` (ecc/bn254/fr/fft; pinned at
// /root/reference/gnark_backend_ffi/go.mod:5; reached through groth16.Prove main.go:131 and plonk.Prove
// backend/plonk/plonk.go:67), plus gnark v0.8.0's `computeH` fused on the device.
//
// Structure: the log2(N) butterfly stages are grouped in passes; a pass keeps a tile of 2^k * L elements in LDS and
// runs k stages on it (one workgroup per tile), so HBM is touched once per pass instead of once per stage.
//   * tile  = every value of the k transformed index bits  x  L consecutive values of the lower bits  (so global
//     loads/stores are L*32-byte contiguous runs; the pass over the lowest bits has L = 1 and is fully contiguous)
//   * LDS layout = two uint4 arrays (low / high 16 bytes of each element): a wave reading consecutive elements
//     issues conflict-free ds_read_b128 / ds_write_b128
//   * the in-place DIF (natural -> bit-reversed) and DIT (bit-reversed -> natural) orders fall out of doing the
//     butterflies in place -- there is no transpose and no separate permutation pass
//   * coset / 1/N scalings are folded into the first stage's loads (pre table) or the last stage's stores (post)
// Roofline: 64 B per element per transform algorithmic (read + write once).  On CDNA4 the transform is VALU-bound, not HBM-bound: a butterfly is 327
// VALU instructions, 206 of them the 9 x 29-bit Montgomery product (162 v_mad_u64_u32, which issue at the rate of an add-with-carry -- 4.4-4.8 cycles per
// wave instruction, NOT quarter rate: DESIGN.md 3.1, tools/ubench.hip) -- see DESIGN.md 3.3.
#include <vector>

#include <algorithm>

#include "ctx.hpp"
#include "ff.hpp"
#include "host_ff.hpp"
#include "ntt.hpp"
#include "multidev.hpp"
#include "ff29.hpp"

namespace zkmi {

// TILE_LOG, K_STRIDED and plan_passes() below are re-stated in tests/ntt_shapes.py (plan_passes), from which tests/test_ntt_shapes_cpu.py checks that the swept
// sizes run every pass shape: change them there too.
static constexpr unsigned TILE_LOG = 11;        // 2048 elements = 64 KiB of LDS per workgroup
static constexpr unsigned K_STRIDED = 9;         // strided passes: k <= 9, rows of L >= 4 elements (128-byte runs); 2^20 = 11 + 9 bits = two passes

struct PowBasis {
    Fr pw[28];  // base^(2^b)
};

__device__ __forceinline__ unsigned bitrev_u32(unsigned i, unsigned logn) { return logn ? (__brev(i) >> (32 - logn)) : 0; }

// out[i] = scale * base^(i) or base^(bitrev(i))
__global__ void k_pow_table(Fr* out, size_t n, unsigned logn, PowBasis basis, Fr scale, int reversed, size_t offset) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    unsigned e = reversed ? bitrev_u32((unsigned)(i + offset), logn) : (unsigned)(i + offset);
    Fr acc = scale;
    for (unsigned b = 0; b < 28; b++)
        if ((e >> b) & 1) acc = acc * basis.pw[b];
    out[i] = acc;
}

struct PassArgs {
    Fr* data;
    const Fr* tw;        // w^i, i < N/2  (forward or inverse table)
    const Fr* pre;       // multiply element i by pre[i] on entry of the pass's first stage (or null)
    const Fr* post;      // multiply element i by post[i] on exit of the pass's last stage (or null)
    Fr post_const;       // if has_post_const: multiply by this constant on exit
    unsigned logn, bit_lo, k, logL;
    int dif, has_post_const;
    int canonical;       // 29-bit-limb passes: last pass of the transform -> canonical image; else a lazily reduced 256-bit intermediate
    const Fr* tw2;       // fused inverse-then-forward pass (k_ntt_pass29_if): twiddles of the forward half
    const Fr* src;       // 29-bit-limb passes: read the tile from here instead of `data` (first pass of an out-of-place transform) or null
    const Fr* sub;       // 29-bit-limb passes, last stage: after `post`, element i becomes (x - sub[i]) * post_const  (computeH's closing step) or null
    Fr* data2;           // 29-bit-limb passes launched with gridDim.y = 2 or 3: the workgroups with blockIdx.y = 1 / 2 run the same pass on these vectors
    const Fr* src2;      // (src2 -> data2, src3 -> data3).  In k_ntt_pass29_if the third vector only takes the inverse half, closed by post_const (computeH's c)
    Fr* data3;
    const Fr* src3;
    uint32_t unit_skip;  // 1: the stage on index bit 0 skips its product by the unit twiddle (0: A/B switch ZKMI_NTT_UNIT=0)
    uint32_t tw_and;     // EXPERIMENT (ZKMI_NTT_TWMASK): twiddle index mask -- 0xffffffff in production; a small mask makes every twiddle load an L1 hit
                         // (wrong results, right timing): the upper bound of what any twiddle-staging scheme could gain
};

__device__ __forceinline__ Fr lds_load(const uint4* lo, const uint4* hi, unsigned t) {
    uint4 a = lo[t], b = hi[t];
    Fr r;
    r.l[0] = a.x; r.l[1] = a.y; r.l[2] = a.z; r.l[3] = a.w;
    r.l[4] = b.x; r.l[5] = b.y; r.l[6] = b.z; r.l[7] = b.w;
    return r;
}
__device__ __forceinline__ void lds_store(uint4* lo, uint4* hi, unsigned t, const Fr& v) {
    lo[t] = make_uint4(v.l[0], v.l[1], v.l[2], v.l[3]);
    hi[t] = make_uint4(v.l[4], v.l[5], v.l[6], v.l[7]);
}
__device__ __forceinline__ Fr gload_fr(const Fr* p) {
    const uint4* q = reinterpret_cast<const uint4*>(p);
    uint4 a = q[0], b = q[1];
    Fr r;
    r.l[0] = a.x; r.l[1] = a.y; r.l[2] = a.z; r.l[3] = a.w;
    r.l[4] = b.x; r.l[5] = b.y; r.l[6] = b.z; r.l[7] = b.w;
    return r;
}

// ------------------------------------------------------------------------------------------------ 29-bit-limb passes
// The butterflies run in the unsaturated representation of ff29.hpp (Fr29): 1.4x fewer instructions per product than 8 x 32-bit
// limbs, additions without carries.  Elements sit in LDS as 9 limbs (two 16-byte halves + the top limb) between the stage
// groups of a pass and as 8 packed words at its ends; A.tw is the w * 2^261 table.  Schedules and bounds: tools/u29_ntt_model.py.
__device__ __forceinline__ U29 lds_load9(const uint4* lo, const uint4* hi, const uint32_t* top, unsigned t) {
    uint4 a = lo[t], b = hi[t];
    U29 r;
    r.l[0] = a.x; r.l[1] = a.y; r.l[2] = a.z; r.l[3] = a.w;
    r.l[4] = b.x; r.l[5] = b.y; r.l[6] = b.z; r.l[7] = b.w;
    r.l[8] = top[t];
    return r;
}
__device__ __forceinline__ void lds_store9(uint4* lo, uint4* hi, uint32_t* top, unsigned t, const U29& v) {
    lo[t] = make_uint4(v.l[0], v.l[1], v.l[2], v.l[3]);
    hi[t] = make_uint4(v.l[4], v.l[5], v.l[6], v.l[7]);
    top[t] = v.l[8];
}

// What a pass does at its two ends is a compile-time MODE, resolved against the kernel arguments where it is used (a struct of pointers built once per kernel
// keeps them all in scalar registers for the whole kernel, and the hot loop pays for the spills: measured 4 % on a 2^24-point transform):
//   0  a plain pass: A.tw, entry table A.pre, exit table A.post or the constant A.post_const, canonical image if A.canonical
//   1  inverse half of k_ntt_pass29_if: A.tw, exit table A.post, limbs stay unpacked
//   2  forward half of k_ntt_pass29_if: A.tw2, no tables, canonical image if A.canonical
//   3  k_ntt_pass29_if's third vector, a plain FFTInverse ending: A.tw, * A.post_const, canonical image
// SUB (compile-time too: its extra live values would cost every other pass a wave of occupancy) adds computeH's closing step.
// op_off: `pre` and `sub` may be operands of the workgroup's row, found op_off elements further on (0 where every row shares the table).
template <int G, bool DIF, unsigned THREADS, bool SUB, int MODE, bool UNIT>
__device__ __forceinline__ void ntt_group29(const PassArgs& A, uint4* lo, uint4* hi, uint32_t* top, size_t base, unsigned E, unsigned s0,
                                            bool load_packed, bool apply_pre, bool apply_post, bool store_packed, size_t op_off) {
    constexpr unsigned NE = 1u << G;
    const unsigned L = 1u << A.logL;
    const unsigned ql = DIF ? (A.k - s0 - G) : s0;
    for (unsigned u = threadIdx.x; u < (E >> G); u += THREADS) {
        const unsigned l = u & (L - 1), r = u >> A.logL;
        const unsigned mid0 = ((r >> ql) << (ql + G)) | (r & ((1u << ql) - 1));
        U29 x[NE];
#pragma unroll
        for (unsigned e = 0; e < NE; e++) {
            const unsigned t = ((mid0 | (e << ql)) << A.logL) + l;
            x[e] = load_packed ? u29_unpack(lds_load(lo, hi, t)) : lds_load9(lo, hi, top, t);
            if (MODE == 0 && apply_pre && A.pre) x[e] = u29r_mul(x[e], u29r_load5(gload_fr(A.pre + op_off + base + ((size_t)(mid0 | (e << ql)) << A.bit_lo) + l)));
        }
#pragma unroll
        for (int sl = 0; sl < G; sl++) {
            const unsigned bitl = DIF ? (unsigned)(G - 1 - sl) : (unsigned)sl;
            const unsigned b = A.bit_lo + ql + bitl;
#pragma unroll
            for (unsigned e0 = 0; e0 < NE; e0++) {
                if (e0 & (1u << bitl)) continue;
                const unsigned e1 = e0 | (1u << bitl);
                const size_t g0 = base + ((size_t)(mid0 | (e0 << ql)) << A.bit_lo) + l;
                const size_t j = g0 & (((size_t)1 << b) - 1);
                // the stage on index bit 0 (the last of a DIF transform, the first of a DIT one) has no twiddles: its product by the unit is replaced by a
                // partial reduction (DIF) or dropped (DIT) -- one product in 20 at 2^20; same values mod r, bounds in tools/u29_ntt_model.py (`unit`).
                // UNIT is a property of the GROUP (it holds index bit 0), chosen by the caller: a run-time test here would sit in every group's bitl == 0
                // stage and cut the butterflies' instruction streams apart -- measured: 3 % on a 2^26-point transform, more than the skipped product gives
                // In that group the stage on bit 1 has unit twiddles too, for the butterflies whose low element has bit 0 clear (e0 even): half of them.
                // (Stage 2's quarter would meet sums of four elements, whose limbs no bias covers.)
                constexpr bool unit_ct = UNIT;
                const bool unit = unit_ct && (bitl == 0 || (bitl == 1 && (e0 & 1u) == 0));
                U29 w;
                if (!unit) w = u29_unpack(gload_fr((MODE == 2 ? A.tw2 : A.tw) + ((j << (A.logn - 1 - b)) & A.tw_and)));
                if (DIF) {
                    U29 d;
                    if (sl == 0) d = u29r_sub<16>(x[e0], x[e1]);
                    else if (sl == 1) d = u29r_sub<24>(x[e0], x[e1]);
                    else d = u29r_sub<40>(x[e0], x[e1]);
                    x[e0] = u29_wnorm(u29_add(x[e0], x[e1]));
                    x[e1] = unit ? u29r_reduce(u29_wnorm(d)) : u29r_mul(d, w);
                } else {
                    const U29 t = unit ? x[e1] : u29r_mul(x[e1], w);
                    // a unit twiddle on bit 1 meets an element that is already the sum of two (< 4.4 r, limbs < 2^30): 16 r instead of 4 r
                    x[e1] = u29_wnorm((unit && bitl == 1) ? u29r_sub<16>(x[e0], t) : u29r_sub<4>(x[e0], t));
                    x[e0] = u29_add(x[e0], t);
                }
            }
        }
        if (DIF) {
            x[0] = u29r_reduce(x[0]);  // the all-sums output is the only one that grows (8x per group)
        } else {
#pragma unroll
            for (unsigned e = 0; e < NE; e++) x[e] = u29_wnorm(x[e]);
        }
#pragma unroll
        for (unsigned e = 0; e < NE; e++) {
            const unsigned t = ((mid0 | (e << ql)) << A.logL) + l;
            if (apply_post) {
                if ((MODE == 0 || MODE == 1) && A.post) x[e] = u29r_mul(x[e], u29r_load5(gload_fr(A.post + base + ((size_t)(mid0 | (e << ql)) << A.bit_lo) + l)));
                else if (MODE == 3 || (MODE == 0 && A.has_post_const)) x[e] = u29r_mul(x[e], u29r_load5(A.post_const));
                if (SUB) {  // x < 2 r after the product above; sub[i] canonical: the difference stays below 6 r, a legal multiplicand (tools/u29_ntt_model.py)
                    const U29 c = u29_unpack(gload_fr(A.sub + op_off + base + ((size_t)(mid0 | (e << ql)) << A.bit_lo) + l));
                    x[e] = u29r_mul(u29r_sub<4>(x[e], c), u29r_load5(A.post_const));
                }
            }
            if (store_packed) lds_store(lo, hi, t, u29r_pack(u29r_reduce(x[e]), MODE == 3 || A.canonical != 0));
            else lds_store9(lo, hi, top, t, x[e]);
        }
    }
}

// all k stages of a pass, GMAX at a time.  packed_in / packed_out: the tile sits in LDS as 8 packed words before / after.
template <int GMAX, unsigned THREADS, bool DIF, bool SUB, int MODE>
__device__ __forceinline__ void ntt_stages29(const PassArgs& A, uint4* lo, uint4* hi, uint32_t* top, size_t base, unsigned E, bool packed_in, bool packed_out,
                                             size_t op_off) {
    for (unsigned s0 = 0; s0 < A.k;) {
        const unsigned G = (A.k - s0 >= (unsigned)GMAX) ? (unsigned)GMAX : (A.k - s0);
        const bool first = (s0 == 0), last = (s0 + G == A.k);
        const bool lp = first && packed_in, sp = last && packed_out;
        const bool ug = A.unit_skip && A.bit_lo == 0 && (DIF ? last : first);  // the group that holds index bit 0 (uniform)
        if (ug) {
            if (GMAX >= 3 && G == 3) ntt_group29<(GMAX >= 3 ? 3 : 1), DIF, THREADS, SUB, MODE, true>(A, lo, hi, top, base, E, s0, lp, first, last, sp, op_off);
            else if (G == 2) ntt_group29<2, DIF, THREADS, SUB, MODE, true>(A, lo, hi, top, base, E, s0, lp, first, last, sp, op_off);
            else ntt_group29<1, DIF, THREADS, SUB, MODE, true>(A, lo, hi, top, base, E, s0, lp, first, last, sp, op_off);
        } else {
            if (GMAX >= 3 && G == 3) ntt_group29<(GMAX >= 3 ? 3 : 1), DIF, THREADS, SUB, MODE, false>(A, lo, hi, top, base, E, s0, lp, first, last, sp, op_off);
            else if (G == 2) ntt_group29<2, DIF, THREADS, SUB, MODE, false>(A, lo, hi, top, base, E, s0, lp, first, last, sp, op_off);
            else ntt_group29<1, DIF, THREADS, SUB, MODE, false>(A, lo, hi, top, base, E, s0, lp, first, last, sp, op_off);
        }
        s0 += G;
        __syncthreads();
    }
}

// which vector a workgroup works on (gridDim.y = 1 .. 3): resolved once, in scalar registers.  Masks instead of ?: on purpose -- a conditional between two
// members of the kernel-argument struct is a conditional between their ADDRESSES, which makes the compiler keep a copy of the whole struct in scratch memory
__device__ __forceinline__ uintptr_t pick3(uintptr_t v0, uintptr_t v1, uintptr_t v2) {
    const uintptr_t m1 = (uintptr_t)0 - (uintptr_t)(blockIdx.y == 1), m2 = (uintptr_t)0 - (uintptr_t)(blockIdx.y == 2);
    return (v0 & ~(m1 | m2)) | (v1 & m1) | (v2 & m2);
}

// One launch takes the pass over MANY vectors of one domain: blockIdx.z is the row (a single vector is rows = 1), blockIdx.y the vector a / b / c of computeH.
// What belongs to a row moves by row * stride elements (stride >= N): data / data2 / data3, src / src2 / src3, and `pre` / `sub` where they are operands of the
// row (computeH's closing transform: pre = b, sub = c; op_stride = 0 where every row shares the table).  Twiddles, a coset table in `post`, tw2: one per domain.
// One workgroup handles one tile of one row, so a domain below 2^11 leaves lanes of its 512 idle.
struct RowArgs {
    size_t stride, op_stride;  // in Fr elements
};
// the row's byte offset joins the vector's address before tile_copy_in / tile_copy_out restate its address space: resolved once per workgroup, in scalar registers
__device__ __forceinline__ Fr* row_data(const PassArgs& A, size_t off) {
    return reinterpret_cast<Fr*>(pick3((uintptr_t)A.data, (uintptr_t)A.data2, (uintptr_t)A.data3) + off * sizeof(Fr));
}
__device__ __forceinline__ const Fr* row_src(const PassArgs& A, const Fr* data, size_t off) {
    const uintptr_t src = pick3((uintptr_t)A.src, (uintptr_t)A.src2, (uintptr_t)A.src3);
    return src ? reinterpret_cast<const Fr*>(src + off * sizeof(Fr)) : data;
}
template <unsigned THREADS>
__device__ __forceinline__ void tile_copy_in(const Fr* src, unsigned logL, unsigned bit_lo, uint4* lo, uint4* hi, size_t base, unsigned E) {
    const unsigned L = 1u << logL;
    // the pointer went through integer masks (pick3): tell the compiler again that it is global memory, or it emits flat_load / flat_store
#ifdef __HIP_DEVICE_COMPILE__
    typedef __attribute__((address_space(1))) const uint4 g_uint4;
    const g_uint4* g = (const g_uint4*)(uintptr_t)src;
#else
    const uint4* g = reinterpret_cast<const uint4*>(src);  // host pass: never executed
#endif
    for (unsigned h = threadIdx.x; h < 2 * E; h += THREADS) {
        unsigned e = h >> 1, half = h & 1;
        unsigned mid = e >> logL, l = e & (L - 1);
        size_t gi = base + ((size_t)mid << bit_lo) + l;
        (half ? hi : lo)[e] = g[gi * 2 + half];
    }
}
template <unsigned THREADS>
__device__ __forceinline__ void tile_copy_out(Fr* dst, unsigned logL, unsigned bit_lo, const uint4* lo, const uint4* hi, size_t base, unsigned E) {
    const unsigned L = 1u << logL;
#ifdef __HIP_DEVICE_COMPILE__
    typedef __attribute__((address_space(1))) uint4 g_uint4;
    g_uint4* g = (g_uint4*)(uintptr_t)dst;
#else
    uint4* g = reinterpret_cast<uint4*>(dst);
#endif
    for (unsigned h = threadIdx.x; h < 2 * E; h += THREADS) {
        unsigned e = h >> 1, half = h & 1;
        unsigned mid = e >> logL, l = e & (L - 1);
        size_t gi = base + ((size_t)mid << bit_lo) + l;
        g[gi * 2 + half] = (half ? hi : lo)[e];
    }
}

// The passes are launched with radix-4 groups on 512 lanes: two workgroups per CU (4 waves per SIMD, <= 128 VGPRs).  The register counts are
// what -Rpass-analysis=kernel-resource-usage shows (121, 125 with SUB, 107 for k_ntt_pass29_if); asking for them with __launch_bounds__(512, 4) gives the same
// counts and a schedule that is 1.5 % slower on a 2^26-point transform (measured), so the bound stays implicit -- check the remark when touching the kernels.
#define ZK_NTT_BOUNDS(THREADS) __launch_bounds__(THREADS)

template <int GMAX, unsigned THREADS, bool SUB = false>
__global__ ZK_NTT_BOUNDS(THREADS) void k_ntt_pass29(PassArgs A, RowArgs R) {
    prio_mid();
    extern __shared__ uint4 lds[];
    const unsigned E = 1u << (A.k + A.logL);
    uint4* lo = lds;
    uint4* hi = lds + E;
    uint32_t* top = reinterpret_cast<uint32_t*>(lds + 2 * E);
    const unsigned lo_blks = (1u << A.bit_lo) >> A.logL;  // >= 1
    const size_t tile = blockIdx.x;
    const size_t hi_idx = tile / lo_blks;
    const unsigned lo_blk = (unsigned)(tile % lo_blks);
    const size_t base = (hi_idx << (A.bit_lo + A.k)) + ((size_t)lo_blk << A.logL);
    const size_t row = blockIdx.z;
    Fr* const data = row_data(A, row * R.stride);
    tile_copy_in<THREADS>(row_src(A, data, row * R.stride), A.logL, A.bit_lo, lo, hi, base, E);
    __syncthreads();
    if (A.dif) ntt_stages29<GMAX, THREADS, true, SUB, 0>(A, lo, hi, top, base, E, true, true, row * R.op_stride);
    else ntt_stages29<GMAX, THREADS, false, SUB, 0>(A, lo, hi, top, base, E, true, true, row * R.op_stride);
    tile_copy_out<THREADS>(data, A.logL, A.bit_lo, lo, hi, base, E);
}

// computeH runs FFTInverse(DIF) immediately followed by FFT(DIT, coset) on the same vector: the inverse transform ENDS with the
// contiguous pass over the low index bits and the forward transform BEGINS with it, on the same tiles -- so the two passes are one
// kernel: load tile, k DIF stages (A.tw), * A.post (1/N * g^bitrev(i): the domain's table, shared by the rows), k DIT stages (A.tw2), store.
// One HBM round trip saved per vector.
template <int GMAX, unsigned THREADS>
__global__ ZK_NTT_BOUNDS(THREADS) void k_ntt_pass29_if(PassArgs A, RowArgs R) {
    prio_mid();
    extern __shared__ uint4 lds[];
    const unsigned E = 1u << (A.k + A.logL);
    uint4* lo = lds;
    uint4* hi = lds + E;
    uint32_t* top = reinterpret_cast<uint32_t*>(lds + 2 * E);
    const size_t base = (size_t)blockIdx.x << A.k;  // contiguous tiles only (bit_lo = 0, logL = 0)
    const size_t off = (size_t)blockIdx.z * R.stride;
    Fr* const data = row_data(A, off);
    tile_copy_in<THREADS>(row_src(A, data, off), 0, 0, lo, hi, base, E);
    __syncthreads();
    if (blockIdx.y == 2) {  // the third vector: a plain FFTInverse ending (* post_const, canonical image)
        ntt_stages29<GMAX, THREADS, true, false, 3>(A, lo, hi, top, base, E, true, true, 0);
    } else {
        ntt_stages29<GMAX, THREADS, true, false, 1>(A, lo, hi, top, base, E, true, false, 0);   // inverse half; its post table is applied, limbs stay unpacked
        ntt_stages29<GMAX, THREADS, false, false, 2>(A, lo, hi, top, base, E, false, true, 0);  // forward half
    }
    tile_copy_out<THREADS>(data, 0, 0, lo, hi, base, E);
}

// a[row * stride] *= t[0]: the N == 1 transform of `rows` rows of one element
__global__ void k_scale_table_rows(Fr* a, size_t stride, const Fr* t, size_t rows) {
    prio_mid();
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < rows) a[i * stride] = a[i * stride] * gload_fr(t);
}

// a[i] *= t[i]  (the coset factor a sharded transform applies outside its block transform)
__global__ void k_scale_table(Fr* a, const Fr* t, size_t n) {
    prio_mid();
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) a[i] = a[i] * gload_fr(t + i);
}

__global__ void k_bit_reverse(Fr* a, unsigned logn) {
    prio_mid();
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t n = (size_t)1 << logn;
    if (i >= n) return;
    size_t j = bitrev_u32((unsigned)i, logn);
    if (i < j) {
        Fr x = gload_fr(a + i), y = gload_fr(a + j);
        a[i] = y;
        a[j] = x;
    }
}

// h = (a*b - c) * den    (gnark computeH pointwise step)
__global__ void k_h_pointwise(Fr* a, const Fr* b, const Fr* c, Fr den, size_t n) {
    prio_mid();
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Fr x = gload_fr(a + i) * gload_fr(b + i) - gload_fr(c + i);
    a[i] = x * den;
}

// h = (u - c) * den: the last step of computeH when c stays in coefficient form (see compute_h_rows_inplace)
__global__ void k_h_final(Fr* u, const Fr* c, Fr den, size_t n) {
    prio_mid();
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    u[i] = (gload_fr(u + i) - gload_fr(c + i)) * den;
}

__global__ void k_fr_mul(Fr* out, const Fr* a, const Fr* b, size_t n) {
    prio_mid();
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = gload_fr(a + i) * gload_fr(b + i);
}

// ---------------------------------------------------------------------------------------------- domain tables
static const uint64_t ROOT_2_28_MONT[4] = {0x636e735580d13d9cULL, 0xa22bf3742445ffd6ULL, 0x56452ac01eb203d8ULL, 0x1860ef942963f9e7ULL};

static std::mutex g_dom_mu;
static std::map<unsigned, Domain*> g_domains;  // by (device entry, log n): the tables live in the HBM of the entry that built them

static Fr to_dev(const HFr& h) {
    Fr r;
    memcpy(&r, &h, 32);
    return r;
}

static int make_pow_table(Slot* s, hipStream_t st, Fr** out, size_t n, unsigned logn, HFr base, HFr scale, int reversed, size_t offset = 0) {
    ZK_HIP(hipMalloc((void**)out, (n ? n : 1) * sizeof(Fr)));
    PowBasis pb;
    HFr p = base;
    for (int b = 0; b < 28; b++) {
        pb.pw[b] = to_dev(p);
        p = p.sqr();
    }
    unsigned grid = (unsigned)((n + 255) / 256);
    ZK_LAUNCH(s, st, "pow_table", k_pow_table, dim3(grid ? grid : 1), dim3(256), 0, *out, n, logn, pb, to_dev(scale), reversed, offset);
    return ZK_OK;
}

int get_domain(Slot* s, hipStream_t st, unsigned logn, unsigned need, Domain** out) {
    if (logn > 28) return set_err(ZK_ERR_ARG, "log_n = %u exceeds Fr two-adicity 28", logn);
    std::lock_guard<std::mutex> lk(g_dom_mu);
    Domain*& d = g_domains[((unsigned)current_entry() << 8) | logn];
    if (!d) {
        d = new Domain();
        d->logn = logn;
        HFr w;
        memcpy(&w, ROOT_2_28_MONT, 32);
        for (unsigned i = logn; i < 28; i++) w = w.sqr();
        d->gen = w;
        d->gen_inv = w.inv();
        HFr n = HFr{{(uint64_t)1 << logn, 0, 0, 0}}.to_mont();
        d->card_inv = n.inv();
        d->coset = HFr{{5, 0, 0, 0}}.to_mont();
        d->coset_inv = d->coset.inv();
    }
    size_t N = (size_t)1 << logn, H = N > 1 ? N / 2 : 1;
    bool made = false;
    if ((need & DOM_TW) && !d->tw) { ZK_TRY(make_pow_table(s, st, &d->tw, H, logn, d->gen, HFr::one(), 0)); made = true; }
    if ((need & DOM_TW_INV) && !d->tw_inv) { ZK_TRY(make_pow_table(s, st, &d->tw_inv, H, logn, d->gen_inv, HFr::one(), 0)); made = true; }
    // the same powers times 2^5: w * 2^261 mod r, the multiplier form of the 29-bit-limb passes
    const HFr two5 = HFr{{32, 0, 0, 0}}.to_mont();
    if ((need & DOM_TW) && !d->tw29) { ZK_TRY(make_pow_table(s, st, &d->tw29, H, logn, d->gen, two5, 0)); made = true; }
    if ((need & DOM_TW_INV) && !d->tw29_inv) { ZK_TRY(make_pow_table(s, st, &d->tw29_inv, H, logn, d->gen_inv, two5, 0)); made = true; }
    if ((need & DOM_COSET) && !d->coset_tab) { ZK_TRY(make_pow_table(s, st, &d->coset_tab, N, logn, d->coset, HFr::one(), 0)); made = true; }
    if ((need & DOM_COSET_REV) && !d->coset_rev) { ZK_TRY(make_pow_table(s, st, &d->coset_rev, N, logn, d->coset, HFr::one(), 1)); made = true; }
    if ((need & DOM_COSET_INV_N) && !d->coset_inv_n) { ZK_TRY(make_pow_table(s, st, &d->coset_inv_n, N, logn, d->coset_inv, d->card_inv, 0)); made = true; }
    if ((need & DOM_COSET_INV_N_REV) && !d->coset_inv_n_rev) { ZK_TRY(make_pow_table(s, st, &d->coset_inv_n_rev, N, logn, d->coset_inv, d->card_inv, 1)); made = true; }
    if ((need & DOM_COSET_REV_N) && !d->coset_rev_n) { ZK_TRY(make_pow_table(s, st, &d->coset_rev_n, N, logn, d->coset, d->card_inv, 1)); made = true; }
    if (made) ZK_HIP(hipStreamSynchronize(st));  // tables are shared by every stream from here on
    *out = d;
    return ZK_OK;
}

// A transform runs its log2(N) stages as a sequence of tile passes, each with radix-4 stage groups on 512 lanes per tile (4 waves per SIMD): measured
// 8 % faster than radix-8 groups on 256 lanes (2 waves per SIMD) -- the waves of a pass spend ~40 % of their time parked on twiddle / tile loads and
// barriers, which more resident waves hide.
struct PassPlan { unsigned bit_lo, k, logL; };
// split of the index bits: the lowest kc bits form the contiguous pass (L = 1); the rest go to strided passes (increasing bit order)
static std::vector<PassPlan> plan_passes(unsigned logn) {
    unsigned kc = logn < TILE_LOG ? logn : TILE_LOG;
    unsigned rest = logn - kc;
    unsigned np = (rest + K_STRIDED - 1) / K_STRIDED;
    std::vector<PassPlan> passes;
    passes.push_back({0, kc, 0});
    unsigned bit = kc;
    for (unsigned i = 0; i < np; i++) {
        unsigned k = (rest - (bit - kc) + (np - i) - 1) / (np - i);
        unsigned logL = TILE_LOG - k;
        if (logL > bit) logL = bit;  // rows of L consecutive low-order neighbours; the tile always holds up to 2^TILE_LOG elements
        passes.push_back({bit, k, logL});
        bit += k;
    }
    return passes;
}

static const uint32_t g_tw_and = (uint32_t)ZK_EXP("ZKMI_NTT_TWMASK", 0xffffffffL);
static const uint32_t g_unit_skip = ZK_EXP("ZKMI_NTT_UNIT", 1) != 0;

// Every transform below takes `rows` vectors of one domain, `stride` elements apart (one vector: rows = 1, stride unused), in the launches of ONE vector:
// gridDim.z = rows, up to the 65535 a grid's z extent holds; more rows are taken in several launches, never folded into x.
static constexpr size_t ROWS_PER_LAUNCH = 65535;

// rows of `width` bytes: one plain copy where both sides are contiguous, else a pitched one
static int copy_rows(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t rows, hipMemcpyKind kind, hipStream_t st) {
    if (!width || !rows) return ZK_OK;
    if (rows == 1 || (dpitch == width && spitch == width)) ZK_HIP(hipMemcpyAsync(dst, src, width * rows, kind, st));
    else ZK_HIP(hipMemcpy2DAsync(dst, dpitch, src, spitch, width, rows, kind, st));
    return ZK_OK;
}

// One pass: k_ntt_pass29_if where A.tw2 is set, else k_ntt_pass29.  A launch over one row carries the name the benchmark's roofline prices as one vector
// per launch; a launch over more rows the `_rows` name.
static int launch_pass(Slot* s, hipStream_t st, const PassArgs& A_, const RowArgs& R, size_t rows) {
    static const char* const names[2][3] = {{"ntt_pass_contig", "ntt_pass_strided", "ntt_pass_contig_if"},
                                            {"ntt_pass_contig_rows", "ntt_pass_strided_rows", "ntt_pass_contig_if_rows"}};
    const unsigned E = 1u << (A_.k + A_.logL);
    const unsigned tiles = (unsigned)(((size_t)1 << A_.logn) / E);
    const unsigned ny = 1 + (A_.data2 ? 1 : 0) + (A_.data2 && A_.data3 ? 1 : 0);
    for (size_t r0 = 0; r0 < rows; r0 += ROWS_PER_LAUNCH) {
        const unsigned nz = (unsigned)std::min(rows - r0, ROWS_PER_LAUNCH);
        const char* name = names[nz > 1][A_.tw2 ? 2 : (A_.logL ? 1 : 0)];
        PassArgs A = A_;
        A.tw_and = g_tw_and;
        A.unit_skip = g_unit_skip;
        const size_t d = r0 * R.stride, o = r0 * R.op_stride;
        A.data += d;
        if (A.data2) A.data2 += d;
        if (A.data3) A.data3 += d;
        if (A.src) A.src += d;
        if (A.src2) A.src2 += d;
        if (A.src3) A.src3 += d;
        if (A.pre) A.pre += o;
        if (A.sub) A.sub += o;
        const dim3 grid(tiles, ny, nz);
        if (A.tw2) ZK_LAUNCH(s, st, name, (k_ntt_pass29_if<2, 512>), grid, dim3(512), (size_t)E * 36, A, R);
        else if (A.sub) ZK_LAUNCH(s, st, name, (k_ntt_pass29<2, 512, true>), grid, dim3(512), (size_t)E * 36, A, R);
        else ZK_LAUNCH(s, st, name, (k_ntt_pass29<2, 512>), grid, dim3(512), (size_t)E * 36, A, R);
    }
    return ZK_OK;
}

// Runs the log2(N) stages of one transform (of each row) as a sequence of tile passes.
static int run_passes(Slot* s, hipStream_t st, Fr* data, size_t stride, size_t rows, const Domain* dom, int inverse, int dif, const Fr* pre, const Fr* post,
                      const Fr* post_const, const Fr* src = nullptr, const Fr* sub = nullptr, bool row_ops = false) {
    // src (optional): the rows of the input live there, `stride` apart like the data, and stay untouched -- the first pass reads them and writes `data`
    // sub (with `post` AND `post_const`): the last stage leaves (x * post[i] - sub[i]) * post_const
    // row_ops: `pre` and `sub` are operands of each row, `stride` apart like the data (else one table for every row)
    const unsigned logn = dom->logn;
    if (src == data) src = nullptr;
    if (logn == 0) {  // rows of one element: a transform of one point is its scaling (1/N = 1)
        if ((row_ops && pre) || sub) return set_err(ZK_ERR_ARG, "per-row operands need a domain of at least two points");
        if (src) ZK_TRY(copy_rows(data, stride * sizeof(Fr), src, stride * sizeof(Fr), sizeof(Fr), rows, hipMemcpyDeviceToDevice, st));
        const unsigned grid = (unsigned)((rows + 255) / 256);
        const char* name = rows > 1 ? "ntt_scale_rows" : "ntt_scale";
        if (pre) ZK_LAUNCH(s, st, name, k_scale_table_rows, dim3(grid), dim3(256), 0, data, stride, pre, rows);
        if (post) ZK_LAUNCH(s, st, name, k_scale_table_rows, dim3(grid), dim3(256), 0, data, stride, post, rows);
        return ZK_OK;
    }
    const Fr* tw = inverse ? dom->tw29_inv : dom->tw29;
    const RowArgs R = {stride, row_ops ? stride : 0};
    std::vector<PassPlan> passes = plan_passes(logn);
    const size_t npass = passes.size();
    for (size_t idx = 0; idx < npass; idx++) {
        // DIF walks the bits from the top, DIT from the bottom
        const PassPlan& p = dif ? passes[npass - 1 - idx] : passes[idx];
        PassArgs A;
        A.data2 = nullptr; A.src2 = nullptr; A.data3 = nullptr; A.src3 = nullptr;
        A.data = data; A.tw = tw; A.tw2 = nullptr; A.src = (idx == 0) ? src : nullptr; A.logn = logn; A.bit_lo = p.bit_lo; A.k = p.k; A.logL = p.logL; A.dif = dif;
        A.pre = (idx == 0) ? pre : nullptr;
        A.post = (idx + 1 == npass) ? post : nullptr;
        A.has_post_const = (idx + 1 == npass && post_const && !post) ? 1 : 0;
        A.sub = (idx + 1 == npass) ? sub : nullptr;
        if (A.has_post_const || A.sub) A.post_const = *post_const; else A.post_const = Fr::zero();
        A.canonical = (idx + 1 == npass) ? 1 : 0;
        ZK_TRY(launch_pass(s, st, A, R, rows));
    }
    return ZK_OK;
}

// FFTInverse(DIF) with `mid` applied at its end (1/N and whatever scaling follows), then FFT(DIT): as run_passes twice, but the two
// contiguous passes in the middle are ONE kernel (k_ntt_pass29_if).
static int run_inverse_forward(Slot* s, hipStream_t st, Fr* data, size_t stride, size_t rows, const Domain* dom, const Fr* mid, const Fr* src = nullptr,
                               Fr* data2 = nullptr, const Fr* src2 = nullptr, Fr* data3 = nullptr, const Fr* src3 = nullptr, const Fr* end3 = nullptr) {
    // src (optional): the input lives there and stays untouched -- the first pass reads it and writes `data`
    // data2 / src2 (optional): a second vector taken through the same passes by the same launches (gridDim.y = 2)
    // data3 / src3 / end3 (optional, with data2): a third vector that only takes the INVERSE transform, closed by the constant *end3 (computeH's c), in the
    // launches of the inverse half (gridDim.y = 3)
    // rows of data2 / data3 / src* lie `stride` apart like those of `data`
    const unsigned logn = dom->logn;
    if (logn == 0) {  // one point has no passes to fuse: the inverse transform is its scaling by mid[0], the forward one the identity, *end3 is 1/N = 1
        ZK_TRY(run_passes(s, st, data, stride, rows, dom, 1, 1, nullptr, mid, nullptr, src));
        if (data2) ZK_TRY(run_passes(s, st, data2, stride, rows, dom, 1, 1, nullptr, mid, nullptr, src2));
        return (data2 && data3) ? run_passes(s, st, data3, stride, rows, dom, 1, 1, nullptr, nullptr, end3, src3) : ZK_OK;
    }
    const RowArgs R = {stride, 0};
    std::vector<PassPlan> passes = plan_passes(logn);
    const size_t npass = passes.size();
    PassArgs A;
    A.data = data; A.logn = logn; A.pre = nullptr; A.post = nullptr; A.has_post_const = 0; A.post_const = Fr::zero(); A.tw2 = nullptr;
    A.sub = nullptr;
    A.src = (src && src != data) ? src : nullptr;  // consumed by whichever pass runs first
    A.data2 = data2;
    A.src2 = (data2 && src2 && src2 != data2) ? src2 : nullptr;
    A.data3 = data2 ? data3 : nullptr;
    A.src3 = (A.data3 && src3 && src3 != data3) ? src3 : nullptr;
    if (A.data3) A.post_const = *end3;
    for (size_t idx = npass - 1; idx >= 1; idx--) {  // strided passes of the inverse transform, top bits first
        const PassPlan& p = passes[idx];
        A.tw = dom->tw29_inv; A.bit_lo = p.bit_lo; A.k = p.k; A.logL = p.logL; A.dif = 1; A.canonical = 0;
        ZK_TRY(launch_pass(s, st, A, R, rows));
        A.src = nullptr;
        A.src2 = nullptr;
        A.src3 = nullptr;
    }
    {  // the contiguous passes of both transforms: one launch
        A.tw = dom->tw29_inv; A.tw2 = dom->tw29; A.bit_lo = 0; A.k = passes[0].k; A.logL = 0; A.dif = 1; A.post = mid;
        A.canonical = (npass == 1) ? 1 : 0;
        ZK_TRY(launch_pass(s, st, A, R, rows));
        A.post = nullptr;
        A.tw2 = nullptr;
        A.src = nullptr;
        A.src2 = nullptr;
        A.data3 = nullptr;  // c is done
        A.src3 = nullptr;
    }
    for (size_t idx = 1; idx < npass; idx++) {  // strided passes of the forward transform, low bits first
        const PassPlan& p = passes[idx];
        A.tw = dom->tw29; A.bit_lo = p.bit_lo; A.k = p.k; A.logL = p.logL; A.dif = 0; A.canonical = (idx + 1 == npass) ? 1 : 0;
        ZK_TRY(launch_pass(s, st, A, R, rows));
    }
    return ZK_OK;
}

static std::mutex g_lds_mu;
static uint64_t g_lds_attr_set = 0;  // bit e: done for device entry e (the attribute belongs to the device's copy of the function)
static int ensure_lds_attr() {
    std::lock_guard<std::mutex> lk(g_lds_mu);
    const uint64_t bit = (uint64_t)1 << current_entry();
    if (!(g_lds_attr_set & bit)) {
        ZK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_ntt_pass29<2, 512>), hipFuncAttributeMaxDynamicSharedMemorySize, (1 << TILE_LOG) * 36));
        ZK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_ntt_pass29<2, 512, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (1 << TILE_LOG) * 36));
        ZK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_ntt_pass29_if<2, 512>), hipFuncAttributeMaxDynamicSharedMemorySize, (1 << TILE_LOG) * 36));
        g_lds_attr_set |= bit;
    }
    return ZK_OK;
}

// (*Domain).FFT / FFTInverse on device memory: `rows` vectors, row i at d_a + i * row_stride (row_stride >= 2^logn), one launch per pass for all of them
int ntt_rows_dev(Slot* s, hipStream_t st, Fr* d_a, unsigned logn, size_t rows, size_t row_stride, int inverse, int decimation, int coset) {
    if (rows == 0) return ZK_OK;
    ZK_TRY(ensure_lds_attr());
    unsigned need = inverse ? DOM_TW_INV : DOM_TW;
    if (coset) {
        if (!inverse) need |= (decimation == ZK_DIT) ? DOM_COSET_REV : DOM_COSET;
        else need |= (decimation == ZK_DIT) ? DOM_COSET_INV_N : DOM_COSET_INV_N_REV;
    }
    Domain* d;
    ZK_TRY(get_domain(s, st, logn, need, &d));
    const int dif = (decimation == ZK_DIF);
    if (!inverse) {
        // FFT: coset scaling first -- DIF by CosetTable[i], DIT (bit-reversed memory order) by CosetTableReversed[i]
        const Fr* pre = coset ? (dif ? d->coset_tab : d->coset_rev) : nullptr;
        return run_passes(s, st, d_a, row_stride, rows, d, 0, dif, pre, nullptr, nullptr);
    }
    // FFTInverse: TwiddlesInv, then * CardinalityInv (and CosetTableInv[i] for DIT / CosetTableInvReversed[i] for DIF)
    const Fr* post = coset ? (dif ? d->coset_inv_n_rev : d->coset_inv_n) : nullptr;
    const Fr cinv = to_dev(d->card_inv);
    return run_passes(s, st, d_a, row_stride, rows, d, 1, dif, nullptr, post, &cinv);
}

int ntt_dev(Slot* s, hipStream_t st, Fr* d_a, unsigned logn, int inverse, int decimation, int coset) { return ntt_rows_dev(s, st, d_a, logn, 1, 0, inverse, decimation, coset); }

int bit_reverse_dev(Slot* s, hipStream_t st, Fr* d_a, unsigned logn) {
    size_t n = (size_t)1 << logn;
    ZK_LAUNCH(s, st, "bit_reverse", k_bit_reverse, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, d_a, logn);
    return ZK_OK;
}

// gnark v0.8.0 computeH on `rows` triples of device buffers, row i at a / b / c + i * row_stride: a (in/out, N), b, c (scratch, N); h of row i is left in
// a + i * row_stride, bit-reversed order.
//   3 x FFTInverse(DIF) ; 3 x FFT(DIT, coset) ; a = (a*b - c) / (g^N - 1) ; FFTInverse(a, DIF, coset)
// The 1/N of the first inverse and the coset pre-scale g^bitrev(i) of the following forward transform are one table (coset_rev_n) applied while the
// inverse transform stores its last stage.  The row is a grid dimension: as many launches as ONE computeH whatever the row count.
int compute_h_rows_inplace(Slot* s, hipStream_t st, Fr* a, Fr* b, Fr* c, unsigned logN, size_t rows, size_t row_stride, const Fr* const* src) {
    // src (optional): the rows of the three inputs live in src[0..2] (full 2^logN vectors, row_stride apart) and are left untouched; a, b, c are then pure
    // outputs / scratch
    if (rows == 0) return ZK_OK;
    ZK_TRY(ensure_lds_attr());
    Domain* d;
    ZK_TRY(get_domain(s, st, logN, DOM_TW | DOM_TW_INV | DOM_COSET_REV_N | DOM_COSET_INV_N_REV, &d));
    HFr gN = d->coset;
    for (unsigned i = 0; i < logN; i++) gN = gN.sqr();
    const Fr den = to_dev((gN - HFr::one()).inv());
    if (logN == 0) {  // one point: per-row operands need two, so gnark's literal sequence, a row at a time
        for (size_t i = 0; i < rows; i++) {
            Fr* v[3] = {a + i * row_stride, b + i * row_stride, c + i * row_stride};
            for (int j = 0; j < 3; j++) ZK_TRY(run_inverse_forward(s, st, v[j], 0, 1, d, d->coset_rev_n, src ? src[j] + i * row_stride : nullptr));
            ZK_LAUNCH(s, st, "h_pointwise", k_h_pointwise, dim3(1), dim3(256), 0, v[0], (const Fr*)v[1], (const Fr*)v[2], den, (size_t)1);
            ZK_TRY(run_passes(s, st, v[0], 0, 1, d, 1, 1, nullptr, d->coset_inv_n_rev, nullptr));
        }
        return ZK_OK;
    }
    // By linearity (exact field arithmetic, so bit for bit for ANY input): FFTInverse(coset)((a'b' - c') den) = den (FFTInverse(coset)(a'b') - FFTInverse(c)),
    // where c' = FFT(coset)(FFTInverse(c)) -- the coset transform of c and its way back cancel.  c therefore only needs its first FFTInverse(DIF)
    // (coefficients, bit-reversed like the result): six transforms instead of gnark's seven.
    // a, b (and c for the inverse half) go through their passes in the SAME launches (gridDim.y = vector): at 2^20 a pass is ONE round of workgroups moving
    // in lock-step (load, butterflies, store); with two or three rounds per launch one round's loads and stores run under another's butterflies, and seven
    // launches disappear.
    const Fr cinv = to_dev(d->card_inv);
    ZK_TRY(run_inverse_forward(s, st, a, row_stride, rows, d, d->coset_rev_n, src ? src[0] : nullptr, b, src ? src[1] : nullptr, c, src ? src[2] : nullptr, &cinv));
    // the product a*b rides on the loads of the closing transform's first stage (`pre` = b) and (x - c) * den on the stores of its last one (`sub` = c)
    // instead of two element-wise kernels (96 B per element each)
    return run_passes(s, st, a, row_stride, rows, d, 1, 1, b, d->coset_inv_n_rev, &den, nullptr, c, true);
}

int compute_h_inplace(Slot* s, hipStream_t st, Fr* a, Fr* b, Fr* c, unsigned logN, const Fr* const* src) { return compute_h_rows_inplace(s, st, a, b, c, logN, 1, 0, src); }

int fr_mul_dev(Slot* s, hipStream_t st, Fr* out, const Fr* a, const Fr* b, size_t n) {
    ZK_LAUNCH(s, st, "fr_mul", k_fr_mul, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, out, a, b, n);
    return ZK_OK;
}


// ------------------------------------------------------------------------------------ computeH sharded over G = 2^g GPUs
// Rank rho owns the block [rho*M, (rho+1)*M) of every length-D array (M = D/G).  A radix-2 transform over D splits into
//   * g CROSS stages on the top g index bits (the first g stages of a DIF transform, the last g of a DIT transform), and
//   * a plain size-M transform of the block (omega_M = omega_D^G), which is the single-GPU code above.
// For the cross stages the ranks transpose (all-to-all, done by the host over RCCL): rank rho then holds T[s][j], s < G,
// j < C = M/G, = element s*M + rho*C + j, and one lane runs the g butterflies of column j in registers (G <= 8: the
// radix-8 of SURVEY.md 8e).  Twiddles come from the size-D table: DIF stage t pairs s, s + (G >> (t+1)) with
// w^(((s mod h)*M + rho*C + j) << t); DIT cross stage u pairs s, s + 2^u with w^(((s mod 2^u)*M + rho*C + j) * (G >> (u+1))).
template <int LOGG, bool DIF>
__global__ __launch_bounds__(256) void k_ntt_cross(Fr* __restrict__ T, const Fr* __restrict__ tw, unsigned logM, unsigned rank) {
    prio_mid();
    constexpr unsigned G = 1u << LOGG;
    const size_t C = ((size_t)1 << logM) >> LOGG;
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= C) return;
    const size_t low = (size_t)rank * C + j;
    Fr x[G];
#pragma unroll
    for (unsigned s = 0; s < G; s++) x[s] = gload_fr(T + s * C + j);
#pragma unroll
    for (int st = 0; st < LOGG; st++) {
        const unsigned h = DIF ? (G >> (st + 1)) : (1u << st);  // pair distance in s
        const unsigned mul_shift = DIF ? st : (LOGG - 1 - st);  // exponent multiplier 2^t (DIF) / G/(2h) (DIT)
#pragma unroll
        for (unsigned s = 0; s < G; s++) {
            if (s & h) continue;
            const size_t e = (((size_t)(s & (h - 1)) << logM) + low) << mul_shift;
            Fr w = gload_fr(tw + e);
            if (DIF) {
                Fr u = x[s] + x[s + h];
                x[s + h] = (x[s] - x[s + h]) * w;
                x[s] = u;
            } else {
                Fr v = x[s + h] * w;
                x[s + h] = x[s] - v;
                x[s] = x[s] + v;
            }
        }
    }
#pragma unroll
    for (unsigned s = 0; s < G; s++) T[s * C + j] = x[s];
}

template <bool DIF>
static int launch_cross(Slot* s, hipStream_t st, Fr* T, const Fr* tw, unsigned logM, unsigned logg, unsigned rank) {
    const size_t C = ((size_t)1 << logM) >> logg;
    dim3 grid((unsigned)((C + 255) / 256)), block(256);
    switch (logg) {
        case 0: return ZK_OK;
        case 1: ZK_LAUNCH(s, st, "ntt_cross", (k_ntt_cross<1, DIF>), grid, block, 0, T, tw, logM, rank); return ZK_OK;
        case 2: ZK_LAUNCH(s, st, "ntt_cross", (k_ntt_cross<2, DIF>), grid, block, 0, T, tw, logM, rank); return ZK_OK;
        case 3: ZK_LAUNCH(s, st, "ntt_cross", (k_ntt_cross<3, DIF>), grid, block, 0, T, tw, logM, rank); return ZK_OK;
        default: return set_err(ZK_ERR_ARG, "computeH shards over at most 8 ranks (log_g = %u)", logg);
    }
}

struct ShardTables {
    Fr *coset_rev_n = nullptr, *coset_inv_n_rev = nullptr;  // this rank's M-entry slices of the size-D tables
    Fr *coset_nat = nullptr, *coset_rev = nullptr, *coset_inv_n_nat = nullptr;  // standalone sharded transforms (lazily): g^i, g^bitrev(i), g^-i / D
};
static std::mutex g_shard_mu;
static std::map<uint64_t, ShardTables> g_shard_tables;

static int get_shard_tables(Slot* s, hipStream_t st, Domain* dD, unsigned logD, unsigned logg, unsigned rank, ShardTables* out) {
    std::lock_guard<std::mutex> lk(g_shard_mu);
    const uint64_t key = ((uint64_t)current_entry() << 48) | ((uint64_t)logD << 32) | ((uint64_t)logg << 16) | rank;
    ShardTables& t = g_shard_tables[key];
    if (!t.coset_rev_n) {
        const size_t M = ((size_t)1 << logD) >> logg;
        ZK_TRY(make_pow_table(s, st, &t.coset_rev_n, M, logD, dD->coset, dD->card_inv, 1, (size_t)rank * M));
        ZK_TRY(make_pow_table(s, st, &t.coset_inv_n_rev, M, logD, dD->coset_inv, dD->card_inv, 1, (size_t)rank * M));
        ZK_HIP(hipStreamSynchronize(st));
    }
    *out = t;
    return ZK_OK;
}

// One compute phase of the sharded computeH (the host exchanges between phases; see include/zkmi.h).
int compute_h_shard_phase(Slot* s, hipStream_t st, int phase, Fr* a, Fr* b, Fr* c, unsigned logD, unsigned logg, unsigned rank) {
    if (logg > 3 || logD < 2 * logg || logD > 28) return set_err(ZK_ERR_ARG, "bad shard geometry (log_D = %u, log_g = %u)", logD, logg);
    if (rank >= (1u << logg)) return set_err(ZK_ERR_ARG, "rank %u out of range", rank);
    ZK_TRY(ensure_lds_attr());
    const unsigned logM = logD - logg;
    const size_t M = (size_t)1 << logM;
    Domain *dD, *dM;
    ZK_TRY(get_domain(s, st, logD, logg ? (DOM_TW | DOM_TW_INV) : 0u, &dD));
    ZK_TRY(get_domain(s, st, logM, DOM_TW | DOM_TW_INV, &dM));
    ShardTables tb;
    ZK_TRY(get_shard_tables(s, st, dD, logD, logg, rank, &tb));
    switch (phase) {
        case 0:  // transposed a, b, c (any subset: null arrays are skipped): cross stages of FFTInverse(DIF)
            for (Fr* v : {a, b, c})
                if (v) ZK_TRY(launch_cross<true>(s, st, v, dD->tw_inv, logM, logg, rank));
            return ZK_OK;
        case 1:  // blocks (any subset): rest of FFTInverse(DIF), * 1/D * g^bitrev(i), block part of FFT(DIT, coset)
            for (Fr* v : {a, b, c})
                if (v) ZK_TRY(run_inverse_forward(s, st, v, 0, 1, dM, tb.coset_rev_n));
            return ZK_OK;
        case 4:  // first third of phase 2, per array: cross stages of FFT(DIT) on the transposed arrays given
            for (Fr* v : {a, b, c})
                if (v) ZK_TRY(launch_cross<false>(s, st, v, dD->tw, logM, logg, rank));
            return ZK_OK;
        case 2:    // transposed: cross stages of FFT(DIT); pointwise; cross stages of the final FFTInverse(DIF, coset)
        case 5: {  // the rest of phase 2 after phase 4 ran on a, b, c: pointwise + cross stages of the final FFTInverse(DIF, coset)
            if (!a || !b || !c) return set_err(ZK_ERR_ARG, "phase %d needs a, b and c", phase);
            if (phase == 2)
                for (Fr* v : {a, b, c}) ZK_TRY(launch_cross<false>(s, st, v, dD->tw, logM, logg, rank));
            HFr gN = dD->coset;
            for (unsigned i = 0; i < logD; i++) gN = gN.sqr();
            HFr den = (gN - HFr::one()).inv();
            ZK_LAUNCH(s, st, "h_pointwise", k_h_pointwise, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, a, (const Fr*)b, (const Fr*)c, to_dev(den), M);
            return launch_cross<true>(s, st, a, dD->tw_inv, logM, logg, rank);
        }
        case 3:  // block of a: rest of FFTInverse(DIF, coset) -> this rank's block of h (gnark's bit-reversed order)
            return run_passes(s, st, a, 0, 1, dM, 1, 1, nullptr, tb.coset_inv_n_rev, nullptr);
        // ---- the six-transform schedule (c stays in coefficient form: compute_h_rows_inplace's shortcut, sharded; one transpose and two transforms of c fewer)
        case 6: {  // blocks (any subset; the schedule uses it for c): rest of FFTInverse(DIF) with 1/D -> block of the coefficients, bit-reversed order
            const Fr cinv = to_dev(dD->card_inv);
            for (Fr* v : {a, b, c})
                if (v) ZK_TRY(run_passes(s, st, v, 0, 1, dM, 1, 1, nullptr, nullptr, &cinv));
            return ZK_OK;
        }
        case 7:  // transposed a, b (after phase 4 on each): a = a * b, then the cross stages of the final FFTInverse(DIF, coset) on a
            if (!a || !b) return set_err(ZK_ERR_ARG, "phase 7 needs a and b");
            ZK_LAUNCH(s, st, "fr_mul", k_fr_mul, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, a, (const Fr*)a, (const Fr*)b, M);
            return launch_cross<true>(s, st, a, dD->tw_inv, logM, logg, rank);
        case 8: {  // block of a and block of c's coefficients (phase 6): rest of FFTInverse(DIF, coset), then h = (a - c) / (g^D - 1)
            if (!a || !c) return set_err(ZK_ERR_ARG, "phase 8 needs a and c");
            ZK_TRY(run_passes(s, st, a, 0, 1, dM, 1, 1, nullptr, tb.coset_inv_n_rev, nullptr));
            HFr gN = dD->coset;
            for (unsigned i = 0; i < logD; i++) gN = gN.sqr();
            const HFr den = (gN - HFr::one()).inv();
            ZK_LAUNCH(s, st, "h_final", k_h_final, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, a, (const Fr*)c, to_dev(den), M);
            return ZK_OK;
        }
        default: return set_err(ZK_ERR_ARG, "phase must be 0..8");
    }
}

// One step of a standalone transform sharded by blocks over G = 2^g ranks (BASELINE configs[4] on several GPUs; the same decomposition as computeH's):
// (*Domain).FFT / FFTInverse over D = G * M points, rank rho holding block rho of the STORED order (natural for DIF input / DIT output, bit-reversed
// for DIF output / DIT input).  The host sequences the steps with its all-to-all transposes (X):
//     FFT(DIF):         [SCALE if coset]  X  CROSS  X  BLOCK             FFT(DIT):         BLOCK  X  CROSS  X
//     FFTInverse(DIF):                    X  CROSS  X  BLOCK             FFTInverse(DIT):  BLOCK  X  CROSS  X  [SCALE if coset]
//   step 0 CROSS: the g stages on the top index bits, on transposed data;  step 1 BLOCK: the size-M transform of the block with whatever scaling
//   can ride on it (1/D always; g^bitrev(i) before a forward DIT, g^-bitrev(i) after an inverse DIF);  step 2 SCALE: the coset factor that must act on
//   the natural-order block outside the block transform (g^i before a forward DIF's cross stages, g^-i after an inverse DIT's).
int ntt_shard_step(Slot* s, hipStream_t st, int step, Fr* a, unsigned logD, unsigned logg, unsigned rank, int inverse, int dif, int coset) {
    if (logg > 3 || logD < 2 * logg || logD > 28) return set_err(ZK_ERR_ARG, "bad shard geometry (log_D = %u, log_g = %u)", logD, logg);
    if (rank >= (1u << logg)) return set_err(ZK_ERR_ARG, "rank %u out of range", rank);
    ZK_TRY(ensure_lds_attr());
    const unsigned logM = logD - logg;
    const size_t M = (size_t)1 << logM;
    Domain *dD, *dM;
    ZK_TRY(get_domain(s, st, logD, logg ? (DOM_TW | DOM_TW_INV) : 0u, &dD));
    ZK_TRY(get_domain(s, st, logM, DOM_TW | DOM_TW_INV, &dM));
    ShardTables tb;
    ZK_TRY(get_shard_tables(s, st, dD, logD, logg, rank, &tb));
    if (coset) {
        std::lock_guard<std::mutex> lk(g_shard_mu);
        ShardTables& t = g_shard_tables[((uint64_t)current_entry() << 48) | ((uint64_t)logD << 32) | ((uint64_t)logg << 16) | rank];  // the key of get_shard_tables
        if (!t.coset_nat) {
            ZK_TRY(make_pow_table(s, st, &t.coset_nat, M, logD, dD->coset, HFr::one(), 0, (size_t)rank * M));
            ZK_TRY(make_pow_table(s, st, &t.coset_rev, M, logD, dD->coset, HFr::one(), 1, (size_t)rank * M));
            ZK_TRY(make_pow_table(s, st, &t.coset_inv_n_nat, M, logD, dD->coset_inv, HFr::one(), 0, (size_t)rank * M));
            ZK_HIP(hipStreamSynchronize(st));
        }
        tb = t;
    }
    const Fr cinv = to_dev(dD->card_inv);  // 1/D: the block transform is linear, so the whole scaling rides on it
    switch (step) {
        case 0:
            return dif ? launch_cross<true>(s, st, a, inverse ? dD->tw_inv : dD->tw, logM, logg, rank)
                       : launch_cross<false>(s, st, a, inverse ? dD->tw_inv : dD->tw, logM, logg, rank);
        case 1:
            if (!inverse) return run_passes(s, st, a, 0, 1, dM, 0, dif, (coset && !dif) ? tb.coset_rev : nullptr, nullptr, nullptr);
            return run_passes(s, st, a, 0, 1, dM, 1, dif, nullptr, (coset && dif) ? tb.coset_inv_n_rev : nullptr, &cinv);
        case 2: {
            if (!coset || (!inverse && !dif) || (inverse && dif)) return ZK_OK;  // nothing left outside the block transform
            const Fr* t = inverse ? tb.coset_inv_n_nat : tb.coset_nat;
            ZK_LAUNCH(s, st, "ntt_scale", k_scale_table, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, a, t, M);
            return ZK_OK;
        }
        default: return set_err(ZK_ERR_ARG, "step must be 0 (cross), 1 (block) or 2 (scale)");
    }
}

}  // namespace zkmi

using namespace zkmi;

extern "C" {

int zk_bn254_ntt_dev(void* d_a, uint32_t log_n, int inverse, int decimation, int coset, void* stream) {
    if (!d_a) return set_err(ZK_ERR_ARG, "null data pointer");
    if (log_n > 28) return set_err(ZK_ERR_ARG, "log_n = %u exceeds Fr two-adicity 28", log_n);
    if (decimation != ZK_DIT && decimation != ZK_DIF) return set_err(ZK_ERR_ARG, "decimation must be ZK_DIT or ZK_DIF");
    SlotGuard g;
    ZK_TRY(acquire_slot(&g.s));
    hipStream_t st = stream ? (hipStream_t)stream : g.s->stream;
    ZK_TRY(ntt_dev(g.s, st, (Fr*)d_a, log_n, inverse, decimation, coset));
    // no workspace is used: safe to return without synchronising a caller-provided stream
    if (!stream || profiling_on()) ZK_TRY(slot_sync(g.s, st));
    return ZK_OK;
}

// device_mask: bit i = device entry i takes a block of the array (2, 4 or 8 entries: multidev.hip); 0 = the process default, which only spreads transforms
// of at least 2^18 points per entry
int zk_bn254_ntt_devices(zk_fr* a, uint32_t log_n, int inverse, int decimation, int coset, uint32_t device_mask) {
    if (!a) return set_err(ZK_ERR_ARG, "null data pointer");
    if (log_n > 28) return set_err(ZK_ERR_ARG, "log_n = %u exceeds Fr two-adicity 28", log_n);
    if (decimation != ZK_DIT && decimation != ZK_DIF) return set_err(ZK_ERR_ARG, "decimation must be ZK_DIT or ZK_DIF");
    std::vector<int> ents;
    ZK_TRY(md_entries_for(device_mask, (size_t)1 << log_n, (size_t)1 << 18, &ents));
    if (ents.size() > 1 && (device_mask || ents.size() == 2 || ents.size() == 4 || ents.size() == 8)) return md_ntt_host(a, log_n, inverse, decimation, coset, ents);
    CtxScope sc(ents[0]);
    if (sc.rc != ZK_OK) return sc.rc;
    SlotGuard g;
    ZK_TRY(acquire_slot(&g.s));
    size_t bytes = ((size_t)1 << log_n) * 32;
    ZK_TRY(g.s->reserve(bytes));
    Fr* d = (Fr*)g.s->alloc(bytes);
    hipStream_t st = g.s->stream;
    ZK_HIP(hipMemcpyAsync(d, a, bytes, hipMemcpyHostToDevice, st));
    ZK_TRY(ntt_dev(g.s, st, d, log_n, inverse, decimation, coset));
    ZK_HIP(hipMemcpyAsync(a, d, bytes, hipMemcpyDeviceToHost, st));
    return slot_sync(g.s, st);
}
int zk_bn254_ntt(zk_fr* a, uint32_t log_n, int inverse, int decimation, int coset) { return zk_bn254_ntt_devices(a, log_n, inverse, decimation, coset, 0); }

// ---- row batches: many vectors of one domain per call (one launch per pass for all rows)
static constexpr size_t ROWS_SCRATCH = (size_t)1 << 30;  // arena bytes one batch entry takes at a time; more rows than fit go in chunks, on the same slot

static int ntt_batch_args(const void* a, uint32_t log_n, size_t row_stride, int decimation) {
    if (!a) return set_err(ZK_ERR_ARG, "null data pointer");
    if (log_n > 28) return set_err(ZK_ERR_ARG, "log_n = %u exceeds Fr two-adicity 28", log_n);
    if (decimation != ZK_DIT && decimation != ZK_DIF) return set_err(ZK_ERR_ARG, "decimation must be ZK_DIT or ZK_DIF");
    if (row_stride < ((size_t)1 << log_n)) return set_err(ZK_ERR_ARG, "row_stride = %zu is below the domain size %zu", row_stride, (size_t)1 << log_n);
    return ZK_OK;
}

int zk_bn254_ntt_batch_dev(void* d_a, uint32_t log_n, size_t rows, size_t row_stride, int inverse, int decimation, int coset, void* stream) {
    ZK_TRY(ntt_batch_args(d_a, log_n, row_stride, decimation));
    if (rows == 0) return ZK_OK;
    if (rows == 1) return zk_bn254_ntt_dev(d_a, log_n, inverse, decimation, coset, stream);
    SlotGuard g;
    ZK_TRY(acquire_slot(&g.s));
    hipStream_t st = stream ? (hipStream_t)stream : g.s->stream;
    ZK_TRY(ntt_rows_dev(g.s, st, (Fr*)d_a, log_n, rows, row_stride, inverse, decimation, coset));
    if (!stream || profiling_on()) ZK_TRY(slot_sync(g.s, st));  // in place, no workspace
    return ZK_OK;
}

// host rows, contiguous (row i at a + i * 2^log_n); one device: a batch of small transforms is not worth a transpose between GPUs
int zk_bn254_ntt_batch(zk_fr* a, uint32_t log_n, size_t rows, int inverse, int decimation, int coset) {
    ZK_TRY(ntt_batch_args(a, log_n, (size_t)-1, decimation));  // contiguous rows: no stride to check
    if (rows == 0) return ZK_OK;
    const size_t N = (size_t)1 << log_n, row_bytes = N * 32;
    const size_t chunk = std::min(rows, std::max<size_t>(1, ROWS_SCRATCH / row_bytes));
    SlotGuard g;
    ZK_TRY(acquire_slot(&g.s));
    ZK_TRY(g.s->reserve(chunk * row_bytes));
    Fr* d = (Fr*)g.s->alloc(chunk * row_bytes);
    if (!d) return set_err(ZK_ERR_ARG, "ntt batch: workspace");
    hipStream_t st = g.s->stream;
    for (size_t first = 0; first < rows; first += chunk) {
        const size_t R = std::min(chunk, rows - first);
        char* h = (char*)a + first * row_bytes;
        ZK_HIP(hipMemcpyAsync(d, h, R * row_bytes, hipMemcpyHostToDevice, st));
        ZK_TRY(ntt_rows_dev(g.s, st, d, log_n, R, N, inverse, decimation, coset));
        ZK_HIP(hipMemcpyAsync(h, d, R * row_bytes, hipMemcpyDeviceToHost, st));
    }
    return slot_sync(g.s, st);
}

int zk_bn254_bit_reverse_dev(void* d_a, uint32_t log_n, void* stream) {
    if (!d_a || log_n > 28) return set_err(ZK_ERR_ARG, "bad argument");
    SlotGuard g;
    ZK_TRY(acquire_slot(&g.s));
    hipStream_t st = stream ? (hipStream_t)stream : g.s->stream;
    ZK_TRY(bit_reverse_dev(g.s, st, (Fr*)d_a, log_n));
    if (!stream || profiling_on()) ZK_TRY(slot_sync(g.s, st));
    return ZK_OK;
}

int zk_bn254_bit_reverse(zk_fr* a, uint32_t log_n) {
    if (!a || log_n > 28) return set_err(ZK_ERR_ARG, "bad argument");
    SlotGuard g;
    ZK_TRY(acquire_slot(&g.s));
    size_t bytes = ((size_t)1 << log_n) * 32;
    ZK_TRY(g.s->reserve(bytes));
    Fr* d = (Fr*)g.s->alloc(bytes);
    hipStream_t st = g.s->stream;
    ZK_HIP(hipMemcpyAsync(d, a, bytes, hipMemcpyHostToDevice, st));
    ZK_TRY(bit_reverse_dev(g.s, st, d, log_n));
    ZK_HIP(hipMemcpyAsync(a, d, bytes, hipMemcpyDeviceToHost, st));
    return slot_sync(g.s, st);
}

int zk_bn254_groth16_compute_h_dev(const void* d_a, const void* d_b, const void* d_c, size_t n, uint32_t log_N, void* d_h_out, void* stream) {
    if (!d_a || !d_b || !d_c || !d_h_out) return set_err(ZK_ERR_ARG, "null pointer");
    if (log_N > 28) return set_err(ZK_ERR_ARG, "log_N exceeds 28");
    size_t N = (size_t)1 << log_N;
    if (n > N) return set_err(ZK_ERR_ARG, "n = %zu exceeds the domain size %zu", n, N);
    SlotGuard g;
    ZK_TRY(acquire_slot(&g.s));
    hipStream_t st = stream ? (hipStream_t)stream : g.s->stream;
    ZK_TRY(g.s->reserve(2 * N * 32 + 512));
    Fr* a = (Fr*)d_h_out;
    Fr* b = (Fr*)g.s->alloc(N * 32);
    Fr* c = (Fr*)g.s->alloc(N * 32);
    const void* src[3] = {d_a, d_b, d_c};
    Fr* dst[3] = {a, b, c};
    for (int i = 0; i < 3; i++) {
        if (src[i] != dst[i]) ZK_HIP(hipMemcpyAsync(dst[i], src[i], n * 32, hipMemcpyDeviceToDevice, st));
        if (n < N) ZK_HIP(hipMemsetAsync(dst[i] + n, 0, (N - n) * 32, st));
    }
    ZK_TRY(compute_h_inplace(g.s, st, a, b, c, log_N));
    return slot_sync(g.s, st);  // scratch lives in the slot's arena
}

int zk_bn254_groth16_compute_h(const zk_fr* a, const zk_fr* b, const zk_fr* c, size_t n, uint32_t log_N, zk_fr* h_out) {
    if (!a || !b || !c || !h_out) return set_err(ZK_ERR_ARG, "null pointer");
    if (log_N > 28) return set_err(ZK_ERR_ARG, "log_N exceeds 28");
    size_t N = (size_t)1 << log_N;
    if (n > N) return set_err(ZK_ERR_ARG, "n = %zu exceeds the domain size %zu", n, N);
    SlotGuard g;
    ZK_TRY(acquire_slot(&g.s));
    hipStream_t st = g.s->stream;
    ZK_TRY(g.s->reserve(3 * N * 32 + 1024));
    Fr* d[3];
    const zk_fr* src[3] = {a, b, c};
    for (int i = 0; i < 3; i++) {
        d[i] = (Fr*)g.s->alloc(N * 32);
        ZK_HIP(hipMemcpyAsync(d[i], src[i], n * 32, hipMemcpyHostToDevice, st));
        if (n < N) ZK_HIP(hipMemsetAsync(d[i] + n, 0, (N - n) * 32, st));
    }
    ZK_TRY(compute_h_inplace(g.s, st, d[0], d[1], d[2], log_N));
    ZK_HIP(hipMemcpyAsync(h_out, d[0], N * 32, hipMemcpyDeviceToHost, st));
    return slot_sync(g.s, st);
}

static int zero_rows(Fr* dst, size_t pitch_elems, size_t width_elems, size_t rows, hipStream_t st) {
    if (!width_elems || !rows) return ZK_OK;
    if (rows == 1 || pitch_elems == width_elems) ZK_HIP(hipMemsetAsync(dst, 0, width_elems * rows * 32, st));
    else ZK_HIP(hipMemset2DAsync(dst, pitch_elems * 32, 0, width_elems * 32, rows, st));
    return ZK_OK;
}

static int compute_h_batch_args(const void* a, const void* b, const void* c, const void* h, size_t n, size_t in_stride, uint32_t log_N, size_t out_stride) {
    if (!a || !b || !c || !h) return set_err(ZK_ERR_ARG, "null pointer");
    if (log_N > 28) return set_err(ZK_ERR_ARG, "log_N exceeds 28");
    const size_t N = (size_t)1 << log_N;
    if (n > N) return set_err(ZK_ERR_ARG, "n = %zu exceeds the domain size %zu", n, N);
    if (in_stride < n) return set_err(ZK_ERR_ARG, "in_stride = %zu is below the row length %zu", in_stride, n);
    if (out_stride < N) return set_err(ZK_ERR_ARG, "out_stride = %zu is below the domain size %zu", out_stride, N);
    return ZK_OK;
}

// computeH of `rows` triples resident in HBM.  The a rows are taken to d_h_out (out_stride apart) and transformed there; the b and c rows go to the slot's arena
// at the same stride, so the row kernels see one stride; the caller's inputs are only read.
int zk_bn254_groth16_compute_h_batch_dev(const void* d_a, const void* d_b, const void* d_c, size_t n, size_t in_stride, uint32_t log_N, size_t rows, void* d_h_out,
                                         size_t out_stride, void* stream) {
    ZK_TRY(compute_h_batch_args(d_a, d_b, d_c, d_h_out, n, in_stride, log_N, out_stride));
    if (rows == 0) return ZK_OK;
    const size_t N = (size_t)1 << log_N;
    // d_h_out may be d_a itself where row i of both is the same memory (one row, or equal strides); any other overlap of the output with an input is refused
    const bool in_place = d_h_out == d_a && (rows == 1 || in_stride == out_stride);
    const char* out_lo = (const char*)d_h_out;
    const char* out_hi = out_lo + ((rows - 1) * out_stride + N) * 32;
    const void* ins[3] = {d_a, d_b, d_c};
    for (int i = in_place ? 1 : 0; i < 3; i++) {
        const char* lo = (const char*)ins[i];
        const char* hi = lo + ((rows - 1) * in_stride + n) * 32;
        if (lo < out_hi && out_lo < hi) return set_err(ZK_ERR_ARG, "d_h_out overlaps an input (only d_h_out == d_a with equal strides may alias)");
    }
    if (rows == 1) return zk_bn254_groth16_compute_h_dev(d_a, d_b, d_c, n, log_N, d_h_out, stream);
    SlotGuard g;
    ZK_TRY(acquire_slot(&g.s));
    hipStream_t st = stream ? (hipStream_t)stream : g.s->stream;
    const size_t chunk = std::min(rows, std::max<size_t>(1, ROWS_SCRATCH / (2 * out_stride * 32)));
    Fr *b = nullptr, *c = nullptr;
    ZK_TRY(plan_workspace(g.s, "computeH batch", [&](ArenaPlan& p) { p.take(chunk * out_stride, b, c); }));
    // full rows at the output's stride are read where they are by the first pass (its `src`): no staging copy
    const bool direct = n == N && in_stride == out_stride && log_N > 0;
    for (size_t first = 0; first < rows; first += chunk) {
        const size_t R = std::min(chunk, rows - first);
        Fr* a = (Fr*)d_h_out + first * out_stride;
        const Fr* src[3];
        for (int i = 0; i < 3; i++) src[i] = (const Fr*)ins[i] + first * in_stride;
        if (direct) {
            ZK_TRY(compute_h_rows_inplace(g.s, st, a, b, c, log_N, R, out_stride, src));
            continue;
        }
        Fr* dst[3] = {a, b, c};
        for (int i = 0; i < 3; i++) {
            if ((const Fr*)dst[i] != src[i]) ZK_TRY(copy_rows(dst[i], out_stride * 32, src[i], in_stride * 32, n * 32, R, hipMemcpyDeviceToDevice, st));
            ZK_TRY(zero_rows(dst[i] + n, out_stride, N - n, R, st));
        }
        ZK_TRY(compute_h_rows_inplace(g.s, st, a, b, c, log_N, R, out_stride));
    }
    return slot_sync(g.s, st);  // scratch lives in the slot's arena
}

// host rows, contiguous: a, b, c are (rows, n), h_out is (rows, 2^log_N)
int zk_bn254_groth16_compute_h_batch(const zk_fr* a, const zk_fr* b, const zk_fr* c, size_t n, uint32_t log_N, size_t rows, zk_fr* h_out) {
    ZK_TRY(compute_h_batch_args(a, b, c, h_out, n, n, log_N, (size_t)-1));  // contiguous rows: no strides to check
    if (rows == 0) return ZK_OK;
    if (rows == 1) return zk_bn254_groth16_compute_h(a, b, c, n, log_N, h_out);
    const size_t N = (size_t)1 << log_N;
    const size_t chunk = std::min(rows, std::max<size_t>(1, ROWS_SCRATCH / (3 * N * 32)));
    SlotGuard g;
    ZK_TRY(acquire_slot(&g.s));
    hipStream_t st = g.s->stream;
    Fr* d[3] = {nullptr, nullptr, nullptr};
    ZK_TRY(plan_workspace(g.s, "computeH batch", [&](ArenaPlan& p) { p.take(chunk * N, d[0], d[1], d[2]); }));
    const zk_fr* src[3] = {a, b, c};
    for (size_t first = 0; first < rows; first += chunk) {
        const size_t R = std::min(chunk, rows - first);
        for (int i = 0; i < 3; i++) {
            ZK_TRY(copy_rows(d[i], N * 32, (const char*)src[i] + first * n * 32, n * 32, n * 32, R, hipMemcpyHostToDevice, st));
            ZK_TRY(zero_rows(d[i] + n, N, N - n, R, st));
        }
        ZK_TRY(compute_h_rows_inplace(g.s, st, d[0], d[1], d[2], log_N, R, N));
        ZK_HIP(hipMemcpyAsync((char*)h_out + first * N * 32, d[0], R * N * 32, hipMemcpyDeviceToHost, st));
    }
    return slot_sync(g.s, st);
}

int zk_bn254_groth16_h_shard_dev(int phase, void* d_a, void* d_b, void* d_c, uint32_t log_D, uint32_t log_g, uint32_t rank, void* stream) {
    if ((!d_a && phase != 6) || ((phase == 2 || phase == 5) && (!d_b || !d_c))) return set_err(ZK_ERR_ARG, "null pointer");
    SlotGuard g;
    ZK_TRY(acquire_slot(&g.s));
    // Give it the stream of the proof's msm5 session (zk_bn254_groth16_msm5_session_stream): a foreign stream may share a
    // hardware queue with the stream that prepares the wire scalars of the same proof (measured with a torch-created stream:
    // the two serialised, ~0.5 ms per proof).
    hipStream_t st = stream ? (hipStream_t)stream : g.s->stream;
    ZK_TRY(compute_h_shard_phase(g.s, st, phase, (Fr*)d_a, (Fr*)d_b, (Fr*)d_c, log_D, log_g, rank));
    if (!stream) ZK_TRY(slot_sync(g.s, st));  // in place, no workspace: a caller-provided stream stays asynchronous (profiled or not)
    return ZK_OK;
}

int zk_bn254_ntt_shard_dev(int step, void* d_a, uint32_t log_D, uint32_t log_g, uint32_t rank, int inverse, int decimation, int coset, void* stream) {
    if (!d_a) return set_err(ZK_ERR_ARG, "null data pointer");
    if (decimation != ZK_DIT && decimation != ZK_DIF) return set_err(ZK_ERR_ARG, "decimation must be ZK_DIT or ZK_DIF");
    SlotGuard g;
    ZK_TRY(acquire_slot(&g.s));
    hipStream_t st = stream ? (hipStream_t)stream : g.s->stream;
    ZK_TRY(ntt_shard_step(g.s, st, step, (Fr*)d_a, log_D, log_g, rank, inverse ? 1 : 0, decimation == ZK_DIF, coset ? 1 : 0));
    if (!stream) ZK_TRY(slot_sync(g.s, st));
    return ZK_OK;
}

int zk_bn254_fr_mul_dev(void* d_out, const void* d_a, const void* d_b, size_t n, void* stream) {
    if (!d_out || !d_a || !d_b) return set_err(ZK_ERR_ARG, "null pointer");
    SlotGuard g;
    ZK_TRY(acquire_slot(&g.s));
    hipStream_t st = stream ? (hipStream_t)stream : g.s->stream;
    ZK_TRY(fr_mul_dev(g.s, st, (Fr*)d_out, (const Fr*)d_a, (const Fr*)d_b, n));
    if (!stream || profiling_on()) ZK_TRY(slot_sync(g.s, st));
    return ZK_OK;
}

}  // extern "C"
