// The two scans under the PLONK prover and the KZG openings.
//   Horner suffix scan  S_i = f_i + a S_(i+1): S_0 = f(a), and q_i = S_(i+1) are the coefficients of (f - f(a)) / (X - a) -- polynomial evaluation and
//                       kzg.dividePolyByXminusA in one structure, three passes.  The arithmetic of the passes is written ONCE, as the bodies below
//                       (hscan_local_body, hscan_blocks_body, hscan_apply_body); two kernel families are built over them:
//                         points in the kernel arguments  k_hscan_*_rows (scan.hip), up to HSCAN_BATCH_MAX rows of an HscanRows a launch, launched by
//                                                         hscan_rows_passes: poly_eval_batch_dev, poly_divide_dev and kzg.hip's openings
//                         points in device memory         k_hscan_*_dev (plonk.hip): rounds 4 and 5 of the row-batched prover
//   prefix-product scan z_0 = 1, z_(i+1) = z_i num_i / den_i (Z of the copy-constraint ratio): k_pscan_*_rows in plonk.hip, three passes over pscan_wg256
// Both work on K consecutive elements per lane and nb workgroups of 256 lanes per row: scan_plan.
#pragma once
#include <string.h>

#include <vector>

#include "ctx.hpp"
#include "ff.hpp"
#include "host_ff.hpp"

namespace zkmi {

static inline Fr to_dev(const HFr& h) {
    Fr r;
    memcpy(&r, &h, 32);
    return r;
}
#if defined(__HIPCC__)
__device__ __forceinline__ Fr ld(const Fr* p) {
    const uint4* q = reinterpret_cast<const uint4*>(p);
    uint4 a = q[0], b = q[1];
    Fr r;
    r.l[0] = a.x; r.l[1] = a.y; r.l[2] = a.z; r.l[3] = a.w;
    r.l[4] = b.x; r.l[5] = b.y; r.l[6] = b.z; r.l[7] = b.w;
    return r;
}

// The three passes of the Horner suffix scan.  Field arithmetic is exact, so a step whose other operand is known to be zero is left out.
//
// pass 1, one workgroup of 256 lanes: lane t holds coefficients [base, base + K); `live` lanes of the workgroup start below len (live >= 1).  Returns the
// lane's suffix total val_t = sum_{u >= t} T_u A^(u - t) and leaves val in sh[0 .. 256): sh[t + 1] is the carry into lane t, val_0 the workgroup's total.
__device__ __forceinline__ Fr hscan_local_body(Fr* sh, const Fr* __restrict__ f, size_t len, uint32_t K, size_t base, const Fr& a, const Fr& A, uint32_t live) {
    Fr acc = Fr::zero();
    for (int k = (int)K - 1; k >= 0; k--) {
        const size_t i = base + (size_t)k;
        acc = acc * a;
        if (i < len) acc = acc + ld(f + i);
    }
    sh[threadIdx.x] = acc;
    __syncthreads();
    Fr val = acc, Ad = A;
    for (unsigned d = 1; d < live; d <<= 1) {  // lanes from `live` on hold zero: a step of d >= live adds nothing
        Fr o = threadIdx.x + d < 256 ? sh[threadIdx.x + d] : Fr::zero();
        __syncthreads();
        val = val + Ad * o;
        sh[threadIdx.x] = val;
        __syncthreads();
        Ad = Ad.sqr();
    }
    return val;
}
// pass 2, one workgroup of 1024 lanes over the nb workgroup totals of one polynomial: btot[b] <- C_b = sum_{b' > b} btot[b'] M^(b' - b - 1) (M = A^256);
// returns S_0 = f(a) (the same in every lane).
__device__ __forceinline__ Fr hscan_blocks_body(Fr* sh, Fr* __restrict__ btot, uint32_t nb, const Fr& M) {
    Fr carry = Fr::zero();  // S at the start of the chunk above
    const uint32_t nchunks = (nb + 1023) / 1024;
    Fr M1024 = M;
    if (nchunks > 1)
        for (int i = 0; i < 10; i++) M1024 = M1024.sqr();
    for (int c = (int)nchunks - 1; c >= 0; c--) {
        const uint32_t b = (uint32_t)c * 1024 + threadIdx.x, live = nb - (uint32_t)c * 1024;  // totals in this chunk (more than 1024: all lanes)
        const Fr v = b < nb ? ld(btot + b) : Fr::zero();
        sh[threadIdx.x] = v;
        __syncthreads();
        Fr val = v, Md = M;
        for (unsigned d = 1; d < 1024 && d < live; d <<= 1) {
            Fr o = threadIdx.x + d < 1024 ? sh[threadIdx.x + d] : Fr::zero();
            __syncthreads();
            val = val + Md * o;
            sh[threadIdx.x] = val;
            __syncthreads();
            Md = Md.sqr();
        }
        // val = sum_{u >= t in chunk} v_u M^(u-t); C_b = val_(t+1) + M^(1023 - t) * carry
        Fr C = threadIdx.x < 1023 ? sh[threadIdx.x + 1] : Fr::zero();
        if (c != (int)nchunks - 1) {  // the top chunk has no carry: zero
            const uint32_t e = 1023 - threadIdx.x;
            Fr pw = Fr::one(), bs = M;
            for (int i = 0; i < 10; i++) { if ((e >> i) & 1) pw = pw * bs; bs = bs.sqr(); }
            C = C + pw * carry;
            carry = M1024 * carry;
        }
        carry = sh[0] + carry;  // the chunk's total completes it
        __syncthreads();
        if (b < nb) btot[b] = C;
    }
    return carry;
}
// pass 3, the lane of pass 1: q_i = S_(i+1) for i < qlen (qlen = len - 1: the quotient's coefficients and nothing else; qlen = len: q[len - 1] = 0 as
// well; q may be f).  tc: the lane's carry from pass 1, C: its workgroup's from pass 2.
__device__ __forceinline__ void hscan_apply_body(const Fr* f, Fr* q, size_t len, size_t qlen, uint32_t K, size_t base, const Fr& a, const Fr& A, const Fr& tc,
                                                 const Fr& C) {
    const uint32_t e = 255 - threadIdx.x;
    Fr pw = Fr::one(), bs = A;
    for (int i = 0; i < 8; i++) { if ((e >> i) & 1) pw = pw * bs; bs = bs.sqr(); }
    Fr S = tc + pw * C;
    for (int k = (int)K - 1; k >= 0; k--) {
        const size_t i = base + (size_t)k;
        if (i >= len) continue;
        const Fr fv = ld(f + i);
        if (i < qlen) q[i] = S;
        S = fv + a * S;
    }
}
#endif

constexpr int HSCAN_BATCH_MAX = 8;  // rows per launch of the argument-point scans (blockIdx.y)

// lane and workgroup geometry of a scan over `len` elements: K consecutive elements per lane, nb workgroups of 256 lanes
static inline uint32_t scan_blocks(size_t len, uint32_t K) { return (uint32_t)(((len + K - 1) / K + 255) / 256); }
static inline void scan_plan(size_t len, uint32_t* K, uint32_t* nb) {
    uint32_t k = (uint32_t)((len + 256 * 1024 - 1) / (256 * 1024));
    if (k < 8) k = 8;
    *K = k;
    *nb = scan_blocks(len, k);
}

// one row per polynomial: its coefficients, where its quotient goes (may alias f; unused without pass 3), its point a, A = a^K and M = A^256
struct HscanRows {
    const Fr* f[HSCAN_BATCH_MAX];
    Fr* q[HSCAN_BATCH_MAX];
    size_t len[HSCAN_BATCH_MAX];
    Fr a[HSCAN_BATCH_MAX], A[HSCAN_BATCH_MAX], M[HSCAN_BATCH_MAX];
};
// row r of R for a scan of K coefficients per lane: the point preparation a -> (a, a^K, a^(256 K))
static inline void hscan_row(HscanRows* R, int r, const Fr* f, Fr* q, size_t len, const HFr& a, uint32_t K) {
    HFr A = HFr::one(), base = a;
    for (uint32_t k = K; k; k >>= 1) { if (k & 1) A = A * base; base = base.sqr(); }
    HFr M = A;
    for (int i = 0; i < 8; i++) M = M.sqr();
    R->f[r] = f; R->q[r] = q; R->len[r] = len;
    R->a[r] = to_dev(a); R->A[r] = to_dev(A); R->M[r] = to_dev(M);
}
// the profile names of the three launches
struct HscanNames {
    const char *local, *blocks, *apply;
};
// The passes over `rows` <= HSCAN_BATCH_MAX rows of R (the entries from `rows` on are not read): lane carries to tcarry[(row nb + block) 256 + lane],
// workgroup totals to btot[row nb + block], f_r(a_r) to total[r]; then q_i = S_(i+1) for i < len (q[len - 1] = 0).  tcarry == nullptr: evaluation only, two
// launches and no lane carries kept.
// With a trace (inspection, tests: zk_bn254_hscan_inspect) the stream is synchronised after pass 1 and the rows * nb workgroup totals, which pass 2 overwrites in
// place, are copied to the host; the launches are the same.  Without one nothing is added but the test of the pointer.
struct HscanTrace {
    std::vector<Fr> btot_local;
};
int hscan_rows_passes(Slot* s, hipStream_t st, const HscanNames& names, const HscanRows& R, unsigned rows, uint32_t K, uint32_t nb, Fr* tcarry, Fr* btot, Fr* total,
                      HscanTrace* trace = nullptr);

// scratch carved from the slot arena for the scans over `len` elements
struct ScanBufs {
    uint32_t K = 0, nb = 0;  // scan_plan(len)
    Fr *t = nullptr, *b = nullptr, *total = nullptr;
};
static inline size_t scan_need(size_t len) { return (len / 8 + 4096) * sizeof(Fr) + 8192 + (size_t)8 * (len / 2048 + 2) * sizeof(Fr); }
int scan_bufs(Slot* s, size_t len, ScanBufs* B);
// f_k(a) -> d_out[k] for cnt <= HSCAN_BATCH_MAX polynomials, two launches in all
int poly_eval_batch_dev(Slot* s, hipStream_t st, const Fr* const* f, const size_t* len, int cnt, const HFr& a, const ScanBufs& B, Fr* d_out);
// q = (f - f(a)) / (X - a) (len - 1 coefficients; q may alias f; q[len-1] is set to 0), f(a) -> *d_eval
int poly_divide_dev(Slot* s, hipStream_t st, const Fr* f, size_t len, const HFr& a, const ScanBufs& B, Fr* q, Fr* d_eval);

}  // namespace zkmi
