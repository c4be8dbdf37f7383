// The Horner suffix scan of plonk.hip (polynomial evaluation and kzg.dividePolyByXminusA in one structure) as seen by its two users: the PLONK prover
// (plonk.hip, which holds the kernels) and the KZG openings (kzg.hip, which adds the row-indexed variants); and the bodies of its three passes, over which plonk.hip
// builds the kernels that take a row's point from device memory.
#pragma once
#include <string.h>

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

// The three passes of the Horner suffix scan as bodies a kernel is built over: plonk.hip's k_hscan_*_dev take polynomial, length and point of a row from device
// memory through them.  (k_hscan_local / _batch / _blocks / _apply in plonk.hip and k_hscan_*_rows in kzg.hip are the same passes written out, with their points
// in the kernel arguments: an edit of one belongs in the others.)  Field arithmetic is exact, so a step whose other operand is known to be zero is left out.
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
        const Fr chunk_total = sh[0];
        if (c != (int)nchunks - 1) {  // the top chunk has no carry
            const uint32_t e = 1023 - threadIdx.x;
            Fr pw = Fr::one(), bs = M;
            for (int i = 0; i < 10; i++) { if ((e >> i) & 1) pw = pw * bs; bs = bs.sqr(); }
            C = C + pw * carry;
            carry = chunk_total + M1024 * carry;
        } else {
            carry = chunk_total;
        }
        __syncthreads();
        if (b < nb) btot[b] = C;
    }
    return carry;
}
// pass 3, the lane of pass 1: q_i = S_(i+1) for i < qlen (qlen = len - 1: the quotient's coefficients and nothing else; q may be f).  tc: the lane's carry
// from pass 1, C: its workgroup's from pass 2.
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

constexpr int HSCAN_BATCH_MAX = 8;  // polynomials per launch of the batched scans (blockIdx.y)

// scratch carved from the slot arena for the scans over `len` elements
struct ScanBufs {
    uint32_t K = 0, nb = 0;  // coefficients per lane, workgroups of 256 lanes
    Fr *t = nullptr, *b = nullptr, *total = nullptr;
};
static inline size_t scan_need(size_t len) { return (len / 8 + 4096) * sizeof(Fr) + 8192 + (size_t)8 * (len / 2048 + 2) * sizeof(Fr); }
int scan_bufs(Slot* s, size_t len, ScanBufs* B);
// f_k(a) -> d_out[k] for cnt <= HSCAN_BATCH_MAX polynomials, two launches in all
int poly_eval_batch_dev(Slot* s, hipStream_t st, const Fr* const* f, const size_t* len, int cnt, const HFr& a, const ScanBufs& B, Fr* d_out);
// q = (f - f(a)) / (X - a) (len - 1 coefficients; q may alias f; q[len-1] is set to 0), f(a) -> *d_eval
int poly_divide_dev(Slot* s, hipStream_t st, const Fr* f, size_t len, const HFr& a, const ScanBufs& B, Fr* q, Fr* d_eval);

}  // namespace zkmi
