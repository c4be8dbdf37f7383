// The Horner suffix scan of plonk.hip (polynomial evaluation and kzg.dividePolyByXminusA in one structure) as seen by its two users: the PLONK prover
// (plonk.hip, which holds the kernels) and the KZG openings (kzg.hip, which adds the row-indexed variants).
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
