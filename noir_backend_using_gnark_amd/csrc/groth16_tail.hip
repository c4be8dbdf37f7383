// The tail of groth16.Prove for MANY rows in one launch: zk_bn254_groth16_finalize_batch / _dev, and the device tail of the batch prover (groth16_batch.hip).
// Row i has n_partials records of 96 limbs -- A, B1, K, Z (G1 XYZZ, 16 limbs each), G2.B (G2 XYZZ, 32 limbs): what zk_bn254_groth16_msm5_* writes -- and (r, s):
//      A = sum parts.A, ..., B2 = sum parts.B2
//      Ar  = A + alpha + r*delta
//      Bs  = B2 + beta2 + s*delta2
//      Krs = K + Z + s*(A + alpha) + r*(B1 + beta) + rs*delta
//      proof = g1_compress(Ar) | g2_compress(Bs) | g1_compress(Krs)
// which is what tail_pre + tail_post of groth16.hip compute on the host (zk_bn254_groth16_finalize).  A proof's bytes are the canonical compressed images of
// three group elements, so any schedule that computes the same elements writes the same bytes.
//
// One kernel, one block of four waves per 64 rows; the wave is the ROLE, the lane the row (a role is wave-uniform: no divergence between roles):
//      wave 0   A + alpha, then s*(A + alpha)                      254 doublings + ~127 additions, the long pole
//      wave 1   B1 + beta, then r*(B1 + beta)                      the same
//      wave 2   Bs = B2 + beta2 + s*delta2                         <= 32 mixed G2 additions from the key's 8-bit window table of delta2
//      wave 3   r*delta and K + Z + rs*delta                       <= 64 mixed G1 additions from the table of delta
// The five intermediate points of a row go through LDS (224 words per row, word-major: lane-contiguous, no bank conflict), then wave 0 adds them up, turns the
// three results affine with ONE inversion (Montgomery's trick over zz*zzz; the Fp2 one through its norm) and writes the 128 bytes.  No global workspace: the
// _dev entry can enqueue behind a caller's stream and return.  A batch is a few waves on a 256-CU machine, so the time is the LATENCY of wave 0 / 1's chain;
// the G2 code sets the kernel's register count (DESIGN.md 3.12 has the figures), which costs nothing while the grid cannot fill the machine anyway.
#include <string.h>

#include <algorithm>

#include "codec_dev.hpp"
#include "ctx.hpp"
#include "curve.hpp"
#include "groth16_batch.hpp"
#include "groth16_tail.hpp"
#include "multidev.hpp"

namespace zkmi {

static constexpr int TAIL_ROWS = 64;  // rows per block = lanes per wave
// LDS words of a row: A + alpha | s*(A + alpha) | r*(B1 + beta) | r*delta | K + Z + rs*delta | Bs
enum { L_AAL = 0, L_SA = 32, L_RB = 64, L_RD = 96, L_KZ = 128, L_BS = 160, L_WORDS = 224 };
typedef uint32_t TailLds[TAIL_ROWS];

ZK_D void lds_put(TailLds* sh, int off, int lane, const Fp& v) {
#pragma unroll
    for (int k = 0; k < 8; k++) sh[off + k][lane] = v.l[k];
}
ZK_D Fp lds_get(const TailLds* sh, int off, int lane) {
    Fp v;
#pragma unroll
    for (int k = 0; k < 8; k++) v.l[k] = sh[off + k][lane];
    return v;
}
ZK_D void lds_put(TailLds* sh, int off, int lane, const XYZZ<Fp>& p) {
    lds_put(sh, off, lane, p.x); lds_put(sh, off + 8, lane, p.y); lds_put(sh, off + 16, lane, p.zz); lds_put(sh, off + 24, lane, p.zzz);
}
ZK_D XYZZ<Fp> lds_get_g1(const TailLds* sh, int off, int lane) {
    return XYZZ<Fp>{lds_get(sh, off, lane), lds_get(sh, off + 8, lane), lds_get(sh, off + 16, lane), lds_get(sh, off + 24, lane)};
}
ZK_D Fp2 lds_get2(const TailLds* sh, int off, int lane) { return Fp2{lds_get(sh, off, lane), lds_get(sh, off + 8, lane)}; }
ZK_D void lds_put2(TailLds* sh, int off, int lane, const Fp2& v) { lds_put(sh, off, lane, v.a0); lds_put(sh, off + 8, lane, v.a1); }

__global__ __launch_bounds__(4 * TAIL_ROWS) void k_groth16_tail(TailKey K, const uint64_t* __restrict__ partials, size_t n_partials, const Fr* __restrict__ r,
                                                                const Fr* __restrict__ s, size_t n, uint32_t* __restrict__ out) {
    __shared__ TailLds sh[L_WORDS];
    const int lane = threadIdx.x & (TAIL_ROWS - 1), role = threadIdx.x / TAIL_ROWS;
    const size_t row = (size_t)blockIdx.x * TAIL_ROWS + lane;
    const bool live = row < n;
    if (live) {
        const uint64_t* rec = partials + row * n_partials * 96;
        if (role < 2) {  // s*(A + alpha) / r*(B1 + beta)
            XYZZ<Fp> m = tail_sum<Fp>(rec, n_partials, 16 * role);
            const Affine<Fp> base = role ? K.beta : K.alpha;
            m.madd(base.x, base.y);
            if (role == 0) lds_put(sh, L_AAL, lane, m);
            const XYZZ<Fp> acc = tail_scaled(m, (role ? r : s)[row]);
            lds_put(sh, role ? L_RB : L_SA, lane, acc);
        } else if (role == 2) {  // Bs
            XYZZ<Fp2> bs = tail_sum<Fp2>(rec, n_partials, 64);
            bs.madd(K.beta2.x, K.beta2.y);
            tail_fixed_add(bs, K.t_delta2, s[row].from_mont());
            lds_put2(sh, L_BS, lane, bs.x); lds_put2(sh, L_BS + 16, lane, bs.y); lds_put2(sh, L_BS + 32, lane, bs.zz); lds_put2(sh, L_BS + 48, lane, bs.zzz);
        } else {  // r*delta, K + Z + rs*delta
            XYZZ<Fp> kz = tail_sum<Fp>(rec, n_partials, 32);
            kz.add(tail_sum<Fp>(rec, n_partials, 48));
            const Fr rm = r[row], sm = s[row];
            XYZZ<Fp> rd = XYZZ<Fp>::inf();
            tail_fixed_add(rd, K.t_delta, rm.from_mont());
            tail_fixed_add(kz, K.t_delta, (rm * sm).from_mont());
            lds_put(sh, L_RD, lane, rd);
            lds_put(sh, L_KZ, lane, kz);
        }
    }
    __syncthreads();
    if (!live || role != 0) return;
    XYZZ<Fp> ar = lds_get_g1(sh, L_AAL, lane);
    ar.add(lds_get_g1(sh, L_RD, lane));
    XYZZ<Fp> krs = lds_get_g1(sh, L_KZ, lane);
    krs.add(lds_get_g1(sh, L_SA, lane));
    krs.add(lds_get_g1(sh, L_RB, lane));
    const XYZZ<Fp2> bs{lds_get2(sh, L_BS, lane), lds_get2(sh, L_BS + 16, lane), lds_get2(sh, L_BS + 32, lane), lds_get2(sh, L_BS + 48, lane)};
    Affine<Fp> a_ar, a_krs;
    Affine<Fp2> a_bs;
    tail_to_affine(ar, bs, krs, &a_ar, &a_bs, &a_krs);
    uint32_t* o = out + row * 32;
    g1_compress_one(a_ar, o);
    g2_compress_one(a_bs, o + 8);
    g1_compress_one(a_krs, o + 24);
}

// the tail of `n` rows on stream `st`: every pointer a device pointer, inputs only read, 128 bytes per row out
int groth16_tail_rows(Slot* sl, hipStream_t st, const Groth16TailView& V, const void* d_partials, size_t n_partials, const void* d_r, const void* d_s, size_t n,
                      void* d_proofs_out) {
    if (!n) return ZK_OK;
    TailKey K;
    K.alpha = V.alpha; K.beta = V.beta; K.beta2 = V.beta2;
    K.t_delta = (const Affine<Fp>*)V.t_delta;
    K.t_delta2 = (const Affine<Fp2>*)V.t_delta2;
    const size_t blocks = (n + TAIL_ROWS - 1) / TAIL_ROWS;
    if (blocks > 0x7fffffffu) return set_err(ZK_ERR_ARG, "n_proofs = %zu exceeds one launch", n);
    ZK_LAUNCH(sl, st, "groth16_tail", k_groth16_tail, dim3((unsigned)blocks), dim3(4 * TAIL_ROWS), 0, K, (const uint64_t*)d_partials, n_partials, (const Fr*)d_r,
              (const Fr*)d_s, n, (uint32_t*)d_proofs_out);
    ZK_HIP(hipGetLastError());
    return ZK_OK;
}

}  // namespace zkmi

using namespace zkmi;

extern "C" {

int zk_bn254_groth16_finalize_batch_dev(uint64_t pk_handle, const void* d_partials, size_t n_partials, const void* d_r, const void* d_s, size_t n_proofs,
                                        void* d_proofs_out, void* stream) {
    if (n_proofs == 0) return ZK_OK;
    if (!d_partials || !n_partials || !d_r || !d_s || !d_proofs_out) return set_err(ZK_ERR_ARG, "null pointer");
    if (md_is_composite(pk_handle)) return set_err(ZK_ERR_ARG, "a key spread over several device entries finalizes from host pointers (zk_bn254_groth16_finalize_batch)");
    ZK_ON_ENTRY_OF(pk_handle);
    Groth16TailView V;
    ZK_TRY(groth16_pk_tail_view(pk_handle, &V));
    SlotGuard g;
    ZK_TRY(acquire_slot(&g.s));
    hipStream_t st = stream ? (hipStream_t)stream : g.s->stream;
    ZK_TRY(groth16_tail_rows(g.s, st, V, d_partials, n_partials, d_r, d_s, n_proofs, d_proofs_out));
    if (!stream || profiling_on()) ZK_TRY(slot_sync(g.s, st));  // no workspace: nothing of the slot's is in use after the return
    return ZK_OK;
}

int zk_bn254_groth16_finalize_batch(uint64_t pk_handle, const uint64_t* partials, size_t n_partials, const zk_fr* r, const zk_fr* s, size_t n_proofs,
                                    uint8_t* proofs_out) {
    if (n_proofs == 0) return ZK_OK;
    if (!partials || !n_partials || !r || !s || !proofs_out) return set_err(ZK_ERR_ARG, "null pointer");
    if (md_is_composite(pk_handle)) {  // alpha, beta, delta are the same in every slice: the composite key's own combine step, row by row
        for (size_t i = 0; i < n_proofs; i++) ZK_TRY(zk_bn254_groth16_finalize(pk_handle, partials + i * n_partials * 96, n_partials, r + i, s + i, proofs_out + 128 * i));
        return ZK_OK;
    }
    ZK_ON_ENTRY_OF(pk_handle);
    Groth16TailView V;
    ZK_TRY(groth16_pk_tail_view(pk_handle, &V));
    // rows per pass: what keeps the staged records near 16 MB
    const size_t rec_bytes = n_partials * 768;
    const size_t chunk = std::min(n_proofs, std::max<size_t>(1, ((size_t)16 << 20) / rec_bytes));
    SlotGuard g;
    ZK_TRY(acquire_slot(&g.s));
    hipStream_t st = g.s->stream;
    uint64_t* d_parts = nullptr;
    Fr *d_r = nullptr, *d_s = nullptr;
    uint8_t* d_out = nullptr;
    ZK_TRY(plan_workspace(g.s, "groth16 finalize batch", [&](ArenaPlan& p) {
        p.take(chunk * n_partials * 96, d_parts);
        p.take(chunk, d_r, d_s);
        p.take(chunk * 128, d_out);
    }));
    for (size_t first = 0; first < n_proofs; first += chunk) {
        const size_t R = std::min(chunk, n_proofs - first);
        ZK_HIP(hipMemcpyAsync(d_parts, partials + first * n_partials * 96, R * rec_bytes, hipMemcpyHostToDevice, st));
        ZK_HIP(hipMemcpyAsync(d_r, r + first, R * 32, hipMemcpyHostToDevice, st));
        ZK_HIP(hipMemcpyAsync(d_s, s + first, R * 32, hipMemcpyHostToDevice, st));
        ZK_TRY(groth16_tail_rows(g.s, st, V, d_parts, n_partials, d_r, d_s, R, d_out));
        ZK_HIP(hipMemcpyAsync(proofs_out + 128 * first, d_out, R * 128, hipMemcpyDeviceToHost, st));
    }
    return slot_sync(g.s, st);
}

}  // extern "C"
