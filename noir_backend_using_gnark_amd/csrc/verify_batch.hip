// Pairings and batch Groth16 verification on the device (include/zkmi.h "Pairings and batch Groth16 verification on the DEVICE").
//   zk_bn254_pair          one Miller loop per lane (k_miller), a product tree (k_f12_fold), one final exponentiation (k_fe_*)
//   zk_bn254_groth16_verify_batch, per chunk of at most 2^16 proofs:
//     decode      Ar / Krs through k_g1_decompress, Bs through k_g2_decompress + the r-torsion test, with a flag per invalid point
//     combine     k_vb_prep: r_i Ar_i (affine), r_i Krs_i, r_i (1, w_i1, ..); k_g1_fold / k_fr_fold sum the last two over the chunk; the host scales the
//                 three fixed-key terms: -(sum r_i) alpha, -sum_j c_j K_j, -sum r_i Krs_i
//     check       n' + 3 Miller loops, product tree, one final exponentiation: prod e(r_i Ar_i, Bs_i) e(-c_0 alpha, beta) e(-sum c_j K_j, gamma)
//                 e(-sum r_i Krs_i, delta) == 1 accepts every valid proof of the chunk
//     fallback    (only when the check fails) k_vb_single: -Ar_i, IC_i = K_0 + sum_j w_ij K_j, Krs_i per lane; 3 n + 1 Miller loops (the last one is
//                 e(alpha, beta)'s); k_fe_easy multiplies each proof's three values and e(alpha, beta)'s, the k_fe_* chain exponentiates, k_fe_last
//                 compares with one
#include <string.h>

#include <algorithm>
#include <vector>

#include "ctx.hpp"
#include "curve.hpp"
#include "host_ff.hpp"
#include "keyio.hpp"
#include "pairing.hpp"
#include "pairing_dev.hpp"
#include "proofio.hpp"
#include "verify.hpp"

using namespace zkmi;
using pdev::F12;
using pdev::PairConsts;

namespace {

template <class A, class B>
A bit_cast_img(const B& b) {
    static_assert(sizeof(A) == sizeof(B), "same memory image");
    A a;
    memcpy(&a, &b, sizeof a);
    return a;
}

// the Frobenius constants of pairing.hpp and 3 b' = 9 / xi
PairConsts pair_consts() {
    PairConsts K;
    const pairing::Consts& C = pairing::consts();
    for (int i = 0; i < 6; i++) {
        K.g1[i] = bit_cast_img<Fp2>(C.g1[i]);
        K.g2[i] = bit_cast_img<Fp>(C.g2[i].a0);  // (g2[i] lies in Fp)
    }
    const HFp three = HFp::one() + HFp::one() + HFp::one(), nine = three + three + three;
    K.b3 = bit_cast_img<Fp2>(HFp2{nine, HFp::zero()} * HFp2{nine, HFp::one()}.inv());
    return K;
}

// pairing.hpp's w-basis -> gnark's E12 order (C0 = c0, c2, c4; C1 = c1, c3, c5)
void f12_to_gt(const pairing::F12& f, zk_gt* out) {
    static const int MAP[6] = {0, 2, 4, 1, 3, 5};
    for (int k = 0; k < 6; k++) memcpy(&out->c[2 * k], &f.c[MAP[k]], 64);
}

constexpr unsigned PAIR_BLOCK = 64;  // lanes per workgroup of the Miller / final-exponentiation kernels (one pairing is thousands of products per lane)
inline unsigned blocks(size_t n, unsigned b) { return (unsigned)((n + b - 1) / b); }

// out[i] = f_{6 x0 + 2, Q_i}(P_i), Q_i = qvar[i] for i < n_var, qfix[(i - n_var) / rep] after
__global__ __launch_bounds__(PAIR_BLOCK) void k_miller(const Affine<Fp>* __restrict__ P, size_t n, const Affine<Fp2>* __restrict__ qvar, size_t n_var,
                                                       const Affine<Fp2>* __restrict__ qfix, size_t rep, PairConsts K, F12* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Affine<Fp2> q = i < n_var ? qvar[i] : qfix[(i - n_var) / rep];
    out[i] = pdev::miller_loop(P[i], q, K);
}
// out[i] = in[2 i] in[2 i + 1] (the last one alone when n is odd)
__global__ __launch_bounds__(PAIR_BLOCK) void k_f12_fold(const F12* __restrict__ in, size_t n, size_t cols, F12* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (n + 1) / 2) return;
    F12 f = in[2 * i];
    if (2 * i + 1 < n) f = f * in[2 * i + 1];
    out[i] = f;
}
// the final exponentiation over a workspace of pdev::FE_SLOTS F12 per lane (ws[k n + i]: slot k of lane i):
//   k_fe_easy   f = prod_{r < rows} in[r n + i] (* mul_by), slot 0 = f^((q^6 - 1)(q^2 + 1))
//   k_fe_expt   slot dst = slot src ^ x0 (three times: slots 1, 2, 3 = f^x, f^(x^2), f^(x^3))
//   k_fe_step   one step of pdev::FE_CHAIN (12 launches); the last one (k_fe_last) writes out[i] (may be null) and verdict[i] = valid[i] && value == 1
using pdev::FE_SLOTS;
__global__ __launch_bounds__(PAIR_BLOCK) void k_fe_easy(const F12* __restrict__ in, size_t n, int rows, const F12* __restrict__ mul_by, PairConsts K,
                                                        F12* __restrict__ ws) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    F12 f = in[i];
    for (int r = 1; r < rows; r++) f = f * in[(size_t)r * n + i];
    if (mul_by) f = f * *mul_by;
    ws[i] = pdev::easy_part(f, K);
}
__global__ __launch_bounds__(PAIR_BLOCK) void k_fe_expt(F12* __restrict__ ws, size_t n, int src, int dst) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    ws[dst * n + i] = pdev::expt(ws[src * n + i]);
}
__global__ __launch_bounds__(PAIR_BLOCK) void k_fe_step(F12* ws, size_t n, pdev::FeStep st, PairConsts K) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const F12 a = ws[st.a * n + i], b = ws[st.b * n + i];
    ws[st.dst * n + i] = pdev::fe_step(a, st.opa, b, st.opb, K);
}
__global__ __launch_bounds__(PAIR_BLOCK) void k_fe_last(const F12* __restrict__ ws, size_t n, pdev::FeStep st, PairConsts K, F12* __restrict__ out,
                                                        const uint8_t* __restrict__ valid, uint8_t* __restrict__ verdict) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const F12 f = pdev::fe_step(ws[st.a * n + i], st.opa, ws[st.b * n + i], st.opb, K);
    if (out) out[i] = f;
    if (verdict) verdict[i] = (valid[i] && f.is_one()) ? 1 : 0;
}
__global__ __launch_bounds__(256) void k_g1_fold(const XYZZ<Fp>* __restrict__ in, size_t n, size_t cols, XYZZ<Fp>* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (n + 1) / 2) return;
    XYZZ<Fp> a = in[2 * i];
    if (2 * i + 1 < n) a.add(in[2 * i + 1]);
    out[i] = a;
}
// column sums of a rows x cols matrix, one halving per launch
__global__ __launch_bounds__(256) void k_fr_fold(const Fr* __restrict__ in, size_t rows, size_t cols, Fr* __restrict__ out) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (rows + 1) / 2 * cols) return;
    const size_t i = t / cols, j = t % cols;
    Fr a = in[2 * i * cols + j];
    if (2 * i + 1 < rows) a = a + in[(2 * i + 1) * cols + j];
    out[t] = a;
}

// per proof: valid = no invalid point; r_i Ar_i (affine; infinity when invalid), r_i Krs_i, and the row r_i (1, w_i1, .., w_i,np) of the mat-vec
__global__ __launch_bounds__(128) void k_vb_prep(const Affine<Fp>* __restrict__ ar, const Affine<Fp>* __restrict__ krs, const uint8_t* __restrict__ bad,
                                                 const uint32_t* __restrict__ rr, const Fr* __restrict__ pub, size_t n, size_t np, uint8_t* __restrict__ valid,
                                                 Affine<Fp>* __restrict__ p_out, XYZZ<Fp>* __restrict__ rk_out, Fr* __restrict__ terms) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const bool ok = !(bad[i] | bad[n + i] | bad[2 * n + i]);
    valid[i] = ok ? 1 : 0;
    const uint32_t k[8] = {rr[4 * i], rr[4 * i + 1], rr[4 * i + 2], rr[4 * i + 3], 0, 0, 0, 0};
    Fr rm = Fr::zero();
    for (int j = 0; j < 4; j++) rm.l[j] = k[j];
    rm = ok ? rm.to_mont() : Fr::zero();
    terms[i * (np + 1)] = rm;
    for (size_t j = 0; j < np; j++) terms[i * (np + 1) + 1 + j] = rm * pub[i * np + j];
    if (!ok) {
        p_out[i] = Affine<Fp>::inf();
        rk_out[i] = XYZZ<Fp>::inf();
        return;
    }
    p_out[i] = scalar_mul(ar[i], k).to_affine();
    rk_out[i] = scalar_mul(krs[i], k);
}
// fallback, per proof: P[i] = -Ar_i, P[n + i] = IC_i = K_0 + sum_j w_ij K_j, P[2 n + i] = Krs_i (all infinity when the proof is invalid)
__global__ __launch_bounds__(128) void k_vb_single(const Affine<Fp>* __restrict__ ar, const Affine<Fp>* __restrict__ krs, const uint8_t* __restrict__ valid,
                                                   const Fr* __restrict__ pub, const Affine<Fp>* __restrict__ kpts, size_t n, size_t np,
                                                   Affine<Fp>* __restrict__ P) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (!valid[i]) {
        P[i] = P[n + i] = P[2 * n + i] = Affine<Fp>::inf();
        return;
    }
    P[i] = ar[i].neg();
    P[2 * n + i] = krs[i];
    XYZZ<Fp> ic = XYZZ<Fp>::from_affine(kpts[0]);
    for (size_t j = 0; j < np; j++) {
        const Fr w = pub[i * np + j].from_mont();
        ic.add(scalar_mul(kpts[1 + j], w.l));
    }
    P[n + i] = ic.to_affine();
}

// halving launches until one element is left; a and b hold at least ceil(n / 2) elements each (a: n); returns where the result is
template <class T, class Kern>
T* fold_all(Slot* s, hipStream_t st, const char* name, Kern kernel, unsigned block, T* a, T* b, size_t n, size_t cols) {
    while (n > 1) {
        const size_t m = (n + 1) / 2;
        ZK_LAUNCH(s, st, name, kernel, dim3(blocks(m * cols, block)), dim3(block), 0, (const T*)a, n, cols, b);
        std::swap(a, b);
        n = m;
    }
    return a;
}

constexpr size_t CHUNK = (size_t)1 << 16;
constexpr size_t SLACK = 64 * 256;  // per-allocation alignment, generously

// final exponentiation of n lanes (see k_fe_easy); d_ws: FE_SLOTS n F12
int final_exp(Slot* s, hipStream_t st, const PairConsts& K, const F12* d_in, size_t n, int rows, const F12* d_mul_by, F12* d_ws, F12* d_out,
              const uint8_t* d_valid, uint8_t* d_verdict) {
    const dim3 grid(blocks(n, PAIR_BLOCK)), block(PAIR_BLOCK);
    ZK_LAUNCH(s, st, "fe_easy", k_fe_easy, grid, block, 0, d_in, n, rows, d_mul_by, K, d_ws);
    for (int k = 0; k < 3; k++) ZK_LAUNCH(s, st, "fe_expt", k_fe_expt, grid, block, 0, d_ws, n, k, k + 1);
    for (int k = 0; k + 1 < pdev::FE_CHAIN_LEN; k++) ZK_LAUNCH(s, st, "fe_step", k_fe_step, grid, block, 0, d_ws, n, pdev::FE_CHAIN[k], K);
    ZK_LAUNCH(s, st, "fe_last", k_fe_last, grid, block, 0, (const F12*)d_ws, n, pdev::FE_CHAIN[pdev::FE_CHAIN_LEN - 1], K, d_out, d_valid, d_verdict);
    return ZK_OK;
}

void sha(const void* p, size_t n, uint8_t out[32]) {
    Sha256 h;
    h.update(p, n);
    h.final(out);
}

}  // namespace

extern "C" {

int zk_bn254_pair_host(const zk_g1_affine* p, const zk_g2_affine* q, size_t n, zk_gt* out) {
    if ((n && (!p || !q)) || !out) return set_err(ZK_ERR_ARG, "null pointer");
    pairing::F12 f = pairing::F12::one();
    for (size_t i = 0; i < n; i++) f = f * pairing::miller_loop(bit_cast_img<Affine<HFp>>(p[i]), bit_cast_img<Affine<HFp2>>(q[i]));
    f12_to_gt(pairing::final_exp(f), out);
    return ZK_OK;
}

int zk_bn254_pair(const zk_g1_affine* p, const zk_g2_affine* q, size_t n, zk_gt* out) {
    if ((n && (!p || !q)) || !out) return set_err(ZK_ERR_ARG, "null pointer");
    ZK_TRY(ensure_init());
    const PairConsts K = pair_consts();
    SlotGuard g;
    ZK_TRY(acquire_slot(&g.s));
    Slot* s = g.s;
    hipStream_t st = s->stream;
    const size_t ch = std::min(std::max(n, (size_t)1), CHUNK);
    ZK_TRY(s->reserve(ch * (64 + 128 + 384 + 384) + (FE_SLOTS + 1) * 384 + SLACK));
    Affine<Fp>* d_p = (Affine<Fp>*)s->alloc(ch * 64);
    Affine<Fp2>* d_q = (Affine<Fp2>*)s->alloc(ch * 128);
    F12* d_m = (F12*)s->alloc(ch * 384);
    F12* d_b = (F12*)s->alloc(ch * 384);
    F12* d_ws = (F12*)s->alloc((FE_SLOTS + 1) * 384);
    if (!d_p || !d_q || !d_m || !d_b || !d_ws) return set_err(ZK_ERR_ARG, "pair: workspace");
    F12 acc = F12::one();  // the chunks' Miller products, multiplied on the host (one product per 2^16 pairs)
    for (size_t c0 = 0; c0 < n; c0 += ch) {
        const size_t m = std::min(ch, n - c0);
        ZK_HIP(hipMemcpyAsync(d_p, p + c0, m * 64, hipMemcpyHostToDevice, st));
        ZK_HIP(hipMemcpyAsync(d_q, q + c0, m * 128, hipMemcpyHostToDevice, st));
        ZK_LAUNCH(s, st, "miller_loop", k_miller, dim3(blocks(m, PAIR_BLOCK)), dim3(PAIR_BLOCK), 0, (const Affine<Fp>*)d_p, m, (const Affine<Fp2>*)d_q, m,
                  (const Affine<Fp2>*)nullptr, (size_t)1, K, d_m);
        const F12* r = fold_all(s, st, "f12_fold", k_f12_fold, PAIR_BLOCK, d_m, d_b, m, 1);
        F12 part;
        ZK_HIP(hipMemcpyAsync(&part, r, 384, hipMemcpyDeviceToHost, st));
        ZK_TRY(slot_sync(s, st));
        acc = acc * part;
    }
    ZK_HIP(hipMemcpyAsync(d_ws + FE_SLOTS, &acc, 384, hipMemcpyHostToDevice, st));
    ZK_TRY(final_exp(s, st, K, d_ws + FE_SLOTS, 1, 1, nullptr, d_ws, d_m, nullptr, nullptr));
    ZK_HIP(hipMemcpyAsync(out, d_m, 384, hipMemcpyDeviceToHost, st));
    return slot_sync(s, st);
}

int zk_bn254_groth16_verify_batch(const uint8_t* proofs, size_t n_proofs, const void* vk, size_t vk_len, int vk_is_hex, const zk_fr* public_inputs,
                                  size_t n_public, uint8_t* accepted, size_t* n_accepted) {
    if (!vk || !n_accepted || (n_proofs && (!proofs || !accepted)) || (n_proofs && n_public && !public_inputs)) return set_err(ZK_ERR_ARG, "null pointer");
    *n_accepted = 0;
    Groth16Vk v;
    ZK_TRY(groth16_vk_parse(vk, vk_len, vk_is_hex, &v));
    const size_t nk = v.K.size();
    if (nk != n_public + 1) return set_err(ZK_ERR_LEN, "invalid witness size, got %zu, expected %zu (public - ONE_WIRE)", n_public, nk ? nk - 1 : 0);  // upstream's message
    if (n_proofs == 0) return ZK_OK;
    ZK_TRY(ensure_init());
    const PairConsts K = pair_consts();
    const size_t np = n_public, cols = np + 1;

    // r_i = low 128 bits of SHA-256(tag || SHA-256(vk) || SHA-256(proofs || public inputs) || u64 i), forced non-zero
    uint8_t pre[18 + 32 + 32 + 8];
    memcpy(pre, "zkmi-groth16-batch", 18);
    sha(v.bytes.data(), v.bytes.size(), pre + 18);
    {
        Sha256 h;
        h.update(proofs, n_proofs * 128);
        if (np) h.update(public_inputs, n_proofs * np * 32);
        h.final(pre + 50);
    }

    SlotGuard g;
    ZK_TRY(acquire_slot(&g.s));
    Slot* s = g.s;
    hipStream_t st = s->stream;
    const size_t ch = std::min(n_proofs, CHUNK);
    const size_t per = 128 + 64 + 64 + 128 + 3 + 1 + 1 + 16 + 128 + 64 + np * 32 + cols * 32 * 2 + 3 * 64 + 3 * 384 + FE_SLOTS * 384 + G2_DECOMPRESS_SCRATCH;
    ZK_TRY(s->reserve(ch * per + nk * 64 + 16 * 384 + 64 * 1024));
    uint8_t* d_raw = (uint8_t*)s->alloc(ch * 128);        // Ar | Bs | Krs, each contiguous
    Affine<Fp>* d_ar = (Affine<Fp>*)s->alloc(ch * 64);
    Affine<Fp>* d_krs = (Affine<Fp>*)s->alloc(ch * 64);
    Affine<Fp2>* d_bs = (Affine<Fp2>*)s->alloc(ch * 128);
    uint8_t* d_bad = (uint8_t*)s->alloc(ch * 3);
    uint8_t* d_valid = (uint8_t*)s->alloc(ch);
    uint32_t* d_rr = (uint32_t*)s->alloc(ch * 16);
    XYZZ<Fp>* d_rk = (XYZZ<Fp>*)s->alloc(ch * 128);
    XYZZ<Fp>* d_rk2 = (XYZZ<Fp>*)s->alloc((ch + 1) / 2 * 128);
    Fr* d_pub = (Fr*)s->alloc(std::max(ch * np, (size_t)1) * 32);
    Fr* d_terms = (Fr*)s->alloc(ch * cols * 32);
    Fr* d_terms2 = (Fr*)s->alloc((ch + 1) / 2 * cols * 32);
    Affine<Fp>* d_p = (Affine<Fp>*)s->alloc((3 * ch + 3) * 64);
    F12* d_m = (F12*)s->alloc((3 * ch + 3) * 384);
    F12* d_ws = (F12*)s->alloc(std::max(FE_SLOTS * ch, 3 * ch + 3) * 384);
    Affine<Fp>* d_kpts = (Affine<Fp>*)s->alloc(nk * 64);
    Affine<Fp2>* d_fix = (Affine<Fp2>*)s->alloc(3 * 128);
    F12* d_one_ws = (F12*)s->alloc(FE_SLOTS * 384);
    uint8_t* d_verdict = (uint8_t*)s->alloc(ch);
    int* d_status = (int*)s->alloc(64);
    uint8_t* d_chk = (uint8_t*)s->alloc(64);
    if (!d_raw || !d_ar || !d_krs || !d_bs || !d_bad || !d_valid || !d_rr || !d_rk || !d_rk2 || !d_pub || !d_terms || !d_terms2 || !d_p || !d_m || !d_ws || !d_kpts ||
        !d_fix || !d_one_ws || !d_verdict || !d_status || !d_chk)
        return set_err(ZK_ERR_ARG, "groth16_verify_batch: workspace");
    ZK_HIP(hipMemcpyAsync(d_kpts, v.K.data(), nk * 64, hipMemcpyHostToDevice, st));
    const size_t arena_mark = s->arena_off;  // g2_decompress_dev takes its scratch from the arena per call: give it back per chunk

    std::vector<uint8_t> raw(ch * 128), valid(ch), one(1);
    std::vector<uint32_t> rr(ch * 4);
    size_t total = 0;
    for (size_t c0 = 0; c0 < n_proofs; c0 += ch) {
        const size_t n = std::min(ch, n_proofs - c0);
        s->arena_off = arena_mark;
        for (size_t i = 0; i < n; i++) {
            const uint8_t* pr = proofs + (c0 + i) * 128;
            memcpy(&raw[i * 32], pr, 32);
            memcpy(&raw[n * 32 + i * 64], pr + 32, 64);
            memcpy(&raw[n * 96 + i * 32], pr + 96, 32);
            const uint64_t idx = c0 + i;
            for (int b = 0; b < 8; b++) pre[82 + b] = (uint8_t)(idx >> (8 * b));
            uint8_t d[32];
            sha(pre, sizeof pre, d);
            uint32_t* r = &rr[4 * i];  // the low 128 bits of the digest read as a big-endian integer
            for (int w = 0; w < 4; w++) r[w] = ((uint32_t)d[28 - 4 * w] << 24) | ((uint32_t)d[29 - 4 * w] << 16) | ((uint32_t)d[30 - 4 * w] << 8) | d[31 - 4 * w];
            if ((r[0] | r[1] | r[2] | r[3]) == 0) r[0] = 1;
        }
        ZK_HIP(hipMemcpyAsync(d_raw, raw.data(), n * 128, hipMemcpyHostToDevice, st));
        ZK_HIP(hipMemcpyAsync(d_rr, rr.data(), n * 16, hipMemcpyHostToDevice, st));
        if (np) ZK_HIP(hipMemcpyAsync(d_pub, public_inputs + c0 * np, n * np * 32, hipMemcpyHostToDevice, st));
        ZK_HIP(hipMemsetAsync(d_bad, 0, n * 3, st));
        ZK_HIP(hipMemsetAsync(d_status, 0, 4, st));
        ZK_TRY(g1_decompress_dev(s, st, d_raw, n, d_ar, d_status, d_bad));
        ZK_TRY(g2_decompress_dev(s, st, d_raw + n * 32, n, d_bs, d_status, d_bad + n));
        ZK_TRY(g1_decompress_dev(s, st, d_raw + n * 96, n, d_krs, d_status, d_bad + 2 * n));
        ZK_LAUNCH(s, st, "vb_prep", k_vb_prep, dim3(blocks(n, 128)), dim3(128), 0, (const Affine<Fp>*)d_ar, (const Affine<Fp>*)d_krs, (const uint8_t*)d_bad,
                  (const uint32_t*)d_rr, (const Fr*)d_pub, n, np, d_valid, d_p, d_rk, d_terms);
        const XYZZ<Fp>* rk_sum = fold_all(s, st, "g1_fold", k_g1_fold, 256, d_rk, d_rk2, n, 1);
        const Fr* c_sum = fold_all(s, st, "fr_fold", k_fr_fold, 256, d_terms, d_terms2, n, cols);
        XYZZ<HFp> rk;
        std::vector<HFr> c(cols);
        ZK_HIP(hipMemcpyAsync(&rk, rk_sum, 128, hipMemcpyDeviceToHost, st));
        ZK_HIP(hipMemcpyAsync(c.data(), c_sum, cols * 32, hipMemcpyDeviceToHost, st));
        ZK_HIP(hipMemcpyAsync(valid.data(), d_valid, n, hipMemcpyDeviceToHost, st));
        ZK_TRY(slot_sync(s, st));
        size_t n_valid = 0;
        for (size_t i = 0; i < n; i++) n_valid += valid[i];
        if (n_valid == 0) {
            memset(accepted + c0, 0, n);
            continue;
        }
        // the three fixed-key terms (O(n_public) host work): -c_0 alpha, -sum_j c_j K_j, -sum_i r_i Krs_i
        Affine<HFp> fixed[3];
        {
            uint32_t k[8];
            to_canonical_u32(c[0], k);
            fixed[0] = scalar_mul(v.alpha, k).to_affine().neg();
            XYZZ<HFp> ic = XYZZ<HFp>::inf();
            for (size_t j = 0; j < cols; j++) {
                to_canonical_u32(c[j], k);
                ic.add(scalar_mul(v.K[j], k));
            }
            fixed[1] = ic.to_affine().neg();
            fixed[2] = rk.to_affine().neg();
        }
        const Affine<HFp2> qfix_b[3] = {v.beta, v.gamma, v.delta};
        ZK_HIP(hipMemcpyAsync(d_p + n, fixed, 3 * 64, hipMemcpyHostToDevice, st));
        ZK_HIP(hipMemcpyAsync(d_fix, qfix_b, 3 * 128, hipMemcpyHostToDevice, st));
        ZK_LAUNCH(s, st, "miller_loop", k_miller, dim3(blocks(n + 3, PAIR_BLOCK)), dim3(PAIR_BLOCK), 0, (const Affine<Fp>*)d_p, n + 3, (const Affine<Fp2>*)d_bs, n,
                  (const Affine<Fp2>*)d_fix, (size_t)1, K, d_m);
        const F12* prod = fold_all(s, st, "f12_fold", k_f12_fold, PAIR_BLOCK, d_m, d_ws, n + 3, 1);
        ZK_HIP(hipMemsetAsync(d_chk, 1, 1, st));  // d_chk[0]: "valid", d_chk[1]: the verdict
        ZK_TRY(final_exp(s, st, K, prod, 1, 1, nullptr, d_one_ws, nullptr, d_chk, d_chk + 1));
        ZK_HIP(hipMemcpyAsync(one.data(), d_chk + 1, 1, hipMemcpyDeviceToHost, st));
        ZK_TRY(slot_sync(s, st));
        if (one[0]) {
            memcpy(accepted + c0, valid.data(), n);
            total += n_valid;
            continue;
        }
        // fallback: every valid proof on its own
        const Affine<HFp2> qfix_f[3] = {v.gamma, v.delta, v.beta};
        ZK_HIP(hipMemcpyAsync(d_fix, qfix_f, 3 * 128, hipMemcpyHostToDevice, st));
        ZK_HIP(hipMemcpyAsync(d_p + 3 * n, &v.alpha, 64, hipMemcpyHostToDevice, st));
        ZK_LAUNCH(s, st, "vb_single", k_vb_single, dim3(blocks(n, 128)), dim3(128), 0, (const Affine<Fp>*)d_ar, (const Affine<Fp>*)d_krs, (const uint8_t*)d_valid,
                  (const Fr*)d_pub, (const Affine<Fp>*)d_kpts, n, np, d_p);
        ZK_LAUNCH(s, st, "miller_loop", k_miller, dim3(blocks(3 * n + 1, PAIR_BLOCK)), dim3(PAIR_BLOCK), 0, (const Affine<Fp>*)d_p, 3 * n + 1,
                  (const Affine<Fp2>*)d_bs, n, (const Affine<Fp2>*)d_fix, n, K, d_m);
        ZK_TRY(final_exp(s, st, K, d_m, n, 3, d_m + 3 * n, d_ws, nullptr, d_valid, d_verdict));
        ZK_HIP(hipMemcpyAsync(accepted + c0, d_verdict, n, hipMemcpyDeviceToHost, st));
        ZK_TRY(slot_sync(s, st));
        for (size_t i = 0; i < n; i++) total += accepted[c0 + i] ? 1 : 0;
    }
    *n_accepted = total;
    return ZK_OK;
}

}  // extern "C"
