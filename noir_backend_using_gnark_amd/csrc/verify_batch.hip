// Pairings and batch Groth16 / PLONK / KZG verification on the device (include/zkmi.h "Pairings and batch Groth16 / PLONK verification on the DEVICE").
//   zk_bn254_pair   one Miller loop per lane (k_miller), a product tree (k_f12_fold), one final exponentiation (k_fe_*)
// The three batch verifiers work in chunks of at most 2^16 lanes and share one pairing check per chunk (PairCheck):
//   coefficients   128 bits per lane from SHA-256 (batch_coeff: on the host in batch_coeffs, PLONK's on the device in k_pv_kzg)
//   combine        the lanes' points times their coefficients, summed by halving folds (k_g1_fold / k_fr_fold); the host adds the fixed-key terms
//   check          Miller loops over the folded points, the product tree, one final exponentiation: a product of one accepts every valid lane
//   fallback       (only when the check fails) each valid lane's own Miller loops, a final exponentiation and a verdict per lane
// The Groth16 and PLONK verifiers have two forms over one core each (groth16_verify_rows, plonk_verify_rows; RowsIn says where the rows are): the host-input
// entries, whose chunks go up into the workspace, and the _dev entries, which read proofs and public inputs where they lie in HBM, a stride apart.  The core takes
// the coefficients' prefix from its entry: the host form hashes proofs || public inputs on the host as it always did, the device form hashes one digest per row on
// the device (k_rows_digest) and the digests on the host -- under another tag, so the two derivations never meet.
// What each adds (the kernels say the rest):
//   groth16 (one lane per proof)   k_vb_gather (the proof's three slots into the decompressors' arrays); k_g1_decompress / k_g2_decompress with a flag per invalid point; k_vb_prep: r_i Ar_i, r_i Krs_i, r_i (1, w_i1, ..); check: n' + 3
//       lanes, prod e(r_i Ar_i, Bs_i) e(-c_0 alpha, beta) e(-sum c_j K_j, gamma) e(-sum r_i Krs_i, delta) == 1; fallback: k_vb_single, 3 n + 1 lanes (the last: e(alpha, beta))
//   groth16, a key per row (groth16_verify_rows_keys; DESIGN §3.9 "Many keys")   the host sorts the chunk's lanes by key (integers only); k_vbk_prep; per-key
//       sums over tiles of 16 sorted items (k_vbk_g1_fold, k_vbk_coef, k_vbk_fr_fold); the fixed terms on the device (k_vbk_fixed, k_vbk_tail); check:
//       n' + 3 K_used lanes; fallback: k_vbk_single, 4 n lanes, every Q the lane's key's
//   plonk (one lane per proof)   k_pv_gather, k_g1_decompress, k_pv_transcript, k_pv_scalars, k_pv_smul + k_pv_digests, k_pv_kzg, k_pv_smul +
//       k_pv_combine (A_i, B_i); check: 2 lanes, e(sum A + the G, S1, S2 terms, [1]2) e(-sum B, [alpha]2) == 1; fallback: k_pv_smul + k_pv_single, 2 n lanes
//   plonk, a key per row (plonk_verify_rows_keys)   the k_pvk_* twins of those kernels read the lane's key from a table in HBM (PvKeyRow, key_of); c_S1 S1 and
//       c_S2 S2 are two more rows of the second k_pvk_smul launch and part of A_i; check: 2 lanes, e(sum A + the G term, [1]2) e(-sum B, [alpha]2) == 1
//   kzg (one lane per opening)   k_kzg_combine (lambda_i T_i, lambda_i H_i and the lane's own pair); check: 2 lanes; fallback: 2 n lanes
#include <string.h>

#include <algorithm>
#include <string>
#include <thread>
#include <vector>

#include "ctx.hpp"
#include "curve.hpp"
#include "fs_dev.hpp"
#include "host_ff.hpp"
#include "keyio.hpp"
#include "pairing.hpp"
#include "pairing_dev.hpp"
#include "proofio.hpp"
#include "sha256_dev.hpp"
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

// The rows of a call as the kernels below read them: row i's proof bytes at proofs + i * stride (any alignment), its public inputs at pub + i * ps elements.
// A little-endian word of a row:
ZK_D uint32_t row_word(const uint8_t* p, bool aligned) {
    if (aligned) return *reinterpret_cast<const uint32_t*>(p);
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

// d_v = SHA-256(a_v || b_v), one lane per row (zkmi.h: zk_bn254_rows_sha256_dev; the device forms of the verifiers derive their coefficients from these)
ZK_D void rows_digest_lane(size_t i, const uint8_t* __restrict__ a, size_t a_len, size_t a_stride, const uint8_t* __restrict__ b, size_t b_len, size_t b_stride,
                           uint8_t* __restrict__ out) {
    Sha256Dev h;
    h.reset();
    if (a_len) h.update(a + i * a_stride, a_len);
    if (b_len) h.update(b + i * b_stride, b_len);
    uint32_t d[8];
    h.final(d);
#pragma unroll
    for (int k = 0; k < 8; k++)
#pragma unroll
        for (int j = 0; j < 4; j++) out[32 * i + 4 * k + j] = (uint8_t)(d[k] >> (24 - 8 * j));
}
__global__ __launch_bounds__(64) void k_rows_digest(const uint8_t* __restrict__ a, size_t a_len, size_t a_stride, const uint8_t* __restrict__ b, size_t b_len,
                                                    size_t b_stride, size_t rows, uint8_t* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows) return;
    rows_digest_lane(i, a, a_len, a_stride, b, b_len, b_stride, out);
}

// the 128-byte Groth16 proof into the arrays the decompressors read: raw = Ar (n x 32 bytes) | Bs (n x 64) | Krs (n x 32), as words
__global__ __launch_bounds__(256) void k_vb_gather(const uint8_t* __restrict__ proofs, size_t stride, size_t n, uint32_t* __restrict__ raw) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint8_t* p = proofs + i * stride;
    const bool al = ((uintptr_t)p & 3) == 0;
#pragma unroll
    for (int j = 0; j < 8; j++) raw[i * 8 + j] = row_word(p + 4 * j, al);
#pragma unroll
    for (int j = 0; j < 16; j++) raw[n * 8 + i * 16 + j] = row_word(p + 32 + 4 * j, al);
#pragma unroll
    for (int j = 0; j < 8; j++) raw[n * 24 + i * 8 + j] = row_word(p + 96 + 4 * j, al);
}

// per proof: valid = no invalid point; r_i Ar_i (affine; infinity when invalid), r_i Krs_i, and the row r_i (1, w_i1, .., w_i,np) of the mat-vec
__global__ __launch_bounds__(128) void k_vb_prep(const Affine<Fp>* __restrict__ ar, const Affine<Fp>* __restrict__ krs, const uint8_t* __restrict__ bad,
                                                 const uint32_t* __restrict__ rr, const Fr* __restrict__ pub, size_t ps, size_t n, size_t np,
                                                 uint8_t* __restrict__ valid, Affine<Fp>* __restrict__ p_out, XYZZ<Fp>* __restrict__ rk_out, Fr* __restrict__ terms) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const bool ok = !(bad[i] | bad[n + i] | bad[2 * n + i]);
    valid[i] = ok ? 1 : 0;
    const uint32_t k[8] = {rr[4 * i], rr[4 * i + 1], rr[4 * i + 2], rr[4 * i + 3], 0, 0, 0, 0};
    Fr rm = Fr::zero();
    for (int j = 0; j < 4; j++) rm.l[j] = k[j];
    rm = ok ? rm.to_mont() : Fr::zero();
    terms[i * (np + 1)] = rm;
    for (size_t j = 0; j < np; j++) terms[i * (np + 1) + 1 + j] = rm * pub[i * ps + j];
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
                                                   const Fr* __restrict__ pub, size_t ps, const Affine<Fp>* __restrict__ kpts, size_t n, size_t np,
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
        const Fr w = pub[i * ps + j].from_mont();
        ic.add(scalar_mul(kpts[1 + j], w.l));
    }
    P[n + i] = ic.to_affine();
}

// ---- Groth16 against many keys (DESIGN 3.9 "Many keys"): row i is a proof for vks[key_of[i]].  The keys share nothing, so a chunk's lanes are sorted by
// key on the host (integers only: perm, the used keys' segments, tile tables) and every per-key sum is a segmented sum over tiles of at most GK_T
// consecutive sorted items that never cross a key: one partial per tile and level, as many levels as GK_T^levels >= the chunk asks for, whatever the keys are.
struct GkKeyRow {
    Affine<Fp> alpha;
    Affine<Fp2> beta, gamma, delta;
    uint32_t np, koff;  // n_public; where K_0 .. K_np lie in the ragged array of all keys' K points
    uint32_t pad[2];
};
// a key used in the chunk: its index in the table, where its np + 1 coefficients c_{k,j} (and fixed terms) lie
struct GkSeg {
    uint32_t key, coff;
};
// one tile of one level: the items [start, start + len) of the level's input give item (the tile's index) of its output.  For the Fr sums the tile is a
// len x cols matrix at fin (levels above the first) and a row of cols at fout
struct GkTile {
    uint32_t start, len, cols, fin, fout;
};
constexpr uint32_t GK_T = 16;

// d_v = SHA-256(row v's 128 bytes || its 32 n_public(key_of[v]) public-input bytes): k_rows_digest_keys over the Groth16 table
__global__ __launch_bounds__(64) void k_vbk_rows_digest(const uint8_t* __restrict__ a, size_t a_len, size_t a_stride, const uint8_t* __restrict__ b, size_t b_stride,
                                                        const GkKeyRow* __restrict__ tab, const uint32_t* __restrict__ key_of, size_t rows,
                                                        uint8_t* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows) return;
    rows_digest_lane(i, a, a_len, a_stride, b, (size_t)tab[key_of[i]].np * 32, b_stride, out);
}
// k_vb_prep per sorted position p (lane i = perm[p]): valid[i] and r_i Ar_i stay in lane order beside Bs_i; r_i Krs_i and r_i (Montgomery; zero when the
// lane is invalid) land in key-sorted order.  The public inputs are read by k_vbk_coef, which knows each key's n_public from its tiles
__global__ __launch_bounds__(128) void k_vbk_prep(const Affine<Fp>* __restrict__ ar, const Affine<Fp>* __restrict__ krs, const uint8_t* __restrict__ bad,
                                                  const uint32_t* __restrict__ rr, const uint32_t* __restrict__ perm, size_t n, uint8_t* __restrict__ valid,
                                                  Affine<Fp>* __restrict__ p_out, XYZZ<Fp>* __restrict__ rk_out, Fr* __restrict__ rm_out) {
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const size_t i = perm[p];
    const bool ok = !(bad[i] | bad[n + i] | bad[2 * n + i]);
    valid[i] = ok ? 1 : 0;
    const uint32_t k[8] = {rr[4 * i], rr[4 * i + 1], rr[4 * i + 2], rr[4 * i + 3], 0, 0, 0, 0};
    Fr rm = Fr::zero();
    for (int j = 0; j < 4; j++) rm.l[j] = k[j];
    rm_out[p] = ok ? rm.to_mont() : Fr::zero();
    if (!ok) {
        p_out[i] = Affine<Fp>::inf();
        rk_out[p] = XYZZ<Fp>::inf();
        return;
    }
    p_out[i] = scalar_mul(ar[i], k).to_affine();
    rk_out[p] = scalar_mul(krs[i], k);
}
// one level of the segmented G1 sums: out[t] = sum of in over tile t
__global__ __launch_bounds__(64) void k_vbk_g1_fold(const XYZZ<Fp>* __restrict__ in, const GkTile* __restrict__ tiles, size_t n_tiles, XYZZ<Fp>* __restrict__ out) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_tiles) return;
    const GkTile T = tiles[t];
    XYZZ<Fp> a = in[T.start];
    for (uint32_t q = 1; q < T.len; q++) a.add(in[T.start + q]);
    out[t] = a;
}
// the first level of c_{k,j} = sum_i r_i w_ij (w_i0 = 1), one workgroup per tile and one lane per j <= n_public(k): the tile's rows of `pub` are read
// through the permutation, and nothing behind a row's own n_public
__global__ __launch_bounds__(64) void k_vbk_coef(const Fr* __restrict__ rm, const uint32_t* __restrict__ perm, const Fr* __restrict__ pub, size_t ps,
                                                 const GkTile* __restrict__ tiles, Fr* __restrict__ out) {
    const GkTile T = tiles[blockIdx.x];
    for (uint32_t j = threadIdx.x; j < T.cols; j += blockDim.x) {
        Fr a = Fr::zero();
        for (uint32_t q = T.start; q < T.start + T.len; q++) a = a + (j ? rm[q] * pub[(size_t)perm[q] * ps + (j - 1)] : rm[q]);
        out[T.fout + j] = a;
    }
}
// the levels above: column sums of the tile's len x cols partial sums
__global__ __launch_bounds__(64) void k_vbk_fr_fold(const Fr* __restrict__ in, const GkTile* __restrict__ tiles, Fr* __restrict__ out) {
    const GkTile T = tiles[blockIdx.x];
    for (uint32_t j = threadIdx.x; j < T.cols; j += blockDim.x) {
        Fr a = in[T.fin + j];
        for (uint32_t q = 1; q < T.len; q++) a = a + in[T.fin + (size_t)q * T.cols + j];
        out[T.fout + j] = a;
    }
}
// the fixed terms, one workgroup per used key u and one lane per term: fx[coff + j] = c_{k,j} K_{k,j} for j <= n_public(k) (full 256-bit scalars), and
// fa[u] = c_{k,0} alpha_k
__global__ __launch_bounds__(64) void k_vbk_fixed(const Fr* __restrict__ c, const GkSeg* __restrict__ segs, const GkKeyRow* __restrict__ tab,
                                                  const Affine<Fp>* __restrict__ kpts, XYZZ<Fp>* __restrict__ fx, XYZZ<Fp>* __restrict__ fa) {
    const GkSeg S = segs[blockIdx.x];
    const uint32_t cols = tab[S.key].np + 1, koff = tab[S.key].koff;
    for (uint32_t j = threadIdx.x; j <= cols; j += blockDim.x) {
        const Fr s = c[S.coff + (j < cols ? j : 0)].from_mont();
        const Affine<Fp> pt = j < cols ? kpts[koff + j] : tab[S.key].alpha;
        const XYZZ<Fp> v = scalar_mul(pt, s.l);
        if (j < cols) fx[S.coff + j] = v;
        else fa[blockIdx.x] = v;
    }
}
// per used key u: the Miller lanes n + 3 u .. of the combined check, P = (-c_{k,0} alpha_k, -IC_k, -sum r_i Krs_i), Q = (beta_k, gamma_k, delta_k)
__global__ __launch_bounds__(64) void k_vbk_tail(const XYZZ<Fp>* __restrict__ fa, const XYZZ<Fp>* __restrict__ ic, const XYZZ<Fp>* __restrict__ rk,
                                                 const GkSeg* __restrict__ segs, const GkKeyRow* __restrict__ tab, size_t n_segs, Affine<Fp>* __restrict__ P,
                                                 Affine<Fp2>* __restrict__ qfix) {
    const size_t u = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= n_segs) return;
    const GkKeyRow* K = tab + segs[u].key;
    P[3 * u] = fa[u].to_affine().neg();
    P[3 * u + 1] = ic[u].to_affine().neg();
    P[3 * u + 2] = rk[u].to_affine().neg();
    qfix[3 * u] = K->beta;
    qfix[3 * u + 1] = K->gamma;
    qfix[3 * u + 2] = K->delta;
}
// fallback, per proof under its own key k: P = (-Ar_i, IC_i, Krs_i, alpha_k) against Q = (Bs_i -- in place already --, gamma_k, delta_k, beta_k), row r of
// both at [r n + i].  Its launch name, vbk_single, is what says "the per-lane fallback ran"
__global__ __launch_bounds__(128) void k_vbk_single(const Affine<Fp>* __restrict__ ar, const Affine<Fp>* __restrict__ krs, const uint8_t* __restrict__ valid,
                                                    const Fr* __restrict__ pub, size_t ps, const GkKeyRow* __restrict__ tab,
                                                    const Affine<Fp>* __restrict__ kpts, const uint32_t* __restrict__ key_of, size_t n,
                                                    Affine<Fp>* __restrict__ P, Affine<Fp2>* __restrict__ Q) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const GkKeyRow* K = tab + key_of[i];
    Q[n + i] = K->gamma;
    Q[2 * n + i] = K->delta;
    Q[3 * n + i] = K->beta;
    if (!valid[i]) {
        P[i] = P[n + i] = P[2 * n + i] = P[3 * n + i] = Affine<Fp>::inf();
        return;
    }
    P[i] = ar[i].neg();
    P[2 * n + i] = krs[i];
    P[3 * n + i] = K->alpha;
    const Affine<Fp>* kp = kpts + K->koff;
    XYZZ<Fp> ic = XYZZ<Fp>::from_affine(kp[0]);
    for (size_t j = 0; j < K->np; j++) {
        const Fr w = pub[i * ps + j].from_mont();
        ic.add(scalar_mul(kp[1 + j], w.l));
    }
    P[n + i] = ic.to_affine();
}

// ---- batch PLONK verification: one lane per proof, Fr values per lane as columns sc[k n + i]
enum PvCol {
    PV_CLAIM = 0,  // 7 claimed values: quotient, linearised polynomial, l, r, o, s1, s2 at zeta (reduced mod r)
    PV_ZU = 7,     // z(omega zeta)
    PV_GAMMA, PV_BETA, PV_ALPHA, PV_ZETA,  // the transcript's challenges (this order: PV_GAMMA + c)
    PV_ZP, PV_ZP2, PV_LR, PV_CS3, PV_CZ,   // the digests' scalars: zeta^(n+2), zeta^(2(n+2)), l r, S3's and Z's coefficients
    PV_T,          // 10 scalars of the combined opening check (k_pv_kzg)
    PV_NCOL = PV_T + 10
};
// points per lane (pts[k n + i]) in proof order: L R O Z H0 H1 H2 BatchH ZShiftH; the key's points (device copy): S1 S2 S3 Ql Qr Qm Qo Qk, then G
enum { PV_L = 0, PV_Z = 3, PV_H0 = 4, PV_W = 7, PV_WS = 8, PV_NPTS = 9 };
struct PvKey {
    uint64_t n;
    uint32_t log_n;
    Fr size_inv, gen, u;
};
// one scalar multiplication per lane: out = k_i P_i (P fixed when step == 0); k_pv_smul runs a table of them, one per grid row
struct PvTerm {
    const Affine<Fp>* pts;
    size_t step;
    const Fr* sc;
};
// The many-key entries (zk_bn254_plonk_verify_batch_keys; DESIGN §3.10 "Many keys"): one row per key in HBM, lane i reads row key_of[i] where the single-key
// kernels take K, kpts, mid and np as arguments.  gamma's prefix "gamma" || RawBytes(S1..Qk) is 517 bytes for every key -- eight blocks and five bytes --, so
// the midstate's length and the tail's are the same for all keys and stay kernel arguments
struct PvKeyRow {
    PvKey K;
    uint64_t np;
    Affine<Fp> pts[9];  // S1 S2 S3 Ql Qr Qm Qo Qk G
    uint32_t mid[8];    // SHA-256 chaining value after the prefix's whole blocks
    uint8_t pre[24];    // the prefix's last bytes, then "betaalphazeta" (k_pv_transcript's pre)
};
// a term of k_pvk_smul: the lane's key's point kpt when kpt >= 0, pts[i] otherwise
struct PvkTerm {
    const Affine<Fp>* pts;
    int kpt;
    const Fr* sc;
};

// 256-bit big-endian word image (8 x u32 read straight from the bytes) -> limbs, reduced mod r as fr.SetBytes, Montgomery
ZK_D Fr fr_from_be_words(const uint32_t* p) {
    uint32_t t[8];
#pragma unroll
    for (int k = 0; k < 8; k++) t[k] = __builtin_bswap32(p[7 - k]);
    Fr r = Fr::reduce_once(t);
#pragma unroll
    for (int k = 0; k < 4; k++) r = Fr::reduce_once(r.l);  // 2^256 < 6 r
    return r.to_mont();
}

// header (bytes 256..259 = 00 00 00 07), the nine compressed points into their own arrays, the eight values reduced mod r
__global__ __launch_bounds__(256) void k_pv_gather(const uint8_t* __restrict__ proofs, size_t stride, size_t n, uint32_t* __restrict__ praw, Fr* __restrict__ sc,
                                                   uint8_t* __restrict__ hdr_bad) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint8_t* p = proofs + i * stride;
    const bool al = ((uintptr_t)p & 3) == 0;
    const int off[PV_NPTS] = {0, 8, 16, 24, 32, 40, 48, 56, 121};
#pragma unroll
    for (int k = 0; k < PV_NPTS; k++)
#pragma unroll
        for (int j = 0; j < 8; j++) praw[(k * n + i) * 8 + j] = row_word(p + 4 * (off[k] + j), al);
    hdr_bad[i] = row_word(p + 4 * 64, al) != 0x07000000u;  // little-endian read of 00 00 00 07
#pragma unroll 1
    for (int k = 0; k < 8; k++) {
        uint32_t w[8];
#pragma unroll
        for (int j = 0; j < 8; j++) w[j] = row_word(p + 4 * ((k < 7 ? 65 + 8 * k : 129) + j), al);
        sc[(PV_CLAIM + k) * n + i] = fr_from_be_words(w);
    }
}

// gamma, beta, alpha, zeta as FsTranscript derives them.  gamma's prefix ("gamma" || S1..Qk) is the same for every lane: the host hashed its whole blocks
// (mid = the chaining value after mid_len bytes) and pre holds the rest, then "beta", "alpha", "zeta"
__global__ __launch_bounds__(64) void k_pv_transcript(const Affine<Fp>* __restrict__ pts, const uint8_t* __restrict__ bad, const uint8_t* __restrict__ hdr_bad,
                                                      const Fr* __restrict__ pub, size_t ps, size_t n, size_t np, const uint32_t* __restrict__ mid, uint64_t mid_len,
                                                      const uint8_t* __restrict__ pre, uint32_t tail_len, uint8_t* __restrict__ valid, Fr* __restrict__ sc) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    // (pvk_transcript_lane below is a copy of these steps: every edit here is to be made there too)
    bool ok = !hdr_bad[i];
    for (int k = 0; k < PV_NPTS; k++) ok = ok && !bad[k * n + i];
    valid[i] = ok;
    if (!ok) return;
    uint32_t prev[8];
#pragma unroll 1
    for (int c = 0; c < 4; c++) {
        Sha256Dev h;
        if (c == 0) h.resume(mid, mid_len);
        else h.reset();
        const uint32_t off = c == 0 ? 0 : c == 1 ? tail_len : c == 2 ? tail_len + 4 : tail_len + 9, len = c == 0 ? tail_len : c == 2 ? 5 : 4;
        h.update(pre + off, len);
        if (c) h.put256(prev);
        // bindings: gamma: public inputs, L, R, O; beta: none; alpha: Z; zeta: H0, H1, H2 -- 32-byte items
        const size_t items = c == 0 ? np + 6 : c == 1 ? 0 : c == 2 ? 2 : 6;
#pragma unroll 1
        for (size_t j = 0; j < items; j++) {
            uint32_t l[8];
            if (c == 0 && j < np) {
                const Fr w = pub[i * ps + j].from_mont();
#pragma unroll
                for (int k = 0; k < 8; k++) l[k] = w.l[k];
            } else {
                const size_t q = c == 0 ? j - np : j;
                const int pt = (c == 0 ? PV_L : c == 2 ? PV_Z : PV_H0) + (int)(q >> 1);
                raw_half(pts[pt * n + i], (int)(q & 1), l);
            }
            h.put256(l);
        }
        uint32_t d[8];
        h.final(d);
        sha_words_to_limbs(d, prev);  // the next challenge binds the raw digest
        sc[(PV_GAMMA + c) * n + i] = fr_from_digest(d);
    }
}
// The many-key kernels (k_pvk_*) read the lane's row of the key table where the single-key kernels take arguments; from k_pv_scalars on, the two kernels of a
// pair call one per-lane function.  Not here: this is a COPY of k_pv_transcript's steps for k_pvk_transcript, because sharing one function made k_pv_transcript
// spill 10 SGPRs instead of 5.  The two bodies are kept in step by hand: every edit of one is to be made in the other
ZK_D void pvk_transcript_lane(size_t i, const Affine<Fp>* __restrict__ pts, const uint8_t* __restrict__ bad, const uint8_t* __restrict__ hdr_bad,
                              const Fr* __restrict__ pub, size_t ps, size_t n, size_t np, const uint32_t* __restrict__ mid, uint64_t mid_len,
                              const uint8_t* __restrict__ pre, uint32_t tail_len, uint8_t* __restrict__ valid, Fr* __restrict__ sc) {
    bool ok = !hdr_bad[i];
    for (int k = 0; k < PV_NPTS; k++) ok = ok && !bad[k * n + i];
    valid[i] = ok;
    if (!ok) return;
    uint32_t prev[8];
#pragma unroll 1
    for (int c = 0; c < 4; c++) {
        Sha256Dev h;
        if (c == 0) h.resume(mid, mid_len);
        else h.reset();
        const uint32_t off = c == 0 ? 0 : c == 1 ? tail_len : c == 2 ? tail_len + 4 : tail_len + 9, len = c == 0 ? tail_len : c == 2 ? 5 : 4;
        h.update(pre + off, len);
        if (c) h.put256(prev);
        // bindings: gamma: public inputs, L, R, O; beta: none; alpha: Z; zeta: H0, H1, H2 -- 32-byte items
        const size_t items = c == 0 ? np + 6 : c == 1 ? 0 : c == 2 ? 2 : 6;
#pragma unroll 1
        for (size_t j = 0; j < items; j++) {
            uint32_t l[8];
            if (c == 0 && j < np) {
                const Fr w = pub[i * ps + j].from_mont();
#pragma unroll
                for (int k = 0; k < 8; k++) l[k] = w.l[k];
            } else {
                const size_t q = c == 0 ? j - np : j;
                const int pt = (c == 0 ? PV_L : c == 2 ? PV_Z : PV_H0) + (int)(q >> 1);
                raw_half(pts[pt * n + i], (int)(q & 1), l);
            }
            h.put256(l);
        }
        uint32_t d[8];
        h.final(d);
        sha_words_to_limbs(d, prev);  // the next challenge binds the raw digest
        sc[(PV_GAMMA + c) * n + i] = fr_from_digest(d);
    }
}
__global__ __launch_bounds__(64) void k_pvk_transcript(const Affine<Fp>* __restrict__ pts, const uint8_t* __restrict__ bad, const uint8_t* __restrict__ hdr_bad,
                                                       const Fr* __restrict__ pub, size_t ps, size_t n, const PvKeyRow* __restrict__ tab,
                                                       const uint32_t* __restrict__ key_of, uint64_t mid_len, uint32_t tail_len, uint8_t* __restrict__ valid,
                                                       Fr* __restrict__ sc) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const PvKeyRow* R = tab + key_of[i];
    pvk_transcript_lane(i, pts, bad, hdr_bad, pub, ps, n, (size_t)R->np, R->mid, mid_len, R->pre, tail_len, valid, sc);
}

// zeta^n, PI(zeta), L1(zeta) and the quotient identity (a lane that fails it is invalid from here on); the digests' scalars.
// PI(zeta) = sum_j w^j / n (zeta^n - 1) w_j / (zeta - w^j) accumulates as one fraction N / D: one inversion for all denominators
ZK_D void pv_scalars_lane(size_t i, const Fr* __restrict__ pub, size_t ps, size_t n, size_t np, const PvKey& K, uint8_t* __restrict__ valid, Fr* __restrict__ sc) {
    const Fr one = Fr::one();
    const Fr gamma = sc[PV_GAMMA * n + i], beta = sc[PV_BETA * n + i], alpha = sc[PV_ALPHA * n + i], zeta = sc[PV_ZETA * n + i];
    Fr zn = zeta;
    for (uint32_t k = 0; k < K.log_n; k++) zn = zn.sqr();
    const Fr zz = zn - one, szz = K.size_inv * zz;
    Fr num = Fr::zero(), den = one, wi = one;
    for (size_t j = 0; j < np; j++) {
        const Fr d = zeta - wi;
        num = num * d + wi * szz * pub[i * ps + j] * den;
        den = den * d;
        wi = wi * K.gen;
    }
    Fr pi = num * den.inv();
    if (den.is_zero()) {  // zeta = w^j for some j: term by term, with inv(0) = 0 as the host
        pi = Fr::zero();
        wi = one;
        for (size_t j = 0; j < np; j++) {
            pi = pi + wi * szz * (zeta - wi).inv() * pub[i * ps + j];
            wi = wi * K.gen;
        }
    }
    const Fr l1 = szz * (zeta - one).inv();
    const Fr quot = sc[(PV_CLAIM + 0) * n + i], lin_z = sc[(PV_CLAIM + 1) * n + i], lz = sc[(PV_CLAIM + 2) * n + i], rz = sc[(PV_CLAIM + 3) * n + i],
             oz = sc[(PV_CLAIM + 4) * n + i], s1z = sc[(PV_CLAIM + 5) * n + i], s2z = sc[(PV_CLAIM + 6) * n + i], zu = sc[PV_ZU * n + i];
    const Fr f1 = lz + beta * s1z + gamma, f2 = rz + beta * s2z + gamma;
    const Fr aa = alpha * alpha;
    if (lin_z + pi + f1 * f2 * (oz + gamma) * alpha * zu - aa * l1 != quot * zz) {
        valid[i] = 0;
        return;
    }
    const Fr zp = zn * zeta.sqr(), bz = beta * zeta;
    sc[PV_ZP * n + i] = zp;
    sc[PV_ZP2 * n + i] = zp.sqr();
    sc[PV_LR * n + i] = lz * rz;
    sc[PV_CS3 * n + i] = f1 * f2 * zu * beta * alpha;
    sc[PV_CZ * n + i] = (lz + bz + gamma).neg() * (rz + bz * K.u + gamma) * (oz + bz * K.u.sqr() + gamma) * alpha + aa * l1;
}
__global__ __launch_bounds__(64) void k_pv_scalars(const Fr* __restrict__ pub, size_t ps, size_t n, size_t np, PvKey K, uint8_t* __restrict__ valid, Fr* __restrict__ sc) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !valid[i]) return;
    pv_scalars_lane(i, pub, ps, n, np, K, valid, sc);
}
// (the lanes of a wave may run different log_n squaring counts and n_public loop lengths: at most 28 squarings and the largest n_public)
__global__ __launch_bounds__(64) void k_pvk_scalars(const Fr* __restrict__ pub, size_t ps, size_t n, const PvKeyRow* __restrict__ tab,
                                                    const uint32_t* __restrict__ key_of, uint8_t* __restrict__ valid, Fr* __restrict__ sc) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !valid[i]) return;
    const PvKeyRow* R = tab + key_of[i];
    pv_scalars_lane(i, pub, ps, n, (size_t)R->np, R->K, valid, sc);
}

// out[t n + i] = k P for term t = blockIdx.y of the table (infinity for an invalid lane)
__global__ __launch_bounds__(64) void k_pv_smul(const PvTerm* __restrict__ terms, size_t n, const uint8_t* __restrict__ valid, XYZZ<Fp>* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const PvTerm T = terms[blockIdx.y];
    XYZZ<Fp> r = XYZZ<Fp>::inf();
    if (valid[i]) {
        const Fr k = T.sc[i].from_mont();
        r = scalar_mul(T.pts[T.step * i], k.l);
    }
    out[blockIdx.y * n + i] = r;
}
// the same over PvkTerm: a fixed-point term is the lane's key's point
__global__ __launch_bounds__(64) void k_pvk_smul(const PvkTerm* __restrict__ terms, const PvKeyRow* __restrict__ tab, const uint32_t* __restrict__ key_of, size_t n,
                                                 const uint8_t* __restrict__ valid, XYZZ<Fp>* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const PvkTerm T = terms[blockIdx.y];
    XYZZ<Fp> r = XYZZ<Fp>::inf();
    if (valid[i]) {
        const Fr k = T.sc[i].from_mont();
        const Affine<Fp>* p = T.kpt >= 0 ? tab[key_of[i]].pts + T.kpt : T.pts + i;  // (both in HBM)
        r = scalar_mul(*p, k.l);
    }
    out[blockIdx.y * n + i] = r;
}

// the folded quotient digest H0 + zeta^(n+2) H1 + zeta^(2(n+2)) H2 and the linearised digest (terms 2..7 + Qk), affine
ZK_D void pv_digests_lane(size_t i, const Affine<Fp>* __restrict__ pts, const XYZZ<Fp>* __restrict__ t, const Affine<Fp>* __restrict__ kpts, size_t n,
                          Affine<Fp>* __restrict__ dig) {
    XYZZ<Fp> fh = t[i];
    fh.add(t[n + i]);
    fh.madd(pts[PV_H0 * n + i]);
    XYZZ<Fp> lin = t[2 * n + i];
    for (int k = 3; k < 8; k++) lin.add(t[k * n + i]);
    lin.madd(kpts[7]);
    dig[i] = fh.to_affine();
    dig[n + i] = lin.to_affine();
}
__global__ __launch_bounds__(64) void k_pv_digests(const Affine<Fp>* __restrict__ pts, const XYZZ<Fp>* __restrict__ t, const Affine<Fp>* __restrict__ kpts, size_t n,
                                                   const uint8_t* __restrict__ valid, Affine<Fp>* __restrict__ dig) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !valid[i]) return;
    pv_digests_lane(i, pts, t, kpts, n, dig);
}
__global__ __launch_bounds__(64) void k_pvk_digests(const Affine<Fp>* __restrict__ pts, const XYZZ<Fp>* __restrict__ t, const PvKeyRow* __restrict__ tab,
                                                    const uint32_t* __restrict__ key_of, size_t n, const uint8_t* __restrict__ valid, Affine<Fp>* __restrict__ dig) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !valid[i]) return;
    pv_digests_lane(i, pts, t, tab[key_of[i]].pts, n, dig);
}

// kzg.deriveGamma over zeta, the seven digests and the claimed values, then the lane's coefficients rho, rho' (SHA-256 of the host's prefix -- mid after 64
// bytes, then rtail's rtail_len -- || u64 index || tag byte) and the scalars of  rho (D - e G + zeta W) + rho' (Z - zu G + zeta omega W')  and  rho W + rho' W':
// per-lane terms into PV_T.., the fixed points' coefficients (G, S1, S2) into fix (columns) and fold (rows, k_fr_fold's input)
// FC: how many of the three are folded (the many-key form folds G's alone: S1 and S2 differ per lane and become two more rows of k_pvk_smul)
template <int FC>
ZK_D void pv_kzg_lane(size_t i, const Affine<Fp>* __restrict__ pts, const Affine<Fp>* __restrict__ dig, const Affine<Fp>* __restrict__ kpts, size_t n, size_t c0,
                      const PvKey& K, const uint32_t* __restrict__ rmid, const uint8_t* __restrict__ rtail, uint32_t rtail_len,
                      const uint8_t* __restrict__ valid, Fr* __restrict__ sc, Fr* __restrict__ fix, Fr* __restrict__ fold) {
    if (!valid[i]) {
        for (int j = 0; j < 3; j++) {
            if (j < FC) fix[j * n + i] = fold[FC * i + j] = Fr::zero();
            else fix[j * n + i] = Fr::zero();
        }
        return;
    }
    const Fr zeta = sc[PV_ZETA * n + i];
    Fr kg;
    {
        Sha256Dev h;
        h.reset();
        const uint64_t name = 0x67616d6d61ull;  // "gamma"
#pragma unroll 1
        for (int k = 4; k >= 0; k--) h.put_byte((uint32_t)(name >> (8 * k)));
#pragma unroll 1
        for (int j = 0; j < 22; j++) {  // zeta, fh lin L R O S1 S2 (X, Y each), the seven claimed values
            uint32_t l[8];
            if (j == 0 || j >= 15) {
                Fr v = zeta;  // (not a ?: of references: that would put zeta in memory)
                if (j) v = sc[(PV_CLAIM + j - 15) * n + i];
                v = v.from_mont();
#pragma unroll
                for (int k = 0; k < 8; k++) l[k] = v.l[k];
            } else {
                const int d = (j - 1) >> 1;
                Affine<Fp> p;
                if (d < 2) p = dig[d * n + i];
                else if (d < 5) p = pts[(PV_L + d - 2) * n + i];
                else p = kpts[d - 5];
                raw_half(p, (j - 1) & 1, l);
            }
            h.put256(l);
        }
        uint32_t dg[8];
        h.final(dg);
        kg = fr_from_digest(dg);
    }
    Fr rho = Fr::zero(), rho2 = Fr::zero();
    const uint64_t idx = c0 + i;
#pragma unroll 1
    for (int tag = 0; tag < 2; tag++) {
        Sha256Dev h;
        h.resume(rmid, 64);
#pragma unroll 1
        for (uint32_t k = 0; k < rtail_len + 8 + 1; k++)
            h.put_byte(k < rtail_len ? rtail[k] : k < rtail_len + 8 ? (uint32_t)(idx >> (8 * (k - rtail_len))) : (uint32_t)tag);
        uint32_t dg[8];
        h.final(dg);
        uint32_t l[8];
        sha_words_to_limbs(dg, l);
        Fr r = Fr::zero();
        batch_coeff(l, r.l);
        r = r.to_mont();
        if (tag == 0) rho = r;
        else rho2 = r;
    }
    Fr p[7], e = Fr::zero();  // p[k] = rho kg^k; e = sum claimed_k kg^k
    Fr acc = Fr::one();
#pragma unroll
    for (int k = 0; k < 7; k++) {
        e = e + sc[(PV_CLAIM + k) * n + i] * acc;
        p[k] = rho * acc;
        acc = acc * kg;
    }
    Fr* T = sc + PV_T * n + i;
    T[0] = p[0];                 // fh
    T[n] = p[1];                 // lin
    T[2 * n] = p[2];             // L
    T[3 * n] = p[3];             // R
    T[4 * n] = p[4];             // O
    T[5 * n] = rho * zeta;       // W
    T[6 * n] = rho2;             // Z
    T[7 * n] = rho2 * zeta * K.gen;  // W'
    T[8 * n] = rho;              // W  (second pairing)
    T[9 * n] = rho2;             // W' (second pairing)
    const Fr f[3] = {(rho * e + rho2 * sc[PV_ZU * n + i]).neg(), p[5], p[6]};
#pragma unroll
    for (int j = 0; j < 3; j++) {
        if (j < FC) fix[j * n + i] = fold[FC * i + j] = f[j];
        else fix[j * n + i] = f[j];
    }
}
__global__ __launch_bounds__(64) void k_pv_kzg(const Affine<Fp>* __restrict__ pts, const Affine<Fp>* __restrict__ dig, const Affine<Fp>* __restrict__ kpts, size_t n,
                                               size_t c0, PvKey K, const uint32_t* __restrict__ rmid, const uint8_t* __restrict__ rtail, uint32_t rtail_len,
                                               const uint8_t* __restrict__ valid, Fr* __restrict__ sc, Fr* __restrict__ fix, Fr* __restrict__ fold) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    pv_kzg_lane<3>(i, pts, dig, kpts, n, c0, K, rmid, rtail, rtail_len, valid, sc, fix, fold);
}
// key_of: the chunk's (the call's array + c0); c0 itself only numbers the lanes for rho, rho'
__global__ __launch_bounds__(64) void k_pvk_kzg(const Affine<Fp>* __restrict__ pts, const Affine<Fp>* __restrict__ dig, const PvKeyRow* __restrict__ tab,
                                                const uint32_t* __restrict__ key_of, size_t n, size_t c0, const uint32_t* __restrict__ rmid,
                                                const uint8_t* __restrict__ rtail, uint32_t rtail_len, const uint8_t* __restrict__ valid, Fr* __restrict__ sc,
                                                Fr* __restrict__ fix, Fr* __restrict__ fold) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const PvKeyRow* R = tab + key_of[i];
    pv_kzg_lane<1>(i, pts, dig, R->pts, n, c0, R->K, rmid, rtail, rtail_len, valid, sc, fix, fold);
}

// A_i = sum of terms 0..7, B_i = terms 8 + 9; a copy of each for the folds (which overwrite their input)
__global__ __launch_bounds__(256) void k_pv_combine(const XYZZ<Fp>* __restrict__ t, size_t n, XYZZ<Fp>* __restrict__ A, XYZZ<Fp>* __restrict__ B,
                                                    XYZZ<Fp>* __restrict__ fa, XYZZ<Fp>* __restrict__ fb) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    XYZZ<Fp> a = t[i];
    for (int k = 1; k < 8; k++) a.add(t[k * n + i]);
    XYZZ<Fp> b = t[8 * n + i];
    b.add(t[9 * n + i]);
    A[i] = fa[i] = a;
    B[i] = fb[i] = b;
}
// the many-key form: terms 10 and 11 are the lane's c_S1 S1 and c_S2 S2, part of A_i
__global__ __launch_bounds__(256) void k_pvk_combine(const XYZZ<Fp>* __restrict__ t, size_t n, XYZZ<Fp>* __restrict__ A, XYZZ<Fp>* __restrict__ B,
                                                     XYZZ<Fp>* __restrict__ fa, XYZZ<Fp>* __restrict__ fb) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    XYZZ<Fp> a = t[i];
    for (int k = 1; k < 8; k++) a.add(t[k * n + i]);
    for (int k = 10; k < 12; k++) a.add(t[k * n + i]);
    XYZZ<Fp> b = t[8 * n + i];
    b.add(t[9 * n + i]);
    A[i] = fa[i] = a;
    B[i] = fb[i] = b;
}

// fallback, per lane: P[i] = A_i + c_G G + c_S1 S1 + c_S2 S2 (t: those three terms), P[n + i] = -B_i (infinity for an invalid lane)
__global__ __launch_bounds__(256) void k_pv_single(const XYZZ<Fp>* __restrict__ A, const XYZZ<Fp>* __restrict__ B, const XYZZ<Fp>* __restrict__ t, size_t n,
                                                   const uint8_t* __restrict__ valid, Affine<Fp>* __restrict__ P) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (!valid[i]) {
        P[i] = P[n + i] = Affine<Fp>::inf();
        return;
    }
    XYZZ<Fp> a = A[i];
    for (int k = 0; k < 3; k++) a.add(t[k * n + i]);
    P[i] = a.to_affine();
    P[n + i] = B[i].to_affine().neg();
}
// the many-key fallback: A_i holds the lane's S1 and S2 terms already, t is c_G G alone.  Its launch name, pvk_single, is what says "the per-lane fallback ran"
__global__ __launch_bounds__(256) void k_pvk_single(const XYZZ<Fp>* __restrict__ A, const XYZZ<Fp>* __restrict__ B, const XYZZ<Fp>* __restrict__ t, size_t n,
                                                    const uint8_t* __restrict__ valid, Affine<Fp>* __restrict__ P) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (!valid[i]) {
        P[i] = P[n + i] = Affine<Fp>::inf();
        return;
    }
    XYZZ<Fp> a = A[i];
    a.add(t[i]);
    P[i] = a.to_affine();
    P[n + i] = B[i].to_affine().neg();
}
// d_v = SHA-256(row v's a_len bytes || its 32 n_public(key_of[v]) public-input bytes): k_rows_digest with the second span's length the row's own
__global__ __launch_bounds__(64) void k_rows_digest_keys(const uint8_t* __restrict__ a, size_t a_len, size_t a_stride, const uint8_t* __restrict__ b, size_t b_stride,
                                                         const PvKeyRow* __restrict__ tab, const uint32_t* __restrict__ key_of, size_t rows,
                                                         uint8_t* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows) return;
    rows_digest_lane(i, a, a_len, a_stride, b, (size_t)tab[key_of[i]].np * 32, b_stride, out);
}

// batch KZG opening check, per lane: T = C - v G + z H;  fa = lambda T and fb = lambda H for the folds;
// the lane's own pair for the fallback: P[i] = T, P[n + i] = -H (affine)
struct KzgLane {
    zk_g1_affine h;
    zk_fr v;
};
__global__ __launch_bounds__(64) void k_kzg_combine(const Affine<Fp>* __restrict__ dig, const KzgLane* __restrict__ op, const Fr* __restrict__ z,
                                                    const uint32_t* __restrict__ rr, size_t n, Affine<Fp> G,
                                                    XYZZ<Fp>* __restrict__ fa, XYZZ<Fp>* __restrict__ fb, Affine<Fp>* __restrict__ P) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Affine<Fp> h = reinterpret_cast<const Affine<Fp>*>(&op[i].h)[0];
    const Fr v = reinterpret_cast<const Fr*>(&op[i].v)[0].from_mont(), zi = z[i].from_mont();
    XYZZ<Fp> t = XYZZ<Fp>::from_affine(dig[i]);
    t.add(scalar_mul(G, v.l).neg());
    t.add(scalar_mul(h, zi.l));
    const Affine<Fp> ta = t.to_affine();
    P[i] = ta;
    P[n + i] = h.neg();
    const uint32_t k[8] = {rr[4 * i], rr[4 * i + 1], rr[4 * i + 2], rr[4 * i + 3], 0, 0, 0, 0};
    fa[i] = scalar_mul(ta, k);
    fb[i] = scalar_mul(h, k);
}

// the two buffers of a fold: a holds the n x cols elements to fold (overwritten), b at least ceil(n / 2) x cols
template <class T>
struct FoldPair {
    T *a = nullptr, *b = nullptr;
    void layout(ArenaPlan& p, size_t n, size_t cols = 1) { p.take(n * cols, a); p.take((n + 1) / 2 * cols, b); }
};
// halving launches until one element is left; returns where the result is
template <class T, class Kern>
T* fold_all(Slot* s, hipStream_t st, const char* name, Kern kernel, unsigned block, FoldPair<T> f, size_t n, size_t cols) {
    while (n > 1) {
        const size_t m = (n + 1) / 2;
        ZK_LAUNCH(s, st, name, kernel, dim3(blocks(m * cols, block)), dim3(block), 0, (const T*)f.a, n, cols, f.b);
        std::swap(f.a, f.b);
        n = m;
    }
    return f.a;
}

constexpr size_t CHUNK = (size_t)1 << 16;

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

// SHA-256 of a || b || c
void sha(uint8_t out[32], const void* a, size_t na, const void* b = nullptr, size_t nb = 0, const void* c = nullptr, size_t nc = 0) {
    Sha256 h;
    h.update(a, na);
    h.update(b, nb);
    h.update(c, nc);
    h.final(out);
}

// out[4 i ..] = the coefficient of lane c0 + i (batch_coeff) for i < n: pre with the lane's index, u64 little-endian, written at idx_offset, hashed
void batch_coeffs(uint8_t* pre, size_t pre_len, size_t idx_offset, size_t c0, size_t n, uint32_t* out) {
    for (size_t i = 0; i < n; i++) {
        const uint64_t idx = c0 + i;
        for (int b = 0; b < 8; b++) pre[idx_offset + b] = (uint8_t)(idx >> (8 * b));
        uint8_t d[32];
        sha(d, pre, pre_len);
        uint32_t l[8];
        for (int w = 0; w < 8; w++) l[w] = ((uint32_t)d[28 - 4 * w] << 24) | ((uint32_t)d[29 - 4 * w] << 16) | ((uint32_t)d[30 - 4 * w] << 8) | d[31 - 4 * w];
        batch_coeff(l, out + 4 * i);
    }
}

// The pairing check of a chunk, shared by the three batch verifiers: its buffers and its steps.  An entry fills d_valid and the points, then
//   sync_valid   waits for what the entry has queued and for the lanes' valid flags; a chunk without a valid lane is rejected whole
//   combined     the Miller loops of the folded points, the product tree, one final exponentiation; a product of one accepts every valid lane
//   per_lane     (only when that fails) rows Miller loops, a final exponentiation and a verdict per lane
// decided: the last step settled the chunk's verdicts (the entry goes on to the next chunk); total: the lanes accepted so far
struct PairCheck {
    Slot* s;
    hipStream_t st;
    PairConsts K;
    size_t ch;                                   // lanes per chunk, at most
    F12 *d_m, *d_ws, *d_one_ws;                  // Miller values; FE_SLOTS per lane (and the product tree's second buffer); the combined check's FE_SLOTS
    uint8_t *d_valid, *d_verdict, *d_chk;        // per lane; the combined check's own "valid" (d_chk[0]) and verdict (d_chk[1])
    std::vector<uint8_t> valid;                  // d_valid on the host
    uint8_t one = 0;
    bool decided = false;
    size_t total = 0;

    PairCheck(Slot* s_, const PairConsts& K_, size_t ch_) : s(s_), st(s_->stream), K(K_), ch(ch_), valid(ch_) {}
    // m_lanes: the most Miller loops of one launch
    void layout(ArenaPlan& p, size_t m_lanes) {
        p.take(m_lanes, d_m);
        p.take(std::max(FE_SLOTS * ch, (m_lanes + 1) / 2), d_ws);
        p.take(FE_SLOTS, d_one_ws);
        p.take(ch, d_valid, d_verdict);
        p.take(64, d_chk);
    }
    void miller(const Affine<Fp>* P, size_t lanes, const Affine<Fp2>* qvar, size_t n_var, const Affine<Fp2>* qfix, size_t rep) {
        ZK_LAUNCH(s, st, "miller_loop", k_miller, dim3(blocks(lanes, PAIR_BLOCK)), dim3(PAIR_BLOCK), 0, P, lanes, qvar, n_var, qfix, rep, K, d_m);
    }
    void tally(const uint8_t* accepted, size_t n) { for (size_t i = 0; i < n; i++) total += accepted[i] ? 1 : 0; }
    int sync_valid(size_t n, uint8_t* accepted) {
        ZK_HIP(hipMemcpyAsync(valid.data(), d_valid, n, hipMemcpyDeviceToHost, st));
        ZK_TRY(slot_sync(s, st));
        decided = std::none_of(valid.begin(), valid.begin() + n, [](uint8_t v) { return v != 0; });
        if (decided) memset(accepted, 0, n);
        return ZK_OK;
    }
    // prod_{i < n_lanes} e(P_i, Q_i) == 1, Q_i = qvar[i] for i < n_var, qfix[i - n_var] after; if so, accepted = valid for the chunk's n lanes
    int combined(const Affine<Fp>* P, size_t n_lanes, const Affine<Fp2>* qvar, size_t n_var, const Affine<Fp2>* qfix, size_t n, uint8_t* accepted) {
        miller(P, n_lanes, qvar, n_var, qfix, 1);
        const F12* prod = fold_all(s, st, "f12_fold", k_f12_fold, PAIR_BLOCK, FoldPair<F12>{d_m, d_ws}, n_lanes, 1);
        ZK_HIP(hipMemsetAsync(d_chk, 1, 1, st));
        ZK_TRY(final_exp(s, st, K, prod, 1, 1, nullptr, d_one_ws, nullptr, d_chk, d_chk + 1));
        ZK_HIP(hipMemcpyAsync(&one, d_chk + 1, 1, hipMemcpyDeviceToHost, st));
        ZK_TRY(slot_sync(s, st));
        decided = one != 0;
        if (decided) {
            memcpy(accepted, valid.data(), n);
            tally(accepted, n);
        }
        return ZK_OK;
    }
    // accepted[i] = valid[i] && prod_{r < rows} e(P[r n + i], Q_r) == 1 -- times e(P[rows n], qfix's last) when shared_lane -- with Q_r = qvar[i] while
    // r n + i < n_var, qfix[r - n_var / n] after
    int per_lane(const Affine<Fp>* P, size_t n, int rows, const Affine<Fp2>* qvar, size_t n_var, const Affine<Fp2>* qfix, bool shared_lane, uint8_t* accepted) {
        miller(P, rows * n + (shared_lane ? 1 : 0), qvar, n_var, qfix, n);
        ZK_TRY(final_exp(s, st, K, d_m, n, rows, shared_lane ? d_m + rows * n : nullptr, d_ws, nullptr, d_valid, d_verdict));
        ZK_HIP(hipMemcpyAsync(accepted, d_verdict, n, hipMemcpyDeviceToHost, st));
        ZK_TRY(slot_sync(s, st));
        tally(accepted, n);
        return ZK_OK;
    }
};

// Where the rows of a Groth16 / PLONK batch are.  on_device: read where they lie, row i's proof at proofs + i * proof_stride bytes and its public inputs at
// pub + i * pub_stride elements.  Otherwise host memory, packed (the strides are the rows): each chunk goes up into the call's workspace first.
struct RowsIn {
    const uint8_t* proofs;
    size_t proof_stride;
    const Fr* pub;
    size_t pub_stride;
    bool on_device;
};
// a chunk's rows in HBM: d_stage / d_pub are the workspace's (proof_bytes and np elements per row)
int rows_of_chunk(const RowsIn& in, hipStream_t st, size_t c0, size_t n, size_t proof_bytes, size_t np, uint8_t* d_stage, Fr* d_pub, RowsIn* at) {
    if (in.on_device) {
        *at = RowsIn{in.proofs + c0 * in.proof_stride, in.proof_stride, np ? in.pub + c0 * in.pub_stride : nullptr, in.pub_stride, true};
        return ZK_OK;
    }
    ZK_HIP(hipMemcpyAsync(d_stage, in.proofs + c0 * proof_bytes, n * proof_bytes, hipMemcpyHostToDevice, st));
    if (np) ZK_HIP(hipMemcpyAsync(d_pub, in.pub + c0 * np, n * np * 32, hipMemcpyHostToDevice, st));
    *at = RowsIn{d_stage, proof_bytes, d_pub, np, true};
    return ZK_OK;
}
int rows_in_args(const void* d_proofs, size_t proof_stride, size_t proof_bytes, size_t n_proofs, const void* d_pub, size_t pub_stride, size_t n_public) {
    if (n_proofs > 1 && proof_stride < proof_bytes) return set_err(ZK_ERR_ARG, "proof_stride = %zu is below the %zu bytes of a proof", proof_stride, proof_bytes);
    if (n_proofs > 1 && pub_stride < n_public) return set_err(ZK_ERR_ARG, "pub_stride = %zu is below the %zu public inputs of a row", pub_stride, n_public);
    return ZK_OK;
}

// d_out[32 v ..] = SHA-256(a_v || b_v) for `rows` rows, enqueued on st
void rows_digest_launch(Slot* s, hipStream_t st, const void* d_a, size_t a_len, size_t a_stride, const void* d_b, size_t b_len, size_t b_stride, size_t rows,
                        void* d_out) {
    ZK_LAUNCH(s, st, "rows_digest", k_rows_digest, dim3(blocks(rows, 64)), dim3(64), 0, (const uint8_t*)d_a, a_len, a_stride, (const uint8_t*)d_b, b_len, b_stride, rows,
              (uint8_t*)d_out);
}
// D = SHA-256(d_0 || .. || d_{n-1}), d_v = SHA-256(row v's proof bytes || its public inputs as they lie in memory): what stands for the host entries'
// SHA-256(proofs || public inputs) in the device forms (zkmi.h).  A slot of its own, given back before the verifier takes one; 32 bytes per row come down.
int rows_digest_of_call(const RowsIn& in, size_t proof_bytes, size_t n, size_t np, uint8_t D[32]) {
    SlotGuard g;
    ZK_TRY(acquire_slot(&g.s));
    Slot* s = g.s;
    hipStream_t st = s->stream;
    uint8_t* d_dig;
    ZK_TRY(plan_workspace(s, "rows_digest", [&](ArenaPlan& p) { p.take(n * 32, d_dig); }));
    rows_digest_launch(s, st, in.proofs, proof_bytes, in.proof_stride, in.pub, np * 32, in.pub_stride * 32, n, d_dig);
    std::vector<uint8_t> dig(n * 32);
    ZK_HIP(hipMemcpyAsync(dig.data(), d_dig, n * 32, hipMemcpyDeviceToHost, st));
    ZK_TRY(slot_sync(s, st));
    sha(D, dig.data(), dig.size());
    return ZK_OK;
}

// groth16.Verify for the rows `in` against the parsed key.  pre: the coefficients' prefix, tag || SHA-256(vk) || the call's data digest || 8 bytes for the index:
// r_i = batch_coeff(SHA-256(pre with i)) -- the entry's to derive (zkmi.h states both derivations), so that one core serves the host and the device form
int groth16_verify_rows(const Groth16Vk& v, const RowsIn& in, size_t n_proofs, size_t np, std::vector<uint8_t>& pre, uint8_t* accepted, size_t* n_accepted) {
    const PairConsts K = pair_consts();
    const size_t nk = v.K.size(), cols = np + 1;
    SlotGuard g;
    ZK_TRY(acquire_slot(&g.s));
    Slot* s = g.s;
    hipStream_t st = s->stream;
    const size_t ch = std::min(n_proofs, CHUNK);
    PairCheck pc(s, K, ch);
    uint8_t *d_stage, *d_bad;
    uint32_t* d_raw;  // Ar | Bs | Krs, each contiguous
    Affine<Fp> *d_ar, *d_krs, *d_p, *d_kpts;
    Affine<Fp2> *d_bs, *d_fix;
    uint32_t* d_rr;
    Fr* d_pub;
    FoldPair<XYZZ<Fp>> rk_fold;
    FoldPair<Fr> terms;
    int* d_status;
    ZK_TRY(plan_workspace(s, "groth16_verify_batch", [&](ArenaPlan& p) {
        p.take(in.on_device ? 1 : ch * 128, d_stage);
        p.take(ch * 32, d_raw);
        p.take(ch, d_ar, d_krs, d_bs);
        p.take(ch * 3, d_bad);
        p.take(ch * 4, d_rr);
        p.take(in.on_device ? 1 : std::max(ch * np, (size_t)1), d_pub);
        rk_fold.layout(p, ch);
        terms.layout(p, ch, cols);
        p.take(3 * ch + 3, d_p);
        pc.layout(p, 3 * ch + 3);
        p.take(nk, d_kpts);
        p.take(3, d_fix);
        p.take(16, d_status);
        p.later(ch * G2_DECOMPRESS_SCRATCH);  // g2_decompress_dev's, per chunk
    }));
    ZK_HIP(hipMemcpyAsync(d_kpts, v.K.data(), nk * 64, hipMemcpyHostToDevice, st));
    const size_t arena_mark = s->arena_off;  // g2_decompress_dev takes its scratch from the arena per call: give it back per chunk

    std::vector<uint32_t> rr(ch * 4);
    for (size_t c0 = 0; c0 < n_proofs; c0 += ch) {
        const size_t n = std::min(ch, n_proofs - c0);
        s->arena_off = arena_mark;
        RowsIn at;
        ZK_TRY(rows_of_chunk(in, st, c0, n, 128, np, d_stage, d_pub, &at));
        batch_coeffs(pre.data(), pre.size(), pre.size() - 8, c0, n, rr.data());
        ZK_HIP(hipMemcpyAsync(d_rr, rr.data(), n * 16, hipMemcpyHostToDevice, st));
        ZK_HIP(hipMemsetAsync(d_bad, 0, n * 3, st));
        ZK_HIP(hipMemsetAsync(d_status, 0, 4, st));
        ZK_LAUNCH(s, st, "vb_gather", k_vb_gather, dim3(blocks(n, 256)), dim3(256), 0, at.proofs, at.proof_stride, n, d_raw);
        const uint8_t* raw = (const uint8_t*)d_raw;
        ZK_TRY(g1_decompress_dev(s, st, raw, n, d_ar, d_status, d_bad));
        ZK_TRY(g2_decompress_dev(s, st, raw + n * 32, n, d_bs, d_status, d_bad + n));
        ZK_TRY(g1_decompress_dev(s, st, raw + n * 96, n, d_krs, d_status, d_bad + 2 * n));
        ZK_LAUNCH(s, st, "vb_prep", k_vb_prep, dim3(blocks(n, 128)), dim3(128), 0, (const Affine<Fp>*)d_ar, (const Affine<Fp>*)d_krs, (const uint8_t*)d_bad,
                  (const uint32_t*)d_rr, at.pub, at.pub_stride, n, np, pc.d_valid, d_p, rk_fold.a, terms.a);
        const XYZZ<Fp>* rk_sum = fold_all(s, st, "g1_fold", k_g1_fold, 256, rk_fold, n, 1);
        const Fr* c_sum = fold_all(s, st, "fr_fold", k_fr_fold, 256, terms, n, cols);
        XYZZ<HFp> rk;
        std::vector<HFr> c(cols);
        ZK_HIP(hipMemcpyAsync(&rk, rk_sum, 128, hipMemcpyDeviceToHost, st));
        ZK_HIP(hipMemcpyAsync(c.data(), c_sum, cols * 32, hipMemcpyDeviceToHost, st));
        ZK_TRY(pc.sync_valid(n, accepted + c0));
        if (pc.decided) continue;
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
        ZK_TRY(pc.combined(d_p, n + 3, d_bs, n, d_fix, n, accepted + c0));
        if (pc.decided) continue;
        // fallback: every valid proof on its own; the shared lane is e(alpha, beta)'s
        const Affine<HFp2> qfix_f[3] = {v.gamma, v.delta, v.beta};
        ZK_HIP(hipMemcpyAsync(d_fix, qfix_f, 3 * 128, hipMemcpyHostToDevice, st));
        ZK_HIP(hipMemcpyAsync(d_p + 3 * n, &v.alpha, 64, hipMemcpyHostToDevice, st));
        ZK_LAUNCH(s, st, "vb_single", k_vb_single, dim3(blocks(n, 128)), dim3(128), 0, (const Affine<Fp>*)d_ar, (const Affine<Fp>*)d_krs,
                  (const uint8_t*)pc.d_valid, at.pub, at.pub_stride, (const Affine<Fp>*)d_kpts, n, np, d_p);
        ZK_TRY(pc.per_lane(d_p, n, 3, d_bs, n, d_fix, true, accepted + c0));
    }
    *n_accepted = pc.total;
    return ZK_OK;
}

// The tile tables of one segmented sum: segment u has len[u] >= 1 items (consecutive, in segment order) and cols[u] Fr columns.  Level l folds the level
// below in tiles of at most GK_T items of one segment; after `levels` levels (GK_T^levels >= the longest segment possible) one item per segment is left, and
// the Fr rows of the last level lie at the prefix sums of cols.  lev[l] = (first tile, tiles) of level l; fr_elems: the largest Fr output of a level
struct GkLevels {
    std::vector<GkTile> tiles;
    std::vector<std::pair<size_t, size_t>> lev;
    size_t fr_elems = 0, items1 = 0;  // items1: the tiles of the first level
    bool build(const std::vector<uint32_t>& len, const std::vector<uint32_t>& cols, int levels) {
        std::vector<uint64_t> m(len.begin(), len.end());
        tiles.clear();
        lev.clear();
        for (int l = 0; l < levels; l++) {
            uint64_t item = 0, fin = 0, fout = 0;
            const size_t first = tiles.size();
            for (size_t u = 0; u < m.size(); u++) {
                const uint64_t out = (m[u] + GK_T - 1) / GK_T;
                for (uint64_t b = 0; b < out; b++)
                    tiles.push_back(GkTile{(uint32_t)(item + b * GK_T), (uint32_t)std::min<uint64_t>(GK_T, m[u] - b * GK_T), cols[u],
                                           (uint32_t)(fin + b * GK_T * cols[u]), (uint32_t)(fout + b * cols[u])});
                item += m[u];
                fin += m[u] * cols[u];
                fout += out * cols[u];
                m[u] = out;
            }
            if (fin >> 31) return false;
            lev.emplace_back(first, tiles.size() - first);
            fr_elems = std::max<size_t>(fr_elems, fout);
            if (l == 0) items1 = tiles.size();
        }
        return true;
    }
};
int gk_level_count(size_t longest) {
    int l = 1;
    for (size_t r = GK_T; r < longest; r *= GK_T) l++;
    return l;
}
// a chunk's lanes grouped by key (a stable counting sort: O(n + K) integer work, no field or curve arithmetic)
struct GkChunk {
    std::vector<uint32_t> perm;  // perm[p]: the lane at sorted position p
    std::vector<GkSeg> segs;     // the keys used, in key order
    GkLevels rows, fixed;        // the sums over a key's lanes; the sums over a key's np + 1 fixed terms
    size_t n_cols = 0;           // sum over the used keys of np + 1
};

// groth16_verify_rows with a key per row.  pre: tag || KD || 32 bytes of data digest || 8 for the index; the data digest is the entry's in the host form and
// made here in the device form (k_vbk_rows_digest needs the key table).  No host curve arithmetic: the 3 K_used fixed terms are made on the device
int groth16_verify_rows_keys(const std::vector<Groth16Vk>& vs, const RowsIn& in, size_t n_proofs, const uint32_t* key_of, std::vector<uint8_t>& pre,
                             uint8_t* accepted, size_t* n_accepted) {
    const PairConsts PK = pair_consts();
    const size_t nk = vs.size(), ps = in.pub_stride, ch = std::min(n_proofs, CHUNK);
    std::vector<GkKeyRow> tab(nk);
    std::vector<Affine<HFp>> kpts;
    size_t max_np = 0;
    for (size_t j = 0; j < nk; j++) {
        GkKeyRow& R = tab[j];
        memset(&R, 0, sizeof R);
        R.alpha = bit_cast_img<Affine<Fp>>(vs[j].alpha);
        R.beta = bit_cast_img<Affine<Fp2>>(vs[j].beta);
        R.gamma = bit_cast_img<Affine<Fp2>>(vs[j].gamma);
        R.delta = bit_cast_img<Affine<Fp2>>(vs[j].delta);
        R.np = (uint32_t)(vs[j].K.size() - 1);
        R.koff = (uint32_t)kpts.size();
        max_np = std::max(max_np, (size_t)R.np);
        kpts.insert(kpts.end(), vs[j].K.begin(), vs[j].K.end());
        if (kpts.size() >> 31) return set_err(ZK_ERR_LEN, "the keys hold %zu K points", kpts.size());
    }
    // every chunk's grouping first: the workspace is sized by the largest
    const int fixed_levels = gk_level_count(max_np + 1);
    std::vector<GkChunk> plan((n_proofs + ch - 1) / ch);
    size_t max_segs = 0, max_cols = 0, max_tiles = 0, max_fr = 1, max_rows1 = 1, max_fixed1 = 1;
    {
        std::vector<uint32_t> cnt(nk + 1), len, cols;
        for (size_t c = 0; c < plan.size(); c++) {
            const size_t c0 = c * ch, n = std::min(ch, n_proofs - c0);
            GkChunk& C = plan[c];
            std::fill(cnt.begin(), cnt.end(), 0);
            for (size_t i = 0; i < n; i++) cnt[key_of[c0 + i] + 1]++;
            len.clear();
            cols.clear();
            for (size_t k = 0; k < nk; k++) {
                if (cnt[k + 1]) {
                    C.segs.push_back(GkSeg{(uint32_t)k, (uint32_t)C.n_cols});
                    len.push_back(cnt[k + 1]);
                    cols.push_back(tab[k].np + 1);
                    C.n_cols += tab[k].np + 1;
                }
                cnt[k + 1] += cnt[k];
            }
            C.perm.resize(n);
            for (size_t i = 0; i < n; i++) C.perm[cnt[key_of[c0 + i]]++] = (uint32_t)i;
            if (!C.rows.build(len, cols, gk_level_count(n)) || !C.fixed.build(cols, std::vector<uint32_t>(cols.size(), 0), fixed_levels))
                return set_err(ZK_ERR_LEN, "the chunk at row %zu sums more than 2^31 public-input terms", c0);
            max_segs = std::max(max_segs, C.segs.size());
            max_cols = std::max(max_cols, C.n_cols);
            max_tiles = std::max(max_tiles, C.rows.tiles.size() + C.fixed.tiles.size());
            max_fr = std::max(max_fr, C.rows.fr_elems);
            max_rows1 = std::max(max_rows1, C.rows.items1);
            max_fixed1 = std::max(max_fixed1, C.fixed.items1);
        }
    }
    // a chunk's public inputs as they come up in the host form: whole rows of the caller's stride but for the last, which ends with its own n_public
    const size_t pub_elems = max_np ? (ch - 1) * ps + max_np : 0;

    SlotGuard g;
    ZK_TRY(acquire_slot(&g.s));
    Slot* s = g.s;
    hipStream_t st = s->stream;
    PairCheck pc(s, PK, ch);
    const size_t m_lanes = std::max(4 * ch, ch + 3 * max_segs);
    uint8_t *d_stage, *d_bad, *d_rowdig;
    uint32_t *d_raw, *d_rr, *d_key_of, *d_perm;
    Affine<Fp> *d_ar, *d_krs, *d_p, *d_kpts;
    Affine<Fp2> *d_q, *d_fix;  // d_q: Bs per lane, and the fallback's gamma, delta, beta per lane behind them
    Fr *d_pub, *d_rm, *d_c[2];
    XYZZ<Fp> *d_rk, *d_rkf[2], *d_fx, *d_fxf[2], *d_fa;
    GkKeyRow* d_tab;
    GkSeg* d_segs;
    GkTile* d_tiles;
    int* d_status;
    ZK_TRY(plan_workspace(s, "groth16_verify_batch_keys", [&](ArenaPlan& p) {
        p.take(in.on_device ? 1 : ch * 128, d_stage);
        p.take(ch * 32, d_raw);
        p.take(ch, d_ar, d_krs, d_rk, d_rm, d_perm);
        p.take(ch * 4, d_q);
        p.take(ch * 3, d_bad);
        p.take(ch * 4, d_rr);
        p.take(in.on_device ? 1 : std::max(pub_elems, (size_t)1), d_pub);
        p.take(max_rows1, d_rkf[0], d_rkf[1]);
        p.take(max_fr, d_c[0], d_c[1]);
        p.take(std::max(max_cols, (size_t)1), d_fx);
        p.take(max_fixed1, d_fxf[0], d_fxf[1]);
        p.take(std::max(max_segs, (size_t)1), d_fa, d_segs);
        p.take(std::max(max_tiles, (size_t)1), d_tiles);
        p.take(m_lanes, d_p);
        pc.layout(p, m_lanes);
        p.take(3 * std::max(max_segs, (size_t)1), d_fix);
        p.take(nk, d_tab);
        p.take(std::max(kpts.size(), (size_t)1), d_kpts);
        p.take(n_proofs, d_key_of);
        p.take(in.on_device ? n_proofs * 32 : 1, d_rowdig);
        p.take(16, d_status);
        p.later(ch * G2_DECOMPRESS_SCRATCH);  // g2_decompress_dev's, per chunk
    }));
    ZK_HIP(hipMemcpyAsync(d_tab, tab.data(), nk * sizeof(GkKeyRow), hipMemcpyHostToDevice, st));
    ZK_HIP(hipMemcpyAsync(d_kpts, kpts.data(), kpts.size() * 64, hipMemcpyHostToDevice, st));
    ZK_HIP(hipMemcpyAsync(d_key_of, key_of, n_proofs * 4, hipMemcpyHostToDevice, st));
    if (in.on_device) {
        // D = SHA-256(d_0 || .. || d_{n-1}) over the whole call, d_v = SHA-256(row v's proof || its own 32 n_public(key_of[v]) public-input bytes as they lie)
        ZK_LAUNCH(s, st, "vbk_rows_digest", k_vbk_rows_digest, dim3(blocks(n_proofs, 64)), dim3(64), 0, in.proofs, (size_t)128, in.proof_stride,
                  (const uint8_t*)in.pub, ps * 32, (const GkKeyRow*)d_tab, (const uint32_t*)d_key_of, n_proofs, d_rowdig);
        std::vector<uint8_t> dig(n_proofs * 32);
        ZK_HIP(hipMemcpyAsync(dig.data(), d_rowdig, dig.size(), hipMemcpyDeviceToHost, st));
        ZK_TRY(slot_sync(s, st));
        sha(pre.data() + pre.size() - 40, dig.data(), dig.size());
    }
    const size_t arena_mark = s->arena_off;  // g2_decompress_dev takes its scratch from the arena per call: give it back per chunk

    std::vector<uint32_t> rr(ch * 4);
    for (size_t c0 = 0; c0 < n_proofs; c0 += ch) {
        const size_t n = std::min(ch, n_proofs - c0);
        const GkChunk& C = plan[c0 / ch];
        const size_t U = C.segs.size();
        s->arena_off = arena_mark;
        RowsIn at;
        if (in.on_device) {
            at = RowsIn{in.proofs + c0 * in.proof_stride, in.proof_stride, max_np ? in.pub + c0 * ps : nullptr, ps, true};
        } else {
            ZK_HIP(hipMemcpyAsync(d_stage, in.proofs + c0 * 128, n * 128, hipMemcpyHostToDevice, st));
            const size_t last = vs[key_of[c0 + n - 1]].K.size() - 1;
            if (max_np && (n - 1) * ps + last) ZK_HIP(hipMemcpyAsync(d_pub, in.pub + c0 * ps, ((n - 1) * ps + last) * 32, hipMemcpyHostToDevice, st));
            at = RowsIn{d_stage, 128, d_pub, ps, true};
        }
        batch_coeffs(pre.data(), pre.size(), pre.size() - 8, c0, n, rr.data());
        ZK_HIP(hipMemcpyAsync(d_rr, rr.data(), n * 16, hipMemcpyHostToDevice, st));
        ZK_HIP(hipMemcpyAsync(d_perm, C.perm.data(), n * 4, hipMemcpyHostToDevice, st));
        ZK_HIP(hipMemcpyAsync(d_segs, C.segs.data(), U * sizeof(GkSeg), hipMemcpyHostToDevice, st));
        ZK_HIP(hipMemcpyAsync(d_tiles, C.rows.tiles.data(), C.rows.tiles.size() * sizeof(GkTile), hipMemcpyHostToDevice, st));
        const GkTile* d_ftiles = d_tiles + C.rows.tiles.size();
        ZK_HIP(hipMemcpyAsync((void*)d_ftiles, C.fixed.tiles.data(), C.fixed.tiles.size() * sizeof(GkTile), hipMemcpyHostToDevice, st));
        ZK_HIP(hipMemsetAsync(d_bad, 0, n * 3, st));
        ZK_HIP(hipMemsetAsync(d_status, 0, 4, st));
        ZK_LAUNCH(s, st, "vb_gather", k_vb_gather, dim3(blocks(n, 256)), dim3(256), 0, at.proofs, at.proof_stride, n, d_raw);
        const uint8_t* raw = (const uint8_t*)d_raw;
        ZK_TRY(g1_decompress_dev(s, st, raw, n, d_ar, d_status, d_bad));
        ZK_TRY(g2_decompress_dev(s, st, raw + n * 32, n, d_q, d_status, d_bad + n));
        ZK_TRY(g1_decompress_dev(s, st, raw + n * 96, n, d_krs, d_status, d_bad + 2 * n));
        ZK_LAUNCH(s, st, "vbk_prep", k_vbk_prep, dim3(blocks(n, 128)), dim3(128), 0, (const Affine<Fp>*)d_ar, (const Affine<Fp>*)d_krs, (const uint8_t*)d_bad,
                  (const uint32_t*)d_rr, (const uint32_t*)d_perm, n, pc.d_valid, d_p, d_rk, d_rm);
        // per key: sum r_i Krs_i and the c_{k,j}, level by level
        const XYZZ<Fp>* rk_in = d_rk;
        const Fr* c_in = nullptr;
        for (size_t l = 0; l < C.rows.lev.size(); l++) {
            const GkTile* t = d_tiles + C.rows.lev[l].first;
            const size_t nt = C.rows.lev[l].second;
            ZK_LAUNCH(s, st, "vbk_g1_fold", k_vbk_g1_fold, dim3(blocks(nt, 64)), dim3(64), 0, rk_in, t, nt, d_rkf[l & 1]);
            if (l == 0)
                ZK_LAUNCH(s, st, "vbk_coef", k_vbk_coef, dim3((unsigned)nt), dim3(64), 0, (const Fr*)d_rm, (const uint32_t*)d_perm, at.pub, at.pub_stride, t,
                          d_c[0]);
            else
                ZK_LAUNCH(s, st, "vbk_fr_fold", k_vbk_fr_fold, dim3((unsigned)nt), dim3(64), 0, c_in, t, d_c[l & 1]);
            rk_in = d_rkf[l & 1];
            c_in = d_c[l & 1];
        }
        // the fixed terms c_{k,j} K_{k,j} and c_{k,0} alpha_k, the sums IC_k of the former, and the 3 K_used lanes behind the chunk's n
        ZK_LAUNCH(s, st, "vbk_fixed", k_vbk_fixed, dim3((unsigned)U), dim3(64), 0, c_in, (const GkSeg*)d_segs, (const GkKeyRow*)d_tab, (const Affine<Fp>*)d_kpts,
                  d_fx, d_fa);
        const XYZZ<Fp>* ic_in = d_fx;
        for (size_t l = 0; l < C.fixed.lev.size(); l++) {
            const size_t nt = C.fixed.lev[l].second;
            ZK_LAUNCH(s, st, "vbk_g1_fold", k_vbk_g1_fold, dim3(blocks(nt, 64)), dim3(64), 0, ic_in, d_ftiles + C.fixed.lev[l].first, nt, d_fxf[l & 1]);
            ic_in = d_fxf[l & 1];
        }
        ZK_LAUNCH(s, st, "vbk_tail", k_vbk_tail, dim3(blocks(U, 64)), dim3(64), 0, (const XYZZ<Fp>*)d_fa, ic_in, rk_in, (const GkSeg*)d_segs,
                  (const GkKeyRow*)d_tab, U, d_p + n, d_fix);
        ZK_TRY(pc.sync_valid(n, accepted + c0));
        if (pc.decided) continue;
        ZK_TRY(pc.combined(d_p, n + 3 * U, d_q, n, d_fix, n, accepted + c0));
        if (pc.decided) continue;
        // fallback: every valid proof on its own, four pairings under its own key (no e(alpha, beta) lane is shared across keys)
        ZK_LAUNCH(s, st, "vbk_single", k_vbk_single, dim3(blocks(n, 128)), dim3(128), 0, (const Affine<Fp>*)d_ar, (const Affine<Fp>*)d_krs,
                  (const uint8_t*)pc.d_valid, at.pub, at.pub_stride, (const GkKeyRow*)d_tab, (const Affine<Fp>*)d_kpts, (const uint32_t*)(d_key_of + c0), n, d_p,
                  d_q);
        ZK_TRY(pc.per_lane(d_p, n, 4, d_q, 4 * n, nullptr, false, accepted + c0));
    }
    *n_accepted = pc.total;
    return ZK_OK;
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
    Affine<Fp>* d_p;
    Affine<Fp2>* d_q;
    FoldPair<F12> fm;  // the Miller values and their product tree
    F12* d_ws;
    ZK_TRY(plan_workspace(s, "pair", [&](ArenaPlan& p) {
        p.take(ch, d_p, d_q);
        fm.layout(p, ch);
        p.take(FE_SLOTS + 1, d_ws);
    }));
    F12 acc = F12::one();  // the chunks' Miller products, multiplied on the host (one product per 2^16 pairs)
    for (size_t c0 = 0; c0 < n; c0 += ch) {
        const size_t m = std::min(ch, n - c0);
        ZK_HIP(hipMemcpyAsync(d_p, p + c0, m * 64, hipMemcpyHostToDevice, st));
        ZK_HIP(hipMemcpyAsync(d_q, q + c0, m * 128, hipMemcpyHostToDevice, st));
        ZK_LAUNCH(s, st, "miller_loop", k_miller, dim3(blocks(m, PAIR_BLOCK)), dim3(PAIR_BLOCK), 0, (const Affine<Fp>*)d_p, m, (const Affine<Fp2>*)d_q, m,
                  (const Affine<Fp2>*)nullptr, (size_t)1, K, fm.a);
        const F12* r = fold_all(s, st, "f12_fold", k_f12_fold, PAIR_BLOCK, fm, m, 1);
        F12 part;
        ZK_HIP(hipMemcpyAsync(&part, r, 384, hipMemcpyDeviceToHost, st));
        ZK_TRY(slot_sync(s, st));
        acc = acc * part;
    }
    ZK_HIP(hipMemcpyAsync(d_ws + FE_SLOTS, &acc, 384, hipMemcpyHostToDevice, st));
    ZK_TRY(final_exp(s, st, K, d_ws + FE_SLOTS, 1, 1, nullptr, d_ws, fm.a, nullptr, nullptr));
    ZK_HIP(hipMemcpyAsync(out, fm.a, 384, hipMemcpyDeviceToHost, st));
    return slot_sync(s, st);
}

// what both forms of the Groth16 entry decide before a device is looked for; pre = tag || SHA-256(vk) || 32 bytes for the data digest || 8 for the index
static int groth16_batch_head(const void* vk, size_t vk_len, int vk_is_hex, size_t n_public, const char* tag, Groth16Vk* v, std::vector<uint8_t>* pre) {
    ZK_TRY(groth16_vk_parse(vk, vk_len, vk_is_hex, v));
    const size_t nk = v->K.size();
    if (nk != n_public + 1) return set_err(ZK_ERR_LEN, "invalid witness size, got %zu, expected %zu (public - ONE_WIRE)", n_public, nk ? nk - 1 : 0);  // upstream's message
    const size_t tl = strlen(tag);
    pre->assign(tl + 32 + 32 + 8, 0);
    memcpy(pre->data(), tag, tl);
    sha(pre->data() + tl, v->bytes.data(), v->bytes.size());
    return ZK_OK;
}

int zk_bn254_groth16_verify_batch(const uint8_t* proofs, size_t n_proofs, const void* vk, size_t vk_len, int vk_is_hex, const zk_fr* public_inputs,
                                  size_t n_public, uint8_t* accepted, size_t* n_accepted) {
    if (!vk || !n_accepted || (n_proofs && (!proofs || !accepted)) || (n_proofs && n_public && !public_inputs)) return set_err(ZK_ERR_ARG, "null pointer");
    *n_accepted = 0;
    Groth16Vk v;
    std::vector<uint8_t> pre;
    ZK_TRY(groth16_batch_head(vk, vk_len, vk_is_hex, n_public, "zkmi-groth16-batch", &v, &pre));
    if (n_proofs == 0) return ZK_OK;
    ZK_TRY(ensure_init());
    // r_i = low 128 bits of SHA-256(tag || SHA-256(vk) || SHA-256(proofs || public inputs) || u64 i), forced non-zero
    sha(pre.data() + pre.size() - 40, proofs, n_proofs * 128, public_inputs, n_proofs * n_public * 32);
    return groth16_verify_rows(v, RowsIn{proofs, 128, (const Fr*)public_inputs, n_public, false}, n_proofs, n_public, pre, accepted, n_accepted);
}

int zk_bn254_groth16_verify_batch_dev(const void* d_proofs, size_t proof_stride, size_t n_proofs, const void* vk, size_t vk_len, int vk_is_hex,
                                      const void* d_public_inputs, size_t pub_stride, size_t n_public, uint8_t* accepted, size_t* n_accepted) {
    if (!vk || !n_accepted || (n_proofs && (!d_proofs || !accepted)) || (n_proofs && n_public && !d_public_inputs)) return set_err(ZK_ERR_ARG, "null pointer");
    *n_accepted = 0;
    Groth16Vk v;
    std::vector<uint8_t> pre;
    ZK_TRY(groth16_batch_head(vk, vk_len, vk_is_hex, n_public, "zkmi-groth16-batch-rows", &v, &pre));
    ZK_TRY(rows_in_args(d_proofs, proof_stride, 128, n_proofs, d_public_inputs, pub_stride, n_public));
    if (n_proofs == 0) return ZK_OK;
    ZK_TRY(ensure_init());
    const RowsIn in{(const uint8_t*)d_proofs, proof_stride, (const Fr*)d_public_inputs, pub_stride, true};
    // r_i = low 128 bits of SHA-256(tag || SHA-256(vk) || SHA-256(d_0 || .. || d_{n-1}) || u64 i), d_v the rows' digests made on the device
    ZK_TRY(rows_digest_of_call(in, 128, n_proofs, n_public, pre.data() + pre.size() - 40));
    return groth16_verify_rows(v, in, n_proofs, n_public, pre, accepted, n_accepted);
}

// ---- Groth16 against many keys (DESIGN 3.9 "Many keys"): row i is a proof for vks[key_of[i]]
// What both forms decide before a device is looked for: the keys parse (a malformed key j: the host verifier's code and message, "key j" in front), every
// key_of[i] names a key, pub_stride holds the widest key's public inputs.  pre = tag || KD || 32 bytes for the data digest || 8 for the index, KD as in zkmi.h
static int groth16_keys_head(size_t n_proofs, const void* const* vks, const size_t* vk_lens, size_t n_keys, int vk_is_hex, const uint32_t* key_of,
                             const void* pub, size_t pub_stride, const char* tag, std::vector<Groth16Vk>* vs, std::vector<uint8_t>* pre) {
    if (n_keys == 0 && n_proofs > 0) return set_err(ZK_ERR_ARG, "n_keys == 0 with %zu proofs", n_proofs);
    vs->resize(n_keys);
    size_t max_np = 0;
    Sha256 kd;
    uint8_t d[32];
    const uint64_t nk = n_keys;
    for (int b = 0; b < 8; b++) d[b] = (uint8_t)(nk >> (8 * b));
    kd.update(d, 8);
    // a key is about 0.7 ms of host decompression (three G2 subgroup checks among it) and the keys are independent: up to 16 threads, every n-th key each.
    // The error text is per thread, so a worker keeps its key's; the first malformed key in key order is the one reported
    std::vector<int> rcs(n_keys, ZK_OK);
    std::vector<std::string> msgs(n_keys);
    const size_t n_thr = std::min<size_t>(std::min<size_t>(16, n_keys), std::max(1u, std::thread::hardware_concurrency()));
    auto parse = [&](size_t first) {
        for (size_t j = first; j < n_keys; j += n_thr) {
            if (!vks[j]) {
                rcs[j] = ZK_ERR_ARG;
                msgs[j] = "null pointer";
                continue;
            }
            rcs[j] = groth16_vk_parse(vks[j], vk_lens[j], vk_is_hex, &(*vs)[j]);
            if (rcs[j] != ZK_OK) msgs[j] = zk_last_error();
        }
    };
    {
        std::vector<std::thread> pool;
        for (size_t t = 1; t < n_thr; t++) pool.emplace_back(parse, t);
        if (n_thr) parse(0);
        for (std::thread& t : pool) t.join();
    }
    for (size_t j = 0; j < n_keys; j++) {
        if (rcs[j] != ZK_OK) return set_err(rcs[j], "key %zu: %s", j, msgs[j].c_str());
        if ((*vs)[j].K.empty()) return set_err(ZK_ERR_LEN, "key %zu: no K point", j);
        max_np = std::max(max_np, (*vs)[j].K.size() - 1);
        sha(d, (*vs)[j].bytes.data(), (*vs)[j].bytes.size());
        kd.update(d, 32);
    }
    for (size_t i = 0; i < n_proofs; i++) {
        if (key_of[i] >= n_keys) return set_err(ZK_ERR_ARG, "key_of[%zu] = %u is not below n_keys = %zu", i, key_of[i], n_keys);
        for (int b = 0; b < 4; b++) d[b] = (uint8_t)(key_of[i] >> (8 * b));
        kd.update(d, 4);
    }
    if (n_proofs > 1 && pub_stride < max_np)
        return set_err(ZK_ERR_LEN, "pub_stride = %zu is below the %zu public inputs of the widest key", pub_stride, max_np);
    if (n_proofs && max_np && !pub) return set_err(ZK_ERR_ARG, "null pointer");
    const size_t tl = strlen(tag);
    pre->assign(tl + 32 + 32 + 8, 0);
    memcpy(pre->data(), tag, tl);
    kd.final(pre->data() + tl);
    return ZK_OK;
}

int zk_bn254_groth16_verify_batch_keys(const uint8_t* proofs, size_t n_proofs, const void* const* vks, const size_t* vk_lens, size_t n_keys, int vk_is_hex,
                                       const uint32_t* key_of, const zk_fr* public_inputs, size_t pub_stride, uint8_t* accepted, size_t* n_accepted) {
    if (n_accepted) *n_accepted = 0;
    if (!n_accepted || (n_keys && (!vks || !vk_lens)) || (n_proofs && (!proofs || !accepted || !key_of))) return set_err(ZK_ERR_ARG, "null pointer");
    std::vector<Groth16Vk> vs;
    std::vector<uint8_t> pre;
    ZK_TRY(groth16_keys_head(n_proofs, vks, vk_lens, n_keys, vk_is_hex, key_of, public_inputs, pub_stride, "zkmi-groth16-batch-keys", &vs, &pre));
    if (n_proofs == 0) return ZK_OK;
    ZK_TRY(ensure_init());
    // r_i = the low 128 bits of SHA-256(tag || KD || SHA-256(proofs || each row's own public inputs) || u64 i), forced non-zero
    Sha256 h;
    h.update(proofs, n_proofs * 128);
    for (size_t i = 0; i < n_proofs; i++) {
        const size_t np = vs[key_of[i]].K.size() - 1;
        if (np) h.update(public_inputs + i * pub_stride, np * 32);
    }
    h.final(pre.data() + pre.size() - 40);
    return groth16_verify_rows_keys(vs, RowsIn{proofs, 128, (const Fr*)public_inputs, pub_stride, false}, n_proofs, key_of, pre, accepted, n_accepted);
}

int zk_bn254_groth16_verify_batch_keys_dev(const void* d_proofs, size_t proof_stride, size_t n_proofs, const void* const* vks, const size_t* vk_lens,
                                           size_t n_keys, int vk_is_hex, const uint32_t* key_of, const void* d_public_inputs, size_t pub_stride,
                                           uint8_t* accepted, size_t* n_accepted) {
    if (n_accepted) *n_accepted = 0;
    if (!n_accepted || (n_keys && (!vks || !vk_lens)) || (n_proofs && (!d_proofs || !accepted || !key_of))) return set_err(ZK_ERR_ARG, "null pointer");
    std::vector<Groth16Vk> vs;
    std::vector<uint8_t> pre;
    ZK_TRY(groth16_keys_head(n_proofs, vks, vk_lens, n_keys, vk_is_hex, key_of, d_public_inputs, pub_stride, "zkmi-groth16-batch-keys-rows", &vs, &pre));
    if (n_proofs > 1 && proof_stride < 128) return set_err(ZK_ERR_ARG, "proof_stride = %zu is below the %zu bytes of a proof", proof_stride, (size_t)128);
    if (n_proofs == 0) return ZK_OK;
    ZK_TRY(ensure_init());
    // the same with D = SHA-256(d_0 || .. || d_{n-1}) for the data digest, made by the core once the key table is in HBM
    const RowsIn in{(const uint8_t*)d_proofs, proof_stride, (const Fr*)d_public_inputs, pub_stride, true};
    return groth16_verify_rows_keys(vs, in, n_proofs, key_of, pre, accepted, n_accepted);
}

// what both forms of the PLONK entry decide before a device is looked for; pre = tag || SHA-256(vk) || SHA-256(srs_g2) || 32 bytes for the data digest
static int plonk_batch_head(const void* vk, size_t vk_len, int vk_is_hex, const zk_g2_affine srs_g2[2], size_t n_public, const char* tag, PlonkVk* v,
                            std::vector<uint8_t>* pre) {
    ZK_TRY(plonk_vk_parse(vk, vk_len, vk_is_hex, v));
    if (v->npub != n_public) return set_err(ZK_ERR_LEN, "invalid witness size, got %zu, expected %llu", n_public, (unsigned long long)v->npub);  // upstream's message
    const size_t tl = strlen(tag);
    pre->assign(tl + 3 * 32, 0);
    memcpy(pre->data(), tag, tl);
    sha(pre->data() + tl, v->bytes.data(), v->bytes.size());
    sha(pre->data() + tl + 32, srs_g2, 2 * sizeof(zk_g2_affine));
    return ZK_OK;
}

// plonk.Verify for the rows `in` against the parsed key.  pre: the coefficients' prefix, complete (64 to 127 bytes: one whole SHA-256 block, hashed here into the
// lanes' midstate, and a rest): rho_i, rho'_i = batch_coeff(SHA-256(pre || u64 i || 0 / 1)) -- the entry's to
// derive (zkmi.h states both derivations), so that one core serves the host and the device form
static int plonk_verify_rows(const PlonkVk& v, const zk_g2_affine srs_g2[2], const RowsIn& in, size_t n_proofs, size_t np, const std::vector<uint8_t>& pre,
                             uint8_t* accepted, size_t* n_accepted) {
    const PairConsts PK = pair_consts();
    PvKey K;
    K.n = v.n;
    K.log_n = 0;
    while (((uint64_t)1 << K.log_n) < v.n) K.log_n++;
    K.size_inv = bit_cast_img<Fr>(v.size_inv);
    K.gen = bit_cast_img<Fr>(v.gen);
    K.u = bit_cast_img<Fr>(v.u);
    const Affine<HFp> G{HFp::one(), HFp::one() + HFp::one()};
    Affine<HFp> kp[9];  // S1 S2 S3 Ql Qr Qm Qo Qk G
    for (int k = 0; k < 8; k++) kp[k] = v.pts[k];
    kp[8] = G;

    // gamma's common prefix: "gamma" || RawBytes(S1 .. Qk); the lanes start from the chaining value after its whole blocks
    Sha256 tg;
    tg.update("gamma", 5);
    for (int k = 0; k < 8; k++) {
        uint8_t b[64];
        g1_raw_bytes(v.pts[k], b);
        tg.update(b, 64);
    }
    const uint32_t tail_len = (uint32_t)tg.fill;
    if (pre.size() < 64 || pre.size() >= 128) return set_err(ZK_ERR_ARG, "coefficient prefix of %zu bytes", pre.size());
    Sha256 tr;
    tr.update(pre.data(), pre.size());  // one whole block, the rest (48 bytes in the host form, 53 in the device form) left in buf
    const uint32_t rtail_len = (uint32_t)(pre.size() - 64);
    std::vector<uint8_t> hbytes(tail_len + 13 + rtail_len);
    memcpy(hbytes.data(), tg.buf, tail_len);
    memcpy(hbytes.data() + tail_len, "betaalphazeta", 13);
    memcpy(hbytes.data() + tail_len + 13, tr.buf, rtail_len);
    uint32_t mids[16];
    memcpy(mids, tg.h, 32);
    memcpy(mids + 8, tr.h, 32);

    SlotGuard g;
    ZK_TRY(acquire_slot(&g.s));
    Slot* s = g.s;
    hipStream_t st = s->stream;
    const size_t ch = std::min(n_proofs, CHUNK);
    PairCheck pc(s, PK, ch);
    uint32_t *d_praw, *d_mids;
    Affine<Fp> *d_pts, *d_dig, *d_p, *d_kpts;
    uint8_t *d_stage, *d_bad, *d_hdr, *d_hbytes;
    Fr *d_sc, *d_pub, *d_fix;
    XYZZ<Fp> *d_t, *d_A, *d_B;
    FoldPair<XYZZ<Fp>> fa, fb;
    FoldPair<Fr> fold;
    Affine<Fp2>* d_g2;
    PvTerm* d_terms;
    int* d_status;
    ZK_TRY(plan_workspace(s, "plonk_verify_batch", [&](ArenaPlan& p) {
        p.take(in.on_device ? 1 : ch * 548, d_stage);
        p.take(ch * PV_NPTS * 8, d_praw);
        p.take(ch * PV_NPTS, d_pts, d_bad);
        p.take(ch * PV_NCOL, d_sc);
        p.take(in.on_device ? 1 : std::max(ch * np, (size_t)1), d_pub);
        p.take(ch * 10, d_t);
        p.take(ch * 3, d_fix);
        p.take(ch * 2, d_dig, d_p);
        p.take(ch, d_hdr, d_A, d_B);
        fa.layout(p, ch);
        fb.layout(p, ch);
        fold.layout(p, ch, 3);
        pc.layout(p, ch * 2);
        p.take(9, d_kpts);
        p.take(2, d_g2);
        p.take(16, d_mids, d_status);
        p.take(hbytes.size(), d_hbytes);
        p.take(21, d_terms);
    }));
    uint8_t* const d_valid = pc.d_valid;
    ZK_HIP(hipMemcpyAsync(d_kpts, kp, sizeof kp, hipMemcpyHostToDevice, st));
    ZK_HIP(hipMemcpyAsync(d_g2, srs_g2, 2 * 128, hipMemcpyHostToDevice, st));
    ZK_HIP(hipMemcpyAsync(d_mids, mids, sizeof mids, hipMemcpyHostToDevice, st));
    ZK_HIP(hipMemcpyAsync(d_hbytes, hbytes.data(), hbytes.size(), hipMemcpyHostToDevice, st));

    std::vector<PvTerm> terms(21);
    size_t tn = 0;  // the table is rebuilt per chunk: its column pointers depend on the chunk's length
    for (size_t c0 = 0; c0 < n_proofs; c0 += ch) {
        const size_t n = std::min(ch, n_proofs - c0);
        if (n != tn) {
            auto col = [&](int c) { return (const Fr*)(d_sc + (size_t)c * n); };
            auto lane = [&](int k) { return (const Affine<Fp>*)(d_pts + (size_t)k * n); };
            // digests: H1 zp, H2 zp^2 | Ql l, Qr r, Qm lr, Qo o, S3 c_s3, Z c_z
            terms[0] = {lane(PV_H0 + 1), 1, col(PV_ZP)};
            terms[1] = {lane(PV_H0 + 2), 1, col(PV_ZP2)};
            terms[2] = {d_kpts + 3, 0, col(PV_CLAIM + 2)};
            terms[3] = {d_kpts + 4, 0, col(PV_CLAIM + 3)};
            terms[4] = {d_kpts + 5, 0, col(PV_LR)};
            terms[5] = {d_kpts + 6, 0, col(PV_CLAIM + 4)};
            terms[6] = {d_kpts + 2, 0, col(PV_CS3)};
            terms[7] = {lane(PV_Z), 1, col(PV_CZ)};
            // the combined opening check: fh lin L R O W Z W' | W W'
            const Affine<Fp>* cp[10] = {d_dig, d_dig + n, lane(PV_L), lane(PV_L + 1), lane(PV_L + 2), lane(PV_W), lane(PV_Z), lane(PV_WS), lane(PV_W), lane(PV_WS)};
            for (int k = 0; k < 10; k++) terms[8 + k] = {cp[k], 1, col(PV_T + k)};
            // fallback: G, S1, S2
            terms[18] = {d_kpts + 8, 0, d_fix};
            terms[19] = {d_kpts + 0, 0, d_fix + n};
            terms[20] = {d_kpts + 1, 0, d_fix + 2 * n};
            ZK_HIP(hipMemcpyAsync(d_terms, terms.data(), terms.size() * sizeof(PvTerm), hipMemcpyHostToDevice, st));
            tn = n;
        }
        RowsIn at;
        ZK_TRY(rows_of_chunk(in, st, c0, n, 548, np, d_stage, d_pub, &at));
        ZK_HIP(hipMemsetAsync(d_bad, 0, n * PV_NPTS, st));
        ZK_HIP(hipMemsetAsync(d_status, 0, 4, st));
        const dim3 g64(blocks(n, 64)), g256(blocks(n, 256));
        ZK_LAUNCH(s, st, "pv_gather", k_pv_gather, g256, dim3(256), 0, at.proofs, at.proof_stride, n, d_praw, d_sc, d_hdr);
        ZK_TRY(g1_decompress_dev(s, st, d_praw, PV_NPTS * n, d_pts, d_status, d_bad));
        ZK_LAUNCH(s, st, "pv_transcript", k_pv_transcript, g64, dim3(64), 0, (const Affine<Fp>*)d_pts, (const uint8_t*)d_bad, (const uint8_t*)d_hdr,
                  at.pub, at.pub_stride, n, np, (const uint32_t*)d_mids, (uint64_t)(tg.len - tail_len), (const uint8_t*)d_hbytes, tail_len, d_valid, d_sc);
        ZK_LAUNCH(s, st, "pv_scalars", k_pv_scalars, g64, dim3(64), 0, at.pub, at.pub_stride, n, np, K, d_valid, d_sc);
        ZK_LAUNCH(s, st, "pv_smul", k_pv_smul, dim3(blocks(n, 64), 8), dim3(64), 0, (const PvTerm*)d_terms, n, (const uint8_t*)d_valid, d_t);
        ZK_LAUNCH(s, st, "pv_digests", k_pv_digests, g64, dim3(64), 0, (const Affine<Fp>*)d_pts, (const XYZZ<Fp>*)d_t, (const Affine<Fp>*)d_kpts, n,
                  (const uint8_t*)d_valid, d_dig);
        ZK_LAUNCH(s, st, "pv_kzg", k_pv_kzg, g64, dim3(64), 0, (const Affine<Fp>*)d_pts, (const Affine<Fp>*)d_dig, (const Affine<Fp>*)d_kpts, n, c0, K,
                  (const uint32_t*)(d_mids + 8), (const uint8_t*)(d_hbytes + tail_len + 13), rtail_len, (const uint8_t*)d_valid, d_sc, d_fix, fold.a);
        ZK_LAUNCH(s, st, "pv_smul", k_pv_smul, dim3(blocks(n, 64), 10), dim3(64), 0, (const PvTerm*)(d_terms + 8), n, (const uint8_t*)d_valid, d_t);
        ZK_LAUNCH(s, st, "pv_combine", k_pv_combine, g256, dim3(256), 0, (const XYZZ<Fp>*)d_t, n, d_A, d_B, fa.a, fb.a);
        const XYZZ<Fp>* a_sum = fold_all(s, st, "g1_fold", k_g1_fold, 256, fa, n, 1);
        const XYZZ<Fp>* b_sum = fold_all(s, st, "g1_fold", k_g1_fold, 256, fb, n, 1);
        const Fr* c_sum = fold_all(s, st, "fr_fold", k_fr_fold, 256, fold, n, 3);
        XYZZ<HFp> sa, sb;
        HFr c[3];
        ZK_HIP(hipMemcpyAsync(&sa, a_sum, 128, hipMemcpyDeviceToHost, st));
        ZK_HIP(hipMemcpyAsync(&sb, b_sum, 128, hipMemcpyDeviceToHost, st));
        ZK_HIP(hipMemcpyAsync(c, c_sum, 3 * 32, hipMemcpyDeviceToHost, st));
        ZK_TRY(pc.sync_valid(n, accepted + c0));
        if (pc.decided) continue;
        // e(sum A_i + c_G G + c_S1 S1 + c_S2 S2, [1]2) e(-sum B_i, [alpha]2) == 1 (the fixed points scaled here: three host multiplications per chunk)
        Affine<HFp> two[2];
        {
            const Affine<HFp> fp[3] = {G, v.pts[0], v.pts[1]};
            for (int j = 0; j < 3; j++) {
                uint32_t k[8];
                to_canonical_u32(c[j], k);
                sa.add(scalar_mul(fp[j], k));
            }
            two[0] = sa.to_affine();
            two[1] = sb.to_affine().neg();
        }
        ZK_HIP(hipMemcpyAsync(d_p, two, 2 * 64, hipMemcpyHostToDevice, st));
        ZK_TRY(pc.combined(d_p, 2, nullptr, 0, d_g2, n, accepted + c0));
        if (pc.decided) continue;
        // fallback: each valid proof's own two-pairing check, with its own rho_i, rho'_i
        ZK_LAUNCH(s, st, "pv_smul", k_pv_smul, dim3(blocks(n, 64), 3), dim3(64), 0, (const PvTerm*)(d_terms + 18), n, (const uint8_t*)d_valid, d_t);
        ZK_LAUNCH(s, st, "pv_single", k_pv_single, g256, dim3(256), 0, (const XYZZ<Fp>*)d_A, (const XYZZ<Fp>*)d_B, (const XYZZ<Fp>*)d_t, n,
                  (const uint8_t*)d_valid, d_p);
        ZK_TRY(pc.per_lane(d_p, n, 2, nullptr, 0, d_g2, false, accepted + c0));
    }
    *n_accepted = pc.total;
    return ZK_OK;
}

int zk_bn254_plonk_verify_batch(const uint8_t* proofs, size_t n_proofs, const void* vk, size_t vk_len, int vk_is_hex, const zk_g2_affine srs_g2[2],
                                const zk_fr* public_inputs, size_t n_public, uint8_t* accepted, size_t* n_accepted) {
    if (!vk || !srs_g2 || !n_accepted || (n_proofs && (!proofs || !accepted)) || (n_proofs && n_public && !public_inputs))
        return set_err(ZK_ERR_ARG, "null pointer");
    *n_accepted = 0;
    PlonkVk v;
    std::vector<uint8_t> pre;
    ZK_TRY(plonk_batch_head(vk, vk_len, vk_is_hex, srs_g2, n_public, "zkmi-plonk-batch", &v, &pre));
    if (n_proofs == 0) return ZK_OK;
    ZK_TRY(ensure_init());
    // rho_i, rho'_i = the low 128 bits of SHA-256(tag || SHA-256(vk) || SHA-256(srs_g2) || SHA-256(proofs || public inputs) || u64 i || 0 / 1)
    sha(pre.data() + pre.size() - 32, proofs, n_proofs * 548, public_inputs, n_proofs * n_public * 32);
    return plonk_verify_rows(v, srs_g2, RowsIn{proofs, 548, (const Fr*)public_inputs, n_public, false}, n_proofs, n_public, pre, accepted, n_accepted);
}

int zk_bn254_plonk_verify_batch_dev(const void* d_proofs, size_t proof_stride, size_t n_proofs, const void* vk, size_t vk_len, int vk_is_hex,
                                    const zk_g2_affine srs_g2[2], const void* d_public_inputs, size_t pub_stride, size_t n_public, uint8_t* accepted,
                                    size_t* n_accepted) {
    if (!vk || !srs_g2 || !n_accepted || (n_proofs && (!d_proofs || !accepted)) || (n_proofs && n_public && !d_public_inputs))
        return set_err(ZK_ERR_ARG, "null pointer");
    *n_accepted = 0;
    PlonkVk v;
    std::vector<uint8_t> pre;
    ZK_TRY(plonk_batch_head(vk, vk_len, vk_is_hex, srs_g2, n_public, "zkmi-plonk-batch-rows", &v, &pre));
    ZK_TRY(rows_in_args(d_proofs, proof_stride, 548, n_proofs, d_public_inputs, pub_stride, n_public));
    if (n_proofs == 0) return ZK_OK;
    ZK_TRY(ensure_init());
    const RowsIn in{(const uint8_t*)d_proofs, proof_stride, (const Fr*)d_public_inputs, pub_stride, true};
    // the same with SHA-256(d_0 || .. || d_{n-1}) for the data digest, d_v the rows' digests made on the device
    ZK_TRY(rows_digest_of_call(in, 548, n_proofs, n_public, pre.data() + pre.size() - 32));
    return plonk_verify_rows(v, srs_g2, in, n_proofs, n_public, pre, accepted, n_accepted);
}

// ---- PLONK against many keys (DESIGN 3.10 "Many keys"): row i is a proof for vks[key_of[i]]
// What both forms decide before a device is looked for: the keys parse (a malformed key j: the host verifier's code and message, "key j" in front), every
// key_of[i] names a key, pub_stride holds the widest key's public inputs.  pre = tag || KD || SHA-256(srs_g2) || 32 bytes for the data digest, KD as in zkmi.h
static int plonk_keys_head(size_t n_proofs, const void* const* vks, const size_t* vk_lens, size_t n_keys, int vk_is_hex, const zk_g2_affine srs_g2[2],
                           const uint32_t* key_of, const void* pub, size_t pub_stride, const char* tag, std::vector<PlonkVk>* vs, std::vector<uint8_t>* pre) {
    if (n_keys == 0 && n_proofs > 0) return set_err(ZK_ERR_ARG, "n_keys == 0 with %zu proofs", n_proofs);
    vs->resize(n_keys);
    size_t max_np = 0;
    Sha256 kd;
    uint8_t d[32];
    const uint64_t nk = n_keys;
    for (int b = 0; b < 8; b++) d[b] = (uint8_t)(nk >> (8 * b));
    kd.update(d, 8);
    for (size_t j = 0; j < n_keys; j++) {
        if (!vks[j]) return set_err(ZK_ERR_ARG, "key %zu: null pointer", j);
        const int rc = plonk_vk_parse(vks[j], vk_lens[j], vk_is_hex, &(*vs)[j]);
        if (rc != ZK_OK) return set_err(rc, "key %zu: %s", j, zk_last_error());
        max_np = std::max(max_np, (size_t)(*vs)[j].npub);
        sha(d, (*vs)[j].bytes.data(), (*vs)[j].bytes.size());
        kd.update(d, 32);
    }
    for (size_t i = 0; i < n_proofs; i++) {
        if (key_of[i] >= n_keys) return set_err(ZK_ERR_ARG, "key_of[%zu] = %u is not below n_keys = %zu", i, key_of[i], n_keys);
        for (int b = 0; b < 4; b++) d[b] = (uint8_t)(key_of[i] >> (8 * b));
        kd.update(d, 4);
    }
    if (n_proofs > 1 && pub_stride < max_np)
        return set_err(ZK_ERR_LEN, "pub_stride = %zu is below the %zu public inputs of the widest key", pub_stride, max_np);
    if (n_proofs && max_np && !pub) return set_err(ZK_ERR_ARG, "null pointer");
    const size_t tl = strlen(tag);
    pre->assign(tl + 3 * 32, 0);
    memcpy(pre->data(), tag, tl);
    kd.final(pre->data() + tl);
    sha(pre->data() + tl + 32, srs_g2, 2 * sizeof(zk_g2_affine));
    return ZK_OK;
}

// plonk_verify_rows with a key per row.  pre: the coefficients' prefix (64 to 127 bytes); its last 32 bytes, the data digest, are the entry's in the host form
// and made here in the device form (k_rows_digest_keys needs the key table).  What differs from the single-key core: the key table and key_of in HBM; c_S1 S1
// and c_S2 S2 as two more rows of the second scalar-multiplication launch, inside A_i; only G's coefficient is folded, so the host multiplies once per chunk
static int plonk_verify_rows_keys(const std::vector<PlonkVk>& vs, const zk_g2_affine srs_g2[2], const RowsIn& in, size_t n_proofs, const uint32_t* key_of,
                                  std::vector<uint8_t>& pre, uint8_t* accepted, size_t* n_accepted) {
    const PairConsts PK = pair_consts();
    const Affine<HFp> G{HFp::one(), HFp::one() + HFp::one()};
    const size_t nk = vs.size();
    std::vector<PvKeyRow> tab(nk);
    uint64_t mid_len = 0;
    uint32_t tail_len = 0;
    size_t max_np = 0;
    for (size_t j = 0; j < nk; j++) {
        const PlonkVk& v = vs[j];
        PvKeyRow& R = tab[j];
        memset(&R, 0, sizeof R);
        R.K.n = v.n;
        while (((uint64_t)1 << R.K.log_n) < v.n) R.K.log_n++;
        R.K.size_inv = bit_cast_img<Fr>(v.size_inv);
        R.K.gen = bit_cast_img<Fr>(v.gen);
        R.K.u = bit_cast_img<Fr>(v.u);
        R.np = v.npub;
        max_np = std::max(max_np, (size_t)v.npub);
        memcpy(R.pts, v.pts, 8 * sizeof(Affine<Fp>));
        memcpy(R.pts + 8, &G, sizeof G);
        Sha256 tg;
        tg.update("gamma", 5);
        for (int k = 0; k < 8; k++) {
            uint8_t b[64];
            g1_raw_bytes(v.pts[k], b);
            tg.update(b, 64);
        }
        tail_len = (uint32_t)tg.fill;  // 5 for every key: the prefix is 517 bytes
        mid_len = tg.len - tail_len;
        if (tail_len + 13 > sizeof R.pre) return set_err(ZK_ERR_ARG, "transcript prefix of %llu bytes", (unsigned long long)tg.len);
        memcpy(R.mid, tg.h, 32);
        memcpy(R.pre, tg.buf, tail_len);
        memcpy(R.pre + tail_len, "betaalphazeta", 13);
    }
    if (pre.size() < 64 || pre.size() >= 128) return set_err(ZK_ERR_ARG, "coefficient prefix of %zu bytes", pre.size());
    const uint32_t rtail_len = (uint32_t)(pre.size() - 64);
    // a chunk's public inputs as they come up in the host form: whole rows of the caller's stride but for the last, which ends with its own n_public
    const size_t ps = in.pub_stride, pub_elems = max_np ? (std::min(n_proofs, CHUNK) - 1) * ps + max_np : 0;

    SlotGuard g;
    ZK_TRY(acquire_slot(&g.s));
    Slot* s = g.s;
    hipStream_t st = s->stream;
    const size_t ch = std::min(n_proofs, CHUNK);
    PairCheck pc(s, PK, ch);
    uint32_t *d_praw, *d_rmid, *d_key_of;
    Affine<Fp> *d_pts, *d_dig, *d_p;
    uint8_t *d_stage, *d_bad, *d_hdr, *d_rtail, *d_rowdig;
    Fr *d_sc, *d_pub, *d_fix;
    XYZZ<Fp> *d_t, *d_A, *d_B;
    FoldPair<XYZZ<Fp>> fa, fb;
    FoldPair<Fr> fold;
    Affine<Fp2>* d_g2;
    PvKeyRow* d_tab;
    PvkTerm* d_terms;
    int* d_status;
    ZK_TRY(plan_workspace(s, "plonk_verify_batch_keys", [&](ArenaPlan& p) {
        p.take(in.on_device ? 1 : ch * 548, d_stage);
        p.take(ch * PV_NPTS * 8, d_praw);
        p.take(ch * PV_NPTS, d_pts, d_bad);
        p.take(ch * PV_NCOL, d_sc);
        p.take(in.on_device ? 1 : std::max(pub_elems, (size_t)1), d_pub);
        p.take(ch * 12, d_t);
        p.take(ch * 3, d_fix);
        p.take(ch * 2, d_dig, d_p);
        p.take(ch, d_hdr, d_A, d_B);
        fa.layout(p, ch);
        fb.layout(p, ch);
        fold.layout(p, ch, 1);
        pc.layout(p, ch * 2);
        p.take(nk, d_tab);
        p.take(n_proofs, d_key_of);
        p.take(in.on_device ? n_proofs * 32 : 1, d_rowdig);
        p.take(2, d_g2);
        p.take(8, d_rmid);
        p.take(64, d_rtail);
        p.take(16, d_status);
        p.take(21, d_terms);
    }));
    uint8_t* const d_valid = pc.d_valid;
    ZK_HIP(hipMemcpyAsync(d_tab, tab.data(), nk * sizeof(PvKeyRow), hipMemcpyHostToDevice, st));
    ZK_HIP(hipMemcpyAsync(d_key_of, key_of, n_proofs * 4, hipMemcpyHostToDevice, st));
    ZK_HIP(hipMemcpyAsync(d_g2, srs_g2, 2 * 128, hipMemcpyHostToDevice, st));
    if (in.on_device) {
        // D = SHA-256(d_0 || .. || d_{n-1}) over the whole call, d_v = SHA-256(row v's proof || its own 32 n_public(key_of[v]) public-input bytes as they lie)
        ZK_LAUNCH(s, st, "rows_digest_keys", k_rows_digest_keys, dim3(blocks(n_proofs, 64)), dim3(64), 0, in.proofs, (size_t)548, in.proof_stride,
                  (const uint8_t*)in.pub, ps * 32, (const PvKeyRow*)d_tab, (const uint32_t*)d_key_of, n_proofs, d_rowdig);
        std::vector<uint8_t> dig(n_proofs * 32);
        ZK_HIP(hipMemcpyAsync(dig.data(), d_rowdig, dig.size(), hipMemcpyDeviceToHost, st));
        ZK_TRY(slot_sync(s, st));
        sha(pre.data() + pre.size() - 32, dig.data(), dig.size());
    }
    Sha256 tr;
    tr.update(pre.data(), pre.size());  // one whole block into the lanes' midstate, the rest left in buf
    ZK_HIP(hipMemcpyAsync(d_rmid, tr.h, 32, hipMemcpyHostToDevice, st));
    ZK_HIP(hipMemcpyAsync(d_rtail, tr.buf, rtail_len, hipMemcpyHostToDevice, st));

    std::vector<PvkTerm> terms(21);
    size_t tn = 0;  // the table is rebuilt per chunk: its column pointers depend on the chunk's length
    for (size_t c0 = 0; c0 < n_proofs; c0 += ch) {
        const size_t n = std::min(ch, n_proofs - c0);
        if (n != tn) {
            auto col = [&](int c) { return (const Fr*)(d_sc + (size_t)c * n); };
            auto lane = [&](int k) { return (const Affine<Fp>*)(d_pts + (size_t)k * n); };
            // digests: H1 zp, H2 zp^2 | Ql l, Qr r, Qm lr, Qo o, S3 c_s3, Z c_z
            terms[0] = {lane(PV_H0 + 1), -1, col(PV_ZP)};
            terms[1] = {lane(PV_H0 + 2), -1, col(PV_ZP2)};
            terms[2] = {nullptr, 3, col(PV_CLAIM + 2)};
            terms[3] = {nullptr, 4, col(PV_CLAIM + 3)};
            terms[4] = {nullptr, 5, col(PV_LR)};
            terms[5] = {nullptr, 6, col(PV_CLAIM + 4)};
            terms[6] = {nullptr, 2, col(PV_CS3)};
            terms[7] = {lane(PV_Z), -1, col(PV_CZ)};
            // the combined opening check: fh lin L R O W Z W' | W W' | the lane's key's S1, S2
            const Affine<Fp>* cp[10] = {d_dig, d_dig + n, lane(PV_L), lane(PV_L + 1), lane(PV_L + 2), lane(PV_W), lane(PV_Z), lane(PV_WS), lane(PV_W), lane(PV_WS)};
            for (int k = 0; k < 10; k++) terms[8 + k] = {cp[k], -1, col(PV_T + k)};
            terms[18] = {nullptr, 0, d_fix + n};
            terms[19] = {nullptr, 1, d_fix + 2 * n};
            // fallback: G
            terms[20] = {nullptr, 8, d_fix};
            ZK_HIP(hipMemcpyAsync(d_terms, terms.data(), terms.size() * sizeof(PvkTerm), hipMemcpyHostToDevice, st));
            tn = n;
        }
        RowsIn at;
        if (in.on_device) {
            at = RowsIn{in.proofs + c0 * in.proof_stride, in.proof_stride, max_np ? in.pub + c0 * ps : nullptr, ps, true};
        } else {
            ZK_HIP(hipMemcpyAsync(d_stage, in.proofs + c0 * 548, n * 548, hipMemcpyHostToDevice, st));
            const size_t last = (size_t)vs[key_of[c0 + n - 1]].npub;
            if (max_np && (n - 1) * ps + last)
                ZK_HIP(hipMemcpyAsync(d_pub, in.pub + c0 * ps, ((n - 1) * ps + last) * 32, hipMemcpyHostToDevice, st));
            at = RowsIn{d_stage, 548, d_pub, ps, true};
        }
        const uint32_t* kof = d_key_of + c0;  // lane i of this chunk is row c0 + i of the call
        ZK_HIP(hipMemsetAsync(d_bad, 0, n * PV_NPTS, st));
        ZK_HIP(hipMemsetAsync(d_status, 0, 4, st));
        const dim3 g64(blocks(n, 64)), g256(blocks(n, 256));
        ZK_LAUNCH(s, st, "pv_gather", k_pv_gather, g256, dim3(256), 0, at.proofs, at.proof_stride, n, d_praw, d_sc, d_hdr);
        ZK_TRY(g1_decompress_dev(s, st, d_praw, PV_NPTS * n, d_pts, d_status, d_bad));
        ZK_LAUNCH(s, st, "pvk_transcript", k_pvk_transcript, g64, dim3(64), 0, (const Affine<Fp>*)d_pts, (const uint8_t*)d_bad, (const uint8_t*)d_hdr, at.pub,
                  at.pub_stride, n, (const PvKeyRow*)d_tab, kof, mid_len, tail_len, d_valid, d_sc);
        ZK_LAUNCH(s, st, "pvk_scalars", k_pvk_scalars, g64, dim3(64), 0, at.pub, at.pub_stride, n, (const PvKeyRow*)d_tab, kof, d_valid, d_sc);
        ZK_LAUNCH(s, st, "pvk_smul", k_pvk_smul, dim3(blocks(n, 64), 8), dim3(64), 0, (const PvkTerm*)d_terms, (const PvKeyRow*)d_tab, kof, n,
                  (const uint8_t*)d_valid, d_t);
        ZK_LAUNCH(s, st, "pvk_digests", k_pvk_digests, g64, dim3(64), 0, (const Affine<Fp>*)d_pts, (const XYZZ<Fp>*)d_t, (const PvKeyRow*)d_tab, kof, n,
                  (const uint8_t*)d_valid, d_dig);
        ZK_LAUNCH(s, st, "pvk_kzg", k_pvk_kzg, g64, dim3(64), 0, (const Affine<Fp>*)d_pts, (const Affine<Fp>*)d_dig, (const PvKeyRow*)d_tab, kof, n, c0,
                  (const uint32_t*)d_rmid, (const uint8_t*)d_rtail, rtail_len, (const uint8_t*)d_valid, d_sc, d_fix, fold.a);
        ZK_LAUNCH(s, st, "pvk_smul", k_pvk_smul, dim3(blocks(n, 64), 12), dim3(64), 0, (const PvkTerm*)(d_terms + 8), (const PvKeyRow*)d_tab, kof, n,
                  (const uint8_t*)d_valid, d_t);
        ZK_LAUNCH(s, st, "pvk_combine", k_pvk_combine, g256, dim3(256), 0, (const XYZZ<Fp>*)d_t, n, d_A, d_B, fa.a, fb.a);
        const XYZZ<Fp>* a_sum = fold_all(s, st, "g1_fold", k_g1_fold, 256, fa, n, 1);
        const XYZZ<Fp>* b_sum = fold_all(s, st, "g1_fold", k_g1_fold, 256, fb, n, 1);
        const Fr* c_sum = fold_all(s, st, "fr_fold", k_fr_fold, 256, fold, n, 1);
        XYZZ<HFp> sa, sb;
        HFr c;
        ZK_HIP(hipMemcpyAsync(&sa, a_sum, 128, hipMemcpyDeviceToHost, st));
        ZK_HIP(hipMemcpyAsync(&sb, b_sum, 128, hipMemcpyDeviceToHost, st));
        ZK_HIP(hipMemcpyAsync(&c, c_sum, 32, hipMemcpyDeviceToHost, st));
        ZK_TRY(pc.sync_valid(n, accepted + c0));
        if (pc.decided) continue;
        // e(sum A_i + c_G G, [1]2) e(-sum B_i, [alpha]2) == 1: G is every key's, one host multiplication per chunk however many keys there are
        Affine<HFp> two[2];
        {
            uint32_t k[8];
            to_canonical_u32(c, k);
            sa.add(scalar_mul(G, k));
            two[0] = sa.to_affine();
            two[1] = sb.to_affine().neg();
        }
        ZK_HIP(hipMemcpyAsync(d_p, two, 2 * 64, hipMemcpyHostToDevice, st));
        ZK_TRY(pc.combined(d_p, 2, nullptr, 0, d_g2, n, accepted + c0));
        if (pc.decided) continue;
        // fallback: each valid proof's own two-pairing check; A_i lacks only the lane's c_G G
        ZK_LAUNCH(s, st, "pvk_smul", k_pvk_smul, dim3(blocks(n, 64), 1), dim3(64), 0, (const PvkTerm*)(d_terms + 20), (const PvKeyRow*)d_tab, kof, n,
                  (const uint8_t*)d_valid, d_t);
        ZK_LAUNCH(s, st, "pvk_single", k_pvk_single, g256, dim3(256), 0, (const XYZZ<Fp>*)d_A, (const XYZZ<Fp>*)d_B, (const XYZZ<Fp>*)d_t, n,
                  (const uint8_t*)d_valid, d_p);
        ZK_TRY(pc.per_lane(d_p, n, 2, nullptr, 0, d_g2, false, accepted + c0));
    }
    *n_accepted = pc.total;
    return ZK_OK;
}

int zk_bn254_plonk_verify_batch_keys(const uint8_t* proofs, size_t n_proofs, const void* const* vks, const size_t* vk_lens, size_t n_keys, int vk_is_hex,
                                     const zk_g2_affine srs_g2[2], const uint32_t* key_of, const zk_fr* public_inputs, size_t pub_stride, uint8_t* accepted,
                                     size_t* n_accepted) {
    if (n_accepted) *n_accepted = 0;
    if (!srs_g2 || !n_accepted || (n_keys && (!vks || !vk_lens)) || (n_proofs && (!proofs || !accepted || !key_of))) return set_err(ZK_ERR_ARG, "null pointer");
    std::vector<PlonkVk> vs;
    std::vector<uint8_t> pre;
    ZK_TRY(plonk_keys_head(n_proofs, vks, vk_lens, n_keys, vk_is_hex, srs_g2, key_of, public_inputs, pub_stride, "zkmi-plonk-batch-keys", &vs, &pre));
    if (n_proofs == 0) return ZK_OK;
    ZK_TRY(ensure_init());
    // rho_i, rho'_i = the low 128 bits of SHA-256(tag || KD || SHA-256(srs_g2) || SHA-256(proofs || each row's own public inputs) || u64 i || 0 / 1)
    Sha256 h;
    h.update(proofs, n_proofs * 548);
    for (size_t i = 0; i < n_proofs; i++) {
        const size_t np = (size_t)vs[key_of[i]].npub;
        if (np) h.update(public_inputs + i * pub_stride, np * 32);
    }
    h.final(pre.data() + pre.size() - 32);
    return plonk_verify_rows_keys(vs, srs_g2, RowsIn{proofs, 548, (const Fr*)public_inputs, pub_stride, false}, n_proofs, key_of, pre, accepted, n_accepted);
}

int zk_bn254_plonk_verify_batch_keys_dev(const void* d_proofs, size_t proof_stride, size_t n_proofs, const void* const* vks, const size_t* vk_lens, size_t n_keys,
                                         int vk_is_hex, const zk_g2_affine srs_g2[2], const uint32_t* key_of, const void* d_public_inputs, size_t pub_stride,
                                         uint8_t* accepted, size_t* n_accepted) {
    if (n_accepted) *n_accepted = 0;
    if (!srs_g2 || !n_accepted || (n_keys && (!vks || !vk_lens)) || (n_proofs && (!d_proofs || !accepted || !key_of))) return set_err(ZK_ERR_ARG, "null pointer");
    std::vector<PlonkVk> vs;
    std::vector<uint8_t> pre;
    ZK_TRY(plonk_keys_head(n_proofs, vks, vk_lens, n_keys, vk_is_hex, srs_g2, key_of, d_public_inputs, pub_stride, "zkmi-plonk-batch-keys-rows", &vs, &pre));
    if (n_proofs > 1 && proof_stride < 548) return set_err(ZK_ERR_ARG, "proof_stride = %zu is below the %zu bytes of a proof", proof_stride, (size_t)548);
    if (n_proofs == 0) return ZK_OK;
    ZK_TRY(ensure_init());
    // the same with D = SHA-256(d_0 || .. || d_{n-1}) for the data digest, made by the core once the key table is in HBM
    const RowsIn in{(const uint8_t*)d_proofs, proof_stride, (const Fr*)d_public_inputs, pub_stride, true};
    return plonk_verify_rows_keys(vs, srs_g2, in, n_proofs, key_of, pre, accepted, n_accepted);
}

int zk_bn254_rows_sha256_dev(const void* d_a, size_t a_len, size_t a_stride, const void* d_b, size_t b_len, size_t b_stride, size_t rows, void* d_out, void* stream) {
    if ((a_len && !d_a) || (b_len && !d_b) || (rows && !d_out)) return set_err(ZK_ERR_ARG, "null pointer");
    if (rows > 1 && (a_stride < a_len || b_stride < b_len))
        return set_err(ZK_ERR_ARG, "strides %zu / %zu are below the %zu / %zu bytes of a row", a_stride, b_stride, a_len, b_len);
    if (rows == 0) return ZK_OK;
    SlotGuard g;
    ZK_TRY(acquire_slot(&g.s));
    hipStream_t st = stream ? (hipStream_t)stream : g.s->stream;
    rows_digest_launch(g.s, st, d_a, a_len, a_stride, d_b, b_len, b_stride, rows, d_out);
    if (!stream || profiling_on()) ZK_TRY(slot_sync(g.s, st));
    return ZK_OK;
}

// kzg.BatchVerifyMultiPoints with a verdict per opening (include/zkmi.h)
int zk_bn254_kzg_verify_batch(const zk_g1_affine* digests, const zk_kzg_opening* openings, const zk_fr* points, size_t n_openings, const zk_g2_affine srs_g2[2],
                              uint8_t* accepted, size_t* n_accepted) {
    static_assert(sizeof(zk_kzg_opening) == 96 && sizeof(KzgLane) == 96, "opening image");
    if (!srs_g2 || !n_accepted || (n_openings && (!digests || !openings || !points || !accepted))) return set_err(ZK_ERR_ARG, "null pointer");
    *n_accepted = 0;
    if (n_openings == 0) return ZK_OK;
    ZK_TRY(ensure_init());
    const PairConsts PK = pair_consts();
    const Affine<Fp> G = bit_cast_img<Affine<Fp>>(Affine<HFp>{HFp::one(), HFp::one() + HFp::one()});
    // lambda_i = the low 128 bits of SHA-256("zkmi-kzg-batch" || SHA-256(srs_g2) || SHA-256(digests || openings || points) || u64 i), forced non-zero
    uint8_t pre[14 + 32 + 32 + 8];
    memcpy(pre, "zkmi-kzg-batch", 14);
    sha(pre + 14, srs_g2, 2 * sizeof(zk_g2_affine));
    sha(pre + 46, digests, n_openings * 64, openings, n_openings * 96, points, n_openings * 32);
    SlotGuard g;
    ZK_TRY(acquire_slot(&g.s));
    Slot* s = g.s;
    hipStream_t st = s->stream;
    const size_t ch = std::min(n_openings, CHUNK);
    PairCheck pc(s, PK, ch);
    Affine<Fp> *d_dig, *d_p, *d_two;
    KzgLane* d_op;
    Fr* d_z;
    uint32_t* d_rr;
    FoldPair<XYZZ<Fp>> fa, fb;
    Affine<Fp2>* d_g2;
    ZK_TRY(plan_workspace(s, "kzg_verify_batch", [&](ArenaPlan& p) {
        p.take(ch, d_dig, d_op, d_z);
        p.take(ch * 4, d_rr);
        fa.layout(p, ch);
        fb.layout(p, ch);
        p.take(ch * 2, d_p);
        p.take(2, d_two, d_g2);
        pc.layout(p, ch * 2);
    }));
    ZK_HIP(hipMemcpyAsync(d_g2, srs_g2, 2 * 128, hipMemcpyHostToDevice, st));
    ZK_HIP(hipMemsetAsync(pc.d_valid, 1, ch, st));  // the points are not validated: every lane takes part
    std::fill(pc.valid.begin(), pc.valid.end(), 1);
    std::vector<uint32_t> rr(ch * 4);
    for (size_t c0 = 0; c0 < n_openings; c0 += ch) {
        const size_t n = std::min(ch, n_openings - c0);
        batch_coeffs(pre, sizeof pre, 78, c0, n, rr.data());
        ZK_HIP(hipMemcpyAsync(d_dig, digests + c0, n * 64, hipMemcpyHostToDevice, st));
        ZK_HIP(hipMemcpyAsync(d_op, openings + c0, n * 96, hipMemcpyHostToDevice, st));
        ZK_HIP(hipMemcpyAsync(d_z, points + c0, n * 32, hipMemcpyHostToDevice, st));
        ZK_HIP(hipMemcpyAsync(d_rr, rr.data(), n * 16, hipMemcpyHostToDevice, st));
        ZK_LAUNCH(s, st, "kzg_combine", k_kzg_combine, dim3(blocks(n, 64)), dim3(64), 0, (const Affine<Fp>*)d_dig, (const KzgLane*)d_op, (const Fr*)d_z,
                  (const uint32_t*)d_rr, n, G, fa.a, fb.a, d_p);
        const XYZZ<Fp>* a_sum = fold_all(s, st, "g1_fold", k_g1_fold, 256, fa, n, 1);
        const XYZZ<Fp>* b_sum = fold_all(s, st, "g1_fold", k_g1_fold, 256, fb, n, 1);
        XYZZ<HFp> sa, sb;
        ZK_HIP(hipMemcpyAsync(&sa, a_sum, 128, hipMemcpyDeviceToHost, st));
        ZK_HIP(hipMemcpyAsync(&sb, b_sum, 128, hipMemcpyDeviceToHost, st));
        ZK_TRY(slot_sync(s, st));
        // e(sum_i lambda_i (C_i - v_i G + z_i H_i), [1]2) e(-sum_i lambda_i H_i, [alpha]2) == 1: two Miller loops whatever n is
        const Affine<HFp> two[2] = {sa.to_affine(), sb.to_affine().neg()};
        ZK_HIP(hipMemcpyAsync(d_two, two, 2 * 64, hipMemcpyHostToDevice, st));
        ZK_TRY(pc.combined(d_two, 2, nullptr, 0, d_g2, n, accepted + c0));
        if (pc.decided) continue;
        // fallback: each opening's own two-pairing check e(T_i, [1]2) e(-H_i, [alpha]2) == 1 (k_kzg_combine left the pairs in d_p)
        ZK_TRY(pc.per_lane(d_p, n, 2, nullptr, 0, d_g2, false, accepted + c0));
    }
    *n_accepted = pc.total;
    return ZK_OK;
}

}  // extern "C"
