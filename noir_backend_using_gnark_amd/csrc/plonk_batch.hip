// Batch PLONK proving: `rows` witnesses against ONE resident key in one call, every proof assembled on the device.
//
// The rounds are the row forms of plonk.hip (ratio_rows_dev, quotient_rows_dev, linearize_rows_dev, open_rows_dev), the transforms ntt_rows_dev and the
// commitments zk_bn254_msm_bases_rows_dev.  What this file adds is what stands between them:
//   round 1        k_gather_lro_rows, k_blind_tail_rows, (copy, inverse transform,) k_bitrev_rows, k_blind_rows
//   Fiat-Shamir    k_pb_transcript, one lane per row and one launch per challenge: gnark-crypto's fiatshamir.Transcript over SHA-256 as FsTranscript
//                  (proofio.hpp) computes it on the host for the single prover, on the verifier's device pieces (fs_dev.hpp, sha256_dev.hpp)
//   two digests    [fh] = [H0] + zeta^(n+2) [H1] + zeta^(2(n+2)) [H2] and, for a key whose digests are known to be consistent,
//                  [lin] = (alpha c_z + lag) [Z] + alpha c_s3 [S3] + l r [Qm] + l [Ql] + r [Qr] + o [Qo] + [Qk]:  k_pb_scalars, k_pb_smul (one scalar
//                  multiplication per lane, the term as blockIdx.y), k_pb_digests -- the pattern of the verifier's k_pv_scalars / k_pv_smul / k_pv_digests
//   Proof.WriteTo  k_plonk_proof_rows, one lane per row
// One row is rows = 1 of the same kernels; pinned challenges replace a transcript launch by a copy.  Per chunk nothing crosses to the host but the finished
// proofs and the verdicts; the host synchronises a fixed number of times per chunk (once in front of every row MSM, which runs on a slot of its own).
#include <string.h>

#include <algorithm>

#include "ctx.hpp"
#include "curve.hpp"
#include "fs_dev.hpp"
#include "host_ff.hpp"
#include "msm.hpp"
#include "multidev.hpp"
#include "ntt.hpp"
#include "plonk_batch.hpp"
#include "proofio.hpp"
#include "scan.hpp"

namespace zkmi {

// ------------------------------------------------------------------------------------------------ round 1
// k_gather_lro with the row as blockIdx.y: row v reads its solution at sol + v * sol_stride and writes l / r / o + v * stride
__global__ void k_gather_lro_rows(const Fr* __restrict__ sol, size_t sol_stride, const uint32_t* __restrict__ xa, const uint32_t* __restrict__ xb,
                                  const uint32_t* __restrict__ xc, uint32_t npub, uint32_t nc, uint32_t n, Fr* __restrict__ l, Fr* __restrict__ r,
                                  Fr* __restrict__ o, size_t stride) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const size_t row = blockIdx.y;
    const Fr* __restrict__ w = sol + row * sol_stride;
    uint32_t ia = 0, ib = 0, ic = 0;
    if (i < npub) ia = i;
    else if (i < npub + nc) { ia = xa[i - npub]; ib = xb[i - npub]; ic = xc[i - npub]; }
    l[row * stride + i] = ld(w + ia);
    r[row * stride + i] = ld(w + ib);
    o[row * stride + i] = ld(w + ic);
}
// The blinders of a matrix of `total` rows of n + 3 elements, `rows` witnesses per polynomial: matrix row j belongs to witness j % rows and polynomial j / rows,
// whose k blinders are bl[9 (j % rows) + first + k (j / rows) ..).  One lane per (matrix row, tail element).
// k_blind_tail: p[n + i] = b_i behind the n values (zero from k on)
__global__ __launch_bounds__(256) void k_blind_tail_rows(Fr* __restrict__ p, size_t stride, uint32_t n, const Fr* __restrict__ bl, uint32_t rows, uint32_t total,
                                                         uint32_t first, uint32_t k) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, j = t >> 2, i = t & 3;
    if (j >= total || i >= 3) return;
    p[(size_t)j * stride + n + i] = i < k ? ld(bl + 9 * (size_t)(j % rows) + first + k * (j / rows) + i) : Fr::zero();
}
// k_blind: p[i] -= b_i, p[n + i] = b_i (zero from k on)
__global__ __launch_bounds__(256) void k_blind_rows(Fr* __restrict__ p, size_t stride, uint32_t n, const Fr* __restrict__ bl, uint32_t rows, uint32_t total,
                                                    uint32_t first, uint32_t k) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, j = t >> 2, i = t & 3;
    if (j >= total || i >= 3) return;
    Fr* q = p + (size_t)j * stride;
    Fr b = Fr::zero();
    if (i < k) {
        b = ld(bl + 9 * (size_t)(j % rows) + first + k * (j / rows) + i);
        q[i] = ld(q + i) - b;
    }
    q[n + i] = b;
}
// BitReverse of the first 2^logn elements of row blockIdx.y, in place (what bit_reverse_dev does behind the single prover's inverse transform)
__global__ __launch_bounds__(256) void k_bitrev_rows(Fr* __restrict__ p, size_t stride, unsigned logn) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (1u << logn)) return;
    const uint32_t j = logn ? __brev(i) >> (32 - logn) : 0;
    if (i >= j) return;
    Fr* q = p + (size_t)blockIdx.y * stride;
    const Fr a = ld(q + i), b = ld(q + j);
    q[i] = b;
    q[j] = a;
}

// ------------------------------------------------------------------------------------------------ Fiat-Shamir, one lane per row
// One challenge of FsTranscript{"gamma", "beta", "alpha", "zeta"} (stages 0 to 3) or kzg.deriveGamma's (stage 4) per launch.  Every item bound is 32 bytes:
//   0  "gamma" || the key's eight digests -- the same for every row: the host hashed its whole blocks (mid after mid_len bytes; tail holds the rest) --, the row's
//      public inputs, [L], [R], [O]
//   1  "beta" || gamma's raw digest          2  "alpha" || beta's raw digest || [Z]          3  "zeta" || alpha's raw digest || [H0], [H1], [H2]
//   4  "gamma" || zeta || [fh], [lin], [L], [R], [O] (the row's) , [S1], [S2] (the key's) || the seven claimed values
// Points are bound as G1Affine.RawBytes() (raw_half), field elements as their 32 canonical big-endian bytes.
struct PbFsArgs {
    int stage;
    uint32_t rows;
    const uint32_t* mid;  // stage 0
    uint64_t mid_len;
    const uint8_t* tail;
    uint32_t tail_len;
    const Fr* pub;        // stage 0: row v's public inputs at pub + v * pub_stride
    size_t pub_stride;
    uint32_t npub;
    const Affine<Fp>* pts;  // point k of row v at pts[v * pt_row + k * pt_step]
    size_t pt_row, pt_step;
    const uint32_t* prev;   // stages 1 to 3: the previous stage's raw digest, 32 bytes per row; stage 4: zeta, one element per row
    const Fr* values;       // stage 4: eight per row as linearize_rows_dev leaves them, the first seven are bound
    Affine<Fp> s1, s2;      // stage 4
    Fr* out;                // the challenge, reduced as fr.SetBytes
    uint32_t* raw;          // the digest's 32 bytes
};
__global__ __launch_bounds__(64) void k_pb_transcript(PbFsArgs A) {
    const size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= A.rows) return;
    const int stage = A.stage;
    Sha256Dev h;
    if (stage == 0) {
        h.resume(A.mid, A.mid_len);
        h.update(A.tail, A.tail_len);
    } else {
        h.reset();
        // "beta", "alpha", "zeta", "gamma"
        const uint64_t name = stage == 1 ? 0x62657461ull : stage == 2 ? 0x616c706861ull : stage == 3 ? 0x7a657461ull : 0x67616d6d61ull;
#pragma unroll 1
        for (int k = (stage == 2 || stage == 4) ? 4 : 3; k >= 0; k--) h.put_byte((uint32_t)(name >> (8 * k)));
    }
    const uint32_t items = stage == 0 ? A.npub + 6 : stage == 1 ? 1 : stage == 2 ? 3 : stage == 3 ? 7 : 22;
#pragma unroll 1
    for (uint32_t j = 0; j < items; j++) {
        uint32_t l[8];
        if (stage >= 1 && stage <= 3 && j == 0) {  // the raw digest the previous challenge was reduced from
#pragma unroll
            for (int k = 0; k < 8; k++) l[7 - k] = __builtin_bswap32(A.prev[8 * v + k]);
        } else if ((stage == 0 && j < A.npub) || (stage == 4 && (j == 0 || j >= 15))) {
            const Fr* src = A.pub + v * A.pub_stride + j;
            if (stage == 4) src = j ? A.values + 8 * v + (j - 15) : (const Fr*)A.prev + v;
            const Fr w = ld(src).from_mont();
#pragma unroll
            for (int k = 0; k < 8; k++) l[k] = w.l[k];
        } else {
            const uint32_t q = stage == 0 ? j - A.npub : j - 1, d = q >> 1;
            Affine<Fp> p = A.s1;  // (not a ?: of references: that would put the points in memory)
            if (stage == 4 && d == 6) p = A.s2;
            if (stage != 4 || d < 5) p = A.pts[v * A.pt_row + d * A.pt_step];
            raw_half(p, (int)(q & 1), l);
        }
        h.put256(l);
    }
    uint32_t d[8];
    h.final(d);
#pragma unroll
    for (int k = 0; k < 8; k++) A.raw[8 * v + k] = __builtin_bswap32(d[k]);
    A.out[v] = fr_from_digest(d);
}

// gamma's common prefix: "gamma" || RawBytes(S1 S2 S3 Ql Qr Qm Qo Qk), its whole blocks compressed on the host
struct PbPrefix {
    uint32_t mid[8];
    uint8_t tail[64];
    uint32_t tail_len = 0;
    uint64_t mid_len = 0;
};
static void fs_prefix(const PlonkPK* P, PbPrefix* out) {
    Sha256 tg;
    tg.update("gamma", 5);
    for (const Affine<HFp>* d : {&P->vk_s[0], &P->vk_s[1], &P->vk_s[2], &P->vk_ql, &P->vk_qr, &P->vk_qm, &P->vk_qo, &P->vk_qk}) {
        uint8_t b[64];
        g1_raw_bytes(*d, b);
        tg.update(b, 64);
    }
    memcpy(out->mid, tg.h, 32);
    memset(out->tail, 0, sizeof out->tail);
    memcpy(out->tail, tg.buf, tg.fill);
    out->tail_len = (uint32_t)tg.fill;
    out->mid_len = tg.len - tg.fill;
}
static Affine<Fp> g1_to_dev(const Affine<HFp>& p) {
    Affine<Fp> r;
    memcpy(&r, &p, sizeof r);
    return r;
}
// d_prefix: a PbPrefix's mid and tail (the first 96 bytes) in device memory
static int transcript_rows_dev(Slot* s, hipStream_t st, const PlonkPK* P, int stage, size_t rows, const PbPrefix& pre, const void* d_prefix, const Fr* pub,
                               size_t pub_stride, const Affine<Fp>* pts, size_t pt_row, size_t pt_step, const void* prev, const Fr* values, Fr* out, uint32_t* raw) {
    PbFsArgs A = {};
    A.stage = stage;
    A.rows = (uint32_t)rows;
    A.mid = (const uint32_t*)d_prefix;
    A.mid_len = pre.mid_len;
    A.tail = (const uint8_t*)d_prefix + 32;
    A.tail_len = pre.tail_len;
    A.pub = pub; A.pub_stride = pub_stride; A.npub = (uint32_t)P->n_public;
    A.pts = pts; A.pt_row = pt_row; A.pt_step = pt_step;
    A.prev = (const uint32_t*)prev;
    A.values = values;
    A.s1 = g1_to_dev(P->vk_s[0]); A.s2 = g1_to_dev(P->vk_s[1]);
    A.out = out; A.raw = raw;
    ZK_LAUNCH(s, st, "plonk_transcript_rows", k_pb_transcript, dim3((unsigned)((rows + 63) / 64)), dim3(64), 0, A);
    return ZK_OK;
}

// ------------------------------------------------------------------------------------------------ the two digests taken by linearity
// sc (columns of `rows`): zeta^(n+2), zeta^(2(n+2)) and, with `lin`, alpha c_z + lag, alpha c_s3, l r -- k_lin_fold_rows' scalars (plonk.hip), one lane per row
__global__ __launch_bounds__(64) void k_pb_scalars(const Fr* __restrict__ values, const Fr* __restrict__ alpha, const Fr* __restrict__ beta, const Fr* __restrict__ gamma,
                                                   const Fr* __restrict__ zeta, uint32_t rows, unsigned logn, Fr card_inv, Fr u, Fr uu, int lin, Fr* __restrict__ sc) {
    const size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= rows) return;
    const Fr z = ld(zeta + v);
    Fr zn = z;
    for (unsigned i = 0; i < logn; i++) zn = zn.sqr();
    const Fr zp = zn * z.sqr();
    sc[v] = zp;
    sc[rows + v] = zp.sqr();
    if (!lin) return;
    const Fr* ev = values + 8 * v;
    const Fr lz = ld(ev + 2), rz = ld(ev + 3), oz = ld(ev + 4), s1z = ld(ev + 5), s2z = ld(ev + 6), zu = ld(ev + 7);
    const Fr al = ld(alpha + v), be = ld(beta + v), ga = ld(gamma + v), bz = be * z;
    const Fr lag = (zn - Fr::one()) * (z - Fr::one()).inv() * al * al * card_inv;  // inv(0) = 0
    const Fr c_s3 = (lz + be * s1z + ga) * (rz + be * s2z + ga) * zu * be;
    const Fr c_z = ((lz + bz + ga) * (rz + bz * u + ga) * (oz + bz * uu + ga)).neg();
    sc[2 * (size_t)rows + v] = c_z * al + lag;
    sc[3 * (size_t)rows + v] = c_s3 * al;
    sc[4 * (size_t)rows + v] = lz * rz;
}
// out[t rows + v] = k P for term t = blockIdx.y: point pts[v * pt_step] (the key's when pt_step == 0), scalar sc[v * sc_step]
struct PbTerm {
    const Affine<Fp>* pts;
    size_t pt_step;
    const Fr* sc;
    size_t sc_step;
};
struct PbTerms { PbTerm t[8]; };
__global__ __launch_bounds__(64) void k_pb_smul(PbTerms T, uint32_t rows, XYZZ<Fp>* __restrict__ out) {
    const size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= rows) return;
    const PbTerm t = T.t[blockIdx.y];
    const Fr k = ld(t.sc + v * t.sc_step).from_mont();
    out[(size_t)blockIdx.y * rows + v] = scalar_mul(t.pts[v * t.pt_step], k.l);
}
// dig[v] = [fh] = terms 0 + 1 + [H0]; with `lin`, dig[rows + v] = [lin] = terms 2 .. 7 + [Qk]; affine, (0, 0) = infinity.  hpts: [H0] [H1] [H2] per row
__global__ __launch_bounds__(64) void k_pb_digests(const Affine<Fp>* __restrict__ hpts, const XYZZ<Fp>* __restrict__ t, Affine<Fp> qk, uint32_t rows, int lin,
                                                   Affine<Fp>* __restrict__ dig) {
    const size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= rows) return;
    XYZZ<Fp> fh = t[v];
    fh.add(t[rows + v]);
    fh.madd(hpts[3 * v]);
    dig[v] = fh.to_affine();
    if (!lin) return;
    XYZZ<Fp> acc = t[2 * (size_t)rows + v];
#pragma unroll 1
    for (int k = 3; k < 8; k++) acc.add(t[(size_t)k * rows + v]);
    acc.madd(qk);
    dig[rows + v] = acc.to_affine();
}

// ------------------------------------------------------------------------------------------------ Proof.WriteTo, one lane per row
// 548 bytes = 137 words at out + 137 v: [L] [R] [O] [Z] [H0] [H1] [H2] [BatchedProof.H] compressed, 00 00 00 07, the seven claimed values, [ZShiftedOpening.H],
// z(omega zeta); all zero where the row's verdict is not.  lro: [L] of every row, then [R], then [O]; hc: three per row
__global__ __launch_bounds__(64) void k_plonk_proof_rows(const uint32_t* __restrict__ lro, const uint32_t* __restrict__ zc, const uint32_t* __restrict__ hc,
                                                         const uint32_t* __restrict__ wc, const uint32_t* __restrict__ zqc, const Fr* __restrict__ values,
                                                         const int* __restrict__ status, uint32_t rows, uint32_t* __restrict__ out) {
    const size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= rows) return;
    uint32_t* o = out + 137 * v;
    if (status[v]) {
#pragma unroll 1
        for (int i = 0; i < 137; i++) o[i] = 0;
        return;
    }
#pragma unroll 1
    for (int k = 0; k < 9; k++) {
        const uint32_t* src = k < 3 ? lro + 8 * ((size_t)k * rows + v) : k == 3 ? zc + 8 * v : k < 7 ? hc + 8 * (3 * v + (k - 4)) : k == 7 ? wc + 8 * v : zqc + 8 * v;
        uint32_t* dst = o + (k < 8 ? 8 * k : 121);
#pragma unroll
        for (int j = 0; j < 8; j++) dst[j] = src[j];
    }
    o[64] = 0x07000000u;  // 00 00 00 07 as a little-endian word
#pragma unroll 1
    for (int k = 0; k < 8; k++) {
        const Fr c = ld(values + 8 * v + k).from_mont();
        uint32_t* dst = o + (k < 7 ? 65 + 8 * k : 129);
#pragma unroll
        for (int j = 0; j < 8; j++) dst[j] = __builtin_bswap32(c.l[7 - j]);
    }
}

// ------------------------------------------------------------------------------------------------ a chunk's workspace and the chunk size
constexpr size_t PB_ARENA = (size_t)1 << 30;
constexpr size_t PB_MAX_ROWS = 16384;  // 4 * rows and 3 * rows are grid dimensions (<= 65535)
struct PbGeom {
    size_t S, Hs;        // row strides: n + 3 for every small polynomial, 3 (n + 2) for the quotient
    size_t phase;        // per row: the largest workspace a round takes (ratio, quotient, round 4, round 5)
    size_t row;          // per row: everything
    size_t fixed;
};
static PbGeom pb_geom(const PlonkPK* P, bool sol_on_device) {
    PbGeom G;
    const size_t n = P->n;
    G.S = n + 3;
    G.Hs = 3 * (n + 2);
    G.phase = std::max(std::max(ratio_row_bytes(n), quot_row_bytes(P)), std::max(open_row_bytes(n + 3, 6, LIN_PT, 0), open_row_bytes(n + 3, 1, 3, n + 3)));
    // solution; l, r, o in both forms; z; h; lin, fh, zquot, the opening quotient; then, rounded up (plan_workspace reserves what is carved: this only picks
    // the chunk), the points, 9 compressed digests, 10 transcript words, the values, 5 scalars, 8 terms, the blinders, the verdict and the proof
    G.row = ((sol_on_device ? 0 : P->n_vars) + 6 * G.S + G.S + G.Hs + 4 * G.S) * sizeof(Fr) + G.phase + 11 * 64 + 9 * 32 + 10 * 32 + 8 * 32 + 5 * 32 + 8 * 128 + 9 * 32 +
            4 + 548 + 64;
    G.fixed = 64 * 256 + 65536;  // alignment of the carved arrays, the prefix, the key's points, the rounds' own small allocations
    return G;
}
static int pb_chunk(const PlonkPK* P, bool sol_on_device, size_t cap, size_t* chunk, int* batched) {
    size_t msm_chunk = 1;
    int b = 0;
    if (md_is_composite(P->srs)) {  // not on one device entry: row after row through the single prover
        *chunk = 1;
        *batched = 0;
        return ZK_OK;
    }
    ZK_TRY(zk_bn254_msm_rows_info(P->srs, P->n + 3, 0, &msm_chunk, &b));
    const PbGeom G = pb_geom(P, sol_on_device);
    size_t r = std::max<size_t>(1, (PB_ARENA - G.fixed) / G.row);
    r = std::min(r, PB_MAX_ROWS);
    if (b) r = std::min(r, std::max<size_t>(1, msm_chunk / 3));  // l, r, o and the quotient's thirds are 3 r rows of one row MSM
    if (cap) r = std::min(r, cap);
    *chunk = r;
    *batched = b;
    return ZK_OK;
}

struct PbWs {
    Fr *sol, *lag, *can, *z, *h, *lin, *fh, *zquot, *q, *values, *sc, *ch, *bl;
    Affine<Fp> *pts, *kpts;  // pts: prove_chunk says;  kpts: S3 Qm Ql Qr Qo
    XYZZ<Fp>* terms;
    uint32_t *cmp, *raw, *proofs;  // cmp: the compressed [L] | [R] | [O] (columns of R), [Z], [BatchedProof.H], [ZShiftedOpening.H], then [H0] [H1] [H2] per row
    int* status;
    uint8_t* prefix;
};

// the proofs of rows [first, first + R) of the call
static int prove_chunk(Slot* s, hipStream_t st, const PlonkPK* P, const PbWs& W, const PbGeom& G, size_t cap, size_t mark, const PbPrefix& pre, const Domain* d0,
                       const void* solutions, size_t sol_stride, int on_device, const zk_fr* blinders, const zk_fr* challenges, size_t first, size_t R,
                       bool lin_direct, uint8_t* proofs_out, int* status_out) {
    const size_t n = P->n, S = G.S, npub = P->n_public;
    const unsigned logn = P->logn;
    const Fr* sol = W.sol;
    size_t stride = P->n_vars;
    if (on_device) {
        sol = (const Fr*)solutions + first * sol_stride;
        stride = sol_stride;
    } else if (R == 1 || sol_stride == P->n_vars) {  // (one row's stride may be anything)
        ZK_HIP(hipMemcpyAsync(W.sol, (const Fr*)solutions + first * sol_stride, R * P->n_vars * sizeof(Fr), hipMemcpyHostToDevice, st));
    } else {
        ZK_HIP(hipMemcpy2DAsync(W.sol, P->n_vars * sizeof(Fr), (const Fr*)solutions + first * sol_stride, sol_stride * sizeof(Fr), P->n_vars * sizeof(Fr), R,
                                hipMemcpyHostToDevice, st));
    }
    ZK_HIP(hipMemcpyAsync(W.bl, blinders + 9 * first, 9 * R * sizeof(Fr), hipMemcpyHostToDevice, st));
    Fr *gamma = W.ch, *beta = W.ch + cap, *alpha = W.ch + 2 * cap, *zeta = W.ch + 3 * cap, *kg = W.ch + 4 * cap;
    // [fh] [lin] [L] [R] [O] are columns of R (what one commitment of 3 R rows writes; kzg's challenge binds the five), [Z] and the [H] triples start at fixed places
    Affine<Fp> *p_dig = W.pts, *p_lro = W.pts + 2 * R, *p_z = W.pts + 5 * cap, *p_h = W.pts + 6 * cap;
    uint32_t *c_lro = W.cmp, *c_z = W.cmp + 8 * 3 * cap, *c_w = W.cmp + 8 * 4 * cap, *c_zq = W.cmp + 8 * 5 * cap, *c_h = W.cmp + 8 * 6 * cap;
    // challenge c of the chunk: the transcript's launch, or the caller's pinned column
    auto challenge = [&](int c, const Affine<Fp>* pts, size_t pt_row, size_t pt_step) -> int {
        if (challenges)
            return hipMemcpy2DAsync(W.ch + c * cap, sizeof(Fr), challenges + 5 * first + c, 5 * sizeof(Fr), sizeof(Fr), R, hipMemcpyHostToDevice, st) == hipSuccess
                       ? ZK_OK
                       : set_err(ZK_ERR_HIP, "copy of the pinned challenges failed");
        const void* prev = c == 4 ? (const void*)zeta : c ? (const void*)(W.raw + 8 * (c - 1) * cap) : nullptr;
        return transcript_rows_dev(s, st, P, c, R, pre, W.prefix, sol, stride, pts, pt_row, pt_step, prev, W.values, W.ch + c * cap, W.raw + 8 * c * cap);
    };
    auto commit = [&](uint64_t bases, const Fr* rows_, size_t row_stride, size_t len, size_t cnt, uint32_t flags, void* out, void* compressed) -> int {
        ZK_TRY(slot_sync(s, st));  // the row MSM runs on a slot of its own
        return zk_bn254_msm_bases_rows_dev(bases, 0, rows_, row_stride, len, cnt, &kMont, flags, out, compressed);
    };

    // ---- round 1: l, r, o of every row (polynomial-major: the l rows, the r rows, the o rows), their blinders behind the values, the canonical forms
    Fr *l_lag = W.lag, *r_lag = W.lag + R * S, *o_lag = W.lag + 2 * R * S;
    Fr *l = W.can, *r = W.can + R * S, *o = W.can + 2 * R * S;
    const unsigned R3 = (unsigned)(3 * R);
    ZK_LAUNCH(s, st, "plonk_gather_lro_rows", k_gather_lro_rows, dim3(grid_of(n), (unsigned)R), dim3(256), 0, sol, stride, (const uint32_t*)P->xa,
              (const uint32_t*)P->xb, (const uint32_t*)P->xc, (uint32_t)npub, (uint32_t)P->n_constraints, (uint32_t)n, l_lag, r_lag, o_lag, S);
    ZK_LAUNCH(s, st, "plonk_blind_tail_rows", k_blind_tail_rows, dim3(grid_of(4 * (size_t)R3)), dim3(256), 0, W.lag, S, (uint32_t)n, (const Fr*)W.bl, (uint32_t)R, R3, 0u,
              2u);
    ZK_HIP(hipMemcpyAsync(W.can, W.lag, (size_t)R3 * S * sizeof(Fr), hipMemcpyDeviceToDevice, st));
    ZK_TRY(ntt_rows_dev(s, st, W.can, logn, R3, S, 1, ZK_DIF, 0));
    ZK_LAUNCH(s, st, "plonk_bitrev_rows", k_bitrev_rows, dim3(grid_of(n), R3), dim3(256), 0, W.can, S, logn);
    ZK_LAUNCH(s, st, "plonk_blind_rows", k_blind_rows, dim3(grid_of(4 * (size_t)R3)), dim3(256), 0, W.can, S, (uint32_t)n, (const Fr*)W.bl, (uint32_t)R, R3, 0u, 2u);
    if (P->lag_srs) ZK_TRY(commit(P->lag_srs, W.lag, S, n + 2, R3, ZK_MSM_ROWS_SPARSE, p_lro, c_lro));  // from the values: the same points
    else ZK_TRY(commit(P->srs, W.can, S, n + 2, R3, 0, p_lro, c_lro));

    // ---- gamma, beta; round 2
    ZK_TRY(challenge(0, p_lro, 1, R));
    ZK_TRY(challenge(1, nullptr, 0, 0));
    {
        s->arena_off = mark;
        RatioWs RW;
        ZK_TRY(ratio_ws_take(s, n, R, false, &RW));
        ZK_TRY(ratio_rows_dev(s, st, d0, (const Fr*)P->sig, l_lag, r_lag, o_lag, S, R, beta, gamma, W.z, S, RW));
    }
    ZK_TRY(ntt_rows_dev(s, st, W.z, logn, R, S, 1, ZK_DIF, 0));
    ZK_LAUNCH(s, st, "plonk_bitrev_rows", k_bitrev_rows, dim3(grid_of(n), (unsigned)R), dim3(256), 0, W.z, S, logn);
    ZK_LAUNCH(s, st, "plonk_blind_rows", k_blind_rows, dim3(grid_of(4 * R)), dim3(256), 0, W.z, S, (uint32_t)n, (const Fr*)W.bl, (uint32_t)R, (uint32_t)R, 6u, 3u);
    ZK_TRY(commit(P->srs, W.z, S, n + 3, R, 0, p_z, c_z));
    ZK_TRY(challenge(2, p_z, 1, 0));

    // ---- round 3: the quotient and the verdict
    {
        s->arena_off = mark;
        Fr* ws = (Fr*)s->alloc(R * quot_row_bytes(P));
        if (!ws) return set_err(ZK_ERR_HIP, "plonk batch: quotient workspace");
        ZK_TRY(quotient_rows_dev(s, st, P, l, r, o, W.z, S, sol, stride, R, alpha, beta, gamma, W.h, G.Hs, W.status, ws, R));
    }
    ZK_TRY(commit(P->srs, W.h, n + 2, n + 2, R3, 0, p_h, c_h));
    ZK_TRY(challenge(3, p_h, 3, 1));

    // ---- round 4: the evaluations, the opening of z at omega zeta, the linearised polynomial and the folded quotient with their digests
    s->arena_off = mark;
    ZK_TRY(linearize_rows_dev(s, st, P, l, r, o, W.z, S, W.h, G.Hs, R, alpha, beta, gamma, zeta, W.values, W.zquot, W.lin, W.fh, S));
    {
        const HFr uu = P->u * P->u;
        ZK_LAUNCH(s, st, "plonk_digest_scalars_rows", k_pb_scalars, dim3((unsigned)((R + 63) / 64)), dim3(64), 0, (const Fr*)W.values, (const Fr*)alpha, (const Fr*)beta,
                  (const Fr*)gamma, (const Fr*)zeta, (uint32_t)R, logn, to_dev(P->card_inv), to_dev(P->u), to_dev(uu), (int)lin_direct, W.sc);
        PbTerms T = {};
        T.t[0] = {p_h + 1, 3, W.sc, 1};
        T.t[1] = {p_h + 2, 3, W.sc + R, 1};
        T.t[2] = {p_z, 1, W.sc + 2 * R, 1};
        T.t[3] = {W.kpts + 0, 0, W.sc + 3 * R, 1};
        T.t[4] = {W.kpts + 1, 0, W.sc + 4 * R, 1};
        T.t[5] = {W.kpts + 2, 0, W.values + 2, 8};
        T.t[6] = {W.kpts + 3, 0, W.values + 3, 8};
        T.t[7] = {W.kpts + 4, 0, W.values + 4, 8};
        ZK_LAUNCH(s, st, "plonk_digest_smul_rows", k_pb_smul, dim3((unsigned)((R + 63) / 64), lin_direct ? 8 : 2), dim3(64), 0, T, (uint32_t)R, W.terms);
        ZK_LAUNCH(s, st, "plonk_digest_sum_rows", k_pb_digests, dim3((unsigned)((R + 63) / 64)), dim3(64), 0, (const Affine<Fp>*)p_h, (const XYZZ<Fp>*)W.terms,
                  g1_to_dev(P->vk_qk), (uint32_t)R, (int)lin_direct, p_dig);
    }
    ZK_TRY(commit(P->srs, W.zquot, S, n + 2, R, ZK_MSM_ROWS_NO_POINTS, nullptr, c_zq));
    if (!lin_direct) ZK_TRY(commit(P->srs, W.lin, S, n + 3, R, 0, p_dig + R, nullptr));

    // ---- round 5: kzg's folding challenge, the folded opening at zeta
    ZK_TRY(challenge(4, p_dig, 1, R));
    s->arena_off = mark;
    ZK_TRY(open_rows_dev(s, st, P, W.fh, W.lin, l, r, o, S, R, zeta, kg, W.q, S, W.values + 8 * cap));
    ZK_TRY(commit(P->srs, W.q, S, n + 2, R, ZK_MSM_ROWS_NO_POINTS, nullptr, c_w));

    // ---- Proof.WriteTo; the only bytes that cross to the host
    ZK_LAUNCH(s, st, "plonk_proof_rows", k_plonk_proof_rows, dim3((unsigned)((R + 63) / 64)), dim3(64), 0, (const uint32_t*)c_lro, (const uint32_t*)c_z, (const uint32_t*)c_h,
              (const uint32_t*)c_w, (const uint32_t*)c_zq, (const Fr*)W.values, (const int*)W.status, (uint32_t)R, W.proofs);
    ZK_HIP(hipMemcpyAsync(proofs_out + 548 * first, W.proofs, 548 * R, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipMemcpyAsync(status_out + first, W.status, R * sizeof(int), hipMemcpyDeviceToHost, st));
    return slot_sync(s, st);
}

}  // namespace zkmi

using namespace zkmi;

extern "C" {

int zk_bn254_plonk_prove_batch_info(uint64_t pk_handle, size_t* chunk_rows, int* commits_batched, int* lin_by_linearity) {
    PlonkPK* P;
    std::shared_ptr<std::shared_mutex> live;
    std::shared_lock<std::shared_mutex> alive;
    ZK_TRY(live_key(pk_handle, &P, &live, &alive));
    size_t chunk = 1;
    int batched = 0;
    ZK_TRY(pb_chunk(P, true, 0, &chunk, &batched));
    if (chunk_rows) *chunk_rows = chunk;
    if (commits_batched) *commits_batched = batched;
    if (lin_by_linearity) *lin_by_linearity = P->vk_consistent ? 1 : 0;
    return ZK_OK;
}

int zk_bn254_plonk_challenges_batch_dev(uint64_t pk_handle, int stage, size_t rows, const void* d_pub, size_t pub_stride, const void* d_points, const void* d_prev,
                                        const void* d_values, void* d_out, void* stream) {
    if (stage < 0 || stage > 4) return set_err(ZK_ERR_ARG, "stage = %d is not one of the five challenges 0 .. 4", stage);
    if (!d_out || (stage != 1 && !d_points) || (stage != 0 && !d_prev) || (stage == 4 && !d_values)) return set_err(ZK_ERR_ARG, "null pointer");
    if (rows == 0) return ZK_OK;
    PlonkPK* P;
    std::shared_ptr<std::shared_mutex> live;
    std::shared_lock<std::shared_mutex> alive;
    ZK_TRY(live_key(pk_handle, &P, &live, &alive));
    const size_t npub = P->n_public;
    if (stage == 0 && npub && !d_pub) return set_err(ZK_ERR_ARG, "null pointer");
    if (stage == 0 && npub && rows > 1 && pub_stride < npub) return set_err(ZK_ERR_ARG, "pub_stride = %zu is below the %zu public inputs", pub_stride, npub);
    {
        const size_t npts = stage == 0 || stage == 3 ? 3 : stage == 2 ? 1 : stage == 4 ? 5 : 0, ob = 2 * rows * 32;
        const void* in[4] = {stage == 0 && npub ? d_pub : nullptr, d_points, d_prev, d_values};
        const size_t ib[4] = {stage == 0 && npub ? rows_span(rows, pub_stride, npub) : 0, rows * npts * 64, stage ? rows * 32 : 0, stage == 4 ? rows * 8 * 32 : 0};
        for (int k = 0; k < 4; k++)
            if (spans_overlap(d_out, ob, in[k], ib[k])) return set_err(ZK_ERR_ARG, "d_out overlaps an input");
    }
    ZK_ON_ENTRY_OF(pk_handle);
    SlotGuard g;
    ZK_TRY(acquire_slot(&g.s));
    hipStream_t st = stream ? (hipStream_t)stream : g.s->stream;
    PbPrefix pre;
    fs_prefix(P, &pre);
    ZK_TRY(g.s->reserve(4096));
    void* d_prefix = g.s->alloc(96);
    if (!d_prefix) return set_err(ZK_ERR_HIP, "challenges: workspace");
    ZK_HIP(hipMemcpyAsync(d_prefix, &pre, 96, hipMemcpyHostToDevice, st));
    const size_t npts = stage == 0 || stage == 3 ? 3 : stage == 4 ? 5 : 1;
    ZK_TRY(transcript_rows_dev(g.s, st, P, stage, rows, pre, d_prefix, (const Fr*)d_pub, pub_stride, (const Affine<Fp>*)d_points, npts, 1, d_prev, (const Fr*)d_values,
                               (Fr*)d_out, (uint32_t*)((Fr*)d_out + rows)));
    return slot_sync(g.s, st);  // the prefix lives in the slot's arena
}

int zk_bn254_plonk_prove_batch(uint64_t pk_handle, const void* solutions, size_t n_vars, size_t sol_stride, size_t rows, int on_device, const zk_fr* blinders,
                               const zk_fr* challenges, size_t chunk_rows, uint8_t* proofs_out, int* status_out) {
    if (!solutions || !blinders || !proofs_out || !status_out) return set_err(ZK_ERR_ARG, "null pointer");
    if (rows == 0) return ZK_OK;
    PlonkPK* P;
    std::shared_ptr<std::shared_mutex> live;
    std::shared_lock<std::shared_mutex> alive;
    ZK_TRY(live_key(pk_handle, &P, &live, &alive));
    if (n_vars != P->n_vars) return set_err(ZK_ERR_LEN, "len(solution) = %zu != %zu variables of the constraint system", n_vars, P->n_vars);
    if (rows > 1 && sol_stride < n_vars) return set_err(ZK_ERR_ARG, "sol_stride = %zu is below the %zu variables of a row", sol_stride, n_vars);
    const size_t n = P->n, N4 = P->N4;
    if (3 * (n + 2) > N4) return set_err(ZK_ERR_ARG, "a domain of %zu rows has no quotient of 3 (n + 2) coefficients on %zu points", n, N4);
    {
        const size_t pb = rows * 548, sb = rows * sizeof(int);
        const void* in[3] = {blinders, challenges, on_device ? nullptr : solutions};
        const size_t ib[3] = {rows * 9 * sizeof(Fr), challenges ? rows * 5 * sizeof(Fr) : 0, on_device ? 0 : rows_span(rows, sol_stride, n_vars)};
        for (int k = 0; k < 3; k++)
            if (spans_overlap(proofs_out, pb, in[k], ib[k]) || spans_overlap(status_out, sb, in[k], ib[k])) return set_err(ZK_ERR_ARG, "proofs_out or status_out overlaps an input");
        if (spans_overlap(proofs_out, pb, status_out, sb)) return set_err(ZK_ERR_ARG, "proofs_out overlaps status_out");
    }
    if (md_is_composite(P->srs)) {  // the key's bases are not on one device entry: the rows go through the single prover (which takes the key's per-proof mutex)
        alive.unlock();
        for (size_t v = 0; v < rows; v++) {
            const int rc = zk_bn254_plonk_prove(pk_handle, (const Fr*)solutions + v * sol_stride, n_vars, on_device, blinders + 9 * v, challenges ? challenges + 5 * v : nullptr,
                                                proofs_out + 548 * v);
            if (rc != ZK_OK && rc != ZK_ERR_ARG) return rc;
            status_out[v] = rc == ZK_OK ? 0 : 1;
            if (rc != ZK_OK) memset(proofs_out + 548 * v, 0, 548);
        }
        return ZK_OK;
    }
    ZK_ON_ENTRY_OF(pk_handle);
    size_t cap = 1;
    int batched = 0;
    ZK_TRY(pb_chunk(P, on_device != 0, chunk_rows, &cap, &batched));
    cap = std::min(cap, rows);
    SlotGuard g;
    ZK_TRY(acquire_slot(&g.s));
    Slot* s = g.s;
    hipStream_t st = s->stream;
    Domain *d0, *d1;
    ZK_TRY(get_domain(s, st, P->logn, DOM_TW | DOM_TW_INV, &d0));  // every table the transforms ask for, before the arena is carved
    ZK_TRY(get_domain(s, st, P->logN4, DOM_TW | DOM_TW_INV | DOM_COSET | DOM_COSET_INV_N, &d1));
    const PbGeom G = pb_geom(P, on_device != 0);
    PbWs W = {};
    ZK_TRY(plan_workspace(s, "plonk_prove_batch", [&](ArenaPlan& p) {
        if (!on_device) p.take(cap * n_vars, W.sol);
        p.take(3 * cap * G.S, W.lag, W.can);
        p.take(cap * G.S, W.z, W.lin, W.fh, W.zquot, W.q);
        p.take(cap * G.Hs, W.h);
        p.take(9 * cap, W.values, W.bl);  // eight per row and the folded opening's value behind them
        p.take(5 * cap, W.sc, W.ch);
        p.take(9 * cap, W.pts);
        p.take(5, W.kpts);
        p.take(8 * cap, W.terms);
        p.take(8 * 9 * cap, W.cmp);
        p.take(8 * 5 * cap, W.raw);
        p.take(137 * cap, W.proofs);
        p.take(cap, W.status);
        p.take(96, W.prefix);
        p.later(cap * G.phase + 16 * 256);
    }));
    const size_t mark = s->arena_off;
    PbPrefix pre;
    fs_prefix(P, &pre);
    ZK_HIP(hipMemcpyAsync(W.prefix, &pre, 96, hipMemcpyHostToDevice, st));
    const Affine<HFp> kp[5] = {P->vk_s[2], P->vk_qm, P->vk_ql, P->vk_qr, P->vk_qo};
    ZK_HIP(hipMemcpyAsync(W.kpts, kp, sizeof kp, hipMemcpyHostToDevice, st));
    const bool lin_direct = P->vk_consistent;  // read once: a single proof in flight may set it meanwhile, and either way gives the same bytes
    int rc = ZK_OK;
    for (size_t first = 0; first < rows && rc == ZK_OK; first += cap)
        rc = prove_chunk(s, st, P, W, G, cap, mark, pre, d0, solutions, sol_stride, on_device, blinders, challenges, first, std::min(cap, rows - first), lin_direct,
                         proofs_out, status_out);
    if (rc != ZK_OK) (void)hipStreamSynchronize(st);
    return rc;
}

}  // extern "C"
