// PLONK setup and prove on gfx950: gnark v0.8.0 `plonk.Setup` / `plonk.Prove` (internal/backend/bn254/plonk/setup.go, prove.go; pinned at
// /root/reference/gnark_backend_ffi/go.mod:23) -- the reference's only LIVE prove path: PlonkProveWithPK (gnark_backend_ffi/main.go:24-37)
// -> plonk.Prove at backend/plonk/plonk.go:67, plonk.Setup at backend/plonk/plonk.go:21, over the gates the reference emits per ACIR
// arithmetic opcode (backend/plonk/sparse_r1cs.go:44-107: qL*xa + qR*xb + qO*xc + qM*xa*xb + qK = 0).
//
//   Prove, from the solver's output (the values of all variables) onwards  [UPSTREAM-RECALL for the step order]:
//     l, r, o        evaluateLROSmallDomain (gather), FFTInverse -> canonical, Blind(1), kzg.Commit x3           -> gamma, beta
//     z              iop.BuildRatioCopyConstraint: per-row products, batch inversion, prefix product; FFTInverse, Blind(2), Commit -> alpha
//     h              every polynomial on the coset of the big domain (4n): 5 coset FFTs per proof (the key's 9 are cached at setup),
//                    one fused pointwise kernel (gate + alpha * ordering + alpha^2 * (z-1) L1) / (X^n - 1), coset FFTInverse, Commit x3 -> zeta
//     openings       evaluations at zeta / omega*zeta (chunked Horner + block scans), kzg.Open of z (synthetic division as a suffix scan),
//                    linearised polynomial, folded quotient, kzg.BatchOpenSinglePoint (fold, divide, commit)
//   Everything above is device work -- NTTs (ntt.hip), MSMs over the resident SRS with its window tables (msm.hip) and the kernels
//   below -- except the SHA-256 Fiat-Shamir transcript and three G1 scalar multiplications, which stay on the host like upstream.
//   The prover's randomness (9 blinding scalars) is an input; the challenges are derived as upstream does or pinned by the caller.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <functional>
#include <memory>
#include <shared_mutex>
#include <thread>
#include <vector>

#include "ctx.hpp"
#include "curve.hpp"
#include "ff29.hpp"
#include "host_ff.hpp"
#include "msm.hpp"
#include "keyio.hpp"
#include "lagrange.hpp"
#include "multidev.hpp"
#include "ntt.hpp"
#include "plonk_batch.hpp"
#include "proofio.hpp"
#include "scan.hpp"
#include "text_host.hpp"

namespace zkmi {

__device__ __forceinline__ unsigned brev(unsigned i, unsigned logn) { return logn ? (__brev(i) >> (32 - logn)) : 0; }

// ------------------------------------------------------------------------------------------------ small kernels
// evaluateLROSmallDomain: placeholders (l = public input, r = o = solution[0]), gates, padding (all solution[0])
__global__ void k_gather_lro(const Fr* __restrict__ sol, const uint32_t* __restrict__ xa, const uint32_t* __restrict__ xb, const uint32_t* __restrict__ xc,
                             uint32_t npub, uint32_t nc, uint32_t n, Fr* __restrict__ l, Fr* __restrict__ r, Fr* __restrict__ o) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t ia = 0, ib = 0, ic = 0;
    if (i < npub) ia = i;
    else if (i < npub + nc) { ia = xa[i - npub]; ib = xb[i - npub]; ic = xc[i - npub]; }
    l[i] = ld(sol + ia);
    r[i] = ld(sol + ib);
    o[i] = ld(sol + ic);
}
// Lagrange form of a selector on the small domain: [first x npub | coefficients of the gates | 0 ...]
__global__ void k_place_selector(Fr* __restrict__ dst, const Fr* __restrict__ src, uint32_t npub, uint32_t nc, uint32_t n, Fr first) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Fr v = Fr::zero();
    if (i < npub) v = first;
    else if (i < npub + nc) v = ld(src + (i - npub));
    dst[i] = v;
}
__global__ void k_fill(Fr* dst, size_t n, Fr v) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = v;
}
// omega^k from the domain's half table (w^i, i < n/2): w^(k + n/2) = -w^k
__device__ __forceinline__ Fr omega_pow(const Fr* __restrict__ tw, uint32_t k, uint32_t n) {
    uint32_t h = n >> 1;
    if (k < h) return ld(tw + k);
    Fr v = ld(tw + (k - h));
    return Fr::zero() - v;
}
// S_j in Lagrange form: sigma[idx] = id(perm[idx]), id(p) = u^(p / n) * omega^(p mod n)  (setup.go ccomputePermutationPolynomials)
__global__ void k_sigma_lagrange(const uint32_t* __restrict__ perm, const Fr* __restrict__ tw, uint32_t n, Fr u, Fr uu, Fr* __restrict__ out) {
    uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= 3 * n) return;
    uint32_t p = perm[idx], j = p / n, k = p - j * n;
    Fr w = omega_pow(tw, k, n);
    if (j == 1) w = w * u;
    else if (j == 2) w = w * uu;
    out[idx] = w;
}
// rows of the copy-constraint ratio (iop.BuildRatioCopyConstraint): num_i = prod_j (w_j(i) + beta * u^j * omega^i + gamma),
// den_i = prod_j (w_j(i) + beta * sigma_j(i) + gamma)
__global__ void k_z_terms(const Fr* __restrict__ l, const Fr* __restrict__ r, const Fr* __restrict__ o, const Fr* __restrict__ sig, const Fr* __restrict__ tw,
                          uint32_t n, Fr beta, Fr beta_u, Fr beta_uu, Fr gamma, Fr* __restrict__ num, Fr* __restrict__ den) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Fr lv = ld(l + i) + gamma, rv = ld(r + i) + gamma, ov = ld(o + i) + gamma;
    Fr w = omega_pow(tw, i, n);
    num[i] = (lv + beta * w) * (rv + beta_u * w) * (ov + beta_uu * w);
    den[i] = (lv + beta * ld(sig + i)) * (rv + beta * ld(sig + n + i)) * (ov + beta * ld(sig + 2 * (size_t)n + i));
}
// qk completed with the public inputs, on the big coset, WITHOUT transforming it per proof: completed qk = qk + sum_i d_i L_i with d_i = w_i - LQk[i] (the public
// rows), and L_i(x) = L_0(x w^-i): on the coset x_j = g W^j (w = W^rho, rho = 4 or 8) that is the key's L_0 table read rho i places earlier.  Tables are in bit-reversed layout:
// entry p belongs to j = bitrev(p).  Linear and exact, hence the same values as FFT(coset)(canonical(LQk with the public inputs)) -- for any input.
constexpr uint32_t PLONK_PI_DIRECT_MAX = 32;
__global__ __launch_bounds__(256) void k_qk_coset(const Fr* __restrict__ e_cqk, const Fr* __restrict__ e_l1, const Fr* __restrict__ sol, const Fr* __restrict__ lqk,
                                                  uint32_t npub, unsigned logN4, unsigned log_rho, Fr* __restrict__ out) {
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t N4 = (size_t)1 << logN4;
    if (p >= N4) return;
    const uint32_t j = __brev((uint32_t)p) >> (32 - logN4);
    Fr v = ld(e_cqk + p);
    for (uint32_t i = 0; i < npub; i++) {
        const Fr d = ld(sol + i) - ld(lqk + i);
        const uint32_t q = __brev((j - (i << log_rho)) & (uint32_t)(N4 - 1)) >> (32 - logN4);  // w = W^rho, rho = N4 / n
        v = v + d * ld(e_l1 + q);
    }
    out[p] = v;
}

// fr.BatchInvert: a[i] <- 1 / a[i] (0 stays 0); BINV_K elements per lane (strided, coalesced) share one Fermat inversion (~380 products, paid per
// WAVE whatever the lanes do): 3 + 380 / BINV_K products per element.  The prefix products of the forward sweep go through `scratch` (n elements, 160 B of
// traffic per element in all) instead of registers, which is what lets BINV_K be 32 (8 in registers: 1.9 ms at 2^22 elements; 32: see DESIGN 3.8).
constexpr int BINV_K = 32;
__global__ __launch_bounds__(256) void k_batch_inverse(Fr* __restrict__ a, size_t n, Fr* __restrict__ scratch) {
    const size_t T = (size_t)gridDim.x * blockDim.x, g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    Fr acc = Fr::one();
    for (int k = 0; k < BINV_K; k++) {
        const size_t i = g + k * T;
        if (i >= n) break;
        Fr v = ld(a + i);
        if (v.is_zero()) v = Fr::one();  // handled on the way back
        scratch[i] = acc;
        acc = acc * v;
    }
    Fr inv = acc.inv();
    for (int k = BINV_K - 1; k >= 0; k--) {
        const size_t i = g + k * T;
        if (i >= n) continue;
        const Fr v = ld(a + i);
        if (v.is_zero()) continue;  // a zero stays a zero and took no part in the product
        a[i] = inv * ld(scratch + i);
        inv = inv * v;
    }
}

// ------------------------------------------------------------------------------------------------ row form of the ratio (ratio_rows_dev below)
// The ROW as a grid dimension: R witnesses of one domain, every row with its own challenges.  num / den of a chunk of rows are ONE flat array (row v at v * n),
// so k_batch_inverse serves all rows in one launch as it is.  One row -- the single prover's Z -- is R = 1 of the product-scan kernels.
// omega^k as omega_pow, also for the domain of one element (whose half table holds omega^0 alone)
__device__ __forceinline__ Fr omega_pow_any(const Fr* __restrict__ tw, uint32_t k, uint32_t n) { return n > 1 ? omega_pow(tw, k, n) : Fr::one(); }
// k_sigma_lagrange for a caller's permutation: an entry >= 3n raises bit 8 of *status (and counts as 0), as k_perm_from_be does it
__global__ void k_sigma_lagrange_checked(const uint32_t* __restrict__ perm, const Fr* __restrict__ tw, uint32_t n, Fr u, Fr uu, Fr* __restrict__ out,
                                         int* __restrict__ status) {
    size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= 3 * (size_t)n) return;
    uint32_t p = perm[idx];
    if (p >= 3 * (size_t)n) { atomicOr(status, 8); p = 0; }
    uint32_t j = p / n, k = p - j * n;
    Fr w = omega_pow_any(tw, k, n);
    if (j == 1) w = w * u;
    else if (j == 2) w = w * uu;
    out[idx] = w;
}
// k_z_terms, row blockIdx.y: wires at l / r / o + row * in_stride, challenges beta[row], gamma[row].  beta u omega^i is formed as u (beta omega^i): the
// three products of k_z_terms, with u and u^2 as the launch's constants instead of beta u and beta u^2
__global__ void k_z_terms_rows(const Fr* __restrict__ l, const Fr* __restrict__ r, const Fr* __restrict__ o, size_t in_stride, const Fr* __restrict__ sig,
                               const Fr* __restrict__ tw, uint32_t n, const Fr* __restrict__ beta_v, const Fr* __restrict__ gamma_v, Fr u, Fr uu,
                               Fr* __restrict__ num, Fr* __restrict__ den) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const size_t row = blockIdx.y, in = row * in_stride + i, out = row * n + i;
    const Fr beta = ld(beta_v + row), gamma = ld(gamma_v + row);
    Fr lv = ld(l + in) + gamma, rv = ld(r + in) + gamma, ov = ld(o + in) + gamma;
    Fr w = beta * omega_pow_any(tw, i, n);
    num[out] = (lv + w) * (rv + u * w) * (ov + uu * w);
    den[out] = (lv + beta * ld(sig + i)) * (rv + beta * ld(sig + n + i)) * (ov + beta * ld(sig + 2 * (size_t)n + i));
}
// Exclusive prefix product z[0] = 1, z[i+1] = z[i] * num[i] * dinv[i] (the rolling products + ratio of BuildRatioCopyConstraint), K consecutive elements per lane.
// pass 1: lane totals, workgroup-level scan; pass 2: one workgroup per row scans the row's workgroup totals; pass 3: apply.
// The workgroup-level scan: inclusive product scan of one value per lane over a workgroup of 256 (Hillis-Steele in LDS); the caller's lane gets its
// EXCLUSIVE prefix, *total (lane 255's inclusive value) is valid in lane 255
__device__ __forceinline__ Fr pscan_wg256(Fr* sh, Fr tot, Fr* total) {
    sh[threadIdx.x] = tot;
    __syncthreads();
    Fr inc = tot;
    for (unsigned d = 1; d < 256; d <<= 1) {
        Fr o = threadIdx.x >= d ? sh[threadIdx.x - d] : Fr::one();
        __syncthreads();
        inc = inc * o;
        sh[threadIdx.x] = inc;
        __syncthreads();
    }
    *total = inc;
    return threadIdx.x ? sh[threadIdx.x - 1] : Fr::one();
}
// pass 1, row blockIdx.y: num / dinv rows n apart, lane prefixes nb * 256 apart, block totals nb apart (nb = gridDim.x)
__global__ __launch_bounds__(256) void k_pscan_local_rows(const Fr* __restrict__ num, const Fr* __restrict__ dinv, uint32_t n, uint32_t K, Fr* __restrict__ texcl,
                                                          Fr* __restrict__ btot) {
    __shared__ Fr sh[256];
    const size_t row = blockIdx.y, gt = (size_t)blockIdx.x * 256 + threadIdx.x, base = gt * K;
    num += row * n;
    dinv += row * n;
    Fr tot = Fr::one();
    for (uint32_t k = 0; k < K; k++) {
        size_t i = base + k;
        if (i < n) tot = tot * (ld(num + i) * ld(dinv + i));
    }
    Fr inc;
    const Fr excl = pscan_wg256(sh, tot, &inc);
    texcl[row * gridDim.x * 256 + gt] = excl;
    if (threadIdx.x == 255) btot[row * gridDim.x + blockIdx.x] = inc;
}
// pass 2, one workgroup per row: row blockIdx.x's nb block totals in place, btot[b] <- prod_{b' < b} btot[b']
__global__ __launch_bounds__(1024) void k_pscan_blocks_rows(Fr* __restrict__ btot, uint32_t nb) {
    __shared__ Fr sh[1024];
    btot += (size_t)blockIdx.x * nb;
    Fr carry = Fr::one();
    for (uint32_t c0 = 0; c0 < nb; c0 += 1024) {
        uint32_t b = c0 + threadIdx.x;
        Fr v = b < nb ? ld(btot + b) : Fr::one();
        sh[threadIdx.x] = v;
        __syncthreads();
        Fr inc = v;
        for (unsigned d = 1; d < 1024; d <<= 1) {
            Fr o = threadIdx.x >= d ? sh[threadIdx.x - d] : Fr::one();
            __syncthreads();
            inc = inc * o;
            sh[threadIdx.x] = inc;
            __syncthreads();
        }
        Fr excl = carry * (threadIdx.x ? sh[threadIdx.x - 1] : Fr::one());
        Fr total = sh[1023];
        __syncthreads();
        if (b < nb) btot[b] = excl;
        carry = carry * total;
    }
}
// pass 3, row blockIdx.y: row v's n values of Z to z + v * out_stride
__global__ __launch_bounds__(256) void k_pscan_apply_rows(const Fr* __restrict__ num, const Fr* __restrict__ dinv, uint32_t n, uint32_t K, const Fr* __restrict__ texcl,
                                                          const Fr* __restrict__ bexcl, Fr* __restrict__ z, size_t out_stride) {
    const size_t row = blockIdx.y, gt = (size_t)blockIdx.x * 256 + threadIdx.x, base = gt * K;
    if (base >= n) return;
    num += row * n;
    dinv += row * n;
    z += row * out_stride;
    Fr p = ld(bexcl + row * gridDim.x + blockIdx.x) * ld(texcl + row * gridDim.x * 256 + gt);
    for (uint32_t k = 0; k < K; k++) {
        size_t i = base + k;
        if (i >= n) break;
        z[i] = p;
        p = p * (ld(num + i) * ld(dinv + i));
    }
}
// A row that is ONE scan workgroup (n <= 256 K): the blocks pass is the identity, so lane totals, the workgroup scan and the apply are one kernel, one
// workgroup per row (blockIdx.x), and nothing goes through HBM between them.  The products are formed twice, as the three passes form them.
__global__ __launch_bounds__(256) void k_pscan_fused_rows(const Fr* __restrict__ num, const Fr* __restrict__ dinv, uint32_t n, uint32_t K, Fr* __restrict__ z,
                                                          size_t out_stride) {
    __shared__ Fr sh[256];
    const size_t row = blockIdx.x, base = (size_t)threadIdx.x * K;
    num += row * n;
    dinv += row * n;
    z += row * out_stride;
    Fr tot = Fr::one();
    for (uint32_t k = 0; k < K; k++) {
        size_t i = base + k;
        if (i < n) tot = tot * (ld(num + i) * ld(dinv + i));
    }
    Fr inc;
    Fr p = pscan_wg256(sh, tot, &inc);
    for (uint32_t k = 0; k < K; k++) {
        size_t i = base + k;
        if (i >= n) break;
        z[i] = p;
        p = p * (ld(num + i) * ld(dinv + i));
    }
}

// The three passes of the Horner suffix scan (scan.hpp's bodies) with the row as a grid dimension and everything that belongs to a row in device memory.  Row v reads
// polynomial p at f[p] + v * stride[p] and takes its point from the row's prepared points: a, A = a^K, M = A^256 at pts + v * pstride + 3 pt[p], written once per
// row by k_hscan_points_dev / k_lin_points_rows.
constexpr int HSCAN_DEV_POLYS = 6;
struct HscanDev {
    const Fr* f[HSCAN_DEV_POLYS];
    size_t stride[HSCAN_DEV_POLYS];  // 0: a polynomial of the key, the same for every row
    size_t len[HSCAN_DEV_POLYS];     // >= 1
    uint32_t pt[HSCAN_DEV_POLYS];
    const Fr* pts;
    uint32_t pstride, npoly, K, nb;
    int carry_poly;                  // the polynomial that pass 3 divides: its lane carries are kept (-1: none)
    Fr* tcarry;                      // [(row nb + block) 256 + lane]
    Fr* btot;                        // [(row npoly + p) nb + block]
    Fr* total;                       // f_p(a) of row v -> total[v * tstride + p]
    size_t tstride;
    Fr* q;                           // pass 3: (f - f(a)) / (X - a) of polynomial carry_poly, len - 1 coefficients at q + v * qstride (may be that polynomial)
    size_t qstride;
};
// a -> a, a^K, a^(256 K)
__device__ __forceinline__ void hscan_point(const Fr& a, uint32_t K, Fr* __restrict__ out) {
    Fr A = Fr::one(), base = a;
    for (uint32_t k = K; k; k >>= 1) { if (k & 1) A = A * base; base = base.sqr(); }
    Fr M = A;
    for (int i = 0; i < 8; i++) M = M.sqr();
    out[0] = a; out[1] = A; out[2] = M;
}
__global__ __launch_bounds__(256) void k_hscan_points_dev(const Fr* __restrict__ points, uint32_t rows, uint32_t K, Fr* __restrict__ pts) {
    const uint32_t v = blockIdx.x * 256 + threadIdx.x;
    if (v < rows) hscan_point(ld(points + v), K, pts + 3 * (size_t)v);
}
// pass 1: grid (nb, rows, polynomials).  A workgroup wholly above the polynomial's last coefficient contributes zeros.
__global__ __launch_bounds__(256) void k_hscan_local_dev(HscanDev H) {
    __shared__ Fr sh[256];
    const unsigned p = blockIdx.z;
    const size_t row = blockIdx.y, len = H.len[p];
    const size_t blk = (row * H.npoly + p) * H.nb + blockIdx.x, lane0 = (row * H.nb + blockIdx.x) * 256;
    const bool keep = (int)p == H.carry_poly;
    const size_t first = (size_t)blockIdx.x * 256 * H.K;
    if (first >= len) {  // uniform over the workgroup
        if (keep) H.tcarry[lane0 + threadIdx.x] = Fr::zero();
        if (threadIdx.x == 0) H.btot[blk] = Fr::zero();
        return;
    }
    const Fr* __restrict__ pt = H.pts + row * H.pstride + 3 * H.pt[p];
    const Fr a = ld(pt), A = ld(pt + 1);
    const size_t lanes = (len - first + H.K - 1) / H.K;
    const Fr val = hscan_local_body(sh, H.f[p] + row * H.stride[p], len, H.K, first + (size_t)threadIdx.x * H.K, a, A, lanes < 256 ? (uint32_t)lanes : 256u);
    if (keep) H.tcarry[lane0 + threadIdx.x] = threadIdx.x < 255 ? sh[threadIdx.x + 1] : Fr::zero();
    if (threadIdx.x == 0) H.btot[blk] = val;
}
// pass 2: grid (polynomials, rows), one workgroup each
__global__ __launch_bounds__(1024) void k_hscan_blocks_dev(HscanDev H) {
    __shared__ Fr sh[1024];
    const unsigned p = blockIdx.x;
    const size_t row = blockIdx.y;
    const Fr M = ld(H.pts + row * H.pstride + 3 * H.pt[p] + 2);
    const Fr tot = hscan_blocks_body(sh, H.btot + (row * H.npoly + p) * H.nb, H.nb, M);
    if (threadIdx.x == 0) H.total[row * H.tstride + p] = tot;
}
// pass 3: grid (nb, rows), polynomial carry_poly
__global__ __launch_bounds__(256) void k_hscan_apply_dev(HscanDev H) {
    const unsigned p = (unsigned)H.carry_poly;
    const size_t row = blockIdx.y, len = H.len[p];
    const size_t base = ((size_t)blockIdx.x * 256 + threadIdx.x) * H.K;
    if (base >= len) return;
    const Fr* pt = H.pts + row * H.pstride + 3 * H.pt[p];
    const Fr a = ld(pt), A = ld(pt + 1);
    hscan_apply_body(H.f[p] + row * H.stride[p], H.q + row * H.qstride, len, len - 1, H.K, base, a, A, ld(H.tcarry + (row * H.nb + blockIdx.x) * 256 + threadIdx.x),
                     ld(H.btot + (row * H.npoly + p) * H.nb + blockIdx.x));
}

// ------------------------------------------------------------------------------------------------ rounds 4 and 5 with the row as a grid dimension
// x^(r - 2): Field::inv with the exponent's words as constants (no array to index); 0 -> 0
__device__ __forceinline__ Fr fr_inv_fermat(const Fr& x) {
    Fr acc = Fr::one(), base = x;
#pragma unroll
    for (int w = 0; w < 8; w++) {
        const uint32_t e = FrParams::MOD[w] - (w == 0 ? 2u : 0u);
        for (int i = 0; i < 32; i++) {
            if ((e >> i) & 1) acc = acc * base;
            base = base.sqr();
        }
    }
    return acc;
}
// what a row of round 4 needs of its zeta, once per row: LIN_PT elements -- the points zeta and omega zeta (a, a^K, a^(256 K) each), zeta^(n+2), and
// lag = (zeta^n - 1) / (zeta - 1) * alpha^2 / n with 1 / 0 = 0
__global__ __launch_bounds__(256) void k_lin_points_rows(const Fr* __restrict__ zeta, const Fr* __restrict__ alpha, uint32_t rows, uint32_t K, unsigned logn, Fr gen,
                                                         Fr card_inv, Fr* __restrict__ pts) {
    const uint32_t v = blockIdx.x * 256 + threadIdx.x;
    if (v >= rows) return;
    Fr* o = pts + (size_t)v * LIN_PT;
    const Fr z = ld(zeta + v), al = ld(alpha + v);
    hscan_point(z, K, o);
    hscan_point(z * gen, K, o + 3);
    Fr zn = z;
    for (unsigned i = 0; i < logn; i++) zn = zn.sqr();
    o[6] = zn * z.sqr();
    o[7] = (zn - Fr::one()) * fr_inv_fermat(z - Fr::one()) * al * al * card_inv;
}
// The linearised polynomial (k_linearized's formula; n + 3 coefficients) and the folded quotient h1 + zeta^(n+2) h2 + zeta^(2(n+2)) h3 (n + 2) of row blockIdx.y.
// The row's scalars are formed here from its evaluations and challenges: the same in every lane, exact products, so alpha c_z + lag and alpha c_s3 stand for
// k_linearized's (z c_z + s3 c_s3) alpha + z lag.
struct LinRowsArgs {
    const Fr *z, *h;                                  // row 0; row v is v * in_stride / v * h_stride further
    size_t in_stride, h_stride;
    const Fr *s3, *ql, *qr, *qm, *qo, *cqk;           // the key's, canonical
    const Fr *alpha, *beta, *gamma, *zeta, *values;   // one (values: eight, of which [2 .. 8) = l, r, o, s1, s2 at zeta and z at omega zeta are read) per row
    const Fr* pts;                                    // k_lin_points_rows
    Fr u, uu;
    Fr *lin, *fh;
    size_t out_stride;
    uint32_t n;
};
__global__ __launch_bounds__(256) void k_lin_fold_rows(LinRowsArgs A) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, n = A.n;
    if (i >= n + 3) return;
    const size_t row = blockIdx.y;
    const Fr* ev = A.values + 8 * row;
    const Fr lz = ld(ev + 2), rz = ld(ev + 3), oz = ld(ev + 4), s1z = ld(ev + 5), s2z = ld(ev + 6), zu = ld(ev + 7);
    const Fr alpha = ld(A.alpha + row), beta = ld(A.beta + row), gamma = ld(A.gamma + row), bzeta = beta * ld(A.zeta + row);
    const Fr c_s3 = (lz + beta * s1z + gamma) * (rz + beta * s2z + gamma) * zu * beta;
    const Fr c_z = ((lz + bzeta + gamma) * (rz + bzeta * A.u + gamma) * (oz + bzeta * A.uu + gamma)).neg();
    Fr sc[8] = {c_z * alpha + ld(A.pts + row * LIN_PT + 7), c_s3 * alpha, lz * rz, lz, rz, oz, ld(A.pts + row * LIN_PT + 6), Fr::zero()};
    sc[7] = sc[6].sqr();
    // the same for every lane of the workgroup: scalar registers, like the arguments of k_linearized and k_fold they stand for
#pragma unroll
    for (int j = 0; j < 8; j++)
#pragma unroll
        for (int k = 0; k < 8; k++) sc[j].l[k] = __builtin_amdgcn_readfirstlane(sc[j].l[k]);
    Fr v = ld(A.z + row * A.in_stride + i) * sc[0];
    if (i < n) v = v + ld(A.s3 + i) * sc[1] + ld(A.qm + i) * sc[2] + ld(A.ql + i) * sc[3] + ld(A.qr + i) * sc[4] + ld(A.qo + i) * sc[5] + ld(A.cqk + i);
    A.lin[row * A.out_stride + i] = v;
    if (i < n + 2) {
        const Fr* h = A.h + row * A.h_stride + i;
        A.fh[row * A.out_stride + i] = ld(h) + ld(h + (n + 2)) * sc[6] + ld(h + 2 * (size_t)(n + 2)) * sc[7];
    }
}
// kzg.BatchOpenSinglePoint's fold of row blockIdx.y: fh + g lin + g^2 l + g^3 r + g^4 o + g^5 s1 + g^6 s2 (n + 3 coefficients) by Horner's rule in g = kg[row]
// (exact: the sum of k_fold's products), to out + row * (n + 3)
__global__ __launch_bounds__(256) void k_open_fold_rows(const Fr* __restrict__ fh, const Fr* __restrict__ lin, const Fr* __restrict__ l, const Fr* __restrict__ r,
                                                        const Fr* __restrict__ o, size_t in_stride, const Fr* __restrict__ s1, const Fr* __restrict__ s2,
                                                        const Fr* __restrict__ kg, uint32_t n, Fr* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n + 3) return;
    const size_t row = blockIdx.y, at = row * in_stride + i;
    const Fr g = ld(kg + row);
    Fr v = i < n ? ld(s2 + i) * g + ld(s1 + i) : Fr::zero();
    v = v * g;
    if (i < n + 2) v = v + ld(o + at);
    v = v * g;
    if (i < n + 2) v = v + ld(r + at);
    v = v * g;
    if (i < n + 2) v = v + ld(l + at);
    v = v * g + ld(lin + at);
    v = v * g;
    if (i < n + 2) v = v + ld(fh + at);
    out[row * (size_t)(n + 3) + i] = v;
}

// ------------------------------------------------------------------------------------------------ quotient numerator on the big coset
struct QuotArgs {
    const Fr *el, *er, *eo, *ez, *eqk;                                 // the proof's polynomials (blinded l, r, o, z; completed qk)
    const Fr *ql, *qr, *qm, *qo, *s1, *s2, *s3, *l1, *id;              // the key's, all LagrangeCoset on the big domain, bit-reversed layout
    Fr* out;                                                           // may alias eqk
    Fr alpha, beta, gamma, beta_u, beta_uu;
    Fr xn_inv[8];                                                      // 1 / (x^n - 1): x^n takes rho <= 8 values on the coset
    unsigned logN4, log_rho;
};
// The numerator with its 21 products in the 9 x 29-bit representation of ff29.hpp (Fr29: 206 instructions per product instead of ~305; the kernel is bound by
// them, not by its 8.6 GB).  Values loaded from memory are canonical images V = v 2^256; a product needs ONE operand in the multiplier form V << 5 (= v 2^261):
// u29r_mul(X, Y << 5) = X Y / 2^261 stays in the 2^256 domain.  So the second and third factor of each permutation product are BUILT in the 2^261 domain --
// (w << 5) + (gamma << 5) + u29r_mul(x << 5, beta << 5) -- and no in-register shift is ever needed.  Sums are plain limb additions; bounds (units of r; checked with
// tools/u29_ntt_model.py's bound classes): gate < 5.8, first factors < 3.2, 2^261-domain factors < 71.1 (re-normalised once: two operands with
// 31-bit limbs would overflow a 64-bit column), products < 2.4, the last sum < 8.1, t < 2.6 -> one partial reduction, canonical image out.
// The schedule below is restated statement by statement in tools/u29_ntt_model.py (quotient_schedule): bound propagation + exactness against the field formula,
// run by the CPU suite (tests/test_limb_models.py) -- edit both or the suite fails.
// One coset point of it: i the point's position (bit-reversed layout), is that of omega * x, xn_inv = 1 / (x^n - 1) there.  k_quotient29 and its row form
// k_quotient29_rows both call this, so there is ONE schedule for the model to restate.
struct QuotKey {
    const Fr *ql, *qr, *qm, *qo, *s1, *s2, *s3, *l1, *id;              // the key's nine tables, as in QuotArgs
};
__device__ __forceinline__ Fr quotient29_point(const Fr* __restrict__ el, const Fr* __restrict__ er, const Fr* __restrict__ eo, const Fr* __restrict__ ez,
                                               const Fr* eqk, const QuotKey& K, size_t i, size_t is, const Fr& alpha, const Fr& beta, const Fr& gamma,
                                               const Fr& beta_u, const Fr& beta_uu, const Fr& xn_inv) {
    const Fr fl = ld(el + i), fr = ld(er + i), fo = ld(eo + i), fz = ld(ez + i), fx = ld(K.id + i);
    const U29 l = u29_unpack(fl), r = u29_unpack(fr), o = u29_unpack(fo), z = u29_unpack(fz);
    // gate = ql l + qr r + qm (l r) + qo o + qk
    U29 gate = u29r_mul(l, u29r_load5(ld(K.ql + i)));
    gate = u29_add(gate, u29r_mul(r, u29r_load5(ld(K.qr + i))));
    gate = u29_add(gate, u29r_mul(u29r_mul(l, u29r_load5(fr)), u29r_load5(ld(K.qm + i))));
    gate = u29_add(gate, u29r_mul(o, u29r_load5(ld(K.qo + i))));
    gate = u29_add(gate, u29_unpack(ld(eqk + i)));
    const U29 g = u29_unpack(gamma), g5 = u29r_load5(gamma), x5 = u29r_load5(fx);
    // a = (l + g + beta x) (r + g + beta u x) (o + g + beta u^2 x) z
    U29 a = u29_add(u29_add(l, g), u29r_mul(u29_unpack(fx), u29r_load5(beta)));
    a = u29r_mul(a, u29_wnorm(u29_add(u29_add(u29r_load5(fr), g5), u29r_mul(x5, u29r_load5(beta_u)))));
    a = u29r_mul(a, u29_wnorm(u29_add(u29_add(u29r_load5(fo), g5), u29r_mul(x5, u29r_load5(beta_uu)))));
    a = u29r_mul(a, u29r_load5(fz));
    // b = (l + g + beta s1) (r + g + beta s2) (o + g + beta s3) z(omega x)
    const U29 b5 = u29r_load5(beta);
    U29 b = u29_add(u29_add(l, g), u29r_mul(u29_unpack(ld(K.s1 + i)), b5));
    b = u29r_mul(b, u29_wnorm(u29_add(u29_add(u29r_load5(fr), g5), u29r_mul(u29r_load5(ld(K.s2 + i)), b5))));
    b = u29r_mul(b, u29_wnorm(u29_add(u29_add(u29r_load5(fo), g5), u29r_mul(u29r_load5(ld(K.s3 + i)), b5))));
    b = u29r_mul(b, u29r_load5(ld(ez + is)));
    // t = ((one alpha + (b - a)) alpha + gate) / (x^n - 1),  one = (z - 1) L1
    const U29 a5 = u29r_load5(alpha);
    const U29 one = u29r_mul(u29r_sub<4>(z, u29_unpack(Fr::one())), u29r_load5(ld(K.l1 + i)));
    U29 t = u29_add(u29r_mul(one, a5), u29r_sub<4>(b, a));
    t = u29_add(u29r_mul(t, a5), gate);
    t = u29r_mul(t, u29r_load5(xn_inv));
    return u29r_pack(u29r_reduce(t), true);
}
// t(x) = [ gate(x) + alpha * (zs * prod(w + beta s_j + gamma) - z * prod(w + beta u^j x + gamma)) + alpha^2 (z - 1) L1 ] / (x^n - 1)
// (prove.go: fic / fo / fone / fm, then iop.DivideByXMinusOne); index i is the bit-reversed position of natural index j.
__global__ __launch_bounds__(256, 4) void k_quotient29(QuotArgs A) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t N4 = (size_t)1 << A.logN4;
    if (i >= N4) return;
    const unsigned j = brev((unsigned)i, A.logN4);
    const unsigned rho = 1u << A.log_rho;
    const unsigned js = (j + rho) & (unsigned)(N4 - 1);  // z(omega * x): omega = W^rho
    const size_t is = brev(js, A.logN4);
    const QuotKey K = {A.ql, A.qr, A.qm, A.qo, A.s1, A.s2, A.s3, A.l1, A.id};
    A.out[i] = quotient29_point(A.el, A.er, A.eo, A.ez, A.eqk, K, i, is, A.alpha, A.beta, A.gamma, A.beta_u, A.beta_uu, A.xn_inv[j & (rho - 1)]);
}

// ------------------------------------------------------------------------------------------------ row form of the quotient (quotient_rows_dev below)
// Round 3 with the ROW as a grid dimension (blockIdx.y): R witnesses of one key, every row with its own challenges and public inputs.  The workspace of a chunk of
// R rows is 5 R rows of N4 elements, polynomial-major: l rows, r rows, o rows, z rows, qk rows -- so the first 4 R rows are ONE call of ntt_rows_dev.
// zero-padded copies of the four blinded polynomials: blockIdx.z = polynomial (l, r, o: n + 2 coefficients, z: n + 3), row v of it at src + v * in_stride
__global__ __launch_bounds__(256) void k_quot_spread_rows(const Fr* __restrict__ l, const Fr* __restrict__ r, const Fr* __restrict__ o, const Fr* __restrict__ z,
                                                          size_t in_stride, uint32_t n, unsigned logN4, Fr* __restrict__ ws) {
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x, N4 = (size_t)1 << logN4;
    if (p >= N4) return;
    const unsigned k = blockIdx.z;
    const size_t row = blockIdx.y, len = (size_t)n + (k == 3 ? 3 : 2);
    const Fr* __restrict__ src = k == 0 ? l : k == 1 ? r : k == 2 ? o : z;
    ws[((size_t)k * gridDim.y + row) * N4 + p] = p < len ? ld(src + row * in_stride + p) : Fr::zero();
}
// k_qk_coset, row blockIdx.y: public inputs at pub + row * pub_stride, completed qk to out + row * N4
__global__ __launch_bounds__(256) void k_qk_coset_rows(const Fr* __restrict__ e_cqk, const Fr* __restrict__ e_l1, const Fr* __restrict__ pub, size_t pub_stride,
                                                       const Fr* __restrict__ lqk, uint32_t npub, unsigned logN4, unsigned log_rho, Fr* __restrict__ out) {
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t N4 = (size_t)1 << logN4;
    if (p >= N4) return;
    const size_t row = blockIdx.y;
    const Fr* __restrict__ sol = pub + row * pub_stride;
    const uint32_t j = __brev((uint32_t)p) >> (32 - logN4);
    Fr v = ld(e_cqk + p);
    for (uint32_t i = 0; i < npub; i++) {
        const Fr d = ld(sol + i) - ld(lqk + i);
        const uint32_t q = __brev((j - (i << log_rho)) & (uint32_t)(N4 - 1)) >> (32 - logN4);  // w = W^rho, rho = N4 / n
        v = v + d * ld(e_l1 + q);
    }
    out[row * N4 + p] = v;
}
// the literal sequence for more public inputs: LQk with row blockIdx.y's public inputs in front (Lagrange form, n elements per row) ...
__global__ __launch_bounds__(256) void k_qk_complete_rows(const Fr* __restrict__ lqk, const Fr* __restrict__ pub, size_t pub_stride, uint32_t npub, uint32_t n,
                                                          Fr* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const size_t row = blockIdx.y;
    out[row * n + i] = i < npub ? ld(pub + row * pub_stride + i) : ld(lqk + i);
}
// ... and, after the inverse transform (DIF: bit-reversed), its zero-padded copy in regular order in the row's N4 elements: BitReverse folded into the spread
__global__ __launch_bounds__(256) void k_qk_spread_rows(const Fr* __restrict__ small, unsigned logn, unsigned logN4, Fr* __restrict__ out) {
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x, N4 = (size_t)1 << logN4, n = (size_t)1 << logn;
    if (p >= N4) return;
    const size_t row = blockIdx.y;
    out[row * N4 + p] = p < n ? ld(small + row * n + brev((unsigned)p, logn)) : Fr::zero();
}
struct QuotRowsArgs {
    const Fr *el, *er, *eo, *ez, *eqk;                                 // row 0 of each; row v is v * N4 further
    QuotKey key;
    Fr* out;                                                           // rows N4 apart; may alias eqk
    const Fr *alpha, *beta, *gamma;                                    // one per row, on the device
    Fr u, uu;                                                          // the coset shift of the small domain and its square
    Fr xn_inv[8];
    unsigned logN4, log_rho;
};
// k_quotient29, row blockIdx.y: the row's challenges come from device arrays, beta u and beta u^2 are formed here (exact products: the canonical images the
// host hands to k_quotient29)
__global__ __launch_bounds__(256, 4) void k_quotient29_rows(QuotRowsArgs A) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t N4 = (size_t)1 << A.logN4;
    if (i >= N4) return;
    const unsigned j = brev((unsigned)i, A.logN4);
    const unsigned rho = 1u << A.log_rho;
    const unsigned js = (j + rho) & (unsigned)(N4 - 1);  // z(omega * x): omega = W^rho
    const size_t is = brev(js, A.logN4);
    const size_t row = blockIdx.y, off = row * N4;
    const Fr alpha = ld(A.alpha + row), beta = ld(A.beta + row), gamma = ld(A.gamma + row);
    Fr beta_u = beta * A.u, beta_uu = beta * A.uu;
    // the same for every lane of the workgroup: kept in scalar registers like the arguments of k_quotient29 they stand for, not in sixteen vector registers
#pragma unroll
    for (int k = 0; k < 8; k++) {
        beta_u.l[k] = __builtin_amdgcn_readfirstlane(beta_u.l[k]);
        beta_uu.l[k] = __builtin_amdgcn_readfirstlane(beta_uu.l[k]);
    }
    A.out[off + i] = quotient29_point(A.el + off, A.er + off, A.eo + off, A.ez + off, A.eqk + off, A.key, i, is, alpha, beta, gamma, beta_u, beta_uu,
                                      A.xn_inv[j & (rho - 1)]);
}
// row blockIdx.y: h[0 .. keep) to the caller's row; status[row] |= 1 if any of h[keep .. N4) is non-zero (the caller zeroes status first)
__global__ __launch_bounds__(256) void k_quot_tail_rows(const Fr* __restrict__ h, unsigned logN4, size_t keep, Fr* __restrict__ out, size_t out_stride,
                                                        int* __restrict__ status) {
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x, N4 = (size_t)1 << logN4;
    if (p >= N4) return;
    const size_t row = blockIdx.y;
    const Fr v = ld(h + row * N4 + p);
    if (p < keep) out[row * out_stride + p] = v;
    else if (!v.is_zero()) atomicOr(status + row, 1);
}

// linearised polynomial (prove.go computeLinearizedPolynomial), len = n + 3 coefficients
struct LinArgs {
    const Fr *bz, *s3, *ql, *qr, *qm, *qo, *cqk;
    Fr* out;
    Fr c_z, c_s3, alpha, rl, lz, rz, oz, lag;
    uint32_t n, len;
};
__global__ void k_linearized(LinArgs A) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.len) return;
    Fr z = ld(A.bz + i);
    Fr v = z * A.c_z;
    if (i < A.n) v = v + ld(A.s3 + i) * A.c_s3;
    v = v * A.alpha;
    if (i < A.n) v = v + ld(A.qm + i) * A.rl + ld(A.ql + i) * A.lz + ld(A.qr + i) * A.rz + ld(A.qo + i) * A.oz + ld(A.cqk + i);
    A.out[i] = v + z * A.lag;
}
// out = sum_k c_k * p_k (coefficient-wise; p_k has len_k coefficients)  -- folded quotient and kzg.BatchOpenSinglePoint's fold
struct FoldArgs {
    const Fr* p[8];
    uint32_t len[8];
    Fr c[8];
    int k;
    uint32_t n;
    Fr* out;
};
__global__ void k_fold(FoldArgs A) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.n) return;
    Fr v = Fr::zero();
    for (int k = 0; k < A.k; k++)
        if (i < A.len[k]) v = v + ld(A.p[k] + i) * A.c[k];
    A.out[i] = v;
}
// (*Polynomial).Blind: p[i] -= b_i, p[n + i] += b_i  (p[n + i] is zero before: the canonical form has n coefficients)
struct BlindArgs { Fr b[3]; int k; };
__global__ void k_blind(Fr* p, uint32_t n, BlindArgs B) {
    int i = threadIdx.x;
    if (i >= B.k) return;
    p[i] = ld(p + i) - B.b[i];
    p[n + i] = B.b[i];
}
// the blinding scalars behind a vector of n evaluations: p[n + i] = b_i -- the scalars of [tau^n - 1], [tau^(n+1) - tau] in a commitment against the Lagrange-form SRS
__global__ void k_blind_tail(Fr* p, uint32_t n, BlindArgs B) {
    int i = threadIdx.x;
    if (i < B.k) p[n + i] = B.b[i];
}
// *flag |= 1 if any of a[0 .. n) is non-zero
__global__ void k_any_nonzero(const Fr* __restrict__ a, size_t n, int* __restrict__ flag) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && !ld(a + i).is_zero()) atomicOr(flag, 1);
}
// qk[i] = -(ql a + qr b + qo c + qm a b): synthetic satisfiable circuits (bench / tests)
__global__ void k_synth_qk(Fr* qk, const Fr* ql, const Fr* qr, const Fr* qo, const Fr* qm, const uint32_t* xa, const uint32_t* xb, const uint32_t* xc,
                           const Fr* sol, size_t nc) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nc) return;
    Fr a = ld(sol + xa[i]), b = ld(sol + xb[i]), c = ld(sol + xc[i]);
    qk[i] = Fr::zero() - (ld(ql + i) * a + ld(qr + i) * b + ld(qo + i) * c + ld(qm + i) * (a * b));
}

// pk.Permutation on the wire: 3n raw big-endian int64 (encoding/binary, no length prefix) <-> uint32 slots
__global__ void k_perm_from_be(const uint32_t* __restrict__ raw, size_t cnt, uint32_t* __restrict__ out, int* __restrict__ status) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cnt) return;
    uint32_t hi = __builtin_bswap32(raw[2 * i]), lo = __builtin_bswap32(raw[2 * i + 1]);
    if (hi != 0 || lo >= cnt) { atomicOr(status, 8); lo = 0; }
    out[i] = lo;
}
__global__ void k_perm_to_be(const uint32_t* __restrict__ in, size_t cnt, uint32_t* __restrict__ raw) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cnt) return;
    raw[2 * i] = 0;
    raw[2 * i + 1] = __builtin_bswap32(in[i]);
}

// ------------------------------------------------------------------------------------------------ resident key
static std::mutex g_ppk_mu;
static std::map<uint64_t, PlonkPK*> g_ppks;
static uint64_t g_next_ppk = 1;

static int pk_alloc(PlonkPK* P, Fr** out, size_t elems) {
    void* p = nullptr;
    ZK_HIP(hipMalloc(&p, (elems ? elems : 1) * sizeof(Fr)));
    P->allocs.push_back(p);
    P->bytes += (elems ? elems : 1) * sizeof(Fr);
    *out = (Fr*)p;
    return ZK_OK;
}
static void pk_destroy(PlonkPK* P) {
    if (P->lag_srs) (void)zk_bn254_bases_free(P->lag_srs);
    for (void* p : P->allocs) (void)hipFree(p);
    delete P;
}

// kzg.Commit(p, srs) = MultiExp(srs.G1[:len(p)], p), p resident in HBM (Montgomery)
static int commit(const PlonkPK* P, Slot* s, hipStream_t st, const Fr* d_p, size_t len, Affine<HFp>* out) {
    ZK_TRY(slot_sync(s, st));  // the MSM runs on a stream slot of its own
    return zk_bn254_msm_bases_dev(P->srs, 0, d_p, len, &kMont, out);
}

// sum_i k_i P_i for a handful of points on the HOST (digests the prover derives from digests: the linearised polynomial's, the folded quotient's) by the
// interleaved-window method of curve.hpp instead of one double-and-add per term.  The group element, and so the affine result, is the same.
static XYZZ<HFp> host_multi_scalar_mul(const Affine<HFp>* pts, const HFr* ks, int cnt) {
    uint32_t k[8][8];
    if (cnt > 8) cnt = 8;
    for (int t = 0; t < cnt; t++) to_canonical_u32(ks[t], k[t]);
    return multi_scalar_mul(pts, k, cnt);
}

// A commitment in flight on a host thread of its own (the MSM entry point is synchronous and re-entrant: each call takes a stream slot), so that
// independent commitments -- l, r, o; h1, h2, h3; the opening of z next to the linearised polynomial -- and the transforms the main stream keeps
// issuing overlap on the GPU: the bandwidth-bound scalar preparation (digits, sort, task plan) of one MSM runs under the ALU-bound accumulate of another.
struct AsyncCommit {
    std::thread th;
    int rc = ZK_OK;
    std::string err;
    Affine<HFp> out;
    void start(const PlonkPK* P, const Fr* d_p, size_t len) {
        th = std::thread([this, P, d_p, len] {
            rc = zk_bn254_msm_bases_dev(P->srs, 0, d_p, len, &kMont, &out);
            if (rc != ZK_OK) err = zk_last_error();
        });
    }
    int join() {
        if (th.joinable()) th.join();
        return rc == ZK_OK ? ZK_OK : set_err(rc, "%s", err.c_str());
    }
    ~AsyncCommit() { if (th.joinable()) th.join(); }
};
// Three commitments against the same SRS whose polynomials exist at the same moment (l, r, o; h1, h2, h3) as ONE multi-scalar multiplication with three bucket
// sets (msm.hip: k_msm_digits over three scalar vectors, one sort of the 3 x 13 n digits, one task plan, ONE accumulate launch, one reduction per set): three
// concurrent preparations of ~17 dependent launches each, starving each other and whatever the main stream runs meanwhile, become one; the three accumulate kernels
// -- which could not share the machine anyway -- become one launch without seams.  Needs the SRS's window table on ONE device entry; otherwise the thread-per-commit
// path below is used.  Runs on a host thread of its own like AsyncCommit.
struct BatchCommit3 {
    std::thread th;
    int rc = ZK_OK;
    std::string err;
    Affine<HFp> out[3];
    static int run(uint64_t bases, const Fr* const* polys, size_t len, Affine<HFp>* outs, bool wire_values) {
        const void* sc[3] = {polys[0], polys[1], polys[2]};
        if (wire_values) return msm_bases_batch_dev_sparse(bases, 0, sc, 3, len, &kMont, outs);
        return zk_bn254_msm_bases_batch_dev(bases, 0, sc, 3, len, &kMont, outs);
    }
    static bool possible(uint64_t bases, const size_t* lens) {
        const void* d_table = nullptr;
        size_t nbases = 0;
        return lens[0] == lens[1] && lens[1] == lens[2] && bases_table(bases, &d_table, nullptr, &nbases) == ZK_OK && d_table && lens[0] <= nbases;
    }
    void start(uint64_t bases, const Fr* const* polys, size_t len, bool wire_values = false) {
        const Fr* p3[3] = {polys[0], polys[1], polys[2]};
        th = std::thread([this, bases, p3, len, wire_values] {
            rc = run(bases, p3, len, out, wire_values);
            if (rc != ZK_OK) err = zk_last_error();
        });
    }
    int join() {
        if (th.joinable()) th.join();
        return rc == ZK_OK ? ZK_OK : set_err(rc, "%s", err.c_str());
    }
    ~BatchCommit3() { if (th.joinable()) th.join(); }
};
// Lagrange (regular) -> canonical (regular) on the small domain, in place: FFTInverse(DIF) + BitReverse, as setup.go / iop.ToCanonical do
static int to_canonical(Slot* s, hipStream_t st, Fr* d, unsigned logn) {
    ZK_TRY(ntt_dev(s, st, d, logn, 1, ZK_DIF, 0));
    return bit_reverse_dev(s, st, d, logn);
}
// canonical p (len coefficients) -> LagrangeCoset on the big domain in `dst` (bit-reversed layout): zero-pad, FFT(DIF, coset)
static int to_big_coset(Slot* s, hipStream_t st, Fr* dst, const Fr* p, size_t len, const PlonkPK* P) {
    if (dst != p) ZK_HIP(hipMemcpyAsync(dst, p, len * sizeof(Fr), hipMemcpyDeviceToDevice, st));
    ZK_HIP(hipMemsetAsync(dst + len, 0, (P->N4 - len) * sizeof(Fr), st));
    return ntt_dev(s, st, dst, P->logN4, 0, ZK_DIF, 1);
}

// sigma in Lagrange form from the permutation (what BuildRatioCopyConstraint evaluates through pk.Permutation)
static int make_sigma(PlonkPK* P, Slot* s, hipStream_t st, const uint32_t* d_perm) {
    const size_t n = P->n;
    Domain* d0;
    ZK_TRY(get_domain(s, st, P->logn, DOM_TW, &d0));
    P->gen = d0->gen;
    P->u = d0->coset;
    P->card_inv = d0->card_inv;
    ZK_TRY(pk_alloc(P, &P->sig, 3 * n));
    ZK_LAUNCH(s, st, "plonk_sigma_lagrange", k_sigma_lagrange, dim3(grid_of(3 * n)), dim3(256), 0, d_perm, (const Fr*)d0->tw, (uint32_t)n, to_dev(P->u),
              to_dev(P->u * P->u), P->sig);
    return ZK_OK;
}
// From the canonical polynomials (all in P) to a usable key: the nine big-coset tables and the per-proof workspace.
static int finish_pk(PlonkPK* P, Slot* s, hipStream_t st) {
    const size_t n = P->n, N4 = P->N4;
    const Fr* canon[7] = {P->ql, P->qr, P->qm, P->qo, P->s1, P->s2, P->s3};
    for (int k = 0; k < 9; k++) ZK_TRY(pk_alloc(P, &P->e[k], N4));
    for (int k = 0; k < 7; k++) ZK_TRY(to_big_coset(s, st, P->e[k], canon[k], n, P));
    // L_1 = (X^n - 1) / (n (X - 1)) = (1/n) (1 + X + ... + X^(n-1))
    ZK_LAUNCH(s, st, "plonk_fill", k_fill, dim3(grid_of(n)), dim3(256), 0, P->e[7], n, to_dev(P->card_inv));
    ZK_TRY(to_big_coset(s, st, P->e[7], P->e[7], n, P));
    // id = X on the coset: g * W^bitrev(i)
    ZK_HIP(hipMemsetAsync(P->e[8], 0, N4 * sizeof(Fr), st));
    {
        Fr one = Fr::one();
        ZK_HIP(hipMemcpyAsync(P->e[8] + 1, &one, sizeof(Fr), hipMemcpyHostToDevice, st));
        ZK_HIP(hipStreamSynchronize(st));
    }
    ZK_TRY(ntt_dev(s, st, P->e[8], P->logN4, 0, ZK_DIF, 1));
    ZK_TRY(pk_alloc(P, &P->e_cqk, N4));
    ZK_TRY(to_big_coset(s, st, P->e_cqk, P->cqk, n, P));
    for (int k = 0; k < 5; k++) ZK_TRY(pk_alloc(P, &P->w_big[k], N4));
    ZK_TRY(pk_alloc(P, &P->w_small, 16 * (n + 8)));
    P->mu = std::make_shared<std::mutex>();
    P->live = std::make_shared<std::shared_mutex>();
    return slot_sync(s, st);
}

static int check_srs(uint64_t srs, size_t n) {
    size_t cnt = 0;
    int g2 = 0;
    ZK_TRY(bases_info(srs, &cnt, &g2));
    if (g2) return set_err(ZK_ERR_ARG, "the KZG SRS must be a G1 base array");
    if (cnt < n + 3) return set_err(ZK_ERR_ARG, "kzg: invalid polynomial size: the SRS holds %zu points, %zu needed (domain + 3)", cnt, n + 3);
    return ZK_OK;
}

// setup.go buildPermutation, on the host (a sequential pass over the 3n wire slots)
static void build_permutation(size_t n, size_t npub, size_t nc, size_t nvars, const uint32_t* xa, const uint32_t* xb, const uint32_t* xc, std::vector<uint32_t>* perm) {
    std::vector<uint32_t> lro(3 * n, 0);
    for (size_t i = 0; i < npub; i++) lro[i] = (uint32_t)i;
    for (size_t i = 0; i < nc; i++) {
        lro[npub + i] = xa[i];
        lro[n + npub + i] = xb[i];
        lro[2 * n + npub + i] = xc[i];
    }
    const int64_t none = -1;
    std::vector<int64_t> cycle(nvars ? nvars : 1, none), pm(3 * n, none);
    for (size_t i = 0; i < 3 * n; i++) {
        if (cycle[lro[i]] != none) pm[i] = cycle[lro[i]];
        cycle[lro[i]] = (int64_t)i;
    }
    perm->resize(3 * n);
    for (size_t i = 0; i < 3 * n; i++) (*perm)[i] = (uint32_t)(pm[i] == none ? cycle[lro[i]] : pm[i]);
}

static int register_pk(PlonkPK* P, uint64_t* handle) {
    std::lock_guard<std::mutex> lk(g_ppk_mu);
    *handle = hmake(g_next_ppk++);
    g_ppks[*handle] = P;
    return ZK_OK;
}

// the count / domain rules live with the other readers of untrusted bytes (text_host.hpp: host only, sanitizer- and mutation-tested)
static int check_counts(uint64_t n_public, size_t n_vars, size_t n_constraints) {
    std::string e;
    const int rc = plonk_check_counts(n_public, n_vars, n_constraints, &e);
    return rc == ZK_OK ? ZK_OK : set_err(rc, "%s", e.c_str());
}
static int domains_for(size_t size_system, unsigned* logn, unsigned* logN4) {
    std::string e;
    const int rc = plonk_domains_for(size_system, logn, logN4, &e);
    return rc == ZK_OK ? ZK_OK : set_err(rc, "%s", e.c_str());
}

// ------------------------------------------------------------------------------------------------ round 2 for R witnesses of one domain
// iop.BuildRatioCopyConstraint on `rows` triples (l, r, o) that share a domain and a permutation: Z in Lagrange form, regular order, per row.
//   one row     z_chain_dev, the five launches of zk_bn254_plonk_prove's round 2, on the scan plan the prover uses (scan_bufs of n + 8)
//   more rows   k_z_terms_rows (row = blockIdx.y), ONE k_batch_inverse over the rows * n denominators of the chunk, then
//                 n <= 256 K:  k_pscan_fused_rows, one workgroup per row                                    -- three launches in all
//                 above:       k_pscan_local_rows, k_pscan_blocks_rows (one workgroup per row), k_pscan_apply_rows -- five
//               on the plan of n itself: K = max(8, ceil(n / 2^18)) elements per lane, nb = ceil(n / 256 K) workgroups per row
// The workspace comes from the slot's arena, RATIO_SCRATCH bytes at a time: more rows than fit (or than a grid's y holds) go in chunks on the same stream.
constexpr size_t RATIO_SCRATCH = (size_t)1 << 30;
size_t ratio_row_bytes(size_t n) {
    uint32_t K, nb;
    scan_plan(n, &K, &nb);
    return (3 * n + (size_t)nb * 257) * sizeof(Fr);
}
// rows per chunk when every row also takes `extra` bytes of the caller's (the staging rows of the host entry)
static size_t ratio_chunk(size_t n, size_t rows, size_t extra) {
    return std::min(std::min(rows, RATIO_GRID_ROWS), std::max<size_t>(1, RATIO_SCRATCH / (ratio_row_bytes(n) + extra)));
}
size_t ratio_ws_bytes(size_t n, size_t chunk, bool single) {
    return single ? 3 * (n * sizeof(Fr) + 256) + scan_need(n + 8) + 4096 : chunk * ratio_row_bytes(n) + 5 * 256;
}
// after the caller's reserve() of at least ratio_ws_bytes
int ratio_ws_take(Slot* s, size_t n, size_t chunk, bool single, RatioWs* W) {
    W->single = single;
    W->chunk = single ? 1 : chunk;
    W->num = (Fr*)s->alloc(W->chunk * n * sizeof(Fr));
    W->den = (Fr*)s->alloc(W->chunk * n * sizeof(Fr));
    W->scr = (Fr*)s->alloc(W->chunk * n * sizeof(Fr));
    if (!W->num || !W->den || !W->scr) return set_err(ZK_ERR_HIP, "ratio workspace was not reserved");
    if (single) return scan_bufs(s, n + 8, &W->one);
    scan_plan(n, &W->K, &W->nb);
    W->t = (Fr*)s->alloc(W->chunk * W->nb * 256 * sizeof(Fr));
    W->b = (Fr*)s->alloc(W->chunk * W->nb * sizeof(Fr));
    if (!W->t || !W->b) return set_err(ZK_ERR_HIP, "ratio workspace was not reserved");
    return ZK_OK;
}
// the three passes of the product scan over R rows of n products on the plan (K, nb): Z of row v to z + v * out_stride
struct PscanNames {
    const char *local, *blocks, *apply;
};
static const PscanNames kPscanOne = {"plonk_pscan_local", "plonk_pscan_blocks", "plonk_pscan_apply"};
static const PscanNames kPscanRows = {"plonk_pscan_local_rows", "plonk_pscan_blocks_rows", "plonk_pscan_apply_rows"};
static int pscan_passes(Slot* s, hipStream_t st, const PscanNames& names, const Fr* num, const Fr* den, size_t n, unsigned R, uint32_t K, uint32_t nb, Fr* t, Fr* b,
                        Fr* z, size_t out_stride) {
    ZK_LAUNCH(s, st, names.local, k_pscan_local_rows, dim3(nb, R), dim3(256), 0, num, den, (uint32_t)n, K, t, b);
    ZK_LAUNCH(s, st, names.blocks, k_pscan_blocks_rows, dim3(R), dim3(1024), 0, b, nb);
    ZK_LAUNCH(s, st, names.apply, k_pscan_apply_rows, dim3(nb, R), dim3(256), 0, num, den, (uint32_t)n, K, (const Fr*)t, (const Fr*)b, z, out_stride);
    return ZK_OK;
}
// Z of ONE row with its challenges on the host, five launches: k_z_terms, k_batch_inverse and the three passes on the plan of SB (the prover's scan_bufs(n + 8)).
// num, den, scr: n elements each.
static int z_chain_dev(Slot* s, hipStream_t st, const Fr* tw, const HFr& u, const Fr* sig, const Fr* l, const Fr* r, const Fr* o, size_t n, const HFr& beta,
                       const HFr& gamma, Fr* num, Fr* den, Fr* scr, const ScanBufs& SB, Fr* z) {
    ZK_LAUNCH(s, st, "plonk_z_terms", k_z_terms, dim3(grid_of(n)), dim3(256), 0, l, r, o, sig, tw, (uint32_t)n, to_dev(beta), to_dev(beta * u), to_dev(beta * (u * u)),
              to_dev(gamma), num, den);
    const size_t lanes = (n + BINV_K - 1) / BINV_K;
    ZK_LAUNCH(s, st, "plonk_batch_inverse", k_batch_inverse, dim3(grid_of(lanes)), dim3(256), 0, den, n, scr);
    return pscan_passes(s, st, kPscanOne, num, den, n, 1, SB.K, SB.nb, SB.t, SB.b, z, 0);
}
// row v: wires at l / r / o + v * in_stride, challenges d_beta[v], d_gamma[v] (device), Z to z + v * out_stride.  sig = S1 | S2 | S3 in Lagrange form.
int ratio_rows_dev(Slot* s, hipStream_t st, const Domain* d0, const Fr* sig, const Fr* l, const Fr* r, const Fr* o, size_t in_stride, size_t rows,
                   const Fr* d_beta, const Fr* d_gamma, Fr* z, size_t out_stride, const RatioWs& W) {
    const size_t n = (size_t)1 << d0->logn;
    const HFr u = d0->coset;
    const Fr* tw = d0->tw;
    if (W.single) {
        if (rows != 1) return set_err(ZK_ERR_ARG, "internal: one-row ratio workspace for %zu rows", rows);
        HFr bg[2];
        ZK_HIP(hipMemcpyAsync(&bg[0], d_beta, sizeof(Fr), hipMemcpyDeviceToHost, st));
        ZK_HIP(hipMemcpyAsync(&bg[1], d_gamma, sizeof(Fr), hipMemcpyDeviceToHost, st));
        ZK_HIP(hipStreamSynchronize(st));
        return z_chain_dev(s, st, tw, u, sig, l, r, o, n, bg[0], bg[1], W.num, W.den, W.scr, W.one, z);
    }
    for (size_t first = 0; first < rows; first += W.chunk) {
        const unsigned R = (unsigned)std::min(W.chunk, rows - first);
        ZK_LAUNCH(s, st, "plonk_z_terms_rows", k_z_terms_rows, dim3(grid_of(n), R), dim3(256), 0, l + first * in_stride, r + first * in_stride, o + first * in_stride,
                  in_stride, sig, tw, (uint32_t)n, d_beta + first, d_gamma + first, to_dev(u), to_dev(u * u), W.num, W.den);
        {
            const size_t cnt = (size_t)R * n, lanes = (cnt + BINV_K - 1) / BINV_K;
            ZK_LAUNCH(s, st, "plonk_batch_inverse", k_batch_inverse, dim3(grid_of(lanes)), dim3(256), 0, W.den, cnt, W.scr);
        }
        Fr* zc = z + first * out_stride;
        if (W.nb == 1) {
            ZK_LAUNCH(s, st, "plonk_pscan_fused_rows", k_pscan_fused_rows, dim3(R), dim3(256), 0, (const Fr*)W.num, (const Fr*)W.den, (uint32_t)n, W.K, zc, out_stride);
            continue;
        }
        ZK_TRY(pscan_passes(s, st, kPscanRows, W.num, W.den, n, R, W.K, W.nb, W.t, W.b, zc, out_stride));
    }
    return ZK_OK;
}
// S1 | S2 | S3 in Lagrange form from 3n positions; *h_flag != 0 after the stream is synchronised: an entry was out of range
static int sigma_checked_dev(Slot* s, hipStream_t st, const Domain* d0, const uint32_t* d_perm, Fr* d_sigma, int* d_flag) {
    const size_t n = (size_t)1 << d0->logn;
    const HFr u = d0->coset;
    ZK_HIP(hipMemsetAsync(d_flag, 0, 4, st));
    ZK_LAUNCH(s, st, "plonk_sigma_lagrange", k_sigma_lagrange_checked, dim3(grid_of(3 * n)), dim3(256), 0, d_perm, (const Fr*)d0->tw, (uint32_t)n, to_dev(u), to_dev(u * u),
              d_sigma, d_flag);
    return ZK_OK;
}
// the argument contract of the ratio entries that take device rows (sigma_elems: 3n, or 0 where the key supplies it)
static int ratio_dev_args(const void* l, const void* r, const void* o, size_t in_stride, size_t n, size_t rows, const void* sigma, size_t sigma_elems, const void* beta,
                          const void* gamma, const void* z, size_t out_stride) {
    if (in_stride < n) return set_err(ZK_ERR_ARG, "in_stride = %zu is below the domain size %zu", in_stride, n);
    if (out_stride < n) return set_err(ZK_ERR_ARG, "out_stride = %zu is below the domain size %zu", out_stride, n);
    const size_t zb = rows_span(rows, out_stride, n), ib = rows_span(rows, in_stride, n);
    if (spans_overlap(z, zb, l, ib) || spans_overlap(z, zb, r, ib) || spans_overlap(z, zb, o, ib) || spans_overlap(z, zb, sigma, sigma_elems * sizeof(Fr)) ||
        spans_overlap(z, zb, beta, rows * sizeof(Fr)) || spans_overlap(z, zb, gamma, rows * sizeof(Fr)))
        return set_err(ZK_ERR_ARG, "d_z overlaps an input");
    return ZK_OK;
}

// ------------------------------------------------------------------------------------------------ round 3 for R witnesses of one key
// The quotient h = numerator / (X^n - 1) of `rows` witnesses, canonical, 3(n + 2) coefficients each, and a verdict per row.  Per chunk of rows, whatever their number:
//   k_quot_spread_rows            l, r, o, z zero-padded into 4 R rows of N4
//   ntt_rows_dev(4 R rows)        FFT(DIF, coset): the four polynomials of every witness share each pass
//   qk, npub <= PLONK_PI_DIRECT_MAX:  k_qk_coset_rows
//       above:                    k_qk_complete_rows, ntt_rows_dev(R rows of n, inverse, DIF), k_qk_spread_rows (BitReverse folded in), ntt_rows_dev(R rows, DIF, coset)
//   k_quotient29_rows             into the qk rows, as the prover's k_quotient29 overwrites qk
//   ntt_rows_dev(R rows)          FFTInverse(DIT, coset)
//   k_quot_tail_rows              3(n + 2) coefficients out, status[row] = 1 iff anything above them is non-zero
// One row is R = 1 of the same launches.  Workspace: 5 N4 elements per row (+ n where qk takes the literal sequence) from the slot's arena, QUOT_SCRATCH bytes at
// a time; more rows than fit go in chunks on the same stream.  The key's own per-proof workspace is not touched.
constexpr size_t QUOT_SCRATCH = (size_t)1 << 30;
static bool quot_qk_direct(const PlonkPK* P) { return P->n_public <= PLONK_PI_DIRECT_MAX && P->logN4 >= 2; }
size_t quot_row_bytes(const PlonkPK* P) { return (5 * P->N4 + (quot_qk_direct(P) ? 0 : P->n)) * sizeof(Fr); }
static size_t quot_chunk(const PlonkPK* P, size_t rows) { return std::min(std::min(rows, RATIO_GRID_ROWS), std::max<size_t>(1, QUOT_SCRATCH / quot_row_bytes(P))); }
// 1 / (x^n - 1) on the coset of the big domain: x = g W^j  =>  x^n = g^n (W^n)^j, W^n of order rho <= 8
static void quot_xn_inv(const PlonkPK* P, const Domain* d1, Fr out[8]) {
    HFr gn = d1->coset, Wn = d1->gen;
    for (unsigned i = 0; i < P->logn; i++) { gn = gn.sqr(); Wn = Wn.sqr(); }
    HFr cur = gn;
    for (unsigned j = 0; j < 8; j++) {
        out[j] = j < (1u << P->log_rho) ? to_dev((cur - HFr::one()).inv()) : Fr::zero();
        cur = cur * Wn;
    }
}
// row v: blinded canonical l, r, o (n + 2) and z (n + 3) at + v * in_stride, public inputs at pub + v * pub_stride, challenges d_alpha / d_beta / d_gamma[v]
// (device), h to h + v * out_stride, verdict to status[v].  ws: chunk * quot_row_bytes(P) bytes.
int quotient_rows_dev(Slot* s, hipStream_t st, const PlonkPK* P, const Fr* l, const Fr* r, const Fr* o, const Fr* z, size_t in_stride, const Fr* pub,
                      size_t pub_stride, size_t rows, const Fr* d_alpha, const Fr* d_beta, const Fr* d_gamma, Fr* h, size_t out_stride, int* status, Fr* ws,
                      size_t chunk) {
    const size_t n = P->n, N4 = P->N4, keep = 3 * (n + 2);
    const unsigned logN4 = P->logN4;
    const bool direct = quot_qk_direct(P);
    Domain* d1;
    ZK_TRY(get_domain(s, st, logN4, DOM_TW, &d1));
    QuotRowsArgs A;
    A.key = {P->e[0], P->e[1], P->e[2], P->e[3], P->e[4], P->e[5], P->e[6], P->e[7], P->e[8]};
    A.u = to_dev(P->u); A.uu = to_dev(P->u * P->u);
    quot_xn_inv(P, d1, A.xn_inv);
    A.logN4 = logN4; A.log_rho = P->log_rho;
    for (size_t first = 0; first < rows; first += chunk) {
        const unsigned R = (unsigned)std::min(chunk, rows - first);
        Fr *qk = ws + 4 * (size_t)R * N4, *small = qk + (size_t)R * N4;
        const size_t in = first * in_stride;
        ZK_LAUNCH(s, st, "plonk_quotient_spread_rows", k_quot_spread_rows, dim3(grid_of(N4), R, 4), dim3(256), 0, l + in, r + in, o + in, z + in, in_stride, (uint32_t)n,
                  logN4, ws);
        ZK_TRY(ntt_rows_dev(s, st, ws, logN4, 4 * (size_t)R, N4, 0, ZK_DIF, 1));
        const Fr* pubc = pub + first * pub_stride;  // never read when the key has no public inputs
        if (direct) {
            ZK_LAUNCH(s, st, "plonk_qk_coset_rows", k_qk_coset_rows, dim3(grid_of(N4), R), dim3(256), 0, (const Fr*)P->e_cqk, (const Fr*)P->e[7], pubc, pub_stride,
                      (const Fr*)P->lqk, (uint32_t)P->n_public, logN4, P->log_rho, qk);
        } else {
            ZK_LAUNCH(s, st, "plonk_qk_complete_rows", k_qk_complete_rows, dim3(grid_of(n), R), dim3(256), 0, (const Fr*)P->lqk, pubc, pub_stride, (uint32_t)P->n_public,
                      (uint32_t)n, small);
            ZK_TRY(ntt_rows_dev(s, st, small, P->logn, R, n, 1, ZK_DIF, 0));
            ZK_LAUNCH(s, st, "plonk_qk_spread_rows", k_qk_spread_rows, dim3(grid_of(N4), R), dim3(256), 0, (const Fr*)small, P->logn, logN4, qk);
            ZK_TRY(ntt_rows_dev(s, st, qk, logN4, R, N4, 0, ZK_DIF, 1));
        }
        A.el = ws; A.er = ws + (size_t)R * N4; A.eo = ws + 2 * (size_t)R * N4; A.ez = ws + 3 * (size_t)R * N4; A.eqk = qk; A.out = qk;
        A.alpha = d_alpha + first; A.beta = d_beta + first; A.gamma = d_gamma + first;
        ZK_LAUNCH(s, st, "plonk_quotient_rows", k_quotient29_rows, dim3(grid_of(N4), R), dim3(256), 0, A);
        ZK_TRY(ntt_rows_dev(s, st, qk, logN4, R, N4, 1, ZK_DIT, 1));  // LagrangeCoset (bit-reversed) -> canonical (regular)
        ZK_HIP(hipMemsetAsync(status + first, 0, (size_t)R * sizeof(int), st));
        ZK_LAUNCH(s, st, "plonk_quotient_tail_rows", k_quot_tail_rows, dim3(grid_of(N4), R), dim3(256), 0, (const Fr*)qk, logN4, keep, h + first * out_stride, out_stride,
                  status + first);
    }
    return ZK_OK;
}

// ------------------------------------------------------------------------------------------------ rounds 4 and 5 for R witnesses of one key
// The polynomial work after the zeta challenge with the row as a grid dimension and every per-row challenge in device memory: nothing comes back to the host
// between launches, and the launches of a chunk do not depend on its rows.  One row is R = 1 of the same kernels.
//   poly_open_rows_dev (the ingredient)  k_hscan_points_dev, k_hscan_local_dev, k_hscan_blocks_dev [, k_hscan_apply_dev]                     3 or 4
//   linearize_rows_dev (round 4)         k_lin_points_rows, local over (l, r, o, s1, s2 at zeta; z at omega zeta), blocks, apply (z),
//                                        k_lin_fold_rows, local and blocks over (fh, lin)                                                   7
//   open_rows_dev (round 5)              k_hscan_points_dev, k_open_fold_rows, local, blocks, apply                                         5
// on scan_bufs' plan for the longest polynomial: K = max(8, ceil(len / 2^18)) coefficients per lane, nb workgroups of 256 lanes per row.  Workspace per row from
// the slot's arena, OPEN_SCRATCH bytes at a time: the prepared points, nb block totals per polynomial and 256 nb lane carries (+ the n + 3 folded coefficients in
// round 5); more rows than fit, or than a grid's y holds, go in chunks on the same stream.
constexpr size_t OPEN_SCRATCH = (size_t)1 << 30;
struct OpenWs {
    uint32_t K = 0, nb = 0;
    size_t chunk = 0;
    Fr *pts = nullptr, *btot = nullptr, *tcarry = nullptr, *fold = nullptr;
};
size_t open_row_bytes(size_t len, unsigned npoly, size_t pt, size_t fold) {
    uint32_t K, nb;
    scan_plan(len, &K, &nb);
    return (pt + (size_t)npoly * nb + (size_t)nb * 256 + fold) * sizeof(Fr);
}
static int open_ws_take(Slot* s, size_t len, size_t rows, unsigned npoly, size_t pt, size_t fold, OpenWs* W) {
    scan_plan(len, &W->K, &W->nb);
    const size_t row = open_row_bytes(len, npoly, pt, fold);
    W->chunk = std::min(std::min(rows, RATIO_GRID_ROWS), std::max<size_t>(1, OPEN_SCRATCH / row));
    ZK_TRY(s->reserve(W->chunk * row + 5 * 256));
    W->pts = (Fr*)s->alloc(W->chunk * pt * sizeof(Fr));
    W->btot = (Fr*)s->alloc(W->chunk * npoly * W->nb * sizeof(Fr));
    W->tcarry = (Fr*)s->alloc(W->chunk * W->nb * 256 * sizeof(Fr));
    W->fold = fold ? (Fr*)s->alloc(W->chunk * fold * sizeof(Fr)) : nullptr;
    if (!W->pts || !W->btot || !W->tcarry || (fold && !W->fold)) return set_err(ZK_ERR_HIP, "opening rows: workspace");
    return ZK_OK;
}
// the passes over H's polynomials for R rows; pass 3 where H.q is set
static int hscan_dev_passes(Slot* s, hipStream_t st, const HscanDev& H, unsigned R) {
    ZK_LAUNCH(s, st, "plonk_horner_local_rows", k_hscan_local_dev, dim3(H.nb, R, H.npoly), dim3(256), 0, H);
    ZK_LAUNCH(s, st, "plonk_horner_blocks_rows", k_hscan_blocks_dev, dim3(H.npoly, R), dim3(1024), 0, H);
    if (H.q) ZK_LAUNCH(s, st, "plonk_divide_apply_rows", k_hscan_apply_dev, dim3(H.nb, R), dim3(256), 0, H);
    return ZK_OK;
}
static HscanDev hscan_dev_of(const OpenWs& W, unsigned npoly, uint32_t pstride) {
    HscanDev H = {};
    H.pts = W.pts; H.pstride = pstride; H.npoly = npoly; H.K = W.K; H.nb = W.nb;
    H.carry_poly = -1; H.tcarry = W.tcarry; H.btot = W.btot;
    for (int k = 0; k < HSCAN_DEV_POLYS; k++) H.len[k] = 1;
    return H;
}
// values[v] = f_v(points[v]); q_v = (f_v - f_v(points[v])) / (X - points[v]), len - 1 coefficients, where q is given (q == f: in place)
static int poly_open_rows_dev(Slot* s, hipStream_t st, const Fr* f, size_t in_stride, size_t len, size_t rows, const Fr* points, Fr* q, size_t q_stride, Fr* values) {
    OpenWs W;
    ZK_TRY(open_ws_take(s, len, rows, 1, 3, 0, &W));
    for (size_t first = 0; first < rows; first += W.chunk) {
        const unsigned R = (unsigned)std::min(W.chunk, rows - first);
        ZK_LAUNCH(s, st, "plonk_horner_points_rows", k_hscan_points_dev, dim3(grid_of(R)), dim3(256), 0, points + first, (uint32_t)R, W.K, W.pts);
        HscanDev H = hscan_dev_of(W, 1, 3);
        H.f[0] = f + first * in_stride; H.stride[0] = in_stride; H.len[0] = len;
        H.total = values + first; H.tstride = 1;
        if (q) { H.carry_poly = 0; H.q = q + first * q_stride; H.qstride = q_stride; }
        ZK_TRY(hscan_dev_passes(s, st, H, R));
    }
    return ZK_OK;
}
// round 4 (zk_bn254_plonk_linearize_batch_dev in zkmi.h says what goes where)
int linearize_rows_dev(Slot* s, hipStream_t st, const PlonkPK* P, const Fr* l, const Fr* r, const Fr* o, const Fr* z, size_t in_stride, const Fr* h,
                       size_t h_stride, size_t rows, const Fr* d_alpha, const Fr* d_beta, const Fr* d_gamma, const Fr* d_zeta, Fr* values, Fr* zquot, Fr* lin,
                       Fr* fh, size_t out_stride) {
    const size_t n = P->n;
    OpenWs W;
    ZK_TRY(open_ws_take(s, n + 3, rows, 6, LIN_PT, 0, &W));
    LinRowsArgs A;
    A.s3 = P->s3; A.ql = P->ql; A.qr = P->qr; A.qm = P->qm; A.qo = P->qo; A.cqk = P->cqk;
    A.u = to_dev(P->u); A.uu = to_dev(P->u * P->u);
    A.in_stride = in_stride; A.h_stride = h_stride; A.out_stride = out_stride; A.pts = W.pts; A.n = (uint32_t)n;
    for (size_t first = 0; first < rows; first += W.chunk) {
        const unsigned R = (unsigned)std::min(W.chunk, rows - first);
        const size_t in = first * in_stride, out = first * out_stride;
        ZK_LAUNCH(s, st, "plonk_linearize_points_rows", k_lin_points_rows, dim3(grid_of(R)), dim3(256), 0, d_zeta + first, d_alpha + first, (uint32_t)R, W.K, P->logn,
                  to_dev(P->gen), to_dev(P->card_inv), W.pts);
        HscanDev H = hscan_dev_of(W, 6, LIN_PT);
        const Fr* p6[6] = {l + in, r + in, o + in, P->s1, P->s2, z + in};
        const size_t l6[6] = {n + 2, n + 2, n + 2, n, n, n + 3};
        for (int k = 0; k < 6; k++) { H.f[k] = p6[k]; H.len[k] = l6[k]; H.stride[k] = (k == 3 || k == 4) ? 0 : in_stride; H.pt[k] = k == 5; }
        H.total = values + 8 * first + 2; H.tstride = 8;
        H.carry_poly = 5; H.q = zquot + out; H.qstride = out_stride;
        ZK_TRY(hscan_dev_passes(s, st, H, R));
        A.z = z + in; A.h = h + first * h_stride; A.lin = lin + out; A.fh = fh + out;
        A.alpha = d_alpha + first; A.beta = d_beta + first; A.gamma = d_gamma + first; A.zeta = d_zeta + first; A.values = values + 8 * first;
        ZK_LAUNCH(s, st, "plonk_linearize_fold_rows", k_lin_fold_rows, dim3(grid_of(n + 3), R), dim3(256), 0, A);
        HscanDev G = hscan_dev_of(W, 2, LIN_PT);
        G.f[0] = fh + out; G.len[0] = n + 2; G.stride[0] = out_stride;
        G.f[1] = lin + out; G.len[1] = n + 3; G.stride[1] = out_stride;
        G.total = values + 8 * first; G.tstride = 8;
        ZK_TRY(hscan_dev_passes(s, st, G, R));
    }
    return ZK_OK;
}
// round 5's polynomial (zk_bn254_plonk_open_batch_dev)
int open_rows_dev(Slot* s, hipStream_t st, const PlonkPK* P, const Fr* fh, const Fr* lin, const Fr* l, const Fr* r, const Fr* o, size_t in_stride, size_t rows,
                  const Fr* d_zeta, const Fr* d_kg, Fr* q, size_t out_stride, Fr* value) {
    const size_t n = P->n;
    OpenWs W;
    ZK_TRY(open_ws_take(s, n + 3, rows, 1, 3, n + 3, &W));
    for (size_t first = 0; first < rows; first += W.chunk) {
        const unsigned R = (unsigned)std::min(W.chunk, rows - first);
        const size_t in = first * in_stride;
        ZK_LAUNCH(s, st, "plonk_horner_points_rows", k_hscan_points_dev, dim3(grid_of(R)), dim3(256), 0, d_zeta + first, (uint32_t)R, W.K, W.pts);
        ZK_LAUNCH(s, st, "plonk_open_fold_rows", k_open_fold_rows, dim3(grid_of(n + 3), R), dim3(256), 0, fh + in, lin + in, l + in, r + in, o + in, in_stride,
                  (const Fr*)P->s1, (const Fr*)P->s2, d_kg + first, (uint32_t)n, W.fold);
        HscanDev H = hscan_dev_of(W, 1, 3);
        H.f[0] = W.fold; H.stride[0] = n + 3; H.len[0] = n + 3;
        H.total = value + first; H.tstride = 1;
        H.carry_poly = 0; H.q = q + first * out_stride; H.qstride = out_stride;
        ZK_TRY(hscan_dev_passes(s, st, H, R));
    }
    return ZK_OK;
}

// a key that is not being freed, kept alive by `alive` (zk_bn254_plonk_quotient_batch_dev says why the shared lock is granted at once)
int live_key(uint64_t handle, PlonkPK** P, std::shared_ptr<std::shared_mutex>* live, std::shared_lock<std::shared_mutex>* alive) {
    std::lock_guard<std::mutex> lk(g_ppk_mu);
    auto it = g_ppks.find(handle);
    if (it == g_ppks.end()) return set_err(ZK_ERR_HANDLE, "unknown PLONK proving-key handle %llu", (unsigned long long)handle);
    *P = it->second;
    *live = (*P)->live;
    *alive = std::shared_lock<std::shared_mutex>(**live);
    return ZK_OK;
}

}  // namespace zkmi

using namespace zkmi;

extern "C" {

int zk_bn254_plonk_synth_qk_dev(void* d_qk, const void* d_ql, const void* d_qr, const void* d_qo, const void* d_qm, const void* d_xa, const void* d_xb,
                                const void* d_xc, const void* d_solution, size_t nc, void* stream) {
    if (nc && (!d_qk || !d_ql || !d_qr || !d_qo || !d_qm || !d_xa || !d_xb || !d_xc || !d_solution)) return set_err(ZK_ERR_ARG, "null pointer");
    SlotGuard g;
    ZK_TRY(acquire_slot(&g.s));
    hipStream_t st = stream ? (hipStream_t)stream : g.s->stream;
    if (nc)
        ZK_LAUNCH(g.s, st, "plonk_synth_qk", k_synth_qk, dim3(grid_of(nc)), dim3(256), 0, (Fr*)d_qk, (const Fr*)d_ql, (const Fr*)d_qr, (const Fr*)d_qo, (const Fr*)d_qm,
                  (const uint32_t*)d_xa, (const uint32_t*)d_xb, (const uint32_t*)d_xc, (const Fr*)d_solution, nc);
    return stream ? ZK_OK : slot_sync(g.s, st);
}

int zk_bn254_plonk_setup(const zk_plonk_circuit* c, uint64_t srs, uint64_t* handle, zk_plonk_vk* vk) {
    ZK_ON_ENTRY_OF(srs);
    if (!c || !handle) return set_err(ZK_ERR_ARG, "null pointer");
    const size_t npub = c->n_public, nc = c->n_constraints;
    if (nc && (!c->ql || !c->qr || !c->qo || !c->qm || !c->qk || !c->xa || !c->xb || !c->xc)) return set_err(ZK_ERR_ARG, "null pointer");
    if (npub > c->n_vars) return set_err(ZK_ERR_ARG, "more public inputs than variables");
    for (size_t i = 0; i < nc; i++)
        if (c->xa[i] >= c->n_vars || c->xb[i] >= c->n_vars || c->xc[i] >= c->n_vars) return set_err(ZK_ERR_ARG, "gate %zu names a wire outside the %zu variables", i, c->n_vars);
    unsigned logn, logN4;
    ZK_TRY(domains_for(nc + npub, &logn, &logN4));
    ZK_TRY(ensure_init());
    ZK_TRY(check_srs(srs, (size_t)1 << logn));
    std::unique_ptr<PlonkPK, void (*)(PlonkPK*)> P(new PlonkPK(), pk_destroy);
    P->logn = logn; P->logN4 = logN4; P->log_rho = logN4 - logn;
    P->n = (size_t)1 << logn; P->N4 = (size_t)1 << logN4;
    P->n_public = npub; P->n_constraints = nc; P->n_vars = c->n_vars;
    P->srs = srs;
    const size_t n = P->n;
    SlotGuard g;
    ZK_TRY(acquire_slot(&g.s));
    Slot* s = g.s;
    hipStream_t st = s->stream;
    ZK_TRY(s->reserve(5 * nc * sizeof(Fr) + 3 * n * 4 + 65536));
    // selectors: Lagrange form [placeholders | gates | 0], then canonical
    Fr** dst[6] = {&P->ql, &P->qr, &P->qm, &P->qo, &P->cqk, &P->lqk};
    const void* src[6] = {c->ql, c->qr, c->qm, c->qo, c->qk, c->qk};
    const Fr minus_one = to_dev(HFr::zero() - HFr::one());
    Fr* stage[5] = {};
    if (!c->coeffs_on_device)
        for (int k = 0; k < 5; k++) {
            stage[k] = (Fr*)s->alloc(nc * sizeof(Fr) + 16);
            if (nc) ZK_HIP(hipMemcpyAsync(stage[k], src[k], nc * sizeof(Fr), hipMemcpyHostToDevice, st));
        }
    for (int k = 0; k < 6; k++) {
        ZK_TRY(pk_alloc(P.get(), dst[k], n));
        const Fr* from = c->coeffs_on_device ? (const Fr*)src[k] : stage[k < 5 ? k : 4];
        ZK_LAUNCH(s, st, "plonk_place_selector", k_place_selector, dim3(grid_of(n)), dim3(256), 0, *dst[k], from, (uint32_t)npub, (uint32_t)nc, (uint32_t)n,
                  k == 0 ? minus_one : Fr::zero());
        if (k < 5) ZK_TRY(to_canonical(s, st, *dst[k], logn));  // LQk stays in Lagrange form (the prover completes it with the public inputs)
    }
    // wire ids (prove's gather) and the permutation
    uint32_t** wid[3] = {&P->xa, &P->xb, &P->xc};
    const uint32_t* wsrc[3] = {c->xa, c->xb, c->xc};
    for (int k = 0; k < 3; k++) {
        Fr* tmp;
        ZK_TRY(pk_alloc(P.get(), &tmp, (nc * 4 + 31) / 32 + 1));
        *wid[k] = (uint32_t*)tmp;
        if (nc) ZK_HIP(hipMemcpyAsync(*wid[k], wsrc[k], nc * 4, hipMemcpyHostToDevice, st));
    }
    std::vector<uint32_t> perm;
    build_permutation(n, npub, nc, c->n_vars, c->xa, c->xb, c->xc, &perm);
    uint32_t* d_perm;
    {
        Fr* tmp;
        ZK_TRY(pk_alloc(P.get(), &tmp, (3 * n * 4 + 31) / 32 + 1));
        P->perm = d_perm = (uint32_t*)tmp;
    }
    ZK_HIP(hipMemcpyAsync(d_perm, perm.data(), 3 * n * 4, hipMemcpyHostToDevice, st));
    ZK_TRY(pk_alloc(P.get(), &P->s1, n));
    ZK_TRY(pk_alloc(P.get(), &P->s2, n));
    ZK_TRY(pk_alloc(P.get(), &P->s3, n));
    ZK_TRY(make_sigma(P.get(), s, st, d_perm));
    Fr* sc[3] = {P->s1, P->s2, P->s3};
    for (int k = 0; k < 3; k++) {  // S1..S3 canonical
        ZK_HIP(hipMemcpyAsync(sc[k], P->sig + k * n, n * sizeof(Fr), hipMemcpyDeviceToDevice, st));
        ZK_TRY(to_canonical(s, st, sc[k], logn));
    }
    ZK_TRY(finish_pk(P.get(), s, st));
    // verifying key: commitments to the canonical polynomials
    const Fr* cm[8] = {P->s1, P->s2, P->s3, P->ql, P->qr, P->qm, P->qo, P->cqk};
    Affine<HFp>* cmo[8] = {&P->vk_s[0], &P->vk_s[1], &P->vk_s[2], &P->vk_ql, &P->vk_qr, &P->vk_qm, &P->vk_qo, &P->vk_qk};
    for (int k = 0; k < 8; k++) ZK_TRY(commit(P.get(), s, st, cm[k], n, cmo[k]));
    P->vk_consistent = true;
    if (vk) {
        memset(vk, 0, sizeof *vk);
        vk->size = n;
        vk->n_public = npub;
        memcpy(&vk->size_inv, &P->card_inv, 32);
        memcpy(&vk->generator, &P->gen, 32);
        memcpy(&vk->coset_shift, &P->u, 32);
        memcpy(vk->s, P->vk_s, 3 * 64);
        memcpy(&vk->ql, &P->vk_ql, 64); memcpy(&vk->qr, &P->vk_qr, 64); memcpy(&vk->qm, &P->vk_qm, 64);
        memcpy(&vk->qo, &P->vk_qo, 64); memcpy(&vk->qk, &P->vk_qk, 64);
    }
    return register_pk(P.release(), handle);
}

int zk_bn254_plonk_pk_load(const zk_plonk_pk* k, uint64_t srs, uint64_t* handle) {
    ZK_ON_ENTRY_OF(srs);
    if (!k || !handle) return set_err(ZK_ERR_ARG, "null pointer");
    if (!k->ql || !k->qr || !k->qm || !k->qo || !k->cqk || !k->lqk || !k->s1 || !k->s2 || !k->s3 || !k->permutation || !k->vk_s || !k->vk_ql || !k->vk_qr ||
        !k->vk_qm || !k->vk_qo || !k->vk_qk || (k->n_constraints && (!k->xa || !k->xb || !k->xc)))
        return set_err(ZK_ERR_ARG, "null pointer");
    unsigned logn, logN4;
    ZK_TRY(check_counts(k->n_public, k->n_vars, k->n_constraints));
    ZK_TRY(domains_for(k->n_constraints + k->n_public, &logn, &logN4));
    if (logn != k->log_n) return set_err(ZK_ERR_ARG, "log_n = %u does not match %zu constraints + %zu public inputs", k->log_n, k->n_constraints, k->n_public);
    const size_t n = (size_t)1 << logn;
    for (size_t i = 0; i < k->n_constraints; i++)
        if (k->xa[i] >= k->n_vars || k->xb[i] >= k->n_vars || k->xc[i] >= k->n_vars) return set_err(ZK_ERR_ARG, "gate %zu names a wire outside the %zu variables", i, k->n_vars);
    std::vector<uint32_t> perm(3 * n);
    for (size_t i = 0; i < 3 * n; i++) {
        if (k->permutation[i] < 0 || (size_t)k->permutation[i] >= 3 * n) return set_err(ZK_ERR_ARG, "Permutation[%zu] out of range", i);
        perm[i] = (uint32_t)k->permutation[i];
    }
    ZK_TRY(ensure_init());
    ZK_TRY(check_srs(srs, n));
    std::unique_ptr<PlonkPK, void (*)(PlonkPK*)> P(new PlonkPK(), pk_destroy);
    P->logn = logn; P->logN4 = logN4; P->log_rho = logN4 - logn;
    P->n = n; P->N4 = (size_t)1 << logN4;
    P->n_public = k->n_public; P->n_constraints = k->n_constraints; P->n_vars = k->n_vars;
    P->srs = srs;
    SlotGuard g;
    ZK_TRY(acquire_slot(&g.s));
    Slot* s = g.s;
    hipStream_t st = s->stream;
    ZK_TRY(s->reserve(3 * n * 4 + 65536));
    Fr** dst[9] = {&P->ql, &P->qr, &P->qm, &P->qo, &P->cqk, &P->lqk, &P->s1, &P->s2, &P->s3};
    const zk_fr* src[9] = {k->ql, k->qr, k->qm, k->qo, k->cqk, k->lqk, k->s1, k->s2, k->s3};
    for (int i = 0; i < 9; i++) {
        ZK_TRY(pk_alloc(P.get(), dst[i], n));
        ZK_HIP(hipMemcpyAsync(*dst[i], src[i], n * sizeof(Fr), hipMemcpyHostToDevice, st));
    }
    uint32_t** wid[3] = {&P->xa, &P->xb, &P->xc};
    const uint32_t* wsrc[3] = {k->xa, k->xb, k->xc};
    for (int i = 0; i < 3; i++) {
        Fr* tmp;
        ZK_TRY(pk_alloc(P.get(), &tmp, (k->n_constraints * 4 + 31) / 32 + 1));
        *wid[i] = (uint32_t*)tmp;
        if (k->n_constraints) ZK_HIP(hipMemcpyAsync(*wid[i], wsrc[i], k->n_constraints * 4, hipMemcpyHostToDevice, st));
    }
    uint32_t* d_perm;
    {
        Fr* tmp;
        ZK_TRY(pk_alloc(P.get(), &tmp, (3 * n * 4 + 31) / 32 + 1));
        P->perm = d_perm = (uint32_t*)tmp;
    }
    ZK_HIP(hipMemcpyAsync(d_perm, perm.data(), 3 * n * 4, hipMemcpyHostToDevice, st));
    ZK_TRY(make_sigma(P.get(), s, st, d_perm));
    ZK_TRY(finish_pk(P.get(), s, st));
    memcpy(P->vk_s, k->vk_s, 3 * 64);
    memcpy(&P->vk_ql, k->vk_ql, 64); memcpy(&P->vk_qr, k->vk_qr, 64); memcpy(&P->vk_qm, k->vk_qm, 64);
    memcpy(&P->vk_qo, k->vk_qo, 64); memcpy(&P->vk_qk, k->vk_qk, 64);
    return register_pk(P.release(), handle);
}

// ---- plonk.ProvingKey.ReadFrom / WriteTo (gnark v0.8.0 internal/backend/bn254/plonk/marshal.go  [UPSTREAM-RECALL]; the reference ships the key as
// hex of these bytes: internal/backend/helpers.go:49-60,82-87, produced at main.go:58-78, consumed at main.go:24-37):
//   VerifyingKey.WriteTo  Size u64 | SizeInv | Generator | NbPublicVariables u64 | CosetShift | S[0..2] | Ql Qr Qm Qo Qk (compressed G1)   368 B
//   Domain[0], Domain[1]  Cardinality u64 | CardinalityInv | Generator | GeneratorInv | FrMultiplicativeGen | FrMultiplicativeGenInv      168 B each
//   Ql Qr Qm Qo CQk LQk S1Canonical S2Canonical S3Canonical   each u32 BE length | n x 32 B BE
//   Permutation           3n raw big-endian int64
static const size_t PK_HEAD = PLONK_PK_HEAD;

int zk_bn254_plonk_pk_read(const void* data, size_t len, int is_hex, size_t n_vars, size_t n_constraints, const uint32_t* xa, const uint32_t* xb,
                           const uint32_t* xc, uint64_t srs, uint64_t* handle) {
    ZK_ON_ENTRY_OF(srs);
    if (!data || !handle || (n_constraints && (!xa || !xb || !xc))) return set_err(ZK_ERR_ARG, "null pointer");
    PlonkKeyHeader H;  // every size below comes out of this host-side reading of the header and the nine length prefixes (text_host.hpp)
    {
        std::string e;
        const int rc = plonk_pk_header(data, len, is_hex, n_vars, n_constraints, &H, &e);
        if (rc != ZK_OK) return set_err(rc, "%s", e.c_str());
    }
    const size_t n = H.n, nbytes = H.nbytes;
    const uint64_t npub = H.n_public;
    const unsigned logn = H.logn, logN4 = H.logN4;
    const auto t_start = std::chrono::steady_clock::now();
    for (size_t i = 0; i < n_constraints; i++)
        if (xa[i] >= n_vars || xb[i] >= n_vars || xc[i] >= n_vars) return set_err(ZK_ERR_ARG, "gate %zu names a wire outside the %zu variables", i, n_vars);
    ZK_TRY(ensure_init());
    ZK_TRY(check_srs(srs, n));
    std::unique_ptr<PlonkPK, void (*)(PlonkPK*)> P(new PlonkPK(), pk_destroy);
    P->logn = logn; P->logN4 = logN4; P->log_rho = logN4 - logn;
    P->n = n; P->N4 = (size_t)1 << logN4;
    P->n_public = (size_t)npub; P->n_constraints = n_constraints; P->n_vars = n_vars;
    P->srs = srs;
    SlotGuard g;
    ZK_TRY(acquire_slot(&g.s));
    Slot* s = g.s;
    hipStream_t st = s->stream;
    ZK_TRY(s->reserve(len + nbytes + 65536));
    int* d_status = (int*)s->alloc(64);
    ZK_HIP(hipMemsetAsync(d_status, 0, 4, st));
    uint8_t* d_bytes = (uint8_t*)s->alloc(nbytes + 16);
    if (is_hex) {
        void* d_text = s->alloc(len + 16);
        ZK_TRY(h2d_big(d_text, data, len, st));
        ZK_TRY(hex_decode_dev(s, st, d_text, nbytes, d_bytes, d_status));
    } else {
        ZK_TRY(h2d_big(d_bytes, data, nbytes, st));
    }
    Fr** dst[9] = {&P->ql, &P->qr, &P->qm, &P->qo, &P->cqk, &P->lqk, &P->s1, &P->s2, &P->s3};
    for (int k = 0; k < 9; k++) {
        ZK_TRY(pk_alloc(P.get(), dst[k], n));
        ZK_TRY(fr_from_be_dev(s, st, d_bytes + PK_HEAD + (size_t)k * (4 + 32 * n) + 4, n, *dst[k], d_status));
    }
    {
        Fr* tmp;
        ZK_TRY(pk_alloc(P.get(), &tmp, (3 * n * 4 + 31) / 32 + 1));
        P->perm = (uint32_t*)tmp;
        ZK_LAUNCH(s, st, "plonk_perm_from_be", k_perm_from_be, dim3(grid_of(3 * n)), dim3(256), 0, (const uint32_t*)(d_bytes + PK_HEAD + 9 * (4 + 32 * n)), 3 * n, P->perm, d_status);
    }
    // the verifying key's eight digests: compressed G1 at bytes 112 .. 368
    Affine<Fp>* d_vk = (Affine<Fp>*)s->alloc(8 * 64 + 16);
    ZK_TRY(g1_decompress_dev(s, st, d_bytes + 112, 8, d_vk, d_status));
    Affine<HFp> vkp[8];
    int h_status = 0;
    ZK_HIP(hipMemcpyAsync(vkp, d_vk, sizeof vkp, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipMemcpyAsync(&h_status, d_status, 4, hipMemcpyDeviceToHost, st));
    ZK_TRY(slot_sync(s, st));
    if (h_status & 1) return set_err(ZK_ERR_ARG, "proving key: invalid hex character");
    if (h_status & 2) return set_err(ZK_ERR_ARG, "proving key: invalid fr.Element encoding (value >= r)");
    if (h_status & 4) return set_err(ZK_ERR_ARG, "proving key: invalid compressed G1 point in the verifying key");
    if (h_status & 8) return set_err(ZK_ERR_ARG, "proving key: Permutation entry out of range");
    memcpy(P->vk_s, vkp, 3 * 64);
    P->vk_ql = vkp[3]; P->vk_qr = vkp[4]; P->vk_qm = vkp[5]; P->vk_qo = vkp[6]; P->vk_qk = vkp[7];
    uint32_t** wid[3] = {&P->xa, &P->xb, &P->xc};
    const uint32_t* wsrc[3] = {xa, xb, xc};
    for (int i = 0; i < 3; i++) {
        Fr* tmp;
        ZK_TRY(pk_alloc(P.get(), &tmp, (n_constraints * 4 + 31) / 32 + 1));
        *wid[i] = (uint32_t*)tmp;
        if (n_constraints) ZK_HIP(hipMemcpyAsync(*wid[i], wsrc[i], n_constraints * 4, hipMemcpyHostToDevice, st));
    }
    const auto t_decoded = std::chrono::steady_clock::now();
    ZK_TRY(make_sigma(P.get(), s, st, P->perm));
    ZK_TRY(finish_pk(P.get(), s, st));
    prof_host("export.pk_text_to_device", std::chrono::duration<double, std::milli>(t_decoded - t_start).count());
    prof_host("export.pk_coset_forms", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_decoded).count());
    return register_pk(P.release(), handle);
}

int zk_bn254_plonk_pk_write(uint64_t handle, int as_hex, void* out, size_t cap, size_t* out_len) {
    ZK_ON_ENTRY_OF(handle);
    if (!out || !out_len) return set_err(ZK_ERR_ARG, "null pointer");
    PlonkPK* P;
    std::shared_ptr<std::mutex> mu;
    {
        std::lock_guard<std::mutex> lk(g_ppk_mu);
        auto it = g_ppks.find(handle);
        if (it == g_ppks.end()) return set_err(ZK_ERR_HANDLE, "unknown PLONK proving-key handle %llu", (unsigned long long)handle);
        P = it->second;
        mu = P->mu;
    }
    std::lock_guard<std::mutex> key_lock(*mu);
    {
        std::lock_guard<std::mutex> lk(g_ppk_mu);
        auto it = g_ppks.find(handle);
        if (it == g_ppks.end() || it->second != P) return set_err(ZK_ERR_HANDLE, "PLONK proving key %llu was freed", (unsigned long long)handle);
    }
    const size_t n = P->n, nbytes = PK_HEAD + 9 * (4 + 32 * n) + 24 * n, need = as_hex ? 2 * nbytes : nbytes;
    *out_len = need;
    if (cap < need) return set_err(ZK_ERR_ARG, "output holds %zu bytes, %zu needed", cap, need);
    uint8_t head[PK_HEAD];
    memset(head, 0, sizeof head);
    auto put64 = [](uint8_t* p, uint64_t v) { for (int i = 0; i < 8; i++) p[i] = (uint8_t)(v >> (56 - 8 * i)); };
    put64(head, n);
    fr_to_be(P->card_inv, head + 8);
    fr_to_be(P->gen, head + 40);
    put64(head + 72, P->n_public);
    fr_to_be(P->u, head + 80);
    const Affine<HFp>* vkp[8] = {&P->vk_s[0], &P->vk_s[1], &P->vk_s[2], &P->vk_ql, &P->vk_qr, &P->vk_qm, &P->vk_qo, &P->vk_qk};
    for (int k = 0; k < 8; k++) g1_compress(*vkp[k], head + 112 + 32 * k);
    SlotGuard g;
    ZK_TRY(acquire_slot(&g.s));
    Slot* s = g.s;
    hipStream_t st = s->stream;
    Domain *d0, *d1;
    ZK_TRY(get_domain(s, st, P->logn, 0, &d0));
    ZK_TRY(get_domain(s, st, P->logN4, 0, &d1));
    Domain* dd[2] = {d0, d1};
    for (int k = 0; k < 2; k++) {
        uint8_t* o = head + 368 + 168 * k;
        put64(o, (uint64_t)1 << dd[k]->logn);
        fr_to_be(dd[k]->card_inv, o + 8);
        fr_to_be(dd[k]->gen, o + 40);
        fr_to_be(dd[k]->gen_inv, o + 72);
        fr_to_be(dd[k]->coset, o + 104);
        fr_to_be(dd[k]->coset_inv, o + 136);
    }
    ZK_TRY(s->reserve(3 * nbytes + 65536));
    uint8_t* d_bytes = (uint8_t*)s->alloc(nbytes + 16);
    ZK_HIP(hipMemcpyAsync(d_bytes, head, PK_HEAD, hipMemcpyHostToDevice, st));
    const Fr* src[9] = {P->ql, P->qr, P->qm, P->qo, P->cqk, P->lqk, P->s1, P->s2, P->s3};
    uint8_t pre[4] = {(uint8_t)(n >> 24), (uint8_t)(n >> 16), (uint8_t)(n >> 8), (uint8_t)n};
    for (int k = 0; k < 9; k++) {
        uint8_t* o = d_bytes + PK_HEAD + (size_t)k * (4 + 32 * n);
        ZK_HIP(hipMemcpyAsync(o, pre, 4, hipMemcpyHostToDevice, st));
        ZK_TRY(fr_to_be_dev(s, st, src[k], n, o + 4));
    }
    ZK_HIP(hipStreamSynchronize(st));  // `pre` and `head` live on this stack frame
    ZK_LAUNCH(s, st, "plonk_perm_to_be", k_perm_to_be, dim3(grid_of(3 * n)), dim3(256), 0, (const uint32_t*)P->perm, 3 * n, (uint32_t*)(d_bytes + PK_HEAD + 9 * (4 + 32 * n)));
    if (as_hex) {
        void* d_text = s->alloc(2 * nbytes + 16);
        ZK_TRY(hex_encode_dev(s, st, d_bytes, nbytes, d_text));
        ZK_HIP(hipMemcpyAsync(out, d_text, 2 * nbytes, hipMemcpyDeviceToHost, st));
    } else {
        ZK_HIP(hipMemcpyAsync(out, d_bytes, nbytes, hipMemcpyDeviceToHost, st));
    }
    return slot_sync(s, st);
}

int zk_bn254_plonk_pk_info(uint64_t handle, size_t* domain_size, size_t* n_public, size_t* n_constraints, size_t* n_vars) {
    ZK_ON_ENTRY_OF(handle);
    std::lock_guard<std::mutex> lk(g_ppk_mu);
    auto it = g_ppks.find(handle);
    if (it == g_ppks.end()) return set_err(ZK_ERR_HANDLE, "unknown PLONK proving key %llu", (unsigned long long)handle);
    const PlonkPK* P = it->second;
    if (domain_size) *domain_size = P->n;
    if (n_public) *n_public = P->n_public;
    if (n_constraints) *n_constraints = P->n_constraints;
    if (n_vars) *n_vars = P->n_vars;
    return ZK_OK;
}

int zk_bn254_plonk_pk_bytes(uint64_t handle, size_t* bytes) {
    ZK_ON_ENTRY_OF(handle);
    if (!bytes) return set_err(ZK_ERR_ARG, "null pointer");
    std::lock_guard<std::mutex> lk(g_ppk_mu);
    auto it = g_ppks.find(handle);
    if (it == g_ppks.end()) return set_err(ZK_ERR_HANDLE, "unknown PLONK proving key %llu", (unsigned long long)handle);
    *bytes = it->second->bytes;
    return ZK_OK;
}

// The SRS in Lagrange form over this key's domain, built once (lagrange.hip: n/2 log2 n + n point-by-scalar multiplications -- 0.15 s at 2^19 gates, 1.3 s at 2^22):
// from then on zk_bn254_plonk_prove commits l, r, o from the wire values (same digests, a quarter to a third of the additions for the scalars of a real
// circuit).  For a prover that keeps its key; needs the SRS on one device entry.  A key that has it: ZK_OK, untouched.
int zk_bn254_plonk_pk_lagrange_srs(uint64_t handle) {
    ZK_ON_ENTRY_OF(handle);
    PlonkPK* P;
    std::shared_ptr<std::mutex> mu;
    {
        std::lock_guard<std::mutex> lk(g_ppk_mu);
        auto it = g_ppks.find(handle);
        if (it == g_ppks.end()) return set_err(ZK_ERR_HANDLE, "unknown PLONK proving-key handle %llu", (unsigned long long)handle);
        P = it->second;
        mu = P->mu;
    }
    std::lock_guard<std::mutex> work(*mu);
    {
        std::lock_guard<std::mutex> lk(g_ppk_mu);
        auto it = g_ppks.find(handle);
        if (it == g_ppks.end() || it->second != P) return set_err(ZK_ERR_HANDLE, "PLONK proving key %llu was freed", (unsigned long long)handle);
    }
    if (P->lag_srs) return ZK_OK;
    uint64_t h = 0;
    ZK_TRY(zk_bn254_bases_lagrange(P->srs, P->logn, &h));
    P->lag_srs = h;
    const void* d_table = nullptr;
    MsmTable tab;
    size_t nb = 0;
    if (bases_table(h, &d_table, &tab, &nb) == ZK_OK) P->bytes += (P->n + 2) * (64 + (d_table ? (size_t)tab.rows() * msm_table_entry_bytes(0) : 0));
    return ZK_OK;
}

int zk_bn254_plonk_pk_free(uint64_t handle) {
    ZK_ON_ENTRY_OF(handle);
    PlonkPK* P;
    {
        std::lock_guard<std::mutex> lk(g_ppk_mu);
        auto it = g_ppks.find(handle);
        if (it == g_ppks.end()) return set_err(ZK_ERR_HANDLE, "unknown PLONK proving-key handle %llu", (unsigned long long)handle);
        P = it->second;
        g_ppks.erase(it);
    }
    { std::lock_guard<std::mutex> lk(*P->mu); }  // a proof in flight finishes first
    {   // and so does every call that reads the key's tables
        const std::shared_ptr<std::shared_mutex> live = P->live;
        std::unique_lock<std::shared_mutex> lk(*live);
    }
    pk_destroy(P);
    return ZK_OK;
}

int zk_bn254_plonk_pk_export(uint64_t handle, int which, zk_fr* out, size_t cnt) {
    ZK_ON_ENTRY_OF(handle);
    if (!out) return set_err(ZK_ERR_ARG, "null pointer");
    std::lock_guard<std::mutex> lk(g_ppk_mu);
    auto it = g_ppks.find(handle);
    if (it == g_ppks.end()) return set_err(ZK_ERR_HANDLE, "unknown PLONK proving-key handle %llu", (unsigned long long)handle);
    PlonkPK* P = it->second;
    const Fr* src[9] = {P->ql, P->qr, P->qm, P->qo, P->cqk, P->s1, P->s2, P->s3, P->lqk};
    if (which < 0 || which > 8 || cnt > P->n) return set_err(ZK_ERR_ARG, "bad polynomial index / length");
    ZK_HIP(hipMemcpy(out, src[which], cnt * sizeof(Fr), hipMemcpyDeviceToHost));
    return ZK_OK;
}

int zk_bn254_plonk_prove(uint64_t handle, const void* solution, size_t n_vars, int on_device, const zk_fr blinders[9], const zk_fr* challenges,
                         uint8_t proof_out[ZK_PLONK_PROOF_BYTES]) {
    ZK_ON_ENTRY_OF(handle);
    if (!solution || !blinders || !proof_out) return set_err(ZK_ERR_ARG, "null pointer");
    PlonkPK* P;
    std::shared_ptr<std::mutex> mu;
    {
        std::lock_guard<std::mutex> lk(g_ppk_mu);
        auto it = g_ppks.find(handle);
        if (it == g_ppks.end()) return set_err(ZK_ERR_HANDLE, "unknown PLONK proving-key handle %llu", (unsigned long long)handle);
        P = it->second;
        mu = P->mu;
    }
    std::lock_guard<std::mutex> proof_lock(*mu);
    {   // the key may have been freed between the lookup and the lock (pk_free waits on this mutex and then destroys it)
        std::lock_guard<std::mutex> lk(g_ppk_mu);
        auto it = g_ppks.find(handle);
        if (it == g_ppks.end() || it->second != P) return set_err(ZK_ERR_HANDLE, "PLONK proving key %llu was freed", (unsigned long long)handle);
    }
    if (n_vars != P->n_vars) return set_err(ZK_ERR_LEN, "len(solution) = %zu != %zu variables of the constraint system", n_vars, P->n_vars);
    const size_t n = P->n, N4 = P->N4, npub = P->n_public;
    const unsigned logn = P->logn, logN4 = P->logN4;
    SlotGuard g;
    ZK_TRY(acquire_slot(&g.s));
    Slot* s = g.s;
    hipStream_t st = s->stream;
    ZK_TRY(s->reserve(n_vars * sizeof(Fr) + 2 * scan_need(n + 8) + 65536));
    HFr bl[9], pin[5];
    memcpy(bl, blinders, sizeof bl);
    if (challenges) memcpy(pin, challenges, sizeof pin);
    const Fr* d_sol = (const Fr*)solution;
    if (!on_device) {
        Fr* t = (Fr*)s->alloc(n_vars * sizeof(Fr) + 16);
        if (n_vars) ZK_HIP(hipMemcpyAsync(t, solution, n_vars * sizeof(Fr), hipMemcpyHostToDevice, st));
        d_sol = t;
    }
    ScanBufs SB;
    ZK_TRY(scan_bufs(s, n + 8, &SB));
    Fr* d_vals = (Fr*)s->alloc(16 * sizeof(Fr));   // evaluation results
    // small-domain buffers (n + 8 elements each) inside the key's workspace
    const size_t S = n + 8;
    Fr* W = P->w_small;
    Fr *l_lag = W, *r_lag = W + S, *o_lag = W + 2 * S, *bl_ = W + 3 * S, *br_ = W + 4 * S, *bo_ = W + 5 * S, *bz_ = W + 6 * S, *num = W + 7 * S, *den = W + 8 * S,
       *qkc = W + 9 * S, *lin = W + 10 * S, *fh = W + 11 * S, *fold = W + 12 * S, *quo = W + 13 * S;
    Domain* d0;
    ZK_TRY(get_domain(s, st, logn, DOM_TW, &d0));

    // wall clock of the protocol's rounds (reported beside the kernels when profiling is on): each ends in a digest the next challenge needs
    auto lap_t = std::chrono::steady_clock::now();
    auto lap = [&](const char* name) {
        const auto t1 = std::chrono::steady_clock::now();
        prof_host(name, std::chrono::duration<double, std::milli>(t1 - lap_t).count());
        lap_t = t1;
    };
    // ---- l, r, o
    ZK_LAUNCH(s, st, "plonk_gather_lro", k_gather_lro, dim3(grid_of(n)), dim3(256), 0, d_sol, (const uint32_t*)P->xa, (const uint32_t*)P->xb, (const uint32_t*)P->xc,
              (uint32_t)npub, (uint32_t)P->n_constraints, (uint32_t)n, l_lag, r_lag, o_lag);
    std::vector<HFr> pub(npub);
    if (npub) ZK_HIP(hipMemcpyAsync(pub.data(), d_sol, npub * sizeof(Fr), hipMemcpyDeviceToHost, st));
    ZK_TRY(slot_sync(s, st));  // the public inputs are on the host (the transcript binds them); the stream is still almost empty here
    Fr* lag3[3] = {l_lag, r_lag, o_lag};
    Fr* can3[3] = {bl_, br_, bo_};
    Affine<HFp> c_lro[3], c_z, c_h[3], c_zopen, c_lin, c_batch;
    // a group of independent commitments + the work the main stream does meanwhile
    auto commit_group = [&](int cnt, const Fr* const* polys, const size_t* lens, Affine<HFp>* outs, const std::function<int()>& meanwhile) -> int {
        if (cnt == 3 && BatchCommit3::possible(P->srs, lens)) {
            BatchCommit3 bc;
            ZK_TRY(slot_sync(s, st));
            bc.start(P->srs, polys, lens[0]);
            int rc = meanwhile();
            const int r2 = bc.join();
            if (rc == ZK_OK) rc = r2;
            for (int k = 0; k < 3; k++) outs[k] = bc.out[k];
            return rc;
        }
        AsyncCommit ac[3];
        ZK_TRY(slot_sync(s, st));
        for (int k = 0; k < cnt; k++) ac[k].start(P, polys[k], lens[k]);
        int rc = meanwhile();
        for (int k = 0; k < cnt; k++) {
            int r2 = ac[k].join();
            if (rc == ZK_OK) rc = r2;
            outs[k] = ac[k].out;
        }
        return rc;
    };
    // canonical forms of l, r, o with their blinding (rounds 3-5 need them whichever way the digests are made)
    auto lro_canonical = [&]() -> int {
        for (int k = 0; k < 3; k++) {
            ZK_HIP(hipMemcpyAsync(can3[k], lag3[k], n * sizeof(Fr), hipMemcpyDeviceToDevice, st));
            ZK_HIP(hipMemsetAsync(can3[k] + n, 0, 8 * sizeof(Fr), st));
            ZK_TRY(to_canonical(s, st, can3[k], logn));
            BlindArgs B;
            B.k = 2;
            B.b[0] = to_dev(bl[2 * k]); B.b[1] = to_dev(bl[2 * k + 1]); B.b[2] = Fr::zero();
            ZK_LAUNCH(s, st, "plonk_blind", k_blind, dim3(1), dim3(64), 0, can3[k], (uint32_t)n, B);
        }
        return ZK_OK;
    };
    // the three commitments, while this stream already evaluates l, r, o on the big coset (no challenge needed for that)
    const Fr* small5[5] = {bl_, br_, bo_, bz_, qkc};
    const size_t len5[5] = {n + 2, n + 2, n + 2, n + 3, n};
    const size_t lens_lag[3] = {n + 2, n + 2, n + 2};
    if (P->lag_srs && BatchCommit3::possible(P->lag_srs, lens_lag)) {
        // From the WIRE VALUES against the SRS's Lagrange form (lagrange.hip): [l] = sum_i l_i [L_i(tau)] + b0 [tau^n - 1] + b1 [tau^(n+1) - tau] -- the same three
        // points, from scalars that are bits and words instead of uniform coefficients, and without waiting for the inverse transforms (they run meanwhile).
        for (int k = 0; k < 3; k++) {
            BlindArgs B;
            B.k = 2;
            B.b[0] = to_dev(bl[2 * k]); B.b[1] = to_dev(bl[2 * k + 1]); B.b[2] = Fr::zero();
            ZK_LAUNCH(s, st, "plonk_blind_tail", k_blind_tail, dim3(1), dim3(64), 0, lag3[k], (uint32_t)n, B);
        }
        ZK_TRY(slot_sync(s, st));
        BatchCommit3 bc;
        bc.start(P->lag_srs, lag3, n + 2, true);
        int rc = lro_canonical();
        for (int k = 0; k < 3 && rc == ZK_OK; k++) rc = to_big_coset(s, st, P->w_big[k], small5[k], len5[k], P);
        const int r2 = bc.join();
        if (rc == ZK_OK) rc = r2;
        ZK_TRY(rc);
        for (int k = 0; k < 3; k++) c_lro[k] = bc.out[k];
    } else {
        ZK_TRY(lro_canonical());
        const Fr* polys[3] = {bl_, br_, bo_};
        const size_t lens[3] = {n + 2, n + 2, n + 2};
        ZK_TRY(commit_group(3, polys, lens, c_lro, [&]() -> int {
            for (int k = 0; k < 3; k++) ZK_TRY(to_big_coset(s, st, P->w_big[k], small5[k], len5[k], P));
            return ZK_OK;
        }));
    }

    lap("plonk.round1_lro_committed");
    // ---- gamma, beta (transcript "gamma" binds the verifying key and the public inputs, then the three digests)
    FsTranscript fs{"gamma", "beta", "alpha", "zeta"};
    for (const Affine<HFp>* d : {&P->vk_s[0], &P->vk_s[1], &P->vk_s[2], &P->vk_ql, &P->vk_qr, &P->vk_qm, &P->vk_qo, &P->vk_qk}) fs.bind_g1(0, *d);
    for (const HFr& w : pub) fs.bind_fr(0, w);
    for (int k = 0; k < 3; k++) fs.bind_g1(0, c_lro[k]);
    HFr gamma = fs.challenge(0), beta = fs.challenge(1);
    if (challenges) { gamma = pin[0]; beta = pin[1]; }

    // ---- z
    const HFr u = P->u, uu = u * u;
    ZK_TRY(z_chain_dev(s, st, d0->tw, u, P->sig, l_lag, r_lag, o_lag, n, beta, gamma, num, den, W + 14 * S, SB, bz_));
    ZK_HIP(hipMemsetAsync(bz_ + n, 0, 8 * sizeof(Fr), st));
    ZK_TRY(to_canonical(s, st, bz_, logn));
    {
        BlindArgs B;
        B.k = 3;
        for (int i = 0; i < 3; i++) B.b[i] = to_dev(bl[6 + i]);
        ZK_LAUNCH(s, st, "plonk_blind", k_blind, dim3(1), dim3(64), 0, bz_, (uint32_t)n, B);
    }
    // commitment to z; meanwhile: qk completed with the public inputs (canonical), z and qk on the big coset
    {
        const Fr* polys[1] = {bz_};
        const size_t lens[1] = {n + 3};
        ZK_TRY(commit_group(1, polys, lens, &c_z, [&]() -> int {
            if (npub <= PLONK_PI_DIRECT_MAX && logN4 >= 2) {
                ZK_TRY(to_big_coset(s, st, P->w_big[3], small5[3], len5[3], P));
                ZK_LAUNCH(s, st, "plonk_qk_coset", k_qk_coset, dim3(grid_of(P->N4)), dim3(256), 0, (const Fr*)P->e_cqk, (const Fr*)P->e[7], (const Fr*)d_sol, (const Fr*)P->lqk,
                          (uint32_t)npub, logN4, P->log_rho, P->w_big[4]);
                return ZK_OK;
            }
            ZK_HIP(hipMemcpyAsync(qkc, P->lqk, n * sizeof(Fr), hipMemcpyDeviceToDevice, st));
            if (npub) ZK_HIP(hipMemcpyAsync(qkc, d_sol, npub * sizeof(Fr), hipMemcpyDeviceToDevice, st));
            ZK_TRY(to_canonical(s, st, qkc, logn));
            for (int k = 3; k < 5; k++) ZK_TRY(to_big_coset(s, st, P->w_big[k], small5[k], len5[k], P));
            return ZK_OK;
        }));
    }
    lap("plonk.round2_z_committed");
    fs.bind_g1(2, c_z);
    HFr alpha = fs.challenge(2);
    if (challenges) alpha = pin[2];

    // ---- quotient on the coset of the big domain
    {
        QuotArgs A;
        A.el = P->w_big[0]; A.er = P->w_big[1]; A.eo = P->w_big[2]; A.ez = P->w_big[3]; A.eqk = P->w_big[4];
        A.ql = P->e[0]; A.qr = P->e[1]; A.qm = P->e[2]; A.qo = P->e[3]; A.s1 = P->e[4]; A.s2 = P->e[5]; A.s3 = P->e[6]; A.l1 = P->e[7]; A.id = P->e[8];
        A.out = P->w_big[4];
        A.alpha = to_dev(alpha); A.beta = to_dev(beta); A.gamma = to_dev(gamma); A.beta_u = to_dev(beta * u); A.beta_uu = to_dev(beta * uu);
        A.logN4 = logN4; A.log_rho = P->log_rho;
        Domain* d1;
        ZK_TRY(get_domain(s, st, logN4, DOM_TW, &d1));
        // x = g * W^j  =>  x^n = g^n * (W^n)^j, W^n of order rho
        HFr gn = d1->coset, Wn = d1->gen;
        for (unsigned i = 0; i < logn; i++) { gn = gn.sqr(); Wn = Wn.sqr(); }
        HFr cur = gn;
        for (unsigned j = 0; j < (1u << P->log_rho); j++) {
            A.xn_inv[j] = to_dev((cur - HFr::one()).inv());
            cur = cur * Wn;
        }
        for (unsigned j = (1u << P->log_rho); j < 8; j++) A.xn_inv[j] = Fr::zero();
        ZK_LAUNCH(s, st, "plonk_quotient", k_quotient29, dim3(grid_of(N4)), dim3(256), 0, A);
    }
    Fr* h = P->w_big[4];
    ZK_TRY(ntt_dev(s, st, h, logN4, 1, ZK_DIT, 1));  // LagrangeCoset (bit-reversed) -> canonical (regular)
    // the quotient has 3(n+2) coefficients iff the constraints hold: with a violated gate the remainder B = numerator mod (X^n - 1) is not
    // zero and shows up as B_j / (g^N4 - 1) in EVERY block of n coefficients above -- so all of h[3(n+2) .. N4) must vanish (upstream
    // fails earlier, in Solve)
    int* d_flag = (int*)s->alloc(64);
    int h_flag = 0;
    ZK_HIP(hipMemsetAsync(d_flag, 0, 4, st));
    ZK_LAUNCH(s, st, "plonk_quotient_check", k_any_nonzero, dim3(grid_of(N4 - 3 * (n + 2))), dim3(256), 0, (const Fr*)(h + 3 * (n + 2)), N4 - 3 * (n + 2), d_flag);
    ZK_HIP(hipMemcpyAsync(&h_flag, d_flag, 4, hipMemcpyDeviceToHost, st));
    {
        const Fr* polys[3] = {h, h + (n + 2), h + 2 * (n + 2)};
        const size_t lens[3] = {n + 2, n + 2, n + 2};
        ZK_TRY(commit_group(3, polys, lens, c_h, []() -> int { return ZK_OK; }));
    }
    if (h_flag) return set_err(ZK_ERR_ARG, "the solution does not satisfy the constraint system (the quotient is not a polynomial)");
    lap("plonk.round3_quotient_committed");
    for (int k = 0; k < 3; k++) fs.bind_g1(3, c_h[k]);
    HFr zeta = fs.challenge(3);
    if (challenges) zeta = pin[3];

    // ---- evaluations at zeta, opening of z at omega * zeta
    const HFr zeta_sh = zeta * P->gen;
    const Fr* ev_p[5] = {bl_, br_, bo_, P->s1, P->s2};
    const size_t ev_len[5] = {n + 2, n + 2, n + 2, n, n};
    ZK_TRY(poly_eval_batch_dev(s, st, ev_p, ev_len, 5, zeta, SB, d_vals));
    ZK_TRY(poly_divide_dev(s, st, bz_, n + 3, zeta_sh, SB, quo, d_vals + 5));
    HFr ev[8];
    ZK_HIP(hipMemcpyAsync(ev, d_vals, 6 * sizeof(Fr), hipMemcpyDeviceToHost, st));
    ZK_TRY(slot_sync(s, st));  // ev[] is valid, the quotient of z is complete
    AsyncCommit azo;  // the opening of z: finished / joined at the end of the proof, nothing below depends on it
    azo.start(P, quo, n + 2);
    const HFr lz = ev[0], rz = ev[1], oz = ev[2], s1z = ev[3], s2z = ev[4], zu = ev[5];

    // ---- linearised polynomial
    HFr lin_cz, lin_cs3, lin_lag;
    {
        const HFr one = HFr::one();
        HFr c_s3 = (lz + beta * s1z + gamma) * (rz + beta * s2z + gamma) * zu * beta;
        HFr c_zz = HFr::zero() - (lz + beta * zeta + gamma) * (rz + beta * u * zeta + gamma) * (oz + beta * uu * zeta + gamma);
        HFr zn = zeta;
        for (unsigned i = 0; i < logn; i++) zn = zn.sqr();
        HFr lag = (zn - one) * (zeta - one).inv() * alpha * alpha * P->card_inv;
        lin_cz = c_zz; lin_cs3 = c_s3; lin_lag = lag;
        LinArgs A;
        A.bz = bz_; A.s3 = P->s3; A.ql = P->ql; A.qr = P->qr; A.qm = P->qm; A.qo = P->qo; A.cqk = P->cqk; A.out = lin;
        A.c_z = to_dev(c_zz); A.c_s3 = to_dev(c_s3); A.alpha = to_dev(alpha); A.rl = to_dev(lz * rz); A.lz = to_dev(lz); A.rz = to_dev(rz); A.oz = to_dev(oz);
        A.lag = to_dev(lag);
        A.n = (uint32_t)n; A.len = (uint32_t)(n + 3);
        ZK_LAUNCH(s, st, "plonk_linearized", k_linearized, dim3(grid_of(n + 3)), dim3(256), 0, A);
    }
    // Digest of the linearised polynomial.  It is a linear combination of polynomials whose commitments exist already -- the verifying key's and the proof's [Z] --
    // so commit(lin) = (alpha c_z + lag) [Z] + alpha c_s3 [S3] + lz rz [Qm] + lz [Ql] + rz [Qr] + oz [Qo] + [Qk]: the same group element as gnark's kzg.Commit of the
    // polynomial, for seven scalar multiplications on the host (while the GPU runs the kernels above) instead of an (n + 3)-point MSM.  Only for keys whose
    // digests are known to be consistent: Setup's, or -- for a key read from its wire image -- once a first proof has computed both and found them equal.
    Affine<HFp> c_lin_by_linearity;
    {
        const HFr cz_tot = alpha * lin_cz + lin_lag, cs3_tot = alpha * lin_cs3;
        const Affine<HFp> pts[6] = {c_z, P->vk_s[2], P->vk_qm, P->vk_ql, P->vk_qr, P->vk_qo};
        const HFr ks[6] = {cz_tot, cs3_tot, lz * rz, lz, rz, oz};
        XYZZ<HFp> acc = host_multi_scalar_mul(pts, ks, 6);  // one shared doubling chain for the six (1.2 -> 0.45 ms: the host's share of round 4 is the round below 2^20 gates)
        acc.madd(P->vk_qk);
        c_lin_by_linearity = acc.to_affine();
    }
    const bool lin_direct = P->vk_consistent;
    if (lin_direct) c_lin = c_lin_by_linearity;
    else ZK_TRY(commit(P, s, st, lin, n + 3, &c_lin));

    // ---- folded quotient h1 + zeta^(n+2) h2 + zeta^(2(n+2)) h3 and its digest
    HFr zp = HFr::one();
    {
        HFr base = zeta;
        for (size_t e = n + 2; e; e >>= 1) { if (e & 1) zp = zp * base; base = base.sqr(); }
    }
    {
        FoldArgs A = {};
        A.k = 3; A.n = (uint32_t)(n + 2); A.out = fh;
        for (int k = 0; k < 3; k++) { A.p[k] = h + k * (n + 2); A.len[k] = (uint32_t)(n + 2); }
        A.c[0] = Fr::one(); A.c[1] = to_dev(zp); A.c[2] = to_dev(zp * zp);
        ZK_LAUNCH(s, st, "plonk_fold", k_fold, dim3(grid_of(n + 2)), dim3(256), 0, A);
    }
    Affine<HFp> c_fh;
    {
        const Affine<HFp> pts[2] = {c_h[2], c_h[1]};
        const HFr ks[2] = {zp * zp, zp};
        XYZZ<HFp> fhd = host_multi_scalar_mul(pts, ks, 2);
        fhd.madd(c_h[0]);
        c_fh = fhd.to_affine();
    }

    // ---- kzg.BatchOpenSinglePoint of (foldedH, linPol, l, r, o, s1, s2) at zeta
    {
        const Fr* const p2[2] = {fh, lin};
        const size_t l2[2] = {n + 2, n + 3};
        ZK_TRY(poly_eval_batch_dev(s, st, p2, l2, 2, zeta, SB, d_vals + 6));
    }
    ZK_HIP(hipMemcpyAsync(ev + 6, d_vals + 6, 2 * sizeof(Fr), hipMemcpyDeviceToHost, st));
    ZK_TRY(slot_sync(s, st));
    lap("plonk.round4_evaluations_and_linearised");
    if (!lin_direct && c_lin.x == c_lin_by_linearity.x && c_lin.y == c_lin_by_linearity.y)
        const_cast<PlonkPK*>(P)->vk_consistent = true;  // (the key's workspace mutex is held for the whole proof) from the next proof on: by linearity
    const HFr claimed[7] = {ev[6], ev[7], lz, rz, oz, s1z, s2z};
    const Affine<HFp> digests[7] = {c_fh, c_lin, c_lro[0], c_lro[1], c_lro[2], P->vk_s[0], P->vk_s[1]};
    HFr kg;
    {
        FsTranscript ks{"gamma"};
        ks.bind_fr(0, zeta);
        for (const auto& d : digests) ks.bind_g1(0, d);
        for (const auto& v : claimed) ks.bind_fr(0, v);
        kg = ks.challenge(0);
        if (challenges) kg = pin[4];
    }
    {
        FoldArgs A = {};
        const Fr* pp[7] = {fh, lin, bl_, br_, bo_, P->s1, P->s2};
        const size_t pl[7] = {n + 2, n + 3, n + 2, n + 2, n + 2, n, n};
        A.k = 7; A.n = (uint32_t)(n + 3); A.out = fold;
        HFr acc = HFr::one();
        for (int k = 0; k < 7; k++) { A.p[k] = pp[k]; A.len[k] = (uint32_t)pl[k]; A.c[k] = to_dev(acc); acc = acc * kg; }
        ZK_LAUNCH(s, st, "plonk_fold", k_fold, dim3(grid_of(n + 3)), dim3(256), 0, A);
    }
    // dividePolyByXminusA(folded, foldedEvaluations, zeta): the recurrence yields the same quotient (folded(zeta) = sum gamma^i v_i)
    ZK_TRY(poly_divide_dev(s, st, fold, n + 3, zeta, SB, fold, d_vals + 8));
    ZK_TRY(commit(P, s, st, fold, n + 2, &c_batch));
    ZK_TRY(azo.join());
    c_zopen = azo.out;
    lap("plonk.round5_openings_committed");
    // ---- Proof.WriteTo
    uint8_t* o = proof_out;
    for (const Affine<HFp>* d : {&c_lro[0], &c_lro[1], &c_lro[2], &c_z, &c_h[0], &c_h[1], &c_h[2]}) { g1_compress(*d, o); o += 32; }
    g1_compress(c_batch, o); o += 32;
    o[0] = 0; o[1] = 0; o[2] = 0; o[3] = 7; o += 4;
    for (const HFr& v : claimed) { fr_to_be(v, o); o += 32; }
    g1_compress(c_zopen, o); o += 32;
    fr_to_be(zu, o); o += 32;
    return (o - proof_out) == ZK_PLONK_PROOF_BYTES ? ZK_OK : set_err(ZK_ERR_ARG, "internal: proof length");
}

// ---- iop: the copy-constraint ratio of many witnesses (gnark-crypto ecc/bn254/fr/iop BuildRatioCopyConstraint) and its two ingredients behind doors of
// their own.  Every entry decides its argument errors before it looks for a device; the entries with workspace synchronise before they return (the workspace
// is the slot's arena, which the next call on the slot reuses), as zk_bn254_groth16_compute_h_batch_dev does.
int zk_bn254_iop_sigma_dev(const void* d_perm, uint32_t log_n, void* d_sigma, void* stream) {
    if (!d_perm || !d_sigma) return set_err(ZK_ERR_ARG, "null pointer");
    if (log_n > 28) return set_err(ZK_ERR_ARG, "log_n = %u exceeds Fr two-adicity 28", log_n);
    SlotGuard g;
    ZK_TRY(acquire_slot(&g.s));
    hipStream_t st = stream ? (hipStream_t)stream : g.s->stream;
    Domain* d0;
    ZK_TRY(get_domain(g.s, st, log_n, DOM_TW, &d0));
    ZK_TRY(g.s->reserve(4096));
    int* d_flag = (int*)g.s->alloc(64);
    if (!d_flag) return set_err(ZK_ERR_HIP, "sigma: workspace");
    int h_flag = 0;
    ZK_TRY(sigma_checked_dev(g.s, st, d0, (const uint32_t*)d_perm, (Fr*)d_sigma, d_flag));
    ZK_HIP(hipMemcpyAsync(&h_flag, d_flag, 4, hipMemcpyDeviceToHost, st));
    ZK_TRY(slot_sync(g.s, st));  // the status is read here
    if (h_flag) return set_err(ZK_ERR_ARG, "permutation entry out of range (>= 3 * 2^%u)", log_n);
    return ZK_OK;
}

int zk_bn254_iop_ratio_copy_batch_dev(const void* d_l, const void* d_r, const void* d_o, size_t in_stride, uint32_t log_n, size_t rows, const void* d_sigma,
                                      const void* d_beta, const void* d_gamma, void* d_z, size_t out_stride, void* stream) {
    if (!d_l || !d_r || !d_o || !d_sigma || !d_beta || !d_gamma || !d_z) return set_err(ZK_ERR_ARG, "null pointer");
    if (log_n > 28) return set_err(ZK_ERR_ARG, "log_n = %u exceeds Fr two-adicity 28", log_n);
    const size_t n = (size_t)1 << log_n;
    ZK_TRY(ratio_dev_args(d_l, d_r, d_o, in_stride, n, rows, d_sigma, 3 * n, d_beta, d_gamma, d_z, out_stride));
    if (rows == 0) return ZK_OK;
    SlotGuard g;
    ZK_TRY(acquire_slot(&g.s));
    hipStream_t st = stream ? (hipStream_t)stream : g.s->stream;
    Domain* d0;
    ZK_TRY(get_domain(g.s, st, log_n, DOM_TW, &d0));
    const size_t chunk = ratio_chunk(n, rows, 0);
    RatioWs W;
    ZK_TRY(g.s->reserve(ratio_ws_bytes(n, chunk, rows == 1)));
    ZK_TRY(ratio_ws_take(g.s, n, chunk, rows == 1, &W));
    ZK_TRY(ratio_rows_dev(g.s, st, d0, (const Fr*)d_sigma, (const Fr*)d_l, (const Fr*)d_r, (const Fr*)d_o, in_stride, rows, (const Fr*)d_beta, (const Fr*)d_gamma, (Fr*)d_z,
                          out_stride, W));
    return slot_sync(g.s, st);  // the workspace lives in the slot's arena
}

// host rows, contiguous: l, r, o, z_out (rows, n), perm 3n positions, beta and gamma one per row
int zk_bn254_iop_ratio_copy_batch(const zk_fr* l, const zk_fr* r, const zk_fr* o, uint32_t log_n, size_t rows, const uint32_t* perm, const zk_fr* beta,
                                  const zk_fr* gamma, zk_fr* z_out) {
    if (!l || !r || !o || !perm || !beta || !gamma || !z_out) return set_err(ZK_ERR_ARG, "null pointer");
    if (log_n > 28) return set_err(ZK_ERR_ARG, "log_n = %u exceeds Fr two-adicity 28", log_n);
    const size_t n = (size_t)1 << log_n;
    ZK_TRY(ratio_dev_args(l, r, o, n, n, rows, nullptr, 0, beta, gamma, z_out, n));
    if (rows == 0) return ZK_OK;
    SlotGuard g;
    ZK_TRY(acquire_slot(&g.s));
    Slot* s = g.s;
    hipStream_t st = s->stream;
    Domain* d0;
    ZK_TRY(get_domain(s, st, log_n, DOM_TW, &d0));
    const size_t row_bytes = n * sizeof(Fr), chunk = ratio_chunk(n, rows, 4 * row_bytes);
    ZK_TRY(s->reserve(3 * row_bytes + 3 * n * 4 + 2 * rows * sizeof(Fr) + 4 * chunk * row_bytes + ratio_ws_bytes(n, chunk, rows == 1) + 16 * 256));
    Fr* sig = (Fr*)s->alloc(3 * row_bytes);
    uint32_t* d_perm = (uint32_t*)s->alloc(3 * n * 4);
    int* d_flag = (int*)s->alloc(64);
    Fr *d_beta = (Fr*)s->alloc(rows * sizeof(Fr)), *d_gamma = (Fr*)s->alloc(rows * sizeof(Fr));
    Fr* d[4];
    for (int i = 0; i < 4; i++) d[i] = (Fr*)s->alloc(chunk * row_bytes);
    if (!sig || !d_perm || !d_flag || !d_beta || !d_gamma || !d[0] || !d[1] || !d[2] || !d[3]) return set_err(ZK_ERR_HIP, "ratio batch: workspace");
    RatioWs W;
    ZK_TRY(ratio_ws_take(s, n, chunk, rows == 1, &W));
    int h_flag = 0;
    ZK_HIP(hipMemcpyAsync(d_perm, perm, 3 * n * 4, hipMemcpyHostToDevice, st));
    ZK_TRY(sigma_checked_dev(s, st, d0, d_perm, sig, d_flag));
    ZK_HIP(hipMemcpyAsync(&h_flag, d_flag, 4, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipMemcpyAsync(d_beta, beta, rows * sizeof(Fr), hipMemcpyHostToDevice, st));
    ZK_HIP(hipMemcpyAsync(d_gamma, gamma, rows * sizeof(Fr), hipMemcpyHostToDevice, st));
    ZK_TRY(slot_sync(s, st));
    if (h_flag) return set_err(ZK_ERR_ARG, "permutation entry out of range (>= 3 * 2^%u)", log_n);
    const zk_fr* src[3] = {l, r, o};
    for (size_t first = 0; first < rows; first += chunk) {
        const size_t R = std::min(chunk, rows - first);
        for (int i = 0; i < 3; i++) ZK_HIP(hipMemcpyAsync(d[i], (const char*)src[i] + first * row_bytes, R * row_bytes, hipMemcpyHostToDevice, st));
        ZK_TRY(ratio_rows_dev(s, st, d0, sig, d[0], d[1], d[2], n, R, d_beta + first, d_gamma + first, d[3], n, W));
        ZK_HIP(hipMemcpyAsync((char*)z_out + first * row_bytes, d[3], R * row_bytes, hipMemcpyDeviceToHost, st));
    }
    return slot_sync(s, st);
}

// the same through a resident PLONK key: its permutation (S1 | S2 | S3 in Lagrange form), its domain and that domain's twiddles
int zk_bn254_plonk_ratio_batch_dev(uint64_t handle, const void* d_l, const void* d_r, const void* d_o, size_t in_stride, size_t rows, const void* d_beta,
                                   const void* d_gamma, void* d_z, size_t out_stride, void* stream) {
    if (!d_l || !d_r || !d_o || !d_beta || !d_gamma || !d_z) return set_err(ZK_ERR_ARG, "null pointer");
    if (rows == 0) return ZK_OK;
    PlonkPK* P;
    std::shared_ptr<std::mutex> mu;
    {   // the table of keys is the host's: an unknown handle is answered without a device
        std::lock_guard<std::mutex> lk(g_ppk_mu);
        auto it = g_ppks.find(handle);
        if (it == g_ppks.end()) return set_err(ZK_ERR_HANDLE, "unknown PLONK proving-key handle %llu", (unsigned long long)handle);
        P = it->second;
        mu = P->mu;
    }
    ZK_ON_ENTRY_OF(handle);
    std::lock_guard<std::mutex> key_lock(*mu);  // a key in use is not freed (zk_bn254_plonk_pk_free waits on this mutex)
    {
        std::lock_guard<std::mutex> lk(g_ppk_mu);
        auto it = g_ppks.find(handle);
        if (it == g_ppks.end() || it->second != P) return set_err(ZK_ERR_HANDLE, "PLONK proving key %llu was freed", (unsigned long long)handle);
    }
    const size_t n = P->n;
    ZK_TRY(ratio_dev_args(d_l, d_r, d_o, in_stride, n, rows, nullptr, 0, d_beta, d_gamma, d_z, out_stride));
    SlotGuard g;
    ZK_TRY(acquire_slot(&g.s));
    hipStream_t st = stream ? (hipStream_t)stream : g.s->stream;
    Domain* d0;
    ZK_TRY(get_domain(g.s, st, P->logn, DOM_TW, &d0));
    const size_t chunk = ratio_chunk(n, rows, 0);
    RatioWs W;
    ZK_TRY(g.s->reserve(ratio_ws_bytes(n, chunk, rows == 1)));
    ZK_TRY(ratio_ws_take(g.s, n, chunk, rows == 1, &W));
    ZK_TRY(ratio_rows_dev(g.s, st, d0, (const Fr*)P->sig, (const Fr*)d_l, (const Fr*)d_r, (const Fr*)d_o, in_stride, rows, (const Fr*)d_beta, (const Fr*)d_gamma, (Fr*)d_z,
                          out_stride, W));
    return slot_sync(g.s, st);
}

// ---- round 3 for many witnesses of one resident key (quotient_rows_dev above).  Argument errors are decided before a device is looked for; the key's tables are
// only read and the workspace is the slot's arena, so the key's per-proof mutex is not taken: calls overlap each other and a proof in flight.
int zk_bn254_plonk_quotient_batch_dev(uint64_t handle, const void* d_l, const void* d_r, const void* d_o, const void* d_z, size_t in_stride, const void* d_pub,
                                      size_t pub_stride, size_t rows, const void* d_alpha, const void* d_beta, const void* d_gamma, void* d_h, size_t out_stride,
                                      void* d_status, void* stream) {
    if (!d_l || !d_r || !d_o || !d_z || !d_alpha || !d_beta || !d_gamma || !d_h || !d_status) return set_err(ZK_ERR_ARG, "null pointer");
    if (rows == 0) return ZK_OK;
    PlonkPK* P;
    std::shared_ptr<std::shared_mutex> live;
    std::shared_lock<std::shared_mutex> alive;
    {   // the table of keys is the host's: an unknown handle is answered without a device.  A key found here is not being freed yet (zk_bn254_plonk_pk_free
        // erases it under this mutex before it asks for `live`), so the shared lock is granted at once and keeps the key alive from here on
        std::lock_guard<std::mutex> lk(g_ppk_mu);
        auto it = g_ppks.find(handle);
        if (it == g_ppks.end()) return set_err(ZK_ERR_HANDLE, "unknown PLONK proving-key handle %llu", (unsigned long long)handle);
        P = it->second;
        live = P->live;
        alive = std::shared_lock<std::shared_mutex>(*live);
    }
    const size_t n = P->n, N4 = P->N4, npub = P->n_public, keep = 3 * (n + 2);
    if (keep > N4) return set_err(ZK_ERR_ARG, "a domain of %zu rows has no quotient of 3 (n + 2) coefficients on %zu points", n, N4);
    if (npub && !d_pub) return set_err(ZK_ERR_ARG, "null pointer");
    if (in_stride < n + 3) return set_err(ZK_ERR_ARG, "in_stride = %zu is below n + 3 = %zu", in_stride, n + 3);
    if (npub && pub_stride < npub) return set_err(ZK_ERR_ARG, "pub_stride = %zu is below the %zu public inputs", pub_stride, npub);
    if (out_stride < keep) return set_err(ZK_ERR_ARG, "out_stride = %zu is below 3 (n + 2) = %zu", out_stride, keep);
    {
        const size_t hb = rows_span(rows, out_stride, keep), sb = rows * sizeof(int), cb = rows * sizeof(Fr);
        const void* in[8] = {d_l, d_r, d_o, d_z, d_pub, d_alpha, d_beta, d_gamma};
        const size_t ib[8] = {rows_span(rows, in_stride, n + 2), rows_span(rows, in_stride, n + 2), rows_span(rows, in_stride, n + 2), rows_span(rows, in_stride, n + 3),
                              npub ? rows_span(rows, pub_stride, npub) : 0, cb, cb, cb};
        for (int k = 0; k < 8; k++)
            if (spans_overlap(d_h, hb, in[k], ib[k]) || spans_overlap(d_status, sb, in[k], ib[k])) return set_err(ZK_ERR_ARG, "d_h or d_status overlaps an input");
        if (spans_overlap(d_h, hb, d_status, sb)) return set_err(ZK_ERR_ARG, "d_h overlaps d_status");
    }
    ZK_ON_ENTRY_OF(handle);
    SlotGuard g;
    ZK_TRY(acquire_slot(&g.s));
    hipStream_t st = stream ? (hipStream_t)stream : g.s->stream;
    Domain *d0, *d1;
    ZK_TRY(get_domain(g.s, st, P->logn, DOM_TW_INV, &d0));  // every table the transforms below ask for, before the arena is carved
    ZK_TRY(get_domain(g.s, st, P->logN4, DOM_TW | DOM_TW_INV | DOM_COSET | DOM_COSET_INV_N, &d1));
    const size_t chunk = quot_chunk(P, rows);
    ZK_TRY(g.s->reserve(chunk * quot_row_bytes(P) + 4096));
    Fr* ws = (Fr*)g.s->alloc(chunk * quot_row_bytes(P));
    if (!ws) return set_err(ZK_ERR_HIP, "quotient batch: workspace");
    ZK_TRY(quotient_rows_dev(g.s, st, P, (const Fr*)d_l, (const Fr*)d_r, (const Fr*)d_o, (const Fr*)d_z, in_stride, (const Fr*)d_pub, pub_stride, rows, (const Fr*)d_alpha,
                             (const Fr*)d_beta, (const Fr*)d_gamma, (Fr*)d_h, out_stride, (int*)d_status, ws, chunk));
    return slot_sync(g.s, st);  // the workspace lives in the slot's arena
}

// fr.BatchInvert in place on n device elements: a zero stays a zero.  k_batch_inverse with its scratch from the slot's arena, at most RATIO_SCRATCH bytes at a time.
int zk_bn254_fr_batch_invert_dev(void* d_a, size_t n, void* stream) {
    if (!d_a) return set_err(ZK_ERR_ARG, "null pointer");
    if (n == 0) return ZK_OK;
    SlotGuard g;
    ZK_TRY(acquire_slot(&g.s));
    hipStream_t st = stream ? (hipStream_t)stream : g.s->stream;
    const size_t chunk = std::min(n, RATIO_SCRATCH / sizeof(Fr));
    ZK_TRY(g.s->reserve(chunk * sizeof(Fr) + 256));
    Fr* scr = (Fr*)g.s->alloc(chunk * sizeof(Fr));
    if (!scr) return set_err(ZK_ERR_HIP, "batch inverse: workspace");
    for (size_t first = 0; first < n; first += chunk) {
        const size_t cnt = std::min(chunk, n - first), lanes = (cnt + BINV_K - 1) / BINV_K;
        ZK_LAUNCH(g.s, st, "plonk_batch_inverse", k_batch_inverse, dim3(grid_of(lanes)), dim3(256), 0, (Fr*)d_a + first, cnt, scr);
    }
    return slot_sync(g.s, st);  // the scratch lives in the slot's arena
}

// ---- rounds 4 and 5 for many witnesses (poly_open_rows_dev, linearize_rows_dev, open_rows_dev above).  As for round 3: argument errors before a device is looked
// for, the key's `live` lock shared and not its per-proof mutex, the workspace from the slot's arena.
int zk_bn254_fr_poly_open_rows_dev(const void* d_f, size_t in_stride, size_t len, size_t rows, const void* d_points, void* d_q, size_t q_stride, void* d_values,
                                   void* stream) {
    if (!d_f || !d_points || !d_values) return set_err(ZK_ERR_ARG, "null pointer");
    if (rows == 0) return ZK_OK;
    if (len < 1) return set_err(ZK_ERR_ARG, "a polynomial has at least one coefficient");
    if (in_stride < len) return set_err(ZK_ERR_ARG, "in_stride = %zu is below the %zu coefficients of a row", in_stride, len);
    if (d_q && q_stride < len - 1) return set_err(ZK_ERR_ARG, "q_stride = %zu is below the %zu coefficients of a quotient", q_stride, len - 1);
    {
        const size_t fb = rows_span(rows, in_stride, len), qb = d_q && len > 1 ? rows_span(rows, q_stride, len - 1) : 0, cb = rows * sizeof(Fr);
        const bool in_place = d_q == d_f && q_stride == in_stride;
        if (!in_place && spans_overlap(d_q, qb, d_f, fb)) return set_err(ZK_ERR_ARG, "d_q overlaps d_f and is not d_f with its stride");
        if (spans_overlap(d_q, qb, d_points, cb) || spans_overlap(d_q, qb, d_values, cb)) return set_err(ZK_ERR_ARG, "d_q overlaps d_points or d_values");
        if (spans_overlap(d_values, cb, d_f, fb) || spans_overlap(d_values, cb, d_points, cb)) return set_err(ZK_ERR_ARG, "d_values overlaps an input");
    }
    SlotGuard g;
    ZK_TRY(acquire_slot(&g.s));
    hipStream_t st = stream ? (hipStream_t)stream : g.s->stream;
    ZK_TRY(poly_open_rows_dev(g.s, st, (const Fr*)d_f, in_stride, len, rows, (const Fr*)d_points, (Fr*)d_q, q_stride, (Fr*)d_values));
    return slot_sync(g.s, st);  // the workspace lives in the slot's arena
}

int zk_bn254_plonk_linearize_batch_dev(uint64_t handle, const void* d_l, const void* d_r, const void* d_o, const void* d_z, size_t in_stride, const void* d_h,
                                       size_t h_stride, size_t rows, const void* d_alpha, const void* d_beta, const void* d_gamma, const void* d_zeta, void* d_values,
                                       void* d_zquot, void* d_lin, void* d_fh, size_t out_stride, void* stream) {
    if (!d_l || !d_r || !d_o || !d_z || !d_h || !d_alpha || !d_beta || !d_gamma || !d_zeta || !d_values || !d_zquot || !d_lin || !d_fh)
        return set_err(ZK_ERR_ARG, "null pointer");
    if (rows == 0) return ZK_OK;
    PlonkPK* P;
    std::shared_ptr<std::shared_mutex> live;
    std::shared_lock<std::shared_mutex> alive;
    ZK_TRY(live_key(handle, &P, &live, &alive));
    const size_t n = P->n;
    if (in_stride < n + 3) return set_err(ZK_ERR_ARG, "in_stride = %zu is below n + 3 = %zu", in_stride, n + 3);
    if (h_stride < 3 * (n + 2)) return set_err(ZK_ERR_ARG, "h_stride = %zu is below 3 (n + 2) = %zu", h_stride, 3 * (n + 2));
    if (out_stride < n + 3) return set_err(ZK_ERR_ARG, "out_stride = %zu is below n + 3 = %zu", out_stride, n + 3);
    {
        const size_t cb = rows * sizeof(Fr), w2 = rows_span(rows, in_stride, n + 2);
        const void* in[9] = {d_l, d_r, d_o, d_z, d_h, d_alpha, d_beta, d_gamma, d_zeta};
        const size_t ib[9] = {w2, w2, w2, rows_span(rows, in_stride, n + 3), rows_span(rows, h_stride, 3 * (n + 2)), cb, cb, cb, cb};
        const void* out[4] = {d_values, d_zquot, d_lin, d_fh};
        const size_t ob[4] = {8 * cb, rows_span(rows, out_stride, n + 2), rows_span(rows, out_stride, n + 3), rows_span(rows, out_stride, n + 2)};
        for (int a = 0; a < 4; a++) {
            for (int k = 0; k < 9; k++)
                if (spans_overlap(out[a], ob[a], in[k], ib[k])) return set_err(ZK_ERR_ARG, "an output overlaps an input");
            for (int b = a + 1; b < 4; b++)
                if (spans_overlap(out[a], ob[a], out[b], ob[b])) return set_err(ZK_ERR_ARG, "two outputs overlap");
        }
    }
    ZK_ON_ENTRY_OF(handle);
    SlotGuard g;
    ZK_TRY(acquire_slot(&g.s));
    hipStream_t st = stream ? (hipStream_t)stream : g.s->stream;
    ZK_TRY(linearize_rows_dev(g.s, st, P, (const Fr*)d_l, (const Fr*)d_r, (const Fr*)d_o, (const Fr*)d_z, in_stride, (const Fr*)d_h, h_stride, rows, (const Fr*)d_alpha,
                              (const Fr*)d_beta, (const Fr*)d_gamma, (const Fr*)d_zeta, (Fr*)d_values, (Fr*)d_zquot, (Fr*)d_lin, (Fr*)d_fh, out_stride));
    return slot_sync(g.s, st);  // the workspace lives in the slot's arena
}

int zk_bn254_plonk_open_batch_dev(uint64_t handle, const void* d_fh, const void* d_lin, const void* d_l, const void* d_r, const void* d_o, size_t in_stride,
                                  size_t rows, const void* d_zeta, const void* d_kzg_gamma, void* d_q, size_t out_stride, void* d_value, void* stream) {
    if (!d_fh || !d_lin || !d_l || !d_r || !d_o || !d_zeta || !d_kzg_gamma || !d_q || !d_value) return set_err(ZK_ERR_ARG, "null pointer");
    if (rows == 0) return ZK_OK;
    PlonkPK* P;
    std::shared_ptr<std::shared_mutex> live;
    std::shared_lock<std::shared_mutex> alive;
    ZK_TRY(live_key(handle, &P, &live, &alive));
    const size_t n = P->n;
    if (in_stride < n + 3) return set_err(ZK_ERR_ARG, "in_stride = %zu is below n + 3 = %zu", in_stride, n + 3);
    if (out_stride < n + 2) return set_err(ZK_ERR_ARG, "out_stride = %zu is below n + 2 = %zu", out_stride, n + 2);
    {
        const size_t cb = rows * sizeof(Fr), w2 = rows_span(rows, in_stride, n + 2), qb = rows_span(rows, out_stride, n + 2);
        const void* in[7] = {d_fh, d_lin, d_l, d_r, d_o, d_zeta, d_kzg_gamma};
        const size_t ib[7] = {w2, rows_span(rows, in_stride, n + 3), w2, w2, w2, cb, cb};
        for (int k = 0; k < 7; k++)
            if (spans_overlap(d_q, qb, in[k], ib[k]) || spans_overlap(d_value, cb, in[k], ib[k])) return set_err(ZK_ERR_ARG, "d_q or d_value overlaps an input");
        if (spans_overlap(d_q, qb, d_value, cb)) return set_err(ZK_ERR_ARG, "d_q overlaps d_value");
    }
    ZK_ON_ENTRY_OF(handle);
    SlotGuard g;
    ZK_TRY(acquire_slot(&g.s));
    hipStream_t st = stream ? (hipStream_t)stream : g.s->stream;
    ZK_TRY(open_rows_dev(g.s, st, P, (const Fr*)d_fh, (const Fr*)d_lin, (const Fr*)d_l, (const Fr*)d_r, (const Fr*)d_o, in_stride, rows, (const Fr*)d_zeta,
                         (const Fr*)d_kzg_gamma, (Fr*)d_q, out_stride, (Fr*)d_value));
    return slot_sync(g.s, st);  // the workspace lives in the slot's arena
}

// The digests of the rows the entries above produce: zk_bn254_msm_bases_rows_dev against the key's SRS (coefficients) or its Lagrange form (wire values followed
// by the two blinders: the layout round 1 of zk_bn254_plonk_prove commits, zero digits dropped).  Reads the key's two bases handles only: the `live` lock
// shared, neither the per-proof mutex nor w_big / w_small.
int zk_bn254_plonk_commit_batch_dev(uint64_t handle, const void* d_rows, size_t row_stride, size_t len, size_t rows, int from_values, void* d_out, void* d_compressed) {
    if (!d_rows || (!d_out && !d_compressed)) return set_err(ZK_ERR_ARG, "null pointer");
    PlonkPK* P;
    std::shared_ptr<std::shared_mutex> live;
    std::shared_lock<std::shared_mutex> alive;
    ZK_TRY(live_key(handle, &P, &live, &alive));
    if (from_values) {
        if (!P->lag_srs) return set_err(ZK_ERR_ARG, "the key has no Lagrange form of its SRS (zk_bn254_plonk_pk_lagrange_srs)");
        if (len != P->n + 2) return set_err(ZK_ERR_ARG, "len = %zu: a row of values is the n = %zu wire values and two blinders", len, P->n);
    }
    if (rows > 1 && row_stride < len) return set_err(ZK_ERR_ARG, "row_stride = %zu is below len = %zu", row_stride, len);
    if (rows == 0) return ZK_OK;
    return zk_bn254_msm_bases_rows_dev(from_values ? P->lag_srs : P->srs, 0, d_rows, row_stride, len, rows, &kMont, (from_values ? ZK_MSM_ROWS_SPARSE : 0u) | ZK_MSM_ROWS_NO_POINTS,
                                       d_out, d_compressed);
}

}  // extern "C"
