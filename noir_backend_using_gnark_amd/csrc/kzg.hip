// KZG openings on the device (include/zkmi.h "KZG openings"): gnark-crypto v0.9.1 ecc/bn254/fr/kzg  [UPSTREAM-RECALL]
//   kzg.Open(p, point, srs)                                   zk_bn254_kzg_open, count = 1 (count > 1: independent openings in one launch set)
//   kzg.BatchOpenSinglePoint(polys, digests, point, hf, srs)  zk_bn254_kzg_batch_open_single_point (hf = SHA-256, what gnark's PLONK passes)
// An opening is the suffix scan of plonk.hip (S_i = f_i + a S_(i+1): S_0 = f(a), q_i = S_(i+1) are the coefficients of (f - f(a)) / (X - a) --
// kzg.dividePolyByXminusA) followed by kzg.Commit of the quotient over the resident SRS.  The scan kernels of plonk.hip take ONE point per launch and divide one
// row; the variants here index polynomial, length and point by blockIdx.y, so that `count` openings are three launches, not 3 x count.
// The verifying side is host code in verify.hip (kzg.Verify, FoldProof, BatchVerifySinglePoint) and verify_batch.hip (BatchVerifyMultiPoints on the device).
#include <string.h>

#include <algorithm>
#include <vector>

#include "ctx.hpp"
#include "curve.hpp"
#include "host_ff.hpp"
#include "msm.hpp"
#include "multidev.hpp"
#include "proofio.hpp"
#include "scan.hpp"

namespace zkmi {
namespace {

// one row per polynomial: its coefficients, where its quotient goes (may alias f), its point a, A = a^K and M = A^256
struct HscanRows {
    const Fr* f[HSCAN_BATCH_MAX];
    Fr* q[HSCAN_BATCH_MAX];
    size_t len[HSCAN_BATCH_MAX];
    Fr a[HSCAN_BATCH_MAX], A[HSCAN_BATCH_MAX], M[HSCAN_BATCH_MAX];
};

// pass 1 of k_hscan_local with the row's own point: lane Horner totals, workgroup suffix scan; lane carry-ins to tcarry[(row nb + block) 256 + lane], the
// workgroup's total to btot[row nb + block].  A workgroup above the row's last coefficient contributes zeros.
__global__ __launch_bounds__(256) void k_hscan_local_rows(HscanRows R, uint32_t K, uint32_t nb, Fr* __restrict__ tcarry, Fr* __restrict__ btot) {
    __shared__ Fr sh[256];
    const Fr* __restrict__ f = R.f[blockIdx.y];
    const size_t len = R.len[blockIdx.y];
    const size_t blk = (size_t)blockIdx.y * nb + blockIdx.x;
    const size_t gt = (size_t)blockIdx.x * 256 + threadIdx.x, base = gt * K;
    if ((size_t)blockIdx.x * 256 * K >= len) {  // uniform over the workgroup
        tcarry[blk * 256 + threadIdx.x] = Fr::zero();
        if (threadIdx.x == 0) btot[blk] = Fr::zero();
        return;
    }
    const Fr a = R.a[blockIdx.y];
    Fr acc = Fr::zero();
    for (int k = (int)K - 1; k >= 0; k--) {
        const size_t i = base + (size_t)k;
        acc = acc * a;
        if (i < len) acc = acc + ld(f + i);
    }
    sh[threadIdx.x] = acc;
    __syncthreads();
    Fr val = acc, Ad = R.A[blockIdx.y];
    for (unsigned d = 1; d < 256; d <<= 1) {
        Fr o = threadIdx.x + d < 256 ? sh[threadIdx.x + d] : Fr::zero();
        __syncthreads();
        val = val + Ad * o;
        sh[threadIdx.x] = val;
        __syncthreads();
        Ad = Ad.sqr();
    }
    tcarry[blk * 256 + threadIdx.x] = threadIdx.x < 255 ? sh[threadIdx.x + 1] : Fr::zero();
    if (threadIdx.x == 0) btot[blk] = val;
}
// pass 2 of k_hscan_blocks (plonk.hip; the same scan, as are scan.hpp's hscan_*_body under plonk.hip's k_hscan_*_dev -- an edit of one belongs in the others), one
// workgroup per row with the row's own M:
// btot[row nb + b] <- sum_{b' > b} btot[row nb + b'] M^(b'-b-1); total[row] = f(a)
__global__ __launch_bounds__(1024) void k_hscan_blocks_rows(HscanRows R, Fr* __restrict__ btot, uint32_t nb, Fr* __restrict__ total) {
    __shared__ Fr sh[1024];
    btot += (size_t)blockIdx.x * nb;
    const Fr M = R.M[blockIdx.x];
    Fr carry = Fr::zero();
    const uint32_t nchunks = (nb + 1023) / 1024;
    Fr M1024 = M;
    for (int i = 0; i < 10; i++) M1024 = M1024.sqr();
    for (int c = (int)nchunks - 1; c >= 0; c--) {
        const uint32_t b = (uint32_t)c * 1024 + threadIdx.x;
        const Fr v = b < nb ? ld(btot + b) : Fr::zero();
        sh[threadIdx.x] = v;
        __syncthreads();
        Fr val = v, Md = M;
        for (unsigned d = 1; d < 1024; d <<= 1) {
            Fr o = threadIdx.x + d < 1024 ? sh[threadIdx.x + d] : Fr::zero();
            __syncthreads();
            val = val + Md * o;
            sh[threadIdx.x] = val;
            __syncthreads();
            Md = Md.sqr();
        }
        const Fr next = threadIdx.x < 1023 ? sh[threadIdx.x + 1] : Fr::zero();
        const uint32_t e = 1023 - threadIdx.x;
        Fr pw = Fr::one(), bs = M;
        for (int i = 0; i < 10; i++) { if ((e >> i) & 1) pw = pw * bs; bs = bs.sqr(); }
        const Fr C = next + pw * carry;
        const Fr chunk_total = sh[0];
        __syncthreads();
        if (b < nb) btot[b] = C;
        carry = chunk_total + M1024 * carry;
    }
    if (threadIdx.x == 0) total[blockIdx.x] = carry;
}
// pass 3 of k_hscan_apply per row: q_i = S_(i+1) for i < len (q[len - 1] = 0); q may alias f
__global__ __launch_bounds__(256) void k_hscan_apply_rows(HscanRows R, uint32_t K, uint32_t nb, const Fr* __restrict__ tcarry, const Fr* __restrict__ bC) {
    const Fr* f = R.f[blockIdx.y];
    Fr* q = R.q[blockIdx.y];
    const size_t len = R.len[blockIdx.y];
    const size_t blk = (size_t)blockIdx.y * nb + blockIdx.x;
    const size_t gt = (size_t)blockIdx.x * 256 + threadIdx.x, base = gt * K;
    if (base >= len) return;
    const Fr a = R.a[blockIdx.y];
    const uint32_t e = 255 - threadIdx.x;
    Fr pw = Fr::one(), bs = R.A[blockIdx.y];
    for (int i = 0; i < 8; i++) { if ((e >> i) & 1) pw = pw * bs; bs = bs.sqr(); }
    Fr S = ld(tcarry + blk * 256 + threadIdx.x) + pw * ld(bC + blk);
    for (int k = (int)K - 1; k >= 0; k--) {
        const size_t i = base + (size_t)k;
        if (i >= len) continue;
        const Fr fv = ld(f + i);
        q[i] = S;
        S = fv + a * S;
    }
}
// out_i = sum_k g[k] p_k[i] for i < n, any number of rows: a lane per coefficient index, a row shorter than the index contributes nothing
// (kzg.BatchOpenSinglePoint's fold with g[k] = gamma^k)
__global__ __launch_bounds__(256) void k_fold_rows(const Fr* const* __restrict__ p, const size_t* __restrict__ len, const Fr* __restrict__ g, uint32_t rows, size_t n,
                                                   Fr* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Fr v = Fr::zero();
    for (uint32_t k = 0; k < rows; k++)
        if (i < len[k]) v = v + ld(p[k] + i) * ld(g + k);
    out[i] = v;
}

const zk_msm_cfg kMont = {0, 1, 0, 0};
const char* const kErrSize = "kzg: invalid polynomial size (larger than SRS or == 0)";  // ErrInvalidPolynomialSize

HFr hfr(const zk_fr& x) {
    HFr r;
    memcpy(&r, &x, 32);
    return r;
}
HFr pow_u32(HFr base, uint32_t e) {
    HFr r = HFr::one();
    for (; e; e >>= 1) { if (e & 1) r = r * base; base = base.sqr(); }
    return r;
}
// lane and workgroup geometry of a scan over `len` coefficients (scan_bufs' rule)
void scan_geometry(size_t len, uint32_t* K, uint32_t* nb) {
    uint32_t k = (uint32_t)((len + 256 * 1024 - 1) / (256 * 1024));
    if (k < 8) k = 8;
    *K = k;
    *nb = (uint32_t)(((len + k - 1) / k + 255) / 256);
}

// the argument checks that need no handle, then the device, then the SRS: *srs_n = its size
int check_open_args(uint64_t srs, const void* const* polys, const size_t* lens, size_t count, size_t* srs_n, size_t* maxlen) {
    if (count == 0) return set_err(ZK_ERR_ARG, "kzg: no polynomial to open");
    if (!polys || !lens) return set_err(ZK_ERR_ARG, "null pointer");
    size_t mx = 0;
    for (size_t k = 0; k < count; k++) {
        if (!polys[k]) return set_err(ZK_ERR_ARG, "null polynomial %zu", k);
        if (lens[k] == 0) return set_err(ZK_ERR_LEN, "%s", kErrSize);
        mx = std::max(mx, lens[k]);
    }
    ZK_TRY(ensure_init());
    if (md_is_composite(srs)) return set_err(ZK_ERR_ARG, "kzg: openings need the SRS on one device entry");
    int g2 = 0;
    ZK_TRY(bases_info(srs, srs_n, &g2));
    if (g2) return set_err(ZK_ERR_ARG, "the KZG SRS must be a G1 base array");
    if (mx > *srs_n) return set_err(ZK_ERR_LEN, "%s", kErrSize);
    *maxlen = mx;
    return ZK_OK;
}

}  // namespace
}  // namespace zkmi

using namespace zkmi;

extern "C" {

int zk_bn254_kzg_open(uint64_t srs, const void* const* polys, const size_t* lens, const zk_fr* points, size_t count, int on_device, zk_kzg_opening* out) {
    if (count && (!points || !out)) return set_err(ZK_ERR_ARG, "null pointer");
    size_t srs_n = 0, maxlen = 0;
    ZK_TRY(check_open_args(srs, polys, lens, count, &srs_n, &maxlen));
    ZK_ON_ENTRY_OF(srs);
    SlotGuard g;
    ZK_TRY(acquire_slot(&g.s));
    Slot* s = g.s;
    hipStream_t st = s->stream;
    const size_t rows_max = std::min(count, (size_t)HSCAN_BATCH_MAX);
    const size_t row_bytes = align_up(maxlen * sizeof(Fr), 256);
    // ONE number K of coefficients per lane for every chunk, that of the call's longest polynomial: with K fixed the number of workgroups grows with the
    // length, so the reservation below (the longest polynomial's) covers every chunk.  (With K chosen per chunk it would not: K steps up with the length.)
    uint32_t K = 0, nb_max = 0;
    scan_geometry(maxlen, &K, &nb_max);
    const size_t stride = row_bytes;
    ZK_TRY(s->reserve(rows_max * (row_bytes + (size_t)nb_max * 257 * sizeof(Fr)) + 16 * 1024));
    const size_t mark = s->arena_off;
    std::vector<HFr> evals(rows_max);
    for (size_t c0 = 0; c0 < count; c0 += HSCAN_BATCH_MAX) {
        const size_t rows = std::min((size_t)HSCAN_BATCH_MAX, count - c0);
        s->arena_off = mark;
        size_t cmax = 0;
        for (size_t r = 0; r < rows; r++) cmax = std::max(cmax, lens[c0 + r]);
        const uint32_t nb = (uint32_t)(((cmax + K - 1) / K + 255) / 256);  // <= nb_max
        char* d_rows = (char*)s->alloc(rows * stride);  // host input: the uploaded rows, divided in place; device input: the quotients
        Fr* d_t = (Fr*)s->alloc(rows * (size_t)nb * 256 * sizeof(Fr));
        Fr* d_b = (Fr*)s->alloc(rows * (size_t)nb * sizeof(Fr));
        Fr* d_ev = (Fr*)s->alloc(HSCAN_BATCH_MAX * sizeof(Fr));
        if (!d_rows || !d_t || !d_b || !d_ev) return set_err(ZK_ERR_HIP, "kzg_open: workspace was not reserved");
        ZK_HIP(hipMemset2DAsync(d_rows, stride, 0, cmax * sizeof(Fr), rows, st));  // the commitments below read a group's rows up to the group's longest quotient
        HscanRows R;
        for (int r = 0; r < HSCAN_BATCH_MAX; r++) {
            const size_t k = c0 + ((size_t)r < rows ? r : 0);
            Fr* q = (Fr*)(d_rows + ((size_t)r < rows ? r : 0) * stride);
            if (!on_device && (size_t)r < rows) ZK_TRY(h2d_big(q, polys[k], lens[k] * sizeof(Fr), st));
            const HFr a = hfr(points[k]), A = pow_u32(a, K);
            HFr M = A;
            for (int i = 0; i < 8; i++) M = M.sqr();
            R.f[r] = on_device ? (const Fr*)polys[k] : q;
            R.q[r] = q;
            R.len[r] = lens[k];
            R.a[r] = to_dev(a);
            R.A[r] = to_dev(A);
            R.M[r] = to_dev(M);
        }
        ZK_LAUNCH(s, st, "kzg_horner_local", k_hscan_local_rows, dim3(nb, (unsigned)rows), dim3(256), 0, R, K, nb, d_t, d_b);
        ZK_LAUNCH(s, st, "kzg_horner_blocks", k_hscan_blocks_rows, dim3((unsigned)rows), dim3(1024), 0, R, d_b, nb, d_ev);
        ZK_LAUNCH(s, st, "kzg_divide_apply", k_hscan_apply_rows, dim3(nb, (unsigned)rows), dim3(256), 0, R, K, nb, (const Fr*)d_t, (const Fr*)d_b);
        ZK_HIP(hipMemcpyAsync(evals.data(), d_ev, rows * sizeof(Fr), hipMemcpyDeviceToHost, st));
        ZK_TRY(slot_sync(s, st));  // the commitments run on stream slots of their own
        // H_k = Commit(q_k): up to three quotients share one recoding and one accumulate launch (rows zero-padded to the group's longest); a constant
        // polynomial has an empty quotient: H = infinity, no commitment
        std::vector<size_t> live;
        for (size_t r = 0; r < rows; r++) {
            memcpy(&out[c0 + r].claimed_value, &evals[r], 32);
            memset(&out[c0 + r].h, 0, sizeof(zk_g1_affine));
            if (lens[c0 + r] > 1) live.push_back(r);
        }
        for (size_t g0 = 0; g0 < live.size(); g0 += 3) {
            const uint32_t cnt = (uint32_t)std::min((size_t)3, live.size() - g0);
            const void* sc[3] = {nullptr, nullptr, nullptr};
            size_t n = 0;
            for (uint32_t j = 0; j < cnt; j++) {
                sc[j] = d_rows + live[g0 + j] * stride;
                n = std::max(n, lens[c0 + live[g0 + j]] - 1);
            }
            zk_g1_affine h[3];
            ZK_TRY(zk_bn254_msm_bases_batch_dev(srs, 0, sc, cnt, n, &kMont, h));
            for (uint32_t j = 0; j < cnt; j++) out[c0 + live[g0 + j]].h = h[j];
        }
    }
    return ZK_OK;
}

int zk_bn254_kzg_batch_open_single_point(uint64_t srs, const void* const* polys, const size_t* lens, const zk_g1_affine* digests, size_t count, const zk_fr* point,
                                         int on_device, zk_g1_affine* out_h, zk_fr* out_claimed) {
    if (count && (!digests || !point || !out_h || !out_claimed)) return set_err(ZK_ERR_ARG, "null pointer");
    size_t srs_n = 0, maxlen = 0;
    ZK_TRY(check_open_args(srs, polys, lens, count, &srs_n, &maxlen));
    ZK_ON_ENTRY_OF(srs);
    SlotGuard g;
    ZK_TRY(acquire_slot(&g.s));
    Slot* s = g.s;
    hipStream_t st = s->stream;
    size_t upload = 0;
    if (!on_device)
        for (size_t k = 0; k < count; k++) upload += align_up(lens[k] * sizeof(Fr), 256);
    ZK_TRY(s->reserve(upload + align_up(maxlen * sizeof(Fr), 256) + scan_need(maxlen) + count * (2 * sizeof(Fr) + 16) + 16 * 1024));
    std::vector<const Fr*> f(count);
    for (size_t k = 0; k < count; k++) {
        if (on_device) { f[k] = (const Fr*)polys[k]; continue; }
        Fr* d = (Fr*)s->alloc(lens[k] * sizeof(Fr));
        if (!d) return set_err(ZK_ERR_HIP, "kzg_batch_open: workspace was not reserved");
        ZK_TRY(h2d_big(d, polys[k], lens[k] * sizeof(Fr), st));
        f[k] = d;
    }
    Fr* d_fold = (Fr*)s->alloc(maxlen * sizeof(Fr));
    Fr* d_vals = (Fr*)s->alloc((count + 1) * sizeof(Fr));  // the claimed values, then the folded polynomial's
    Fr* d_gpow = (Fr*)s->alloc(count * sizeof(Fr));
    const Fr** d_ptrs = (const Fr**)s->alloc(count * sizeof(Fr*));
    size_t* d_lens = (size_t*)s->alloc(count * sizeof(size_t));
    ScanBufs B;
    ZK_TRY(scan_bufs(s, maxlen, &B));
    if (!d_fold || !d_vals || !d_gpow || !d_ptrs || !d_lens) return set_err(ZK_ERR_HIP, "kzg_batch_open: workspace was not reserved");
    const HFr z = hfr(*point);
    // every claimed value: the batched evaluation scan, HSCAN_BATCH_MAX rows per launch pair
    for (size_t c0 = 0; c0 < count; c0 += HSCAN_BATCH_MAX) {
        const int rows = (int)std::min((size_t)HSCAN_BATCH_MAX, count - c0);
        ZK_TRY(poly_eval_batch_dev(s, st, f.data() + c0, lens + c0, rows, z, B, d_vals + c0));
    }
    std::vector<HFr> claimed(count), gpow(count);
    ZK_HIP(hipMemcpyAsync(claimed.data(), d_vals, count * sizeof(Fr), hipMemcpyDeviceToHost, st));
    ZK_TRY(slot_sync(s, st));
    std::vector<Affine<HFp>> dg(count);
    memcpy(dg.data(), digests, count * 64);
    const HFr gamma = kzg_derive_gamma(z, dg.data(), claimed.data(), count);
    HFr acc = HFr::one();
    for (size_t k = 0; k < count; k++) {
        gpow[k] = acc;
        acc = acc * gamma;
    }
    ZK_HIP(hipMemcpyAsync(d_gpow, gpow.data(), count * sizeof(Fr), hipMemcpyHostToDevice, st));
    ZK_HIP(hipMemcpyAsync(d_ptrs, f.data(), count * sizeof(Fr*), hipMemcpyHostToDevice, st));
    ZK_HIP(hipMemcpyAsync(d_lens, lens, count * sizeof(size_t), hipMemcpyHostToDevice, st));
    ZK_LAUNCH(s, st, "kzg_fold", k_fold_rows, dim3((unsigned)((maxlen + 255) / 256)), dim3(256), 0, (const Fr* const*)d_ptrs, (const size_t*)d_lens, (const Fr*)d_gpow,
              (uint32_t)count, maxlen, d_fold);
    ZK_TRY(poly_divide_dev(s, st, d_fold, maxlen, z, B, d_fold, d_vals + count));
    ZK_TRY(slot_sync(s, st));
    memcpy(out_claimed, claimed.data(), count * 32);
    memset(out_h, 0, sizeof *out_h);
    if (maxlen > 1) ZK_TRY(zk_bn254_msm_bases_dev(srs, 0, d_fold, maxlen - 1, &kMont, out_h));
    return ZK_OK;
}

}  // extern "C"
