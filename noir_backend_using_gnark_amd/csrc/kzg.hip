// KZG openings on the device (include/zkmi.h "KZG openings"): gnark-crypto v0.9.1 ecc/bn254/fr/kzg  [UPSTREAM-RECALL]
//   kzg.Open(p, point, srs)                                   zk_bn254_kzg_open, count = 1 (count > 1: independent openings in one launch set)
//   kzg.BatchOpenSinglePoint(polys, digests, point, hf, srs)  zk_bn254_kzg_batch_open_single_point (hf = SHA-256, what gnark's PLONK passes)
// An opening is the Horner suffix scan of scan.hpp (S_i = f_i + a S_(i+1): S_0 = f(a), q_i = S_(i+1) are the coefficients of (f - f(a)) / (X - a) --
// kzg.dividePolyByXminusA) followed by kzg.Commit of the quotient over the resident SRS.  The scan's kernels index polynomial, length and point by blockIdx.y,
// so that `count` openings are three launches per HSCAN_BATCH_MAX of them, not 3 x count.
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
const HscanNames kOpenNames = {"kzg_horner_local", "kzg_horner_blocks", "kzg_divide_apply"};
const char* const kErrSize = "kzg: invalid polynomial size (larger than SRS or == 0)";  // ErrInvalidPolynomialSize

HFr hfr(const zk_fr& x) {
    HFr r;
    memcpy(&r, &x, 32);
    return r;
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
    scan_plan(maxlen, &K, &nb_max);
    const size_t stride = row_bytes;
    ZK_TRY(s->reserve(rows_max * (row_bytes + (size_t)nb_max * 257 * sizeof(Fr)) + 16 * 1024));
    const size_t mark = s->arena_off;
    std::vector<HFr> evals(rows_max);
    for (size_t c0 = 0; c0 < count; c0 += HSCAN_BATCH_MAX) {
        const size_t rows = std::min((size_t)HSCAN_BATCH_MAX, count - c0);
        s->arena_off = mark;
        size_t cmax = 0;
        for (size_t r = 0; r < rows; r++) cmax = std::max(cmax, lens[c0 + r]);
        const uint32_t nb = scan_blocks(cmax, K);  // <= nb_max
        char* d_rows = (char*)s->alloc(rows * stride);  // host input: the uploaded rows, divided in place; device input: the quotients
        Fr* d_t = (Fr*)s->alloc(rows * (size_t)nb * 256 * sizeof(Fr));
        Fr* d_b = (Fr*)s->alloc(rows * (size_t)nb * sizeof(Fr));
        Fr* d_ev = (Fr*)s->alloc(HSCAN_BATCH_MAX * sizeof(Fr));
        if (!d_rows || !d_t || !d_b || !d_ev) return set_err(ZK_ERR_HIP, "kzg_open: workspace was not reserved");
        ZK_HIP(hipMemset2DAsync(d_rows, stride, 0, cmax * sizeof(Fr), rows, st));  // the commitments below read a group's rows up to the group's longest quotient
        HscanRows R = {};
        for (size_t r = 0; r < rows; r++) {
            const size_t k = c0 + r;
            Fr* q = (Fr*)(d_rows + r * stride);
            if (!on_device) ZK_TRY(h2d_big(q, polys[k], lens[k] * sizeof(Fr), st));
            hscan_row(&R, (int)r, on_device ? (const Fr*)polys[k] : q, q, lens[k], hfr(points[k]), K);
        }
        ZK_TRY(hscan_rows_passes(s, st, kOpenNames, R, (unsigned)rows, K, nb, d_t, d_b, d_ev));
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
