// The Horner suffix scan with its points in the kernel arguments (scan.hpp): the three kernels over scan.hpp's bodies, row = blockIdx.y, and the host functions
// that launch them -- the evaluations and the division of the PLONK prover (plonk.hip) and the openings of kzg.hip.
#include "scan.hpp"

#include <algorithm>

namespace zkmi {

// pass 1, grid (nb, rows): lane Horner totals, workgroup suffix scan; lane carry-ins to tcarry (where given), the workgroup's total to btot.  A workgroup wholly
// above the row's last coefficient contributes zeros.  The body gets the true number of lanes that start below len, as k_hscan_local_dev gives it.
__global__ __launch_bounds__(256) void k_hscan_local_rows(HscanRows R, uint32_t K, uint32_t nb, Fr* __restrict__ tcarry, Fr* __restrict__ btot) {
    __shared__ Fr sh[256];
    const size_t len = R.len[blockIdx.y];
    const size_t blk = (size_t)blockIdx.y * nb + blockIdx.x, first = (size_t)blockIdx.x * 256 * K;
    if (first >= len) {  // uniform over the workgroup
        if (tcarry) tcarry[blk * 256 + threadIdx.x] = Fr::zero();
        if (threadIdx.x == 0) btot[blk] = Fr::zero();
        return;
    }
    const Fr a = R.a[blockIdx.y], A = R.A[blockIdx.y];
    const size_t lanes = (len - first + K - 1) / K;
    const Fr val = hscan_local_body(sh, R.f[blockIdx.y], len, K, first + (size_t)threadIdx.x * K, a, A, lanes < 256 ? (uint32_t)lanes : 256u);
    if (tcarry) tcarry[blk * 256 + threadIdx.x] = threadIdx.x < 255 ? sh[threadIdx.x + 1] : Fr::zero();
    if (threadIdx.x == 0) btot[blk] = val;
}
// pass 2, one workgroup per row: btot[row nb + b] <- sum_{b' > b} btot[row nb + b'] M^(b' - b - 1); total[row] = f(a)
__global__ __launch_bounds__(1024) void k_hscan_blocks_rows(HscanRows R, Fr* __restrict__ btot, uint32_t nb, Fr* __restrict__ total) {
    __shared__ Fr sh[1024];
    const Fr M = R.M[blockIdx.x];
    const Fr tot = hscan_blocks_body(sh, btot + (size_t)blockIdx.x * nb, nb, M);
    if (threadIdx.x == 0) total[blockIdx.x] = tot;
}
// pass 3, grid (nb, rows): q_i = S_(i+1) for every i < len, so q[len - 1] = 0; q may alias f
__global__ __launch_bounds__(256) void k_hscan_apply_rows(HscanRows R, uint32_t K, uint32_t nb, const Fr* __restrict__ tcarry, const Fr* __restrict__ bC) {
    const size_t len = R.len[blockIdx.y];
    const size_t blk = (size_t)blockIdx.y * nb + blockIdx.x, base = ((size_t)blockIdx.x * 256 + threadIdx.x) * K;
    if (base >= len) return;
    const Fr a = R.a[blockIdx.y], A = R.A[blockIdx.y];
    hscan_apply_body(R.f[blockIdx.y], R.q[blockIdx.y], len, len, K, base, a, A, ld(tcarry + blk * 256 + threadIdx.x), ld(bC + blk));
}

int hscan_rows_passes(Slot* s, hipStream_t st, const HscanNames& names, const HscanRows& R, unsigned rows, uint32_t K, uint32_t nb, Fr* tcarry, Fr* btot, Fr* total,
                      HscanTrace* trace) {
    if (rows < 1 || rows > (unsigned)HSCAN_BATCH_MAX) return set_err(ZK_ERR_ARG, "scan over %u rows", rows);
    ZK_LAUNCH(s, st, names.local, k_hscan_local_rows, dim3(nb, rows), dim3(256), 0, R, K, nb, tcarry, btot);
    if (trace) {  // inspection: pass 2 overwrites the totals in place
        trace->btot_local.resize((size_t)rows * nb);
        ZK_HIP(hipStreamSynchronize(st));
        ZK_HIP(hipMemcpy(trace->btot_local.data(), btot, (size_t)rows * nb * sizeof(Fr), hipMemcpyDeviceToHost));
    }
    ZK_LAUNCH(s, st, names.blocks, k_hscan_blocks_rows, dim3(rows), dim3(1024), 0, R, btot, nb, total);
    if (tcarry) ZK_LAUNCH(s, st, names.apply, k_hscan_apply_rows, dim3(nb, rows), dim3(256), 0, R, K, nb, (const Fr*)tcarry, (const Fr*)btot);
    return ZK_OK;
}

int scan_bufs(Slot* s, size_t len, ScanBufs* B) {
    scan_plan(len, &B->K, &B->nb);
    B->t = (Fr*)s->alloc((size_t)B->nb * 256 * sizeof(Fr));
    B->b = (Fr*)s->alloc((size_t)HSCAN_BATCH_MAX * B->nb * sizeof(Fr) + 64);  // HSCAN_BATCH_MAX rows: poly_eval_batch_dev
    B->total = (Fr*)s->alloc(64);
    if (!B->t || !B->b || !B->total) return set_err(ZK_ERR_HIP, "PLONK scan workspace was not reserved");
    return ZK_OK;
}

static const HscanNames kPlonkNames = {"plonk_horner_local", "plonk_horner_blocks", "plonk_divide_apply"};

int poly_eval_batch_dev(Slot* s, hipStream_t st, const Fr* const* f, const size_t* len, int cnt, const HFr& a, const ScanBufs& B, Fr* d_out) {
    if (cnt < 1 || cnt > HSCAN_BATCH_MAX) return set_err(ZK_ERR_ARG, "evaluation batch of %d", cnt);
    HscanRows R = {};
    hscan_row(&R, 0, f[0], nullptr, len[0], a, B.K);
    for (int k = 1; k < cnt; k++) {  // the same point in every row
        R.f[k] = f[k]; R.len[k] = len[k];
        R.a[k] = R.a[0]; R.A[k] = R.A[0]; R.M[k] = R.M[0];
    }
    return hscan_rows_passes(s, st, kPlonkNames, R, (unsigned)cnt, B.K, B.nb, nullptr, B.b, d_out);
}

int poly_divide_dev(Slot* s, hipStream_t st, const Fr* f, size_t len, const HFr& a, const ScanBufs& B, Fr* q, Fr* d_eval) {
    HscanRows R = {};
    hscan_row(&R, 0, f, q, len, a, B.K);
    return hscan_rows_passes(s, st, kPlonkNames, R, 1, B.K, B.nb, B.t, B.b, d_eval);
}

// the scan alone, for inspection / tests (include/zkmi.h): host rows with their guards up, hscan_row and hscan_rows_passes as the provers call them, with a
// trace; every stage and every row, guards included, copied back
static int hscan_inspect_run(Slot* s, const zk_hscan_request* q, zk_hscan_result* r, uint32_t nb) {
    hipStream_t st = s->stream;
    const unsigned rows = q->rows;
    const size_t pad = q->pad, stage = (size_t)rows * nb;
    size_t need = stage * 257 * sizeof(Fr) + 16 * 1024;
    for (unsigned k = 0; k < rows; k++) need += 2 * (align_up((q->len[k] + 2 * pad) * sizeof(Fr), 256) + 256);
    ZK_TRY(s->reserve(need));
    Fr *d_f[HSCAN_BATCH_MAX] = {}, *d_q[HSCAN_BATCH_MAX] = {};
    for (unsigned k = 0; k < rows; k++) {
        const size_t bytes = (q->len[k] + 2 * pad) * sizeof(Fr);
        for (unsigned u = 0; u < k; u++)
            if (q->f[u] == q->f[k]) d_f[k] = d_f[u];  // the same host row twice: the same device row twice
        if (!d_f[k]) {
            d_f[k] = (Fr*)s->alloc(bytes);
            if (!d_f[k]) return set_err(ZK_ERR_HIP, "scan inspection: row buffer was not reserved");
            ZK_TRY(h2d_big(d_f[k], q->f[k], bytes, st));
        }
        if (q->q[k] == q->f[k]) {
            d_q[k] = d_f[k];
        } else if (q->q[k]) {
            d_q[k] = (Fr*)s->alloc(bytes);
            if (!d_q[k]) return set_err(ZK_ERR_HIP, "scan inspection: quotient buffer was not reserved");
            ZK_TRY(h2d_big(d_q[k], q->q[k], bytes, st));
        }
    }
    Fr* d_t = (Fr*)s->alloc(stage * 256 * sizeof(Fr));
    Fr* d_b = (Fr*)s->alloc(stage * sizeof(Fr));
    Fr* d_total = (Fr*)s->alloc(HSCAN_BATCH_MAX * sizeof(Fr));
    if (!d_t || !d_b || !d_total) return set_err(ZK_ERR_HIP, "scan inspection: workspace was not reserved");
    auto up = [&](Fr* dst, const zk_fr* src, size_t count) -> int {  // the caller's content (its poison), or zeros
        if (src) return h2d_big(dst, src, count * sizeof(Fr), st);
        ZK_HIP(hipMemsetAsync(dst, 0, count * sizeof(Fr), st));
        return ZK_OK;
    };
    ZK_TRY(up(d_t, r->tcarry, stage * 256));
    ZK_TRY(up(d_b, r->btot, stage));
    ZK_TRY(up(d_total, r->total, rows));
    HscanRows R = {};
    for (unsigned k = 0; k < rows; k++) {
        HFr a;
        memcpy(&a, &q->a[k], 32);
        hscan_row(&R, (int)k, d_f[k] + pad, d_q[k] ? d_q[k] + pad : nullptr, q->len[k], a, q->K);
    }
    HscanTrace trace;
    ZK_TRY(hscan_rows_passes(s, st, kPlonkNames, R, rows, q->K, nb, q->eval_only ? nullptr : d_t, d_b, d_total, &trace));
    ZK_TRY(slot_sync(s, st));
    auto back = [&](zk_fr* dst, const Fr* src, size_t count) -> int {
        if (dst && count) ZK_HIP(hipMemcpy(dst, src, count * sizeof(Fr), hipMemcpyDeviceToHost));
        return ZK_OK;
    };
    ZK_TRY(back(r->tcarry, d_t, stage * 256));
    if (r->btot_local) memcpy(r->btot_local, trace.btot_local.data(), stage * sizeof(Fr));
    ZK_TRY(back(r->btot, d_b, stage));
    ZK_TRY(back(r->total, d_total, rows));
    for (unsigned k = 0; k < rows; k++) {
        bool first = true;
        for (unsigned u = 0; u < k; u++) first = first && q->f[u] != q->f[k];
        if (first) ZK_TRY(back(q->f[k], d_f[k], q->len[k] + 2 * pad));
        if (d_q[k] && d_q[k] != d_f[k]) ZK_TRY(back(q->q[k], d_q[k], q->len[k] + 2 * pad));
    }
    return ZK_OK;
}

}  // namespace zkmi

using namespace zkmi;

extern "C" int zk_bn254_hscan_inspect(const zk_hscan_request* q, zk_hscan_result* r) {
    if (!q || !r) return set_err(ZK_ERR_ARG, "null pointer");
    if (q->rows < 1 || q->rows > (uint32_t)HSCAN_BATCH_MAX) return set_err(ZK_ERR_ARG, "scan inspection: %u rows (1 to %d)", q->rows, HSCAN_BATCH_MAX);
    if (q->K == 0) return set_err(ZK_ERR_ARG, "scan inspection: K = 0 coefficients per lane");
    size_t maxlen = 0;
    for (unsigned k = 0; k < q->rows; k++) {
        if (!q->f[k]) return set_err(ZK_ERR_ARG, "null pointer");
        if (q->len[k] == 0 || q->len[k] > ((size_t)1 << 28)) return set_err(ZK_ERR_ARG, "scan inspection: row %u of %zu coefficients", k, q->len[k]);
        if (!q->q[k] && !q->eval_only) return set_err(ZK_ERR_ARG, "scan inspection: row %u has no place for its quotient", k);
        for (unsigned u = 0; u < k; u++) {
            if (q->f[u] == q->f[k] && q->len[u] != q->len[k]) return set_err(ZK_ERR_ARG, "scan inspection: rows %u and %u share coefficients of two lengths", u, k);
            if (q->f[u] == q->f[k] && (q->q[u] == q->f[u] || q->q[k] == q->f[k]))
                return set_err(ZK_ERR_ARG, "scan inspection: rows %u and %u share their coefficients, which cannot be divided in place", u, k);
            if (q->q[k] && (q->q[u] == q->q[k] || q->q[k] == q->f[u] || q->q[u] == q->f[k]))
                return set_err(ZK_ERR_ARG, "scan inspection: rows %u and %u overlap in a quotient", u, k);
        }
        maxlen = std::max(maxlen, q->len[k]);
    }
    const uint32_t nb_min = scan_blocks(maxlen, q->K), nb = q->nb ? q->nb : nb_min;
    if (nb < nb_min) return set_err(ZK_ERR_ARG, "scan inspection: nb = %u, the longest row needs %u", nb, nb_min);
    if ((size_t)q->rows * nb > 65536) return set_err(ZK_ERR_ARG, "scan inspection: %u rows of %u workgroups (65536 in all)", q->rows, nb);
    static_assert(ZK_HSCAN_ROWS_MAX == HSCAN_BATCH_MAX, "the inspection's rows are one launch's");
    r->nb = nb;
    SlotGuard g;
    ZK_TRY(acquire_slot(&g.s));
    int rc = hscan_inspect_run(g.s, q, r, nb);
    if (rc != ZK_OK) (void)hipStreamSynchronize(g.s->stream);  // nothing of this call is in flight when the slot goes back
    return rc;
}
