// The Horner suffix scan with its points in the kernel arguments (scan.hpp): the three kernels over scan.hpp's bodies, row = blockIdx.y, and the host functions
// that launch them -- the evaluations and the division of the PLONK prover (plonk.hip) and the openings of kzg.hip.
#include "scan.hpp"

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

int hscan_rows_passes(Slot* s, hipStream_t st, const HscanNames& names, const HscanRows& R, unsigned rows, uint32_t K, uint32_t nb, Fr* tcarry, Fr* btot, Fr* total) {
    if (rows < 1 || rows > (unsigned)HSCAN_BATCH_MAX) return set_err(ZK_ERR_ARG, "scan over %u rows", rows);
    ZK_LAUNCH(s, st, names.local, k_hscan_local_rows, dim3(nb, rows), dim3(256), 0, R, K, nb, tcarry, btot);
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

}  // namespace zkmi
