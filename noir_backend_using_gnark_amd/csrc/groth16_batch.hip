// Groth16 prove for MANY witnesses against ONE resident key in one call: zk_bn254_groth16_prove_batch / zk_bn254_groth16_prove_r1cs_batch.
// The contract is the single prover's, row by row: proofs_out[128 i ..] is byte for byte what zk_bn254_groth16_prove writes for row i with (r[i], s[i]).
// A proof's bytes are the canonical compressed images of three group elements, so any schedule that computes the same elements writes the same bytes.
//
// One small proof cannot fill the machine: below 2^16 constraints it is launch chains, event gaps and the reduction tails of five MSMs of a few waves each
// (3.0 ms at 2^16 against 9.5 ms at 2^20).  The batched path turns the rows of a chunk into ONE instance of each of those chains:
//   * the scalar side of A, B1, K and G2.B: one recoding of the whole w matrix (msm.hip DigitRows: row v feeds bucket set v, key = v * B + digit - 1; zero digits
//     dropped before the sort as in the single prover), one sort, one task plan; the same once more over the h matrix for Z;
//   * one accumulate launch per base array -- G2.B, A, B1, K, Z, chained as in the single prover -- over S bucket sets, and one reduction that yields S sums;
//   * the R1CS step (prove_r1cs_batch) as one launch with the row as a grid dimension (r1cs.hip k_spmv3_rows);
//   * computeH of the whole chunk in the launches of ONE computeH (ntt.hip compute_h_rows_inplace: the row is a grid dimension of every pass);
//   * the tail -- five sums + (r, s) -> 128 proof bytes -- of all S rows in ONE launch (groth16_tail.hip) for domains up to DEVICE_TAIL_MAX_LOG_DOMAIN, on a few
//     host threads per row above it (DESIGN.md 3.12 says where that constant comes from).
#include <string.h>

#include <algorithm>
#include <thread>
#include <vector>

#include "ctx.hpp"
#include "curve.hpp"
#include "groth16_batch.hpp"
#include "host_ff.hpp"
#include "msm.hpp"
#include "multidev.hpp"
#include "ntt.hpp"

namespace zkmi {

// Largest domain the batched path serves (DESIGN.md 3.12 has the table behind it) and the workspace one call may hold over its five slots.
static constexpr unsigned BATCH_MAX_LOG_DOMAIN = 16;
static constexpr size_t BATCH_MAX_ROWS = 256;
static constexpr size_t BATCH_WORKSPACE = (size_t)1 << 30;
// Largest domain whose chunks take the device tail (groth16_tail.hip); above it the rows' tails stay on host threads.  The rule is the parent / this-commit
// table of tools/groth16_batch_bench.py: the device tail serves a size only where the batch time stayed within the 3 % run-to-run band of the
// parent's.  That table has NOT been measured yet, and the estimate in DESIGN.md 3.12 (one launch costs the latency of a 254-bit double-and-add chain, about
// 4 ms, whatever S is; the host tail costs S x 0.35 ms / 8 threads) favours the host below 128 rows per chunk: until the table exists no size takes the device
// tail here (0: every domain is above it).  The public entries (zk_bn254_groth16_finalize_batch[_dev]) do not depend on this.
static constexpr unsigned DEVICE_TAIL_MAX_LOG_DOMAIN = 0;
static const zk_msm_cfg kMontCfg = {0, 1, 0, 0};  // scalars are Montgomery fr.Element images

// Which keys the batched path serves.  It needs ONE device's window tables with every window in one bucket set per row, so: not a composite (multi-device) key,
// not a key without tables (flags bit 0, or tables that did not fit), not a window-sharded key (its rows are a subset) and not a range-sharded slice (nz != N - 1);
// and a domain small enough that a single proof leaves the machine idle.  Everything else goes row by row through zk_bn254_groth16_prove: same bytes.
static bool batch_serves(const Groth16BatchView& V) {
    const size_t N = (size_t)1 << V.log_domain;
    return V.tables && V.tab_w.row_step == 1 && V.tab_h.row_step == 1 && V.tab_w.row_first == 0 && V.tab_h.row_first == 0 && V.nz == N - 1 && N > 1 && V.n_wires > 0 &&
           V.log_domain <= BATCH_MAX_LOG_DOMAIN;
}

// Arena bytes of the five slots for a chunk of S rows: per row and base array one bucket set (partial sums + reduction levels; the G2 set is twice the bytes),
// the sort's key / value arrays of both scalar matrices, and on slot 0 the a, b, c rows of computeH (3 x N x 32 B per row; h replaces a) and the staged w rows.
struct BatchNeed {
    size_t slot[5];
    size_t msm0;  // the MSM's share of slot 0 (prepare(h) + Z), which the layout of the call's own buffers counts as `later`
    size_t total() const { return slot[0] + slot[1] + slot[2] + slot[3] + slot[4]; }
};
static int batch_need(const Groth16BatchView& V, size_t S, BatchNeed* out) {
    const size_t N = (size_t)1 << V.log_domain;
    size_t prep_w = 0, acc1_w = 0, acc2_w = 0, prep_h = 0, acc1_h = 0;
    ZK_TRY(msm_prep_need_table_rows(V.n_wires, (unsigned)S, V.tab_w, nullptr, &prep_w, &acc1_w, &acc2_w));
    ZK_TRY(msm_prep_need_table_rows(V.nz, (unsigned)S, V.tab_h, nullptr, &prep_h, &acc1_h, nullptr));
    out->msm0 = prep_h + acc1_h + 4096;
    out->slot[0] = S * (3 * N + V.n_wires) * 32 + 4 * 256 + out->msm0;
    out->slot[1] = out->slot[2] = out->slot[3] = acc1_w + 4096;
    out->slot[4] = prep_w + acc2_w + msm_compact_need(V.n_wires, (unsigned)S) + 4096;
    return ZK_OK;
}
// rows per chunk: the largest of 256, 128, ..., 1 whose workspace fits BATCH_WORKSPACE (a pure function of the key's geometry)
static int batch_chunk_rows(const Groth16BatchView& V, size_t* rows) {
    size_t S = BATCH_MAX_ROWS;
    for (; S > 1; S >>= 1) {
        BatchNeed need;
        if (batch_need(V, S, &need) == ZK_OK && need.total() <= BATCH_WORKSPACE) break;
    }
    *rows = S;
    return ZK_OK;
}

struct BatchIn {
    const char *a, *b, *c, *w;  // row-major matrices, host or device
    size_t n_constraints;
    const zk_fr *r, *s;
    int on_device;
};

// The tail per row on the host like the single prover's (zk_bn254_groth16_finalize: the same arithmetic from the same five sums), over a few threads: two
// 254-bit scalar multiplications per proof in ONE thread would bound a batch's rate whatever the kernels do.  Serves the domains above DEVICE_TAIL_MAX_LOG_DOMAIN.
static int host_tail(uint64_t pk_handle, const BatchIn& in, size_t first, size_t S, const XYZZ<HFp>* m_a, const XYZZ<HFp>* m_b, const XYZZ<HFp>* m_k,
                     const XYZZ<HFp>* m_z, const XYZZ<HFp2>* m_b2, uint8_t* proofs_out) {
    const unsigned nthreads = (unsigned)std::min<size_t>(8, (S + 3) / 4);
    std::vector<int> rcs(nthreads, ZK_OK);
    std::vector<std::string> msgs(nthreads);
    auto work = [&](unsigned t) {
        for (size_t i = t; i < S; i += nthreads) {
            uint64_t parts[96];
            memcpy(parts, &m_a[i], 128);
            memcpy(parts + 16, &m_b[i], 128);
            memcpy(parts + 32, &m_k[i], 128);
            memcpy(parts + 48, &m_z[i], 128);
            memcpy(parts + 64, &m_b2[i], 256);
            const int r1 = zk_bn254_groth16_finalize(pk_handle, parts, 1, in.r + first + i, in.s + first + i, proofs_out + 128 * (first + i));
            if (r1 != ZK_OK && rcs[t] == ZK_OK) { rcs[t] = r1; msgs[t] = g_err; }
        }
    };
    std::vector<std::thread> pool;
    for (unsigned t = 1; t < nthreads; t++) pool.emplace_back(work, t);
    work(0);
    for (auto& th : pool) th.join();
    for (unsigned t = 0; t < nthreads; t++)
        if (rcs[t] != ZK_OK) return set_err(rcs[t], "%s", msgs[t].c_str());
    return ZK_OK;
}

// one chunk of S rows starting at row `first`, on the call's five slots
static int prove_chunk(uint64_t pk_handle, const Groth16BatchView& V, Slot* sl[5], const BatchIn& in, size_t first, size_t S, uint8_t* proofs_out) {
    const size_t N = (size_t)1 << V.log_domain, nw = V.n_wires, nc = in.n_constraints;
    for (int i = 0; i < 5; i++) sl[i]->reset();
    const bool device_tail = V.log_domain <= DEVICE_TAIL_MAX_LOG_DOMAIN;
    Groth16TailView tail_view;
    if (device_tail) ZK_TRY(groth16_pk_tail_view(pk_handle, &tail_view));  // (a key's first device tail builds its delta tables: before anything is enqueued)
    BatchNeed need;
    ZK_TRY(batch_need(V, S, &need));
    Fr *d_a = nullptr, *d_b = nullptr, *d_c = nullptr, *d_w = nullptr;
    ZK_TRY(plan_workspace(sl[0], "groth16 batch", [&](ArenaPlan& p) {
        p.take(S * N, d_a, d_b, d_c);
        if (!in.on_device) p.take(S * nw, d_w);
        p.later(need.msm0);
    }));
    for (int i = 1; i < 5; i++) ZK_TRY(sl[i]->reserve(need.slot[i]));
    hipStream_t st0 = sl[0]->hi(), st4 = sl[4]->hi();
    const hipMemcpyKind kind = in.on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    MsmPrep prep_w, prep_h;
    MsmJob jobs[5];
    hipEvent_t ev_h = nullptr;
    auto enqueue = [&]() -> int {
        // ---- w rows -> prepare(w) on slot 4's stream, beside computeH as in the single prover (neither needs the other)
        const Fr* w_rows = (const Fr*)(in.w + first * nw * 32);
        if (!in.on_device) {
            ZK_HIP(hipMemcpyAsync(d_w, w_rows, S * nw * 32, kind, st4));
            w_rows = d_w;
        }
        ZK_TRY(msm_prepare_scalars_table_rows(sl[4], st4, w_rows, nw, (unsigned)S, nw, &kMontCfg, V.tab_w, &prep_w, true));
        // ---- a, b, c rows, zero-padded to the domain (the inputs are only read), then h = computeH of all S rows at once, left in the a rows
        Fr* dst[3] = {d_a, d_b, d_c};
        const char* src[3] = {in.a, in.b, in.c};
        for (int m = 0; m < 3; m++) {
            if (nc) ZK_HIP(hipMemcpy2DAsync(dst[m], N * 32, src[m] + first * nc * 32, nc * 32, nc * 32, S, kind, st0));
            if (nc < N) ZK_HIP(hipMemset2DAsync(dst[m] + nc, N * 32, 0, (N - nc) * 32, S, st0));
        }
        ZK_TRY(compute_h_rows_inplace(sl[0], st0, d_a, d_b, d_c, V.log_domain, S, N));
        ZK_HIP(hipEventCreateWithFlags(&ev_h, hipEventDisableTiming));
        ZK_HIP(hipEventRecord(ev_h, st0));
        // ---- accumulate chain G2.B -> A -> B1 -> K -> Z, each launch over all S bucket sets, each reduction tail under the next accumulate
        jobs[4].gate_acc = ev_h;  // a transform under an accumulate kernel is starved (groth16.hip): the chain starts when computeH has left the machine
        jobs[4].want_done = true;
        ZK_TRY(msm_g2_accumulate(sl[4], st4, prep_w, V.t_b2, 0, &jobs[4]));
        hipEvent_t prev = jobs[4].acc_done;
        const void* g1_tabs[4] = {nullptr, V.t_a, V.t_b, V.t_k};  // (the K table is wire-indexed: its public rows are points at infinity)
        for (int j = 1; j <= 3; j++) {
            jobs[j].gate_acc = prev;
            jobs[j].want_done = true;
            ZK_TRY(msm_g1_accumulate(sl[j], sl[j]->stream, prep_w, g1_tabs[j], 0, &jobs[j]));
            if (jobs[j].acc_done) prev = jobs[j].acc_done;
        }
        ZK_TRY(msm_prepare_scalars_table_rows(sl[0], st0, d_a, N, (unsigned)S, V.nz, &kMontCfg, V.tab_h, &prep_h));
        jobs[0].gate_acc = prev;
        ZK_TRY(msm_g1_accumulate(sl[0], st0, prep_h, V.t_z, 0, &jobs[0]));
        return ZK_OK;
    };
    int rc = enqueue();
    const size_t cap = S < 3 ? 3 : S;
    std::vector<XYZZ<HFp>> m_a(cap), m_b(cap), m_k(cap), m_z(cap);
    std::vector<XYZZ<HFp2>> m_b2(cap);
    if (rc == ZK_OK) rc = msm_g2_finish_sets(jobs[4], m_b2.data(), (unsigned)S);
    if (rc == ZK_OK) rc = msm_g1_finish_sets(jobs[1], m_a.data(), (unsigned)S);
    if (rc == ZK_OK) rc = msm_g1_finish_sets(jobs[2], m_b.data(), (unsigned)S);
    if (rc == ZK_OK) rc = msm_g1_finish_sets(jobs[3], m_k.data(), (unsigned)S);
    if (rc == ZK_OK) rc = msm_g1_finish_sets(jobs[0], m_z.data(), (unsigned)S);
    if (rc != ZK_OK) {  // whatever was enqueued drains before the slots go back
        const std::string msg = g_err;
        for (int i = 0; i < 5; i++) { (void)hipStreamSynchronize(sl[i]->stream); sl[i]->sync_hi(); }
        g_err = msg;
    }
    msm_prep_release(&prep_w);
    msm_prep_release(&prep_h);
    for (int i = 0; i < 5; i++)
        if (jobs[i].acc_done) (void)hipEventDestroy(jobs[i].acc_done);
    if (ev_h) (void)hipEventDestroy(ev_h);
    ZK_TRY(rc);
    // ---- the tail of groth16.Prove.  msm_*_finish_sets finished the last reduction step on the host, so the sums are host data: S x 768 bytes go up with the
    // r, s slices, ONE launch computes the S tails (groth16_tail.hip), S x 128 bytes come back.  The slots' streams are idle by now: slot 0's arena is free again.
    if (!device_tail) return host_tail(pk_handle, in, first, S, m_a.data(), m_b.data(), m_k.data(), m_z.data(), m_b2.data(), proofs_out);
    uint64_t* d_parts = nullptr;
    Fr *d_r = nullptr, *d_s = nullptr;
    uint8_t* d_out = nullptr;
    sl[0]->reset();
    ZK_TRY(plan_workspace(sl[0], "groth16 batch tail", [&](ArenaPlan& p) {
        p.take(S * 96, d_parts);
        p.take(S, d_r, d_s);
        p.take(S * 128, d_out);
    }));
    std::vector<uint64_t> parts(S * 96);
    for (size_t i = 0; i < S; i++) {
        uint64_t* q = parts.data() + 96 * i;
        memcpy(q, &m_a[i], 128);
        memcpy(q + 16, &m_b[i], 128);
        memcpy(q + 32, &m_k[i], 128);
        memcpy(q + 48, &m_z[i], 128);
        memcpy(q + 64, &m_b2[i], 256);
    }
    ZK_HIP(hipMemcpyAsync(d_parts, parts.data(), S * 768, hipMemcpyHostToDevice, st0));
    ZK_HIP(hipMemcpyAsync(d_r, in.r + first, S * 32, hipMemcpyHostToDevice, st0));
    ZK_HIP(hipMemcpyAsync(d_s, in.s + first, S * 32, hipMemcpyHostToDevice, st0));
    rc = groth16_tail_rows(sl[0], st0, tail_view, d_parts, 1, d_r, d_s, S, d_out);
    if (rc == ZK_OK && hipMemcpyAsync(proofs_out + 128 * first, d_out, S * 128, hipMemcpyDeviceToHost, st0) != hipSuccess) rc = set_err(ZK_ERR_HIP, "proof download failed");
    const int rc_sync = slot_sync(sl[0], st0);  // also on an error: what was enqueued drains before `parts` goes
    return rc != ZK_OK ? rc : rc_sync;
}

}  // namespace zkmi

using namespace zkmi;

extern "C" {

// rows per chunk of the batched path for this key, and whether the batched path serves it at all (*batched = 0: the rows go through the single prover)
int zk_bn254_groth16_batch_info(uint64_t pk_handle, size_t* chunk_rows, int* batched) {
    if (chunk_rows) *chunk_rows = 1;
    if (batched) *batched = 0;
    if (md_is_composite(pk_handle)) return ZK_OK;
    ZK_ON_ENTRY_OF(pk_handle);
    Groth16BatchView V;
    ZK_TRY(groth16_pk_batch_view(pk_handle, &V));
    if (!batch_serves(V)) return ZK_OK;
    size_t rows = 1;
    ZK_TRY(batch_chunk_rows(V, &rows));
    if (chunk_rows) *chunk_rows = rows;
    if (batched) *batched = 1;
    return ZK_OK;
}

int zk_bn254_groth16_prove_batch(uint64_t pk_handle, const void* a, const void* b, const void* c, size_t n_constraints, const void* w, size_t n_wires, const zk_fr* r,
                                 const zk_fr* s, size_t n_proofs, int on_device, uint8_t* proofs_out) {
    if (n_proofs == 0) return ZK_OK;
    if (!r || !s || !proofs_out) return set_err(ZK_ERR_ARG, "null pointer");
    if ((n_constraints && (!a || !b || !c)) || (n_wires && !w)) return set_err(ZK_ERR_ARG, "null pointer");
    const BatchIn in = {(const char*)a, (const char*)b, (const char*)c, (const char*)w, n_constraints, r, s, on_device};
    auto row_by_row = [&]() -> int {
        for (size_t i = 0; i < n_proofs; i++)
            ZK_TRY(zk_bn254_groth16_prove(pk_handle, in.a + i * n_constraints * 32, in.b + i * n_constraints * 32, in.c + i * n_constraints * 32, n_constraints,
                                          in.w + i * n_wires * 32, n_wires, r + i, s + i, on_device, proofs_out + 128 * i));
        return ZK_OK;
    };
    if (md_is_composite(pk_handle)) return row_by_row();  // a key spread over several device entries: its own prover, row by row
    ZK_ON_ENTRY_OF(pk_handle);
    Groth16BatchView V;
    ZK_TRY(groth16_pk_batch_view(pk_handle, &V));
    const size_t N = (size_t)1 << V.log_domain;
    if (n_wires != V.n_wires) return set_err(ZK_ERR_LEN, "len(w) = %zu != %zu wires of the proving key", n_wires, V.n_wires);
    if (n_constraints > N) return set_err(ZK_ERR_ARG, "n_constraints = %zu exceeds the domain size %zu", n_constraints, N);
    // Dispatch.  Batched: a single-device key WITH its window tables, whole (not window- or range-sharded), log_domain <= 16, at least two rows -- the shapes where
    // one proof is launch chains and reduction tails and S rows share them (batch_serves above says why each condition is there; DESIGN.md 3.12 has the measured
    // table the domain bound comes from).  Everything else -- composite keys above, keys without tables, sharded keys, larger domains, a single row -- runs the rows
    // one after the other through the single prover, which at those shapes fills the machine by itself.
    if (n_proofs < 2 || !batch_serves(V)) return row_by_row();
    size_t chunk = 1;
    ZK_TRY(batch_chunk_rows(V, &chunk));
    SlotsGuard<5> g;  // one slot group for the whole call
    ZK_TRY(acquire_slots(5, g.s));
    for (size_t first = 0; first < n_proofs; first += chunk)
        ZK_TRY(prove_chunk(pk_handle, V, g.s, in, first, std::min(chunk, n_proofs - first), proofs_out));
    return ZK_OK;
}

// groth16.Prove from the witnesses: a, b, c = L w, R w, O w for all rows of a chunk in one launch, then zk_bn254_groth16_prove_batch on resident data
int zk_bn254_groth16_prove_r1cs_batch(uint64_t r1cs_handle, uint64_t pk_handle, const void* w, size_t n_wires, const zk_fr* r, const zk_fr* s, size_t n_proofs, int on_device,
                                      uint8_t* proofs_out) {
    if (n_proofs == 0) return ZK_OK;
    if (!w || !r || !s || !proofs_out) return set_err(ZK_ERR_ARG, "null pointer");
    ZK_ON_ENTRY_OF(r1cs_handle);
    size_t nc = 0, nw = 0;
    ZK_TRY(r1cs_dims(r1cs_handle, &nc, &nw));
    if (n_wires != nw) return set_err(ZK_ERR_LEN, "len(w) = %zu != %zu wires of the constraint system", n_wires, nw);
    // rows per step: what keeps a, b, c and the staged w under a quarter of the batch workspace
    const size_t per_row = (3 * nc + nw) * 32 + 1;
    const size_t step = std::max<size_t>(1, std::min<size_t>(n_proofs, std::min<size_t>(4 * BATCH_MAX_ROWS, BATCH_WORKSPACE / 4 / per_row)));
    void *d_w = nullptr, *d_abc = nullptr;
    struct Free { void** p[2]; ~Free() { for (auto q : p) if (*q) (void)hipFree(*q); } } guard{{&d_w, &d_abc}};
    ZK_HIP(hipMalloc(&d_abc, (nc ? 3 * step * nc : 1) * 32));
    if (!on_device) ZK_HIP(hipMalloc(&d_w, (nw ? step * nw : 1) * 32));
    Fr* abc = (Fr*)d_abc;
    for (size_t first = 0; first < n_proofs; first += step) {
        const size_t R = std::min(step, n_proofs - first);
        const Fr* dw = (const Fr*)((const char*)w + first * nw * 32);
        {
            SlotGuard g;  // given back before the prover asks for its five
            ZK_TRY(acquire_slot(&g.s));
            hipStream_t st = g.s->stream;
            if (!on_device) {
                ZK_HIP(hipMemcpyAsync(d_w, dw, R * nw * 32, hipMemcpyHostToDevice, st));
                dw = (const Fr*)d_w;
            }
            ZK_TRY(r1cs_eval_abc_rows(r1cs_handle, g.s, st, dw, R, nc, abc, abc + R * nc, abc + 2 * R * nc));
            ZK_TRY(slot_sync(g.s, st));
        }
        ZK_TRY(zk_bn254_groth16_prove_batch(pk_handle, abc, abc + R * nc, abc + 2 * R * nc, nc, dw, nw, r + first, s + first, R, 1, proofs_out + 128 * first));
    }
    return ZK_OK;
}

}  // extern "C"
