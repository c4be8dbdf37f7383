// Internal interface between the PLONK prover (plonk.hip: the resident key and the row forms of rounds 2 to 5) and the batch prover (plonk_batch.hip), as
// groth16_batch.hpp stands between groth16.hip and groth16_batch.hip.
#pragma once
#include <map>
#include <memory>
#include <mutex>
#include <shared_mutex>
#include <vector>

#include "ctx.hpp"
#include "curve.hpp"
#include "ff.hpp"
#include "host_ff.hpp"
#include "ntt.hpp"
#include "scan.hpp"

namespace zkmi {

// ------------------------------------------------------------------------------------------------ resident key
struct PlonkPK {
    unsigned logn = 0, logN4 = 0, log_rho = 0;
    size_t n = 0, N4 = 0, n_public = 0, n_constraints = 0, n_vars = 0;
    uint64_t srs = 0;
    uint64_t lag_srs = 0;  // the SRS in Lagrange form over this key's domain + the two points of the blinding (lagrange.hip; zk_bn254_plonk_pk_lagrange_srs), or 0
    HFr gen, u, card_inv;
    // canonical (regular) polynomials of the key, n each, and LQk (Lagrange)
    Fr *ql = nullptr, *qr = nullptr, *qm = nullptr, *qo = nullptr, *cqk = nullptr, *lqk = nullptr, *s1 = nullptr, *s2 = nullptr, *s3 = nullptr;
    uint32_t* perm = nullptr;  // pk.Permutation (3n), kept for ProvingKey.WriteTo
    Fr* sig = nullptr;      // S1 | S2 | S3 in Lagrange form (3n): what BuildRatioCopyConstraint reads through pk.Permutation
    Fr* e_cqk = nullptr;    // CQk (qk WITHOUT the public inputs) as LagrangeCoset on the big domain: per proof only the public inputs' share is added (k_qk_coset)
    Fr* e[9] = {};          // ql, qr, qm, qo, s1, s2, s3, L1, id as LagrangeCoset on the big domain, bit-reversed layout (gnark caches the first 7)
    uint32_t *xa = nullptr, *xb = nullptr, *xc = nullptr;
    Affine<HFp> vk_s[3], vk_ql, vk_qr, vk_qm, vk_qo, vk_qk;
    // the verifying-key digests are known to be the commitments of THIS key's polynomials under ITS SRS (Setup computed them, or a proof has confirmed it):
    // the digest of the linearised polynomial may then be taken by linearity (seven scalar multiplications on the host) instead of an n-point MSM
    bool vk_consistent = false;
    // per-proof workspace (one proof at a time per key)
    Fr *w_big[5] = {}, *w_small = nullptr;
    std::shared_ptr<std::mutex> mu;
    // held shared by a call that only READS the key's tables and brings its own workspace (zk_bn254_plonk_quotient_batch_dev): such calls overlap each other and
    // a proof in flight; zk_bn254_plonk_pk_free takes it exclusively before the key is destroyed
    std::shared_ptr<std::shared_mutex> live;
    std::vector<void*> allocs;
    size_t bytes = 0;  // HBM held by the key
};

static const zk_msm_cfg kMont = {0, 1, 0, 0};

static inline unsigned grid_of(size_t n) { return (unsigned)((n + 255) / 256); }

static inline bool spans_overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
    const char *a0 = (const char*)a, *b0 = (const char*)b;
    return a_bytes && b_bytes && a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}
static inline size_t rows_span(size_t rows, size_t stride, size_t n) { return rows ? ((rows - 1) * stride + n) * sizeof(Fr) : 0; }

// a key that is not being freed, kept alive by `alive` (zk_bn254_plonk_quotient_batch_dev says why the shared lock is granted at once)
int live_key(uint64_t handle, PlonkPK** P, std::shared_ptr<std::shared_mutex>* live, std::shared_lock<std::shared_mutex>* alive);

// ------------------------------------------------------------------------------------------------ the row forms of rounds 2 to 5 (plonk.hip says what each does)
constexpr size_t RATIO_GRID_ROWS = 65535;
struct RatioWs {
    uint32_t K = 0, nb = 0;
    size_t chunk = 0;    // rows per group of launches
    bool single = false; // the one-row form: `one` is the prover's scan plan
    Fr *num = nullptr, *den = nullptr, *scr = nullptr, *t = nullptr, *b = nullptr;
    ScanBufs one;
};
size_t ratio_row_bytes(size_t n);
size_t ratio_ws_bytes(size_t n, size_t chunk, bool single);
int ratio_ws_take(Slot* s, size_t n, size_t chunk, bool single, RatioWs* W);
int ratio_rows_dev(Slot* s, hipStream_t st, const Domain* d0, const Fr* sig, const Fr* l, const Fr* r, const Fr* o, size_t in_stride, size_t rows,
                   const Fr* d_beta, const Fr* d_gamma, Fr* z, size_t out_stride, const RatioWs& W);
size_t quot_row_bytes(const PlonkPK* P);
int quotient_rows_dev(Slot* s, hipStream_t st, const PlonkPK* P, const Fr* l, const Fr* r, const Fr* o, const Fr* z, size_t in_stride, const Fr* pub,
                      size_t pub_stride, size_t rows, const Fr* d_alpha, const Fr* d_beta, const Fr* d_gamma, Fr* h, size_t out_stride, int* status, Fr* ws,
                      size_t chunk);
constexpr uint32_t LIN_PT = 8;
size_t open_row_bytes(size_t len, unsigned npoly, size_t pt, size_t fold);
int linearize_rows_dev(Slot* s, hipStream_t st, const PlonkPK* P, const Fr* l, const Fr* r, const Fr* o, const Fr* z, size_t in_stride, const Fr* h,
                       size_t h_stride, size_t rows, const Fr* d_alpha, const Fr* d_beta, const Fr* d_gamma, const Fr* d_zeta, Fr* values, Fr* zquot, Fr* lin,
                       Fr* fh, size_t out_stride);
int open_rows_dev(Slot* s, hipStream_t st, const PlonkPK* P, const Fr* fh, const Fr* lin, const Fr* l, const Fr* r, const Fr* o, size_t in_stride, size_t rows,
                  const Fr* d_zeta, const Fr* d_kg, Fr* q, size_t out_stride, Fr* value);

}  // namespace zkmi
