// Internal interface between the batch Groth16 prover (groth16_batch.hip) and the modules that own the resident objects it reads.
#pragma once
#include "ctx.hpp"
#include "curve.hpp"
#include "ff.hpp"
#include "msm.hpp"

namespace zkmi {

// a loaded proving key as the batch prover sees it (groth16.hip); the table pointers stay the key's
struct Groth16BatchView {
    uint32_t log_domain;
    size_t n_wires, n_public, nz;
    bool tables;
    MsmTable tab_w, tab_h;
    const void *t_a, *t_b, *t_k, *t_z, *t_b2;
};
int groth16_pk_batch_view(uint64_t handle, Groth16BatchView* v);

// what the device tail (groth16_tail.hip) needs of a key: alpha, beta, beta2 and the 8-bit window tables of delta / delta2 in HBM ([w * 255 + d - 1] =
// d * 2^(8w) * P, affine).  The tables are built at the key's first device tail (once, whichever thread comes first), stay the key's and are freed with it.
struct Groth16TailView {
    Affine<Fp> alpha, beta;
    Affine<Fp2> beta2;
    const void *t_delta, *t_delta2;
};
int groth16_pk_tail_view(uint64_t handle, Groth16TailView* v);
// the tail of `n` rows in one launch on `st` (device pointers; inputs only read; no workspace)
int groth16_tail_rows(Slot* sl, hipStream_t st, const Groth16TailView& V, const void* d_partials, size_t n_partials, const void* d_r, const void* d_s, size_t n,
                      void* d_proofs_out);

// r1cs.hip: the dimensions of a resident constraint system, and a, b, c = L w, R w, O w for `rows` wire vectors in one launch -- row i reads d_w + i * n_wires
// and writes n_constraints elements at d_a / d_b / d_c + i * out_stride
int r1cs_dims(uint64_t handle, size_t* n_constraints, size_t* n_wires);
int r1cs_eval_abc_rows(uint64_t handle, Slot* s, hipStream_t st, const Fr* d_w, size_t rows, size_t out_stride, Fr* d_a, Fr* d_b, Fr* d_c);

}  // namespace zkmi
