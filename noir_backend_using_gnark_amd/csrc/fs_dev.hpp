// Device pieces of the Fiat-Shamir transcript (gnark-crypto fiatshamir.Transcript over SHA-256) shared by the batch PLONK verifier (verify_batch.hip) and the
// batch PLONK prover (plonk_batch.hip): how a digest becomes a challenge and how a point is bound.
#pragma once
#include "curve.hpp"
#include "ff.hpp"
#include "sha256_dev.hpp"

namespace zkmi {

// a digest as fr.SetBytes reads it
ZK_D Fr fr_from_digest(const uint32_t d[8]) {
    uint32_t t[8];
    sha_words_to_limbs(d, t);
    Fr r = Fr::reduce_once(t);
#pragma unroll
    for (int k = 0; k < 4; k++) r = Fr::reduce_once(r.l);
    return r.to_mont();
}
// one 32-byte half of G1Affine.RawBytes() (X || Y big-endian; infinity = 0x40 then zeros) as limbs
ZK_D void raw_half(const Affine<Fp>& p, int half, uint32_t l[8]) {
    Fp c = p.x;
    if (half) c = p.y;
    c = c.from_mont();
#pragma unroll
    for (int k = 0; k < 8; k++) l[k] = c.l[k];
    if (!half && p.is_inf()) l[7] = 0x40000000u;
}

}  // namespace zkmi
