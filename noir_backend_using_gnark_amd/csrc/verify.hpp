// Host pieces of the verifiers (verify.hip) that the batch verifier (verify_batch.hip) shares.
#pragma once
#include <vector>

#include "ctx.hpp"
#include "curve.hpp"
#include "host_ff.hpp"

namespace zkmi {

// a Groth16 VerifyingKey.WriteTo image, decoded ([beta]1 and [delta]1 are read and validated, not used by Verify)
struct Groth16Vk {
    std::vector<uint8_t> bytes;  // the binary image (hex text decoded)
    Affine<HFp> alpha, beta1, delta1;
    Affine<HFp2> beta, gamma, delta;
    std::vector<Affine<HFp>> K;
};
// ZK_ERR_ARG / ZK_ERR_LEN (with the error text set) on a malformed key, exactly as zk_bn254_groth16_verify reports it
int groth16_vk_parse(const void* vk, size_t vk_len, int vk_is_hex, Groth16Vk* out);

// a PLONK VerifyingKey.WriteTo image (368 bytes), decoded
struct PlonkVk {
    std::vector<uint8_t> bytes;  // the binary image (hex text decoded)
    uint64_t n, npub;            // domain size (a power of two <= 2^28), NbPublicVariables
    HFr size_inv, gen, u;        // SizeInv, Generator, CosetShift (reduced mod r, as fr.SetBytes)
    Affine<HFp> pts[8];          // S1, S2, S3, Ql, Qr, Qm, Qo, Qk
};
// ZK_ERR_ARG / ZK_ERR_LEN (with the error text set) on a malformed key, exactly as zk_bn254_plonk_verify reports it
int plonk_vk_parse(const void* vk, size_t vk_len, int vk_is_hex, PlonkVk* out);

}  // namespace zkmi
