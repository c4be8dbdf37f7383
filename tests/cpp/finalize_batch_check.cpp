// groth16::FinalizeBatch of include/zkmi.hpp compiles against the C ABI, and what it can refuse without a device it refuses before one is touched.
#include <stdio.h>

#include "zkmi.hpp"

using namespace zkmi;

#define EXPECT(cond)                                                  \
    do {                                                              \
        if (!(cond)) {                                                \
            printf("FAILED %s (line %d)\n", #cond, __LINE__);         \
            return 1;                                                 \
        }                                                             \
    } while (0)

int main() {
    groth16::ProvingKey pk;  // never loaded: handle 0
    std::vector<groth16::Proof> proofs;
    fr::Vector r(2), s(2), s3(3), none;
    std::vector<uint64_t> parts(2 * 3 * 96), short_parts(2 * 96);
    EXPECT(groth16::FinalizeBatch(pk, parts, 3, r, s3, &proofs).code == ZK_ERR_LEN);
    EXPECT(groth16::FinalizeBatch(pk, parts, 0, r, s, &proofs).code == ZK_ERR_ARG);
    EXPECT(groth16::FinalizeBatch(pk, short_parts, 3, r, s, &proofs).code == ZK_ERR_LEN);
    // no rows: nothing to do, whatever the key
    EXPECT(groth16::FinalizeBatch(pk, std::vector<uint64_t>(), 3, none, none, &proofs).ok() && proofs.empty());
    // the C entries: null pointers and n_partials == 0 are argument errors before anything else is looked at
    uint8_t out[256];
    EXPECT(zk_bn254_groth16_finalize_batch(0, nullptr, 3, r.data(), s.data(), 2, out) == ZK_ERR_ARG);
    EXPECT(zk_bn254_groth16_finalize_batch(0, parts.data(), 0, r.data(), s.data(), 2, out) == ZK_ERR_ARG);
    EXPECT(zk_bn254_groth16_finalize_batch(0, parts.data(), 3, nullptr, s.data(), 2, out) == ZK_ERR_ARG);
    EXPECT(zk_bn254_groth16_finalize_batch(0, parts.data(), 3, r.data(), nullptr, 2, out) == ZK_ERR_ARG);
    EXPECT(zk_bn254_groth16_finalize_batch(0, parts.data(), 3, r.data(), s.data(), 2, nullptr) == ZK_ERR_ARG);
    EXPECT(zk_bn254_groth16_finalize_batch_dev(0, nullptr, 3, r.data(), s.data(), 2, out, nullptr) == ZK_ERR_ARG);
    EXPECT(zk_bn254_groth16_finalize_batch_dev(0, parts.data(), 0, r.data(), s.data(), 2, out, nullptr) == ZK_ERR_ARG);
    EXPECT(zk_bn254_groth16_finalize_batch(0, nullptr, 0, nullptr, nullptr, 0, nullptr) == ZK_OK);
    EXPECT(zk_bn254_groth16_finalize_batch_dev(0, nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr) == ZK_OK);
    printf("ok\n");
    return 0;
}
