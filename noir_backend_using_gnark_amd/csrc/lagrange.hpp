// The KZG SRS in Lagrange form over a domain (lagrange.hip): what lets plonk.Prove commit l, r, o from wire values instead of coefficients.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace zkmi {
// With a trace (inspection, tests: zk_bn254_lagrange_inspect) the stream is synchronised after the scale-in launch, after every stage launch and after the finish,
// and the work array -- which every stage overwrites in place -- is copied each time: work[0] after the scale-in, work[k] after the k-th stage (m = n / 2^k), n raw
// XYZZ points of 16 words each; out: the n + 2 affine points of the finish, 8 words each.  Without one nothing is added but the test of the pointer.
struct LagTrace {
    std::vector<std::vector<uint64_t>> work;
    std::vector<uint64_t> out;
};
// d_srs: at least 2^logn + 2 affine G1 points [tau^j] in HBM -> *handle: 2^logn + 2 registered bases: [L_i(tau)] for i < n, then [tau^n - 1], [tau^(n+1) - tau]
int lagrange_srs_build(const void* d_srs, size_t srs_n, unsigned logn, uint64_t* handle, LagTrace* trace = nullptr);
}  // namespace zkmi
