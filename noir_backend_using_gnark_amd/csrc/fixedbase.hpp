// Fixed-base scalar multiplication by the group generators (util.hip): [k_i] G1 / [k_i] G2 for many scalars -- kzg.NewSRS, groth16.Setup, synthetic bases.
#pragma once
#include "ctx.hpp"
#include "curve.hpp"

namespace zkmi {

// out[i] = [scalars[i]] G1 (is_g2 = 0, 64-byte affine points) or G2 (128-byte); scalars: Montgomery fr.Elements in HBM
int fixed_base_mul_scalars(Slot* s, hipStream_t st, int is_g2, const Fr* d_scalars, size_t n, void* d_out);
// the 8-bit window table of an arbitrary base point, built on the host and left in HBM (hipMalloc; the caller's to free): 32 x 255 affine points,
// [w * 255 + d - 1] = d * 2^(8w) * base.  The base must not be the point at infinity.
int fixed_base_table_g1(const Affine<Fp>& base, Affine<Fp>** d_out);
int fixed_base_table_g2(const Affine<Fp2>& base, Affine<Fp2>** d_out);
static constexpr size_t FIXED_BASE_TABLE_POINTS = 32 * 255;
Affine<Fp> generator_g1();
Affine<Fp2> generator_g2();

}  // namespace zkmi
