// The arithmetic of the Groth16 proof tail, one row at a time, host + device: groth16_tail.hip's kernel is these functions plus the exchange of a row's
// intermediate points between its four lanes; tests/cpp/tail_math_check.cpp runs the same functions on the host against the pure-python expectations.
#pragma once
#include "curve.hpp"
#include "ff.hpp"

namespace zkmi {

struct TailKey {
    Affine<Fp> alpha, beta;
    Affine<Fp2> beta2;
    const Affine<Fp>* t_delta;    // [w * 255 + d - 1] = d * 2^(8w) * delta
    const Affine<Fp2>* t_delta2;
};
// sum over a row's records of the point at limb offset `off` (a record with zz == 0 is the point at infinity whatever its x and y hold: XYZZ::add)
template <class F>
ZK_HD XYZZ<F> tail_sum(const uint64_t* __restrict__ rec, size_t n_partials, int off) {
    XYZZ<F> acc = XYZZ<F>::inf();
#pragma unroll 1
    for (size_t j = 0; j < n_partials; j++) acc.add(*reinterpret_cast<const XYZZ<F>*>(rec + 96 * j + off));
    return acc;
}
// the scalar stays in registers under constant indices: the next bit / byte is taken at one end and the value shifted
ZK_HD uint32_t take_top_bit(Fr& k) {
    const uint32_t b = k.l[7] >> 31;
#pragma unroll
    for (int i = 7; i > 0; i--) k.l[i] = (k.l[i] << 1) | (k.l[i - 1] >> 31);
    k.l[0] <<= 1;
    return b;
}
ZK_HD uint32_t take_low_byte(Fr& k) {
    const uint32_t d = k.l[0] & 255u;
#pragma unroll
    for (int i = 0; i < 7; i++) k.l[i] = (k.l[i] >> 8) | (k.l[i + 1] << 24);
    k.l[7] >>= 8;
    return d;
}

// k * m for a Montgomery scalar k: double-and-add, most significant bit first (m at infinity: add returns at once, the product stays at infinity)
ZK_HD XYZZ<Fp> tail_scaled(const XYZZ<Fp>& m, const Fr& k_mont) {
    Fr k = k_mont.from_mont();
    XYZZ<Fp> acc = XYZZ<Fp>::inf();
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int i = 0; i < 256; i++) {
        acc.dbl();
        if (take_top_bit(k)) acc.add(m);
    }
    return acc;
}
// acc += k * P for a CANONICAL scalar k through P's 8-bit window table
template <class F>
ZK_HD void tail_fixed_add(XYZZ<F>& acc, const Affine<F>* __restrict__ table, Fr k) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int w = 0; w < 32; w++) {
        const uint32_t d = take_low_byte(k);
        if (d) {
            const Affine<F> t = table[w * 255 + (d - 1)];
            acc.madd(t.x, t.y);
        }
    }
}
// the three proof elements, affine, with ONE inversion: 1 / (zz * zzz) of the three points by Montgomery's trick, the Fp2 value through its norm (never zero
// for a non-zero element); a point at infinity is skipped
ZK_HD void tail_to_affine(const XYZZ<Fp>& ar, const XYZZ<Fp2>& bs, const XYZZ<Fp>& krs, Affine<Fp>* a_ar, Affine<Fp2>* a_bs, Affine<Fp>* a_krs) {
    const bool i1 = ar.is_inf(), i2 = krs.is_inf(), i3 = bs.is_inf();
    const Fp d1 = ar.zz * ar.zzz, d2 = krs.zz * krs.zzz;
    const Fp2 d3 = bs.zz * bs.zzz;
    const Fp n3 = d3.a0.sqr() + d3.a1.sqr();
    Fp run = i1 ? Fp::one() : d1;
    const Fp pre2 = run;
    if (!i2) run = run * d2;
    const Fp pre3 = run;
    if (!i3) run = run * n3;
    Fp inv = run.inv();
    const Fp z3 = inv * pre3;
    if (!i3) inv = inv * n3;
    const Fp z2 = inv * pre2;
    if (!i2) inv = inv * d2;
    const Fp z1 = inv;
    *a_ar = Affine<Fp>::inf();
    *a_krs = Affine<Fp>::inf();
    *a_bs = Affine<Fp2>::inf();
    if (!i1) *a_ar = Affine<Fp>{ar.x * (z1 * ar.zzz), ar.y * (z1 * ar.zz)};
    if (!i2) *a_krs = Affine<Fp>{krs.x * (z2 * krs.zzz), krs.y * (z2 * krs.zz)};
    if (!i3) {
        const Fp2 zi{d3.a0 * z3, (d3.a1 * z3).neg()};
        *a_bs = Affine<Fp2>{bs.x * (zi * bs.zzz), bs.y * (zi * bs.zz)};
    }
}

}  // namespace zkmi
