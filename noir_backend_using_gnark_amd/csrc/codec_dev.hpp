// The key / point codecs one element at a time: hex digits, 32-byte big-endian field elements, G1 / G2 compression and decompression (with their
// square roots on the 29-bit multiplier) and the G2 r-torsion test.  keyio.hip's kernels are an index check around one of these functions each;
// probe.hip (the test-only libzkmi_probe.so) runs the same functions on one test vector per lane.  Encodings: see the head of keyio.hip.
#pragma once
#include <string.h>

#include "curve.hpp"
#include "ff.hpp"
#include "ff29.hpp"
#include "host_ff.hpp"

namespace zkmi {

// ---- hex
__device__ __forceinline__ uint32_t hexdig4(uint32_t w, uint32_t* bad) {  // 4 characters -> 2 bytes (text order, low byte first); see wire.hip hex4
    uint32_t nib = (w & 0x0f0f0f0fu) + ((w >> 6) & 0x01010101u) * 9u;
    uint32_t gt9 = ((nib + 0x06060606u) >> 4) & 0x01010101u;
    uint32_t enc = nib + 0x30303030u + gt9 * 0x27u;
    *bad |= (enc ^ (w | ((w >> 1) & 0x20202020u))) | (nib & 0xf0f0f0f0u);
    uint32_t b = ((nib << 4) | (nib >> 8)) & 0x00ff00ffu;
    return (b & 0xffu) | ((b >> 8) & 0xff00u);
}
__device__ __forceinline__ uint32_t hexenc2w(uint32_t b16) {
    uint32_t nib = ((b16 >> 4) & 0x0fu) | ((b16 & 0x0fu) << 8) | (((b16 >> 12) & 0x0fu) << 16) | (((b16 >> 8) & 0x0fu) << 24);
    uint32_t gt9 = ((nib + 0x06060606u) >> 4) & 0x01010101u;
    return nib + 0x30303030u + gt9 * 0x27u;
}

// ---- 32-byte big-endian integers <-> 8 little-endian limbs, through 4-byte loads (the vectors inside a key sit at any 4-byte offset)
template <class F>
__device__ __forceinline__ F load_be32(const uint32_t* p) {
    F x;
#pragma unroll
    for (int k = 0; k < 8; k++) x.l[7 - k] = __builtin_bswap32(p[k]);
    return x;
}
template <class F>
__device__ __forceinline__ void store_be32(uint32_t* p, const F& x) {
#pragma unroll
    for (int k = 0; k < 8; k++) p[k] = __builtin_bswap32(x.l[7 - k]);
}
template <class P>
__device__ __forceinline__ bool geq_mod(const uint32_t x[8]) {
    for (int i = 7; i >= 0; i--)
        if (x[i] != P::MOD[i]) return x[i] > P::MOD[i];
    return true;
}
// false (and *out untouched) on a value >= r: gnark-crypto's "invalid fr.Element encoding"
__device__ __forceinline__ bool fr_from_be_one(const uint32_t raw[8], Fr* out) {
    Fr x = load_be32<Fr>(raw);
    if (geq_mod<FrParams>(x.l)) return false;
    *out = x.to_mont();
    return true;
}
__device__ __forceinline__ void fr_to_be_one(const Fr& in, uint32_t raw[8]) { store_be32(raw, in.from_mont()); }

// ---- square roots: a^((q - 3) / 4) on the 29-bit multiplier (ff29.hpp)
// Both decompressions end in this exponentiation (q = 3 mod 4: sqrt(a) = a^((q+1)/4) = a^((q-3)/4) * a; the Fp2 root takes two).  The saturated
// Field::pow spends 252 squarings + 127 products of ~305 instructions; here the constant exponent is walked in sliding windows of three bits -- 250 squarings
// of ~170 instructions and 55 products of 206 with a, a^3, a^5, a^7 -- 2.1 x fewer instructions.  One byte per window: squarings << 2 | (odd power >> 1),
// most significant window first (the first one only selects the starting power); every value in the chain is a direct product output (< 1.03 p).
__device__ __forceinline__ U29 u29_pow_qm3_4(const U29& a) {
    static const uint8_t W[56] = {9,  29, 12, 16, 23, 23, 22, 9,  20, 17, 21, 8,  42, 17, 19, 30, 24, 26, 14, 14, 14, 33, 38, 13, 30, 9,  13, 22,
                                  15, 38, 14, 18, 12, 26, 14, 31, 27, 22, 8,  21, 8,  23, 4,  20, 24, 21, 34, 14, 14, 4,  31, 9,  23, 15, 18, 16};
    const U29 a2 = u29_sqr(a), a3 = u29_mul(a2, a), a5 = u29_mul(a3, a2), a7 = u29_mul(a5, a2);
    U29 acc = a3;  // W[0] & 3 == 1
#pragma unroll 1
    for (int k = 1; k < 56; k++) {
        const unsigned w = W[k];
#pragma unroll 1
        for (unsigned j = 0; j < (w >> 2); j++) acc = u29_sqr(acc);
        switch (w & 3u) {
            case 0: acc = u29_mul(acc, a); break;
            case 1: acc = u29_mul(acc, a3); break;
            case 2: acc = u29_mul(acc, a5); break;
            default: acc = u29_mul(acc, a7); break;
        }
    }
    return acc;
}
// canonical Montgomery image -> a^((q-3)/4) * a^mul_a as a canonical Montgomery image (mul_a: once more by a, the square-root candidate)
__device__ __forceinline__ Fp fp_pow_qm3_4(const Fp& a, bool times_a) {
    const U29 x = u29_mul(u29_load(a), u29_one());  // contracted: < 1.2 p
    U29 e = u29_pow_qm3_4(x);
    if (times_a) e = u29_mul(e, x);
    return u29_store(e);
}

// ---- G1 points
__device__ __forceinline__ bool fp_lex_largest_dev(const Fp& canonical) {  // value > (q - 1) / 2
    for (int i = 7; i >= 0; i--) {
        uint32_t h = (FpParams::MOD[i] >> 1) | (i < 7 ? FpParams::MOD[i + 1] << 31 : 0);
        if (canonical.l[i] != h) return canonical.l[i] > h;
    }
    return false;
}
// G1Affine.SetBytes on a compressed encoding: y = sqrt(x^3 + 3) = (x^3 + 3)^((q + 1) / 4)  (q = 3 mod 4), sign by the flag.
// false on an invalid encoding (an infinity flag with a payload, an uncompressed encoding inside a compressed slice, x >= q, x not on the curve);
// *out is then the point at infinity.  `reject` runs on each of those paths before *out is written: a kernel flags the element there (status word, bad byte),
// so the flagging stays where it was when this was the kernel's body; a caller that only wants the verdict passes NoReject
struct NoReject { __device__ __forceinline__ void operator()() const {} };
template <class Reject>
__device__ __forceinline__ bool g1_decompress_one(const uint32_t raw[8], Affine<Fp>* out, const Reject& reject) {
    Fp x = load_be32<Fp>(raw);
    const uint32_t flag = x.l[7] >> 30;
    x.l[7] &= 0x3fffffffu;
    Affine<Fp> p = Affine<Fp>::inf();
    if (flag == 1) {  // infinity: the rest must be zero
        const bool ok = x.is_zero();
        if (!ok) reject();
        *out = p;
        return ok;
    }
    if (flag == 0 || geq_mod<FpParams>(x.l)) {  // an uncompressed encoding inside a compressed slice / x >= q
        reject();
        *out = p;
        return false;
    }
    Fp xm = x.to_mont();
    Fp three = Fp::one() + Fp::one() + Fp::one();
    Fp rhs = xm.sqr() * xm + three;
    Fp y = fp_pow_qm3_4(rhs, true);  // rhs^((q + 1) / 4)
    if (y.sqr() != rhs) {  // not on the curve
        reject();
        *out = p;
        return false;
    }
    if (fp_lex_largest_dev(y.from_mont()) != (flag == 3)) y = Fp::zero() - y;
    p.x = xm;
    p.y = y;
    *out = p;
    return true;
}
__device__ __forceinline__ void g1_compress_one(const Affine<Fp>& p, uint32_t raw[8]) {
    Fp x = Fp::zero();
    uint32_t flag = 1;
    if (!p.is_inf()) {
        x = p.x.from_mont();
        flag = fp_lex_largest_dev(p.y.from_mont()) ? 3 : 2;
    }
    x.l[7] |= flag << 30;
    store_be32(raw, x);
}

// ---- G2 points on the device (a Groth16 proving key holds one per wire)
// Square root in Fp2 = Fp[u]/(u^2 + 1), q = 3 mod 4, by the complex method -- two exponentiations in Fp instead of the two in Fp2 of rounds 2-4 (Adj &
// Rodriguez-Henriquez, Alg. 9: 1,778 base-field products per root; this: ~770).  For a = a0 + a1 u with a1 != 0: the norm n = a0^2 + a1^2 is a square in Fp
// exactly when a is one in Fp2; with s^2 = n and t = (a0 + s) / 2, one exponentiation e = t^((q-3)/4) gives c = e t with c^2 = chi t (chi = +-1 the quadratic
// character of t) AND 1 / c = c e^2 -- no inversion --, and the root is (c, a1 / 2c) if chi = 1, (a1 / 2c, c) otherwise (then c^2 = -t = -(a0 + s) / 2 and
// (a1 / 2c)^2 = (a0 - s) / 2).  Either root will do: the caller picks the sign by the encoding's flag.  `half` = 1 / 2 (Montgomery).
__device__ inline bool f2_sqrt_dev(const Fp2& a, const Fp& half, Fp2* out) {
    if (a.is_zero()) { *out = a; return true; }
    // every exponentiation below is by (q - 3) / 4: fp_pow_qm3_4
    if (a.a1.is_zero()) {  // a in Fp: sqrt(a0) or u sqrt(-a0)
        const Fp c = fp_pow_qm3_4(a.a0, true);
        if (c.sqr() == a.a0) *out = Fp2{c, Fp::zero()};
        else *out = Fp2{Fp::zero(), c};
        return out->sqr() == a;
    }
    const Fp n = a.a0.sqr() + a.a1.sqr();
    const Fp s = fp_pow_qm3_4(n, true);
    if (s.sqr() != n) return false;  // the norm is not a square: neither is a
    Fp t = (a.a0 + s) * half;
    // (t = 0 would need a0 = -s, i.e. a1^2 = s^2 - a0^2 = 0: not on this branch)
    const Fp e = fp_pow_qm3_4(t, false), c = e * t;
    const Fp w = a.a1 * (c * e.sqr() * half);  // a1 / (2 c)
    if (c.sqr() == t) *out = Fp2{c, w};
    else *out = Fp2{w, c};
    return out->sqr() == a;
}
__device__ __forceinline__ bool f2_lex_largest_dev(const Fp2& y) {  // gnark-crypto: compares A1 first, A0 when A1 = 0
    return y.a1.is_zero() ? fp_lex_largest_dev(y.a0.from_mont()) : fp_lex_largest_dev(y.a1.from_mont());
}
// G2Affine.SetBytes on a compressed encoding (X.A1 | X.A0 big-endian, flags on the first byte) with the subgroup check the gnark-crypto Decoder
// applies by default (r * P = infinity: the twist has a cofactor).  bt = 3 / (9 + u), Montgomery.
// r-torsion membership on the twist, with the untwist-Frobenius-twist endomorphism psi: (x, y) -> (conj(x) * gx, conj(y) * gy), gx = xi^((q-1)/3),
// gy = xi^((q-1)/2), xi = 9 + u, which acts on G2 as multiplication by q = 6 x0^2 (mod r); x0 = 4965661367192848881.  Two exact tests (both accept exactly
// the points r * P = infinity accepts; tests/codec_edges.py holds twist points outside G2, cofactor-torsion points of small and of full order and G2 points
// shifted by them):
//   psi(P) == [6 x0^2] P                                       127 doublings + 64 additions     (rounds 2-4)
//   [x0 + 1] P + psi([x0] P) + psi^2([x0] P) == psi^3([2 x0] P)  63 doublings + 27 + 4 additions  (eprint 2022/348 sec. 5.1 for BN curves; gnark-crypto's
//                                                               G2Jac.IsInSubGroup): ONE multiplication by the 63-bit x0, three psi, a few additions -- half
//                                                               the work of a decompression's larger half (68 -> see DESIGN.md 3.8 per 2^20 points)
struct PsiConsts { Fp2 gx, gy; Fp half; };  // psi's two coefficients; 1 / 2 for the square root
// The second test runs on the 29-bit multiplier (ff29.hpp: acc29g2_dbl / acc29g2_add, whose class invariant -- every coordinate component < 32 p, weakly
// normalised, in and out -- tools/u29_model.py proves): 63 doublings and 27 + 3 full additions with one reduction per output component instead of three saturated
// products per Fp2 product (29.5-30.5 ms per 2^20 points against 33.4-34.2 for the saturated form in the same kernel: profiles/rnd5_v_g2_subgroup_variants.txt).
// psi keeps the invariant: X and Y times a contracted constant come out below 1.5 p; the conjugated ZZ / ZZZ components are contracted.
__device__ __forceinline__ Acc29G2 g2_psi_dev29(const Acc29G2& t, const U29x2& gx, const U29x2& gy) {
    if (t.inf) return t;
    const U29 one = u29_one();
    Acc29G2 r;
    r.inf = false;
    // conj(v) * g = (v0 g0 + v1 g1) + (v0 g1 - v1 g0) u
    r.x = U29x2{u29_mul2(t.x.c0, gx.c0, t.x.c1, gx.c1), u29_mul2(t.x.c0, gx.c1, u29_neg<32>(t.x.c1), gx.c0)};
    r.y = U29x2{u29_mul2(t.y.c0, gy.c0, t.y.c1, gy.c1), u29_mul2(t.y.c0, gy.c1, u29_neg<32>(t.y.c1), gy.c0)};
    r.zz = U29x2{t.zz.c0, u29_mul(u29_neg<32>(t.zz.c1), one)};
    r.zzz = U29x2{t.zzz.c0, u29_mul(u29_neg<32>(t.zzz.c1), one)};
    return r;
}
__device__ __forceinline__ bool f2_eq29(const U29x2& a, const U29x2& b) {  // exact: through the canonical images
    const Fp2 x = f2_store29(a), y = f2_store29(b);
    return x == y;
}
// *pp is read again wherever P is added (28 times: 128 bytes from L2) instead of being held in 72 registers next to the accumulator and an addition's temporaries
__device__ __forceinline__ void g2_add_affine29(Acc29G2& a, const Affine<Fp2>* __restrict__ pp) {
    const Fp2 one2{Fp::one(), Fp::zero()};
    Acc29G2 P1;
    const Affine<Fp2> q = *pp;
    acc29g2_load(P1, XYZZ<Fp2>{q.x, q.y, one2, one2});
    acc29g2_add(a, P1);
}
// [x0] P, the long half of the test (63 doublings, 27 additions); *pp is not the point at infinity
__device__ __forceinline__ XYZZ<Fp2> g2_x0_mul_one(const Affine<Fp2>* __restrict__ pp) {
    const uint32_t x0[2] = {0x4a6909f1u, 0x44e992b4u};  // 4965661367192848881
    Acc29G2 a;
    a.inf = true;
    a.x = a.y = a.zz = a.zzz = f2_load29(pp->x);  // (defined values; never read while inf)
#pragma unroll 1
    for (int k = 62; k >= 0; k--) {
        acc29g2_dbl(a);
        if ((x0[k >> 5] >> (k & 31)) & 1) g2_add_affine29(a, pp);
    }
    return acc29g2_to_xyzz(a);
}
// the rest: [x0 + 1] P + psi([x0] P) + psi^2([x0] P) == psi^3([2 x0] P)
__device__ inline bool g2_subgroup_tail29(const Affine<Fp2>* __restrict__ pp, const XYZZ<Fp2>& x0p, const PsiConsts& K) {
    Acc29G2 a;
    acc29g2_load(a, x0p);
    const U29x2 gx = f2_contract29(f2_load29(K.gx)), gy = f2_contract29(f2_load29(K.gy));
    const Acc29G2 b = g2_psi_dev29(a, gx, gy);  // psi([x0] P)
    g2_add_affine29(a, pp);                      // [x0 + 1] P
    Acc29G2 lhs = a;
    acc29g2_add(lhs, b);
    const Acc29G2 c = g2_psi_dev29(b, gx, gy);  // psi^2([x0] P)
    acc29g2_add(lhs, c);
    Acc29G2 d = g2_psi_dev29(c, gx, gy);        // psi^3([x0] P)
    acc29g2_dbl(d);                              // psi^3([2 x0] P)
    if (lhs.inf || d.inf) return lhs.inf && d.inf;
    // (a coordinate sum that came out as the point at infinity went through the canonical path of acc29g2_add / _dbl, which sets .inf)
    return f2_eq29(f2_mulFK29<40>(lhs.x, d.zz), f2_mulFK29<40>(d.x, lhs.zz)) && f2_eq29(f2_mulFK29<40>(lhs.y, d.zzz), f2_mulFK29<40>(d.y, lhs.zzz));
}
// the definition, r * P == infinity (four times the work of the two functions above)
__device__ __forceinline__ bool g2_subgroup_full_one(const Affine<Fp2>& p) {
    const uint32_t rk[8] = {FrParams::MOD[0], FrParams::MOD[1], FrParams::MOD[2], FrParams::MOD[3], FrParams::MOD[4], FrParams::MOD[5], FrParams::MOD[6], FrParams::MOD[7]};
    return scalar_mul(p, rk).is_inf();
}
// the first half of G2Affine.SetBytes: the square root and its sign, no subgroup test.  false on an invalid encoding; *out is then the point at infinity
// (reject: as in g1_decompress_one)
template <class Reject>
__device__ __forceinline__ bool g2_decompress_one(const uint32_t raw[16], const Fp2& bt, const Fp& half, Affine<Fp2>* out, const Reject& reject) {
    Fp x1 = load_be32<Fp>(raw), x0 = load_be32<Fp>(raw + 8);
    const uint32_t flag = x1.l[7] >> 30;
    x1.l[7] &= 0x3fffffffu;
    Affine<Fp2> p = Affine<Fp2>::inf();
    if (flag == 1) {
        const bool ok = x1.is_zero() && x0.is_zero();
        if (!ok) reject();
        *out = p;
        return ok;
    }
    if (flag == 0 || geq_mod<FpParams>(x1.l) || geq_mod<FpParams>(x0.l)) {
        reject();
        *out = p;
        return false;
    }
    Fp2 x{x0.to_mont(), x1.to_mont()};
    Fp2 rhs = x.sqr() * x + bt, y;
    if (!f2_sqrt_dev(rhs, half, &y)) {
        reject();
        *out = p;
        return false;
    }
    if (f2_lex_largest_dev(y) != (flag == 3)) y = y.neg();
    p.x = x;
    p.y = y;
    *out = p;
    return true;
}
__device__ __forceinline__ void g2_compress_one(const Affine<Fp2>& p, uint32_t raw[16]) {
    Fp x1 = Fp::zero(), x0 = Fp::zero();
    uint32_t flag = 1;
    if (!p.is_inf()) {
        x1 = p.x.a1.from_mont();
        x0 = p.x.a0.from_mont();
        flag = f2_lex_largest_dev(p.y) ? 3 : 2;
    }
    x1.l[7] |= flag << 30;
    store_be32(raw, x1);
    store_be32(raw + 8, x0);
}

// ---- the constants of the G2 decoder, computed on the host: the twist's b' = 3 / (9 + u), psi's coefficients xi^((q-1)/3) and xi^((q-1)/2), 1 / 2
inline HFp2 f2_pow(HFp2 a, const uint64_t e[4]) {
    HFp2 r = HFp2::one();
    for (int i = 0; i < 256; i++) {
        if ((e[i >> 6] >> (i & 63)) & 1) r = r * a;
        a = a.sqr();
    }
    return r;
}
struct G2CodecConsts { Fp2 bt; PsiConsts psi; };
inline G2CodecConsts g2_codec_consts() {
    HFp nine = HFp::zero(), three = HFp::one() + HFp::one() + HFp::one();
    for (int i = 0; i < 3; i++) nine = nine + three;
    const HFp2 bt = HFp2{three, HFp::zero()} * HFp2{nine, HFp::one()}.inv();
    G2CodecConsts K;
    memcpy(&K.bt, &bt, sizeof bt);
    static const uint64_t E3[4] = {0x69602eb24829a9c2ULL, 0xdd2b2385cd7b4384ULL, 0xe81ac1e7808072c9ULL, 0x10216f7ba065e00dULL};
    static const uint64_t E2h[4] = {0x9e10460b6c3e7ea3ULL, 0xcbc0b548b438e546ULL, 0xdc2822db40c0ac2eULL, 0x183227397098d014ULL};
    const HFp2 xi{nine, HFp::one()}, gx = f2_pow(xi, E3), gy = f2_pow(xi, E2h);
    memcpy(&K.psi.gx, &gx, sizeof gx);
    memcpy(&K.psi.gy, &gy, sizeof gy);
    const HFp half = (HFp::one() + HFp::one()).inv();
    memcpy(&K.psi.half, &half, sizeof half);
    return K;
}

}  // namespace zkmi
