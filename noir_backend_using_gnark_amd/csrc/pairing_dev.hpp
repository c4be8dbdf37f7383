// BN254 optimal ate pairing on the device (host-compilable too: every function is ZK_HD over ff.hpp's Fp / Fp2).
//
// Tower (gnark-crypto's): Fp6 = Fp2[v] / (v^3 - xi), Fp12 = Fp6[w] / (w^2 - v), xi = 9 + u.  The memory image of F12 is therefore gnark's E12
// {C0 {B0, B1, B2}, C1 {B0, B1, B2}} (zk_gt, 384 bytes).  pairing.hpp's flat w-basis c[0..5] maps to it as C0 = (c0, c2, c4), C1 = (c1, c3, c5).
// Miller loop over 6 x0 + 2 with homogeneous projective coordinates on the D-twist E': y^2 = x^3 + b', b' = 3 / xi (no inversion), lines evaluated at
// affine P; its value differs from pairing.hpp's affine loop by factors in Fp2, which the final exponentiation sends to one.
// Final exponentiation: easy part (p^6 - 1)(p^2 + 1), hard part EXACTLY (p^4 - p^2 + 1) / r by Scott et al. 2009 (lambda_0 + lambda_1 p + lambda_2 p^2 +
// lambda_3 p^3 with lambda_3 = 1, lambda_2 = 6 x^2 + 1, lambda_1 = -36 x^3 - 18 x^2 - 12 x + 1, lambda_0 = -36 x^3 - 30 x^2 - 18 x - 2): three
// exponentiations by x0 with cyclotomic squarings and a 10-product addition chain.  Bit-exact with pairing.hpp's final_exp.
#pragma once
#include "curve.hpp"
#include "ff.hpp"

namespace zkmi {
namespace pdev {

// constants computed on the host from pairing.hpp's consts() (verify_batch.hip: pair_consts)
struct PairConsts {
    Fp2 g1[6];  // xi^(i (p - 1) / 6): f^p   maps w-coefficient c_i to conj(c_i) g1[i]
    Fp g2[6];   // xi^(i (p^2 - 1) / 6) (in Fp): f^(p^2) maps c_i to c_i g2[i]
    Fp2 b3;     // 3 b' = 9 / xi
};

ZK_HD Fp2 mul_xi(const Fp2& a) {  // (a0 + a1 u)(9 + u)
    const Fp t0 = a.a0.dbl().dbl().dbl() + a.a0, t1 = a.a1.dbl().dbl().dbl() + a.a1;
    return Fp2{t0 - a.a1, t1 + a.a0};
}
ZK_HD Fp2 conj(const Fp2& a) { return Fp2{a.a0, a.a1.neg()}; }
ZK_HD Fp2 mul_fp(const Fp2& a, const Fp& s) { return Fp2{a.a0 * s, a.a1 * s}; }

struct F6 {
    Fp2 b0, b1, b2;
    static ZK_HD F6 zero() { return F6{Fp2::zero(), Fp2::zero(), Fp2::zero()}; }
    static ZK_HD F6 one() { return F6{Fp2::one(), Fp2::zero(), Fp2::zero()}; }
    friend ZK_HD F6 operator+(const F6& a, const F6& b) { return F6{a.b0 + b.b0, a.b1 + b.b1, a.b2 + b.b2}; }
    friend ZK_HD F6 operator-(const F6& a, const F6& b) { return F6{a.b0 - b.b0, a.b1 - b.b1, a.b2 - b.b2}; }
    ZK_HD F6 neg() const { return F6{b0.neg(), b1.neg(), b2.neg()}; }
    ZK_HD F6 mul_v() const { return F6{mul_xi(b2), b0, b1}; }
    // Karatsuba: 6 Fp2 products
    friend ZK_HD F6 operator*(const F6& a, const F6& b) {
        const Fp2 t0 = a.b0 * b.b0, t1 = a.b1 * b.b1, t2 = a.b2 * b.b2;
        const Fp2 c0 = mul_xi((a.b1 + a.b2) * (b.b1 + b.b2) - t1 - t2) + t0;
        const Fp2 c1 = (a.b0 + a.b1) * (b.b0 + b.b1) - t0 - t1 + mul_xi(t2);
        const Fp2 c2 = (a.b0 + a.b2) * (b.b0 + b.b2) - t0 - t2 + t1;
        return F6{c0, c1, c2};
    }
    // times (c0 + c1 v): 5 Fp2 products
    ZK_HD F6 mul01(const Fp2& c0, const Fp2& c1) const {
        const Fp2 t0 = b0 * c0, t1 = b1 * c1;
        return F6{mul_xi(b2 * c1) + t0, (b0 + b1) * (c0 + c1) - t0 - t1, b2 * c0 + t1};
    }
    ZK_HD F6 inv() const {
        const Fp2 t0 = b0.sqr() - mul_xi(b1 * b2), t1 = mul_xi(b2.sqr()) - b0 * b1, t2 = b1.sqr() - b0 * b2;
        const Fp2 d = (b0 * t0 + mul_xi(b2 * t1 + b1 * t2)).inv();
        return F6{t0 * d, t1 * d, t2 * d};
    }
};

struct F12 {
    F6 c0, c1;
    static ZK_HD F12 one() { return F12{F6::one(), F6::zero()}; }
    ZK_HD bool is_one() const {
        return c0.b0 == Fp2::one() && c0.b1.is_zero() && c0.b2.is_zero() && c1.b0.is_zero() && c1.b1.is_zero() && c1.b2.is_zero();
    }
    // Karatsuba over Fp6: 18 Fp2 products
    friend ZK_HD F12 operator*(const F12& a, const F12& b) {
        const F6 t0 = a.c0 * b.c0, t1 = a.c1 * b.c1;
        const F6 s = (a.c0 + a.c1) * (b.c0 + b.c1);
        return F12{t0 + t1.mul_v(), s - t0 - t1};
    }
    // complex squaring: 12 Fp2 products
    ZK_HD F12 sqr() const {
        const F6 ab = c0 * c1;
        const F6 t = (c0 + c1) * (c0 + c1.mul_v());
        return F12{t - ab - ab.mul_v(), ab + ab};
    }
    ZK_HD F12 conj() const { return F12{c0, c1.neg()}; }  // f^(p^6)
    ZK_HD F12 inv() const {
        const F6 d = (c0 * c0 - (c1 * c1).mul_v()).inv();
        return F12{c0 * d, (c1 * d).neg()};
    }
    // times a D-twist line l0 + l1 w + l3 w^3 (w-basis positions 0, 1, 3: C0.B0, C1.B0, C1.B1): 13 Fp2 products
    ZK_HD F12 mul_line(const Fp2& l0, const Fp2& l1, const Fp2& l3) const {
        const F6 a{c0.b0 * l0, c0.b1 * l0, c0.b2 * l0};  // c0 * (l0, 0, 0)
        const F6 b = c1.mul01(l1, l3);                  // c1 * (l1, l3, 0)
        const F6 s = (c0 + c1).mul01(l0 + l1, l3);
        return F12{a + b.mul_v(), s - a - b};
    }
    // Granger-Scott squaring in the cyclotomic subgroup (after the easy part): with g = (x0, x4), (x3, x2), (x1, x5) the three Fp4 = Fp2[s]/(s^2 - xi)
    // components (x0 = C0.B0, x1 = C0.B1, x2 = C0.B2, x3 = C1.B0, x4 = C1.B1, x5 = C1.B2): 6 Fp2 squarings
    ZK_HD F12 cyc_sqr() const {
        const Fp2 &x0 = c0.b0, &x1 = c0.b1, &x2 = c0.b2, &x3 = c1.b0, &x4 = c1.b1, &x5 = c1.b2;
        // Fp4 squares: (a + b s)^2 = (a^2 + xi b^2) + 2 a b s
        const Fp2 s04a = x0.sqr(), s04b = x4.sqr(), s32a = x3.sqr(), s32b = x2.sqr(), s15a = x1.sqr(), s15b = x5.sqr();
        const Fp2 A0 = s04a + mul_xi(s04b), A1 = (x0 + x4).sqr() - s04a - s04b;  // (x0 + x4 s)^2
        const Fp2 B0 = s32a + mul_xi(s32b), B1 = (x3 + x2).sqr() - s32a - s32b;  // (x3 + x2 s)^2
        const Fp2 C0 = s15a + mul_xi(s15b), C1 = mul_xi((x1 + x5).sqr() - s15a - s15b);  // xi (x1 + x5 s)^2 's s-part
        F12 r;
        r.c0.b0 = (A0 - x0).dbl() + A0;
        r.c1.b1 = (A1 + x4).dbl() + A1;
        r.c0.b1 = (B0 - x1).dbl() + B0;
        r.c1.b2 = (B1 + x5).dbl() + B1;
        r.c0.b2 = (C0 - x2).dbl() + C0;
        r.c1.b0 = (C1 + x3).dbl() + C1;
        return r;
    }
};

// Frobenius maps (w-index i: C0.Bk is c_{2k}, C1.Bk is c_{2k+1})
ZK_HD F12 frob(const F12& f, const PairConsts& K) {
    return F12{F6{conj(f.c0.b0), conj(f.c0.b1) * K.g1[2], conj(f.c0.b2) * K.g1[4]}, F6{conj(f.c1.b0) * K.g1[1], conj(f.c1.b1) * K.g1[3], conj(f.c1.b2) * K.g1[5]}};
}
ZK_HD F12 frob2(const F12& f, const PairConsts& K) {
    return F12{F6{f.c0.b0, mul_fp(f.c0.b1, K.g2[2]), mul_fp(f.c0.b2, K.g2[4])}, F6{mul_fp(f.c1.b0, K.g2[1]), mul_fp(f.c1.b1, K.g2[3]), mul_fp(f.c1.b2, K.g2[5])}};
}

// ---- Miller loop

struct TwistProj { Fp2 x, y, z; };

// T <- 2 T (scaled by 4), line through T's tangent times -2 Y Z (in Fp2): l0 = -2 Y Z yP, l1 = 3 X^2 xP, l3 = 3 b' Z^2 - Y^2
ZK_HD void dbl_step(TwistProj& T, const Fp& xP, const Fp& yP, const Fp2& b3, Fp2& l0, Fp2& l1, Fp2& l3) {
    const Fp2 B = T.y.sqr(), C = T.z.sqr(), E = b3 * C, F = E.dbl() + E, H = (T.y + T.z).sqr() - B - C;
    const Fp2 X2 = T.x.sqr();
    l0 = mul_fp(H, yP).neg();
    l1 = mul_fp(X2.dbl() + X2, xP);
    l3 = E - B;
    const Fp2 xy = T.x * T.y, E2 = E.sqr();
    T.x = (xy * (B - F)).dbl();
    T.y = (B + F).sqr() - (E2.dbl() + E2).dbl().dbl();  // (B + F)^2 - 12 E^2
    T.z = (B * H).dbl().dbl();
}
// T <- T + Q (Q affine), line through T and Q times lambda = X - xQ Z (in Fp2): l0 = lambda yP, l1 = -theta xP, l3 = theta xQ - lambda yQ
ZK_HD void add_step(TwistProj& T, const Fp2& xQ, const Fp2& yQ, const Fp& xP, const Fp& yP, Fp2& l0, Fp2& l1, Fp2& l3) {
    const Fp2 theta = T.y - yQ * T.z, lambda = T.x - xQ * T.z;
    l0 = mul_fp(lambda, yP);
    l1 = mul_fp(theta, xP).neg();
    l3 = theta * xQ - lambda * yQ;
    const Fp2 C = theta.sqr(), D = lambda.sqr(), E = lambda * D, F = T.z * C, G = T.x * D, H = E + F - G.dbl();
    T.y = theta * (G - H) - T.y * E;
    T.x = lambda * H;
    T.z = T.z * E;
}

// f_{6 x0 + 2, Q}(P) with the two Frobenius additions; either point at infinity gives one
ZK_HD F12 miller_loop(const Affine<Fp>& P, const Affine<Fp2>& Q, const PairConsts& K) {
    if (P.is_inf() || Q.is_inf()) return F12::one();
    const uint32_t LOOP[2] = {0xbe763ba8u, 0x9d797039u};  // 6 x0 + 2 = 0x1_9d797039be763ba8: bit 64 is the leading one
    TwistProj T{Q.x, Q.y, Fp2::one()};
    F12 f = F12::one();
    Fp2 l0, l1, l3;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int i = 63; i >= 0; i--) {
        if (i != 63) f = f.sqr();
        dbl_step(T, P.x, P.y, K.b3, l0, l1, l3);
        f = f.mul_line(l0, l1, l3);
        if ((LOOP[i >> 5] >> (i & 31)) & 1) {
            add_step(T, Q.x, Q.y, P.x, P.y, l0, l1, l3);
            f = f.mul_line(l0, l1, l3);
        }
    }
    // pi(Q) = (conj(x) g1[2], conj(y) g1[3]); -pi^2(Q)
    const Fp2 x1 = conj(Q.x) * K.g1[2], y1 = conj(Q.y) * K.g1[3];
    add_step(T, x1, y1, P.x, P.y, l0, l1, l3);
    f = f.mul_line(l0, l1, l3);
    const Fp2 x2 = conj(x1) * K.g1[2], y2 = (conj(y1) * K.g1[3]).neg();
    add_step(T, x2, y2, P.x, P.y, l0, l1, l3);
    return f.mul_line(l0, l1, l3);
}

// ---- final exponentiation

ZK_HD F12 expt(const F12& a) {  // a^x0 in the cyclotomic subgroup, x0 = 0x44e992b4_4a6909f1 (63 bits)
    const uint32_t X0[2] = {0x4a6909f1u, 0x44e992b4u};
    F12 r = a;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int i = 61; i >= 0; i--) {
        r = r.cyc_sqr();
        if ((X0[i >> 5] >> (i & 31)) & 1) r = r * a;
    }
    return r;
}
ZK_HD F12 easy_part(const F12& f, const PairConsts& K) {
    const F12 t = f.conj() * f.inv();  // ^(p^6 - 1)
    return frob2(t, K) * t;            // ^(p^2 + 1)
}
// the hard part after the three exponentiations, as a table of steps  ws[dst] = op_a(ws[a]) * op_b(ws[b]) over the slots
// 0 = f, 1 = f^x, 2 = f^(x^2), 3 = f^(x^3), 4 = T0, 5 = T1, 6 = a temporary; each step is one kernel launch on the device (verify_batch.hip: k_fe_step), so
// that no kernel holds more than two F12 operands in registers.  With y0 = f^p f^(p^2) f^(p^3), y1 = 1 / f, y2 = fx2^(p^2), y3 = 1 / fx^p,
// y4 = 1 / (fx fx2^p), y5 = 1 / fx2, y6 = 1 / (fx3 fx3^p) (in the cyclotomic subgroup the inverse is the conjugate), Scott et al.'s chain:
//   T0 = y6^2 y4 y5, T1 = y3 y5 T0, T0 = T0 y2, T1 = (T1^2 T0)^2, result = (T1 y1)^2 (T1 y0)
enum : int8_t { OP_FROB = 1, OP_FROB2 = 2, OP_CONJ = 4, OP_CSQR = 8 };  // applied in the order frob2, frob, conj, cyclotomic square
struct FeStep { int8_t dst, a, opa, b, opb; };
constexpr int FE_CHAIN_LEN = 13;
constexpr FeStep FE_CHAIN[FE_CHAIN_LEN] = {
    {4, 3, 0, 3, OP_FROB},                     // fx3 fx3^p
    {6, 1, 0, 2, OP_FROB},                     // fx fx2^p
    {4, 4, OP_CONJ | OP_CSQR, 6, OP_CONJ},     // y6^2 y4
    {4, 4, 0, 2, OP_CONJ},                     // T0 = y6^2 y4 y5
    {5, 1, OP_FROB | OP_CONJ, 2, OP_CONJ},     // y3 y5
    {5, 5, 0, 4, 0},                           // T1 = y3 y5 T0
    {4, 4, 0, 2, OP_FROB2},                    // T0 = T0 y2
    {5, 5, OP_CSQR, 4, 0},                     // U = T1^2 T0 (and T1 = U^2, squared where it is used)
    {4, 5, OP_CSQR, 0, OP_CONJ},               // T0 = T1 y1
    {6, 0, OP_FROB, 0, OP_FROB2},              // f^p f^(p^2)
    {6, 6, 0, 0, OP_FROB | OP_FROB2},          // y0
    {5, 5, OP_CSQR, 6, 0},                     // T1 = T1 y0
    {4, 4, OP_CSQR, 5, 0},                     // the result: T0^2 T1
};
constexpr int FE_SLOTS = 7;
ZK_HD F12 fe_op(F12 x, int op, const PairConsts& K) {
    if (op & OP_FROB2) x = frob2(x, K);
    if (op & OP_FROB) x = frob(x, K);
    if (op & OP_CONJ) x = x.conj();
    if (op & OP_CSQR) x = x.cyc_sqr();
    return x;
}
ZK_HD F12 fe_step(const F12& a, int opa, const F12& b, int opb, const PairConsts& K) { return fe_op(a, opa, K) * fe_op(b, opb, K); }
// the whole hard part on one thread (the host check of the table)
ZK_HD F12 hard_part(const F12& f, const PairConsts& K) {
    F12 ws[FE_SLOTS];
    ws[0] = f;
    for (int k = 1; k < 4; k++) ws[k] = expt(ws[k - 1]);
    for (int k = 0; k < FE_CHAIN_LEN; k++) {
        const FeStep& st = FE_CHAIN[k];
        ws[st.dst] = fe_step(ws[st.a], st.opa, ws[st.b], st.opb, K);
    }
    return ws[FE_CHAIN[FE_CHAIN_LEN - 1].dst];
}

}  // namespace pdev
}  // namespace zkmi
