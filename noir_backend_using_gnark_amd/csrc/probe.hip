// Test-only probe of the device arithmetic and codecs: every op runs ONE production inline function (ff.hpp, ff29.hpp, curve.hpp, pairing_dev.hpp,
// sha256_dev.hpp, codec_dev.hpp) on one test vector per lane and writes back the raw limbs it returns -- nothing is canonicalised that the function under test
// did not canonicalise.  Built into libzkmi_probe.so (Makefile `all`), never into libzkmi.so; tests/probe.py binds it.
//
// A vector is a fixed number of 32-bit words (IN), a result another (OUT), both per op (PROBE_OPS).  Lane t reads in[t * IN ..] and writes
// out[t * OUT ..]; no address depends on the data (the SHA-256 op reads at most its own record), so a wrong result is a wrong value, never a fault.
#include <hip/hip_runtime.h>
#include <string.h>

#include "codec_dev.hpp"
#include "ff29.hpp"
#include "pairing_dev.hpp"
#include "sha256_dev.hpp"

namespace zkmi {
namespace probe {

// name, words in, words out
#define PROBE_OPS(X)                                                                                                                         \
    X(FP_MUL, 16, 8) X(FP_SQR, 16, 8) X(FP_ADD, 16, 8) X(FP_SUB, 16, 8) X(FP_NEG, 16, 8) X(FP_INV, 16, 8) X(FP_REDUCE_ONCE, 16, 8)           \
    X(FP_TO_MONT, 16, 8) X(FP_FROM_MONT, 16, 8)                                                                                              \
    X(FR_MUL, 16, 8) X(FR_SQR, 16, 8) X(FR_ADD, 16, 8) X(FR_SUB, 16, 8) X(FR_NEG, 16, 8) X(FR_INV, 16, 8) X(FR_REDUCE_ONCE, 16, 8)           \
    X(FR_TO_MONT, 16, 8) X(FR_FROM_MONT, 16, 8)                                                                                              \
    X(FP2_MUL, 32, 16) X(FP2_SQR, 32, 16) X(FP2_INV, 32, 16)                                                                                 \
    X(F6_MUL, 96, 48) X(F6_INV, 96, 48)                                                                                                      \
    X(F12_MUL, 192, 96) X(F12_SQR, 192, 96) X(F12_CYC_SQR, 192, 96) X(F12_INV, 192, 96) X(F12_MUL_LINE, 192, 96) X(F12_CONJ, 192, 96)       \
    X(F12_FROB, 192, 96) X(F12_FROB2, 192, 96)                                                                                               \
    X(G1_ADD, 72, 32) X(G1_MADD, 72, 32) X(G1_DBL, 72, 32) X(G1_DBL_AFFINE, 72, 32) X(G1_TO_AFFINE, 72, 32) X(G1_SCALAR_MUL, 72, 32)        \
    X(G2_ADD, 136, 64) X(G2_MADD, 136, 64) X(G2_DBL, 136, 64) X(G2_DBL_AFFINE, 136, 64) X(G2_TO_AFFINE, 136, 64) X(G2_SCALAR_MUL, 136, 64)  \
    X(U29_MUL, 72, 9) X(U29_SQR, 72, 9) X(U29_MUL2, 72, 9) X(U29_MUL3, 72, 9) X(U29_MUL4, 72, 9) X(U29_MUL_X2, 72, 18)                      \
    X(U29_SQR_X2, 72, 18) X(U29_ADD, 72, 9)                                                                                                  \
    X(U29_SUB4, 72, 9) X(U29_SUB8, 72, 9) X(U29_SUB12, 72, 9) X(U29_SUB16, 72, 9) X(U29_SUB24, 72, 9) X(U29_SUB32, 72, 9)                   \
    X(U29_SUB40, 72, 9) X(U29_SUB64, 72, 9) X(U29_SUB80, 72, 9)                                                                             \
    X(U29_NEG4, 72, 9) X(U29_NEG8, 72, 9) X(U29_NEG12, 72, 9) X(U29_NEG16, 72, 9) X(U29_NEG24, 72, 9) X(U29_NEG32, 72, 9)                   \
    X(U29_NEG40, 72, 9) X(U29_NEG64, 72, 9) X(U29_NEG80, 72, 9)                                                                             \
    X(U29_WNORM, 72, 9) X(U29_WNORM_FWD, 72, 9) X(U29_RIPPLE, 72, 9) X(U29_LOAD, 72, 9) X(U29_UNPACK, 72, 9) X(U29_STORE, 72, 8)            \
    X(U29P_REDUCE, 72, 9) X(U29P_PACK, 72, 8) X(U29_MULOUT_IS_ZERO, 72, 1) X(U29_MULOUT3_IS_ZERO, 72, 1) X(U29_MAYBE_ZERO16, 72, 1)         \
    X(F2_MUL29, 72, 18) X(F2_SQR29_8, 72, 27) X(F2_MULF29, 72, 18) X(F2_MULFK29_4, 72, 18) X(F2_MULFK29_16, 72, 18)                         \
    X(F2_MULFK29_40, 72, 18) X(F2_CONTRACT29, 72, 18)                                                                                        \
    X(U29R_MUL, 72, 9) X(U29R_SUB4, 72, 9) X(U29R_SUB16, 72, 9) X(U29R_SUB24, 72, 9) X(U29R_SUB40, 72, 9) X(U29R_REDUCE, 72, 9)             \
    X(U29R_LOAD5, 72, 9) X(U29R_PACK0, 72, 8) X(U29R_PACK1, 72, 8)                                                                           \
    X(ACC29_MADD, 74, 37) X(ACC29_ADD, 74, 37) X(ACC29_DBL, 74, 37) X(ACC29_ADD_QUAD, 74, 37) X(ACC29_DBL_QUAD, 74, 37)                     \
    X(ACC29_PACK_LOAD, 74, 69) X(ACC29_MADD_CHAIN, 37 + 16 * 100, 37)                                                                        \
    X(ACC29G2_MADD, 146, 73) X(ACC29G2_ADD, 146, 73) X(ACC29G2_DBL, 146, 73) X(ACC29G2_MADD_CHAIN, 73 + 32 * 100, 73)                       \
    X(SHA256, 12 + SHA_MAX_BYTES / 4, 8)                                                                                                     \
    X(FP_POW_QM3_4, 8, 8) X(FP_SQRT_CAND, 8, 8) X(F2_SQRT, 16, 17) X(G1_DECOMPRESS, 8, 17) X(G1_COMPRESS, 16, 8)                           \
    X(G2_DECOMPRESS, 16, 33) X(G2_COMPRESS, 32, 16) X(G2_IN_SUBGROUP, 32, 1) X(G2_IN_SUBGROUP_FULL, 32, 1)                                  \
    X(FR_FROM_BE, 8, 9) X(FR_TO_BE, 8, 8) X(HEX_DECODE4, 1, 2) X(HEX_ENCODE2, 1, 1)

constexpr int SHA_MAX_BYTES = 320;
constexpr int CHAIN = 100;  // madds per lane of the *_MADD_CHAIN ops

enum Op {
#define PROBE_ENUM(name, i, o) name,
    PROBE_OPS(PROBE_ENUM)
#undef PROBE_ENUM
    N_OPS
};
constexpr int IN_W[] = {
#define PROBE_IN(name, i, o) i,
    PROBE_OPS(PROBE_IN)
#undef PROBE_IN
};
constexpr int OUT_W[] = {
#define PROBE_OUT(name, i, o) o,
    PROBE_OPS(PROBE_OUT)
#undef PROBE_OUT
};
const char* const NAMES[] = {
#define PROBE_NAME(name, i, o) #name,
    PROBE_OPS(PROBE_NAME)
#undef PROBE_NAME
};

// plain word copies between a record and a struct made only of uint32 words
template <class T>
__device__ __forceinline__ T ld(const uint32_t* p) {
    static_assert(sizeof(T) % 4 == 0, "word image");
    T x;
    uint32_t* d = reinterpret_cast<uint32_t*>(&x);
#pragma unroll
    for (int i = 0; i < (int)(sizeof(T) / 4); i++) d[i] = p[i];
    return x;
}
template <class T>
__device__ __forceinline__ void st(uint32_t* p, const T& x) {
    static_assert(sizeof(T) % 4 == 0, "word image");
    const uint32_t* s = reinterpret_cast<const uint32_t*>(&x);
#pragma unroll
    for (int i = 0; i < (int)(sizeof(T) / 4); i++) p[i] = s[i];
}
// Acc29 / Acc29G2 records: the coordinates, then the infinity flag as one word
__device__ __forceinline__ Acc29 ld_acc(const uint32_t* p) {
    Acc29 A;
    A.x = ld<U29>(p);
    A.y = ld<U29>(p + 9);
    A.zz = ld<U29>(p + 18);
    A.zzz = ld<U29>(p + 27);
    A.inf = p[36] != 0;
    return A;
}
__device__ __forceinline__ void st_acc(uint32_t* p, const Acc29& A) {
    st(p, A.x);
    st(p + 9, A.y);
    st(p + 18, A.zz);
    st(p + 27, A.zzz);
    p[36] = A.inf ? 1u : 0u;
}
__device__ __forceinline__ Acc29G2 ld_acc2(const uint32_t* p) {
    Acc29G2 A;
    A.x = ld<U29x2>(p);
    A.y = ld<U29x2>(p + 18);
    A.zz = ld<U29x2>(p + 36);
    A.zzz = ld<U29x2>(p + 54);
    A.inf = p[72] != 0;
    return A;
}
__device__ __forceinline__ void st_acc2(uint32_t* p, const Acc29G2& A) {
    st(p, A.x);
    st(p + 18, A.y);
    st(p + 36, A.zz);
    st(p + 54, A.zzz);
    p[72] = A.inf ? 1u : 0u;
}

// saturated field ops: a = words 0..7, b = words 8..15
template <class F, int BASE, int OP>
__device__ __forceinline__ void field_op(const uint32_t* in, uint32_t* out) {
    const F a = ld<F>(in), b = ld<F>(in + 8);
    constexpr int k = OP - BASE;
    F r;
    if constexpr (k == 0) r = a * b;
    else if constexpr (k == 1) r = a.sqr();
    else if constexpr (k == 2) r = a + b;
    else if constexpr (k == 3) r = a - b;
    else if constexpr (k == 4) r = a.neg();
    else if constexpr (k == 5) r = a.inv();
    else if constexpr (k == 6) r = F::reduce_once(a.l);
    else if constexpr (k == 7) r = a.to_mont();
    else r = a.from_mont();
    st(out, r);
}

// saturated XYZZ ops: A = XYZZ record, B = XYZZ record (madd / dbl_affine / to_affine / scalar_mul read A's or B's x, y as an affine point), k = 8 words
template <class F, int BASE, int OP>
__device__ __forceinline__ void curve_op(const uint32_t* in, uint32_t* out) {
    constexpr int W = (int)(sizeof(F) / 4);
    XYZZ<F> A = ld<XYZZ<F>>(in);
    const XYZZ<F> B = ld<XYZZ<F>>(in + 4 * W);
    const uint32_t* k = in + 8 * W;
    constexpr int c = OP - BASE;
    if constexpr (c == 0) A.add(B);
    else if constexpr (c == 1) A.madd(B.x, B.y);
    else if constexpr (c == 2) A.dbl();
    else if constexpr (c == 3) A = XYZZ<F>::dbl_affine(Affine<F>{A.x, A.y});
    else if constexpr (c == 4) {
        const Affine<F> a = A.to_affine();
        A = XYZZ<F>{a.x, a.y, F::zero(), F::zero()};
    } else {
        uint32_t kk[8];
#pragma unroll
        for (int i = 0; i < 8; i++) kk[i] = k[i];
        A = scalar_mul(Affine<F>{A.x, A.y}, kk);
    }
    st(out, A);
}

template <int K>
__device__ __forceinline__ U29 sub_k(const U29& a, const U29& b) { return u29_sub<K>(a, b); }
template <int K>
__device__ __forceinline__ U29 neg_k(const U29& a) { return u29_neg<K>(a); }

// codec ops (codec_dev.hpp): the bytes of an encoding as they lie in the file, read as 32-bit words; points and field elements as Montgomery images;
// a verdict as one word after the value.  K: the production constants of the G2 decoder (g2_codec_consts)
template <int OP>
__device__ __forceinline__ void codec_op(const uint32_t* in, uint32_t* out, const G2CodecConsts& K) {
    if constexpr (OP == FP_POW_QM3_4 || OP == FP_SQRT_CAND) st(out, fp_pow_qm3_4(ld<Fp>(in), OP == FP_SQRT_CAND));
    else if constexpr (OP == F2_SQRT) {
        Fp2 r = Fp2::zero();
        out[0] = f2_sqrt_dev(ld<Fp2>(in), K.psi.half, &r) ? 1u : 0u;
        st(out + 1, r);
    } else if constexpr (OP == G1_DECOMPRESS) {
        Affine<Fp> p;
        out[16] = g1_decompress_one(in, &p, NoReject()) ? 0u : 1u;
        st(out, p);
    } else if constexpr (OP == G1_COMPRESS) g1_compress_one(ld<Affine<Fp>>(in), out);
    else if constexpr (OP == G2_DECOMPRESS) {
        Affine<Fp2> p;
        out[32] = g2_decompress_one(in, K.bt, K.psi.half, &p, NoReject()) ? 0u : 1u;
        st(out, p);
    } else if constexpr (OP == G2_COMPRESS) g2_compress_one(ld<Affine<Fp2>>(in), out);
    else if constexpr (OP == G2_IN_SUBGROUP || OP == G2_IN_SUBGROUP_FULL) {
        // the two kernels of the production test in one (k_g2_x0_mul, k_g2_subgroup), with their guard: the point at infinity is not tested
        const Affine<Fp2>* pp = reinterpret_cast<const Affine<Fp2>*>(in);
        const Affine<Fp2> p = *pp;
        bool member = true;
        if (!p.is_inf()) {
            if constexpr (OP == G2_IN_SUBGROUP) member = g2_subgroup_tail29(pp, g2_x0_mul_one(pp), K.psi);
            else member = g2_subgroup_full_one(p);
        }
        out[0] = member ? 1u : 0u;
    } else if constexpr (OP == FR_FROM_BE) {
        Fr x = Fr::zero();
        out[8] = fr_from_be_one(in, &x) ? 0u : 2u;  // the kernel's status bit
        st(out, x);
    } else if constexpr (OP == FR_TO_BE) fr_to_be_one(ld<Fr>(in), out);
    else if constexpr (OP == HEX_DECODE4) {
        uint32_t bad = 0;
        out[0] = hexdig4(in[0], &bad);
        out[1] = bad ? 1u : 0u;
    } else out[0] = hexenc2w(in[0] & 0xffffu);
}

template <int OP>
__device__ __forceinline__ void run(const uint32_t* in, uint32_t* out, unsigned lane, const G2CodecConsts& K) {
    (void)lane;
    (void)K;
    if constexpr (OP >= FP_MUL && OP <= FP_FROM_MONT) field_op<Fp, FP_MUL, OP>(in, out);
    else if constexpr (OP >= FR_MUL && OP <= FR_FROM_MONT) field_op<Fr, FR_MUL, OP>(in, out);
    else if constexpr (OP >= FP2_MUL && OP <= FP2_INV) {
        const Fp2 a = ld<Fp2>(in), b = ld<Fp2>(in + 16);
        st(out, OP == FP2_MUL ? a * b : OP == FP2_SQR ? a.sqr() : a.inv());
    } else if constexpr (OP == F6_MUL || OP == F6_INV) {
        const pdev::F6 a = ld<pdev::F6>(in), b = ld<pdev::F6>(in + 48);
        st(out, OP == F6_MUL ? a * b : a.inv());
    } else if constexpr (OP >= F12_MUL && OP <= F12_FROB2) {
        const pdev::F12 a = ld<pdev::F12>(in);
        pdev::F12 r;
        if constexpr (OP == F12_MUL) r = a * ld<pdev::F12>(in + 96);
        else if constexpr (OP == F12_SQR) r = a.sqr();
        else if constexpr (OP == F12_CYC_SQR) r = a.cyc_sqr();
        else if constexpr (OP == F12_INV) r = a.inv();
        else if constexpr (OP == F12_MUL_LINE) r = a.mul_line(ld<Fp2>(in + 96), ld<Fp2>(in + 112), ld<Fp2>(in + 128));
        else if constexpr (OP == F12_CONJ) r = a.conj();
        else {
            // b holds the Frobenius constants: g1[6] (Fp2) for FROB, g2[6] (Fp) for FROB2
            pdev::PairConsts K;
#pragma unroll
            for (int i = 0; i < 6; i++) {
                K.g1[i] = ld<Fp2>(in + 96 + 16 * i);
                K.g2[i] = ld<Fp>(in + 96 + 8 * i);
            }
            K.b3 = Fp2::zero();
            r = OP == F12_FROB ? pdev::frob(a, K) : pdev::frob2(a, K);
        }
        st(out, r);
    } else if constexpr (OP >= G1_ADD && OP <= G1_SCALAR_MUL) curve_op<Fp, G1_ADD, OP>(in, out);
    else if constexpr (OP >= G2_ADD && OP <= G2_SCALAR_MUL) curve_op<Fp2, G2_ADD, OP>(in, out);
    else if constexpr (OP >= U29_MUL && OP <= U29_MAYBE_ZERO16) {
        const U29 a0 = ld<U29>(in), b0 = ld<U29>(in + 9), a1 = ld<U29>(in + 18), b1 = ld<U29>(in + 27);
        if constexpr (OP == U29_MUL) st(out, u29_mul(a0, b0));
        else if constexpr (OP == U29_SQR) st(out, u29_sqr(a0));
        else if constexpr (OP == U29_MUL2) st(out, u29_mul2(a0, b0, a1, b1));
        else if constexpr (OP == U29_MUL3) st(out, u29_mul3(a0, b0, a1, b1, ld<U29>(in + 36), ld<U29>(in + 45)));
        else if constexpr (OP == U29_MUL4) st(out, u29_mul4(a0, b0, a1, b1, ld<U29>(in + 36), ld<U29>(in + 45), ld<U29>(in + 54), ld<U29>(in + 63)));
        else if constexpr (OP == U29_MUL_X2) {
            U29 r0, r1;
            u29_mul_x2(a0, b0, a1, b1, r0, r1);
            st(out, r0);
            st(out + 9, r1);
        } else if constexpr (OP == U29_SQR_X2) {
            U29 r0, r1;
            u29_sqr_x2(a0, a1, r0, r1);
            st(out, r0);
            st(out + 9, r1);
        } else if constexpr (OP == U29_ADD) st(out, u29_add(a0, b0));
        else if constexpr (OP == U29_SUB4) st(out, sub_k<4>(a0, b0));
        else if constexpr (OP == U29_SUB8) st(out, sub_k<8>(a0, b0));
        else if constexpr (OP == U29_SUB12) st(out, sub_k<12>(a0, b0));
        else if constexpr (OP == U29_SUB16) st(out, sub_k<16>(a0, b0));
        else if constexpr (OP == U29_SUB24) st(out, sub_k<24>(a0, b0));
        else if constexpr (OP == U29_SUB32) st(out, sub_k<32>(a0, b0));
        else if constexpr (OP == U29_SUB40) st(out, sub_k<40>(a0, b0));
        else if constexpr (OP == U29_SUB64) st(out, sub_k<64>(a0, b0));
        else if constexpr (OP == U29_SUB80) st(out, sub_k<80>(a0, b0));
        else if constexpr (OP == U29_NEG4) st(out, neg_k<4>(a0));
        else if constexpr (OP == U29_NEG8) st(out, neg_k<8>(a0));
        else if constexpr (OP == U29_NEG12) st(out, neg_k<12>(a0));
        else if constexpr (OP == U29_NEG16) st(out, neg_k<16>(a0));
        else if constexpr (OP == U29_NEG24) st(out, neg_k<24>(a0));
        else if constexpr (OP == U29_NEG32) st(out, neg_k<32>(a0));
        else if constexpr (OP == U29_NEG40) st(out, neg_k<40>(a0));
        else if constexpr (OP == U29_NEG64) st(out, neg_k<64>(a0));
        else if constexpr (OP == U29_NEG80) st(out, neg_k<80>(a0));
        else if constexpr (OP == U29_WNORM) st(out, u29_wnorm(a0));
        else if constexpr (OP == U29_WNORM_FWD) st(out, u29_wnorm_fwd(a0));
        else if constexpr (OP == U29_RIPPLE) st(out, u29_ripple(a0));
        else if constexpr (OP == U29_LOAD) st(out, u29_load(ld<Fp>(in)));
        else if constexpr (OP == U29_UNPACK) st(out, u29_unpack(ld<Fp>(in)));
        else if constexpr (OP == U29_STORE) st(out, u29_store(a0));
        else if constexpr (OP == U29P_REDUCE) st(out, u29p_reduce(a0));
        else if constexpr (OP == U29P_PACK) st(out, u29p_pack(a0));
        else if constexpr (OP == U29_MULOUT_IS_ZERO) out[0] = u29_mulout_is_zero(a0) ? 1u : 0u;
        else if constexpr (OP == U29_MULOUT3_IS_ZERO) out[0] = u29_mulout3_is_zero(a0) ? 1u : 0u;
        else out[0] = u29_maybe_zero16(a0) ? 1u : 0u;
    } else if constexpr (OP >= F2_MUL29 && OP <= F2_CONTRACT29) {
        // a = words 0..17, b = 18..35, na1 (F2_MULF29) = 36..44
        const U29x2 a = ld<U29x2>(in), b = ld<U29x2>(in + 18);
        if constexpr (OP == F2_MUL29) st(out, f2_mul29(a, b));
        else if constexpr (OP == F2_SQR29_8) {
            U29 m;
            st(out, f2_sqr29<8>(a, &m));
            st(out + 18, m);
        } else if constexpr (OP == F2_MULF29) st(out, f2_mulF29(a, b, ld<U29>(in + 36)));
        else if constexpr (OP == F2_MULFK29_4) st(out, f2_mulFK29<4>(a, b));
        else if constexpr (OP == F2_MULFK29_16) st(out, f2_mulFK29<16>(a, b));
        else if constexpr (OP == F2_MULFK29_40) st(out, f2_mulFK29<40>(a, b));
        else st(out, f2_contract29(a));
    } else if constexpr (OP >= U29R_MUL && OP <= U29R_PACK1) {
        const U29 a = ld<U29>(in), b = ld<U29>(in + 9);
        if constexpr (OP == U29R_MUL) st(out, u29r_mul(a, b));
        else if constexpr (OP == U29R_SUB4) st(out, u29r_sub<4>(a, b));
        else if constexpr (OP == U29R_SUB16) st(out, u29r_sub<16>(a, b));
        else if constexpr (OP == U29R_SUB24) st(out, u29r_sub<24>(a, b));
        else if constexpr (OP == U29R_SUB40) st(out, u29r_sub<40>(a, b));
        else if constexpr (OP == U29R_REDUCE) st(out, u29r_reduce(a));
        else if constexpr (OP == U29R_LOAD5) st(out, u29r_load5(ld<Fr>(in)));
        else st(out, u29r_pack(a, OP == U29R_PACK1));
    } else if constexpr (OP >= ACC29_MADD && OP <= ACC29_MADD_CHAIN) {
        Acc29 A = ld_acc(in);
        if constexpr (OP == ACC29_MADD) xyzz_madd29(A, ld<Fp>(in + 37), ld<Fp>(in + 45));
        else if constexpr (OP == ACC29_ADD) acc29_add(A, ld_acc(in + 37));
        else if constexpr (OP == ACC29_DBL) acc29_dbl(A);
        else if constexpr (OP == ACC29_ADD_QUAD) acc29_add_quad(A, ld_acc(in + 37), lane & 3);
        else if constexpr (OP == ACC29_DBL_QUAD) acc29_dbl_quad(A, lane & 3);
        else if constexpr (OP == ACC29_PACK_LOAD) {
            const XYZZ<Fp> c = acc29_to_packed(A);
            st(out + 37, c);
            acc29_load(A, c);
        } else {
#pragma unroll 1
            for (int i = 0; i < CHAIN; i++) xyzz_madd29(A, ld<Fp>(in + 37 + 16 * i), ld<Fp>(in + 45 + 16 * i));
        }
        st_acc(out, A);
    } else if constexpr (OP >= ACC29G2_MADD && OP <= ACC29G2_MADD_CHAIN) {
        Acc29G2 A = ld_acc2(in);
        if constexpr (OP == ACC29G2_MADD) xyzz_madd29(A, ld<Fp2>(in + 73), ld<Fp2>(in + 89));
        else if constexpr (OP == ACC29G2_ADD) acc29g2_add(A, ld_acc2(in + 73));
        else if constexpr (OP == ACC29G2_DBL) acc29g2_dbl(A);
        else {
#pragma unroll 1
            for (int i = 0; i < CHAIN; i++) xyzz_madd29(A, ld<Fp2>(in + 73 + 32 * i), ld<Fp2>(in + 89 + 32 * i));
        }
        st_acc2(out, A);
    } else if constexpr (OP >= FP_POW_QM3_4 && OP <= HEX_ENCODE2) codec_op<OP>(in, out, K);
    else {
        // SHA256 record: mode, length L (bytes, <= SHA_MAX_BYTES), piece size, resume offset, midstate[8], message bytes.
        // mode 0: update in pieces of `piece` bytes; 1: resume(midstate, offset) then update the L bytes; 2: put256 of L / 32 little-endian 8-word integers
        const uint32_t mode = in[0], piece = in[2] ? in[2] : 1u;
        const uint32_t len = in[1] < (uint32_t)SHA_MAX_BYTES ? in[1] : (uint32_t)SHA_MAX_BYTES;
        const uint8_t* msg = reinterpret_cast<const uint8_t*>(in + 12);
        Sha256Dev h;
        h.reset();
        if (mode == 1) {
            uint32_t mid[8];
#pragma unroll
            for (int i = 0; i < 8; i++) mid[i] = in[4 + i];
            h.resume(mid, in[3]);
            h.update(msg, len);
        } else if (mode == 2) {
#pragma unroll 1
            for (uint32_t j = 0; j < len / 32; j++) h.put256(in + 12 + 8 * j);
        } else {
#pragma unroll 1
            for (uint32_t off = 0; off < len; off += piece) h.update(msg + off, len - off < piece ? len - off : piece);
        }
        uint32_t d[8];
        h.final(d);
#pragma unroll
        for (int i = 0; i < 8; i++) out[i] = d[i];
    }
}

constexpr unsigned BLOCK = 64;

template <int OP>
__global__ __launch_bounds__(BLOCK) void k_probe(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, size_t n, G2CodecConsts K) {
    const size_t t = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (t >= n) return;
    run<OP>(in + t * (size_t)IN_W[OP], out + t * (size_t)OUT_W[OP], threadIdx.x, K);
}

int launch(int op, const uint32_t* in, uint32_t* out, size_t n) {
    const dim3 grid((unsigned)((n + BLOCK - 1) / BLOCK)), block(BLOCK);
    const G2CodecConsts K = g2_codec_consts();
    switch (op) {
#define PROBE_CASE(name, i, o)                          \
    case name:                                          \
        k_probe<name><<<grid, block, 0, 0>>>(in, out, n, K); \
        break;
        PROBE_OPS(PROBE_CASE)
#undef PROBE_CASE
        default:
            return -5;
    }
    return (int)hipGetLastError();
}

}  // namespace probe
}  // namespace zkmi

extern "C" {

// op code of a name in PROBE_OPS, or -1
int zk_probe_op(const char* name) {
    using namespace zkmi::probe;
    for (int i = 0; name && i < N_OPS; i++)
        if (!strcmp(name, NAMES[i])) return i;
    return -1;
}

// words per input and per output vector of an op; -5 for an unknown op
int zk_probe_shape(int op, int* in_words, int* out_words) {
    using namespace zkmi::probe;
    if (op < 0 || op >= N_OPS || !in_words || !out_words) return -5;
    *in_words = IN_W[op];
    *out_words = OUT_W[op];
    return 0;
}

// n vectors of op: in holds n * IN words (n_in_bytes checked), out receives n * OUT words.  Quad ops need n % 4 == 0 (four lanes per vector).
// Returns 0, -5 for a bad argument, or the HIP error code.
int zk_probe(int op, const void* in, size_t n_in_bytes, void* out, size_t n) {
    using namespace zkmi::probe;
    if (op < 0 || op >= N_OPS || !in || !out || n == 0) return -5;
    const size_t ib = n * (size_t)IN_W[op] * 4, ob = n * (size_t)OUT_W[op] * 4;
    if (n_in_bytes < ib) return -5;
    if ((op == ACC29_ADD_QUAD || op == ACC29_DBL_QUAD) && n % 4) return -5;
    uint32_t *d_in = nullptr, *d_out = nullptr;
    hipError_t e = hipMalloc(&d_in, ib);
    if (e == hipSuccess) e = hipMalloc(&d_out, ob);
    if (e == hipSuccess) e = hipMemcpy(d_in, in, ib, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(d_out, 0xa5, ob);
    int rc = (int)e;
    if (e == hipSuccess) rc = launch(op, d_in, d_out, n);
    if (rc == 0) rc = (int)hipDeviceSynchronize();
    if (rc == 0) rc = (int)hipMemcpy(out, d_out, ob, hipMemcpyDeviceToHost);
    if (d_in) (void)hipFree(d_in);
    if (d_out) (void)hipFree(d_out);
    return rc;
}

}  // extern "C"
