// Key / SRS wire formats on the device -- SURVEY §8 row f1: what the reference moves between Rust and Go as hex strings and keeps in
// srs.hex  [REF gnark_backend_ffi/internal/backend/helpers.go:49-94 (Serialize/DeserializeProvingKey, VerifyingKey, Proof: hex of gnark's
// WriteTo bytes), backend/common.go:86-125 (LoadSRS / SaveSRS: hex(kzg.SRS.WriteTo) re-read from disk on EVERY prove / verify call,
// backend/plonk/plonk.go:16,34,58)].  Encodings are gnark-crypto v0.9.1's ecc/bn254/marshal.go  [UPSTREAM-RECALL]: integers big-endian,
// fr / fp elements 32 B big-endian canonical, points COMPRESSED (G1: X with two flag bits 0b10 / 0b11 = smallest / largest Y, 0b01 =
// infinity), slices prefixed by a u32 big-endian length.
// The point of doing it here: a compressed point costs a square root (one 254-bit exponentiation: y = (x^3 + 3)^((q+1)/4)), 10^6 of
// them per SRS load on the CPU path; on the device the decoded points land directly in the resident-bases layout (and its window tables)
// and the SRS is read ONCE.  Byte / integer work next to ~380 field products per point.
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <vector>

#include "codec_dev.hpp"
#include "ctx.hpp"
#include "ff.hpp"
#include "ff29.hpp"
#include "keyio.hpp"
#include "text_host.hpp"
#include "msm.hpp"
#include "ntt.hpp"
#include "proofio.hpp"

namespace zkmi {

// ---- hex
// one lane: 8 characters -> 4 bytes
__global__ void k_hex_decode(const uint32_t* __restrict__ text, size_t n_words, uint32_t* __restrict__ out, int* __restrict__ status) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_words) return;
    uint32_t bad = 0;
    uint32_t lo = hexdig4(text[2 * i], &bad), hi = hexdig4(text[2 * i + 1], &bad);
    out[i] = lo | (hi << 16);
    if (bad) atomicOr(status, 1);
}
__global__ void k_hex_encode(const uint32_t* __restrict__ bytes, size_t n_words, uint32_t* __restrict__ text) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_words) return;
    uint32_t w = bytes[i];
    text[2 * i] = hexenc2w(w & 0xffffu);
    text[2 * i + 1] = hexenc2w(w >> 16);
}

// ---- 32-byte big-endian fr.Elements
__global__ void k_fr_from_be(const uint32_t* __restrict__ raw, size_t n, Fr* __restrict__ out, int* __restrict__ status) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (!fr_from_be_one(raw + 8 * i, out + i)) atomicOr(status, 2);
}
__global__ void k_fr_to_be(const Fr* __restrict__ in, size_t n, uint32_t* __restrict__ raw) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    fr_to_be_one(in[i], raw + 8 * i);
}

// ---- G1 points
__global__ __launch_bounds__(256) void k_g1_decompress(const uint32_t* __restrict__ raw, size_t n, Affine<Fp>* __restrict__ out, int* __restrict__ status,
                                                     uint8_t* __restrict__ bad) {  // bad (may be null): 1 per invalid encoding
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    g1_decompress_one(raw + 8 * i, out + i, [&] {
        atomicOr(status, 4);
        if (bad) bad[i] = 1;
    });
}
__global__ void k_g1_compress(const Affine<Fp>* __restrict__ pts, size_t n, uint32_t* __restrict__ raw) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Affine<Fp> p = pts[i];
    g1_compress_one(p, raw + 8 * i);
}

// ---- G2 points (a Groth16 proving key holds one per wire)
// [x0] P, the long half of the subgroup test: a kernel of its own under a two-waves-per-SIMD register bound (256 registers and 132 bytes of
// scratch per lane; with the tail in the same kernel: 256 + 140 registers, one wave per SIMD)
__global__ __launch_bounds__(128, 2) void k_g2_x0_mul(const Affine<Fp2>* __restrict__ pts, size_t n, XYZZ<Fp2>* __restrict__ out) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (pts[i].is_inf()) return;
    out[i] = g2_x0_mul_one(pts + i);
}
__global__ __launch_bounds__(128) void k_g2_decompress(const uint32_t* __restrict__ raw, size_t n, Fp2 bt, PsiConsts psi, Affine<Fp2>* __restrict__ out,
                                                       int* __restrict__ status, uint8_t* __restrict__ bad) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    g2_decompress_one(raw + 16 * i, bt, psi.half, out + i, [&] {
        atomicOr(status, 8);
        if (bad) bad[i] = 1;
    });
}
// second half of G2Affine.SetBytes, a kernel of its own (the square root and the subgroup test in one kernel need 512 registers: one wave per SIMD; apart, each
// runs with two or more): a point outside the r-torsion subgroup becomes the point at infinity and sets status bit 16
template <bool FULL>
__global__ __launch_bounds__(128) void k_g2_subgroup(Affine<Fp2>* __restrict__ pts, size_t n, const XYZZ<Fp2>* __restrict__ x0p, PsiConsts psi, int* __restrict__ status,
                                                     uint8_t* __restrict__ bad) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (pts[i].is_inf()) return;
    bool member;
    if (FULL) {  // ZKMI_G2_FULL_SUBGROUP_CHECK=1: the definition, r * P == infinity (A/B switch, four times the work)
        const Affine<Fp2> p = pts[i];
        member = g2_subgroup_full_one(p);
    } else {
        member = g2_subgroup_tail29(pts + i, x0p[i], psi);
    }
    if (!member) {
        atomicOr(status, 16);
        if (bad) bad[i] = 1;
        pts[i] = Affine<Fp2>::inf();
    }
}
// idx == nullptr: point i; else point idx[i] (a key is stored wire-indexed and written without its points at infinity)
__global__ void k_g2_compress(const Affine<Fp2>* __restrict__ pts, const uint32_t* __restrict__ idx, size_t n, uint32_t* __restrict__ raw) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Affine<Fp2> p = pts[idx ? idx[i] : i];
    g2_compress_one(p, raw + 16 * i);
}
__global__ void k_g1_compress_idx(const Affine<Fp>* __restrict__ pts, const uint32_t* __restrict__ idx, size_t n, uint32_t* __restrict__ raw) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Affine<Fp> p = pts[idx[i]];
    g1_compress_one(p, raw + 8 * i);
}
// InfinityA / InfinityB of a wire-indexed array: one byte per point
template <class F>
__global__ void k_inf_flags(const Affine<F>* __restrict__ pts, size_t n, uint8_t* __restrict__ out) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = pts[i].is_inf() ? 1 : 0;
}

static unsigned grid1(size_t n) { return (unsigned)((n + 255) / 256); }

int hex_decode_dev(Slot* s, hipStream_t st, const void* d_text, size_t n_bytes, void* d_out, int* d_status) {
    if (n_bytes & 3) return set_err(ZK_ERR_ARG, "hex payload of %zu bytes is not a multiple of 4", n_bytes);
    if (n_bytes) ZK_LAUNCH(s, st, "hex_decode", k_hex_decode, dim3(grid1(n_bytes / 4)), dim3(256), 0, (const uint32_t*)d_text, n_bytes / 4, (uint32_t*)d_out, d_status);
    return ZK_OK;
}
int hex_encode_dev(Slot* s, hipStream_t st, const void* d_bytes, size_t n_bytes, void* d_text) {
    if (n_bytes & 3) return set_err(ZK_ERR_ARG, "payload of %zu bytes is not a multiple of 4", n_bytes);
    if (n_bytes) ZK_LAUNCH(s, st, "hex_encode", k_hex_encode, dim3(grid1(n_bytes / 4)), dim3(256), 0, (const uint32_t*)d_bytes, n_bytes / 4, (uint32_t*)d_text);
    return ZK_OK;
}
int fr_from_be_dev(Slot* s, hipStream_t st, const void* d_raw, size_t n, void* d_out, int* d_status) {
    if (n) ZK_LAUNCH(s, st, "fr_from_be", k_fr_from_be, dim3(grid1(n)), dim3(256), 0, (const uint32_t*)d_raw, n, (Fr*)d_out, d_status);
    return ZK_OK;
}
int fr_to_be_dev(Slot* s, hipStream_t st, const void* d_in, size_t n, void* d_raw) {
    if (n) ZK_LAUNCH(s, st, "fr_to_be", k_fr_to_be, dim3(grid1(n)), dim3(256), 0, (const Fr*)d_in, n, (uint32_t*)d_raw);
    return ZK_OK;
}
int g1_decompress_dev(Slot* s, hipStream_t st, const void* d_raw, size_t n, void* d_out, int* d_status, uint8_t* d_bad) {
    if (n) ZK_LAUNCH(s, st, "g1_decompress", k_g1_decompress, dim3(grid1(n)), dim3(256), 0, (const uint32_t*)d_raw, n, (Affine<Fp>*)d_out, d_status, d_bad);
    return ZK_OK;
}
int g1_compress_dev(Slot* s, hipStream_t st, const void* d_pts, size_t n, void* d_raw) {
    if (n) ZK_LAUNCH(s, st, "g1_compress", k_g1_compress, dim3(grid1(n)), dim3(256), 0, (const Affine<Fp>*)d_pts, n, (uint32_t*)d_raw);
    return ZK_OK;
}

int g2_decompress_dev(Slot* s, hipStream_t st, const void* d_raw, size_t n, void* d_out, int* d_status, uint8_t* d_bad) {
    const G2CodecConsts K = g2_codec_consts();
    const Fp2 btd = K.bt;
    const PsiConsts psi = K.psi;
    static const int full = ZK_EXP("ZKMI_G2_FULL_SUBGROUP_CHECK", 0);
    if (n) {
        ZK_LAUNCH(s, st, "g2_decompress", k_g2_decompress, dim3((unsigned)((n + 127) / 128)), dim3(128), 0, (const uint32_t*)d_raw, n, btd, psi, (Affine<Fp2>*)d_out, d_status, d_bad);
        const dim3 grid((unsigned)((n + 127) / 128));
        if (full) {
            ZK_LAUNCH(s, st, "g2_subgroup", (k_g2_subgroup<true>), grid, dim3(128), 0, (Affine<Fp2>*)d_out, n, (const XYZZ<Fp2>*)nullptr, psi, d_status, d_bad);
        } else {
            XYZZ<Fp2>* x0p = (XYZZ<Fp2>*)s->alloc(n * sizeof(XYZZ<Fp2>));  // [x0] P of every point, between the two kernels of the test (the caller reserved it: G2_DECOMPRESS_SCRATCH)
            if (!x0p) return set_err(ZK_ERR_ARG, "G2 decompression: the slot's workspace has no room for %zu scratch points", n);
            ZK_LAUNCH(s, st, "g2_x0_mul", k_g2_x0_mul, grid, dim3(128), 0, (const Affine<Fp2>*)d_out, n, x0p);
            ZK_LAUNCH(s, st, "g2_subgroup", (k_g2_subgroup<false>), grid, dim3(128), 0, (Affine<Fp2>*)d_out, n, (const XYZZ<Fp2>*)x0p, psi, d_status, d_bad);
        }
    }
    return ZK_OK;
}
int g2_compress_dev(Slot* s, hipStream_t st, const void* d_pts, const uint32_t* d_idx, size_t n, void* d_raw) {
    if (n) ZK_LAUNCH(s, st, "g2_compress", k_g2_compress, dim3(grid1(n)), dim3(256), 0, (const Affine<Fp2>*)d_pts, d_idx, n, (uint32_t*)d_raw);
    return ZK_OK;
}
int g1_compress_idx_dev(Slot* s, hipStream_t st, const void* d_pts, const uint32_t* d_idx, size_t n, void* d_raw) {
    if (n) ZK_LAUNCH(s, st, "g1_compress", k_g1_compress_idx, dim3(grid1(n)), dim3(256), 0, (const Affine<Fp>*)d_pts, d_idx, n, (uint32_t*)d_raw);
    return ZK_OK;
}
int inf_flags_dev(Slot* s, hipStream_t st, int is_g2, const void* d_pts, size_t n, void* d_out) {
    if (!n) return ZK_OK;
    if (is_g2) ZK_LAUNCH(s, st, "inf_flags", k_inf_flags<Fp2>, dim3(grid1(n)), dim3(256), 0, (const Affine<Fp2>*)d_pts, n, (uint8_t*)d_out);
    else ZK_LAUNCH(s, st, "inf_flags", k_inf_flags<Fp>, dim3(grid1(n)), dim3(256), 0, (const Affine<Fp>*)d_pts, n, (uint8_t*)d_out);
    return ZK_OK;
}

// ---- G2 on the host (two points per SRS); f2_pow: codec_dev.hpp
// square root in Fp2 = Fp[u]/(u^2 + 1), q = 3 mod 4 (Adj & Rodriguez-Henriquez, Alg. 9)
static bool f2_sqrt(const HFp2& a, HFp2* out) {
    if (a.is_zero()) { *out = a; return true; }
    // (q - 3) / 4 and (q - 1) / 2
    static const uint64_t E1[4] = {0x4f082305b61f3f51ULL, 0x65e05aa45a1c72a3ULL, 0x6e14116da0605617ULL, 0x0c19139cb84c680aULL};
    static const uint64_t E2[4] = {0x9e10460b6c3e7ea3ULL, 0xcbc0b548b438e546ULL, 0xdc2822db40c0ac2eULL, 0x183227397098d014ULL};
    const HFp2 minus_one = HFp2{HFp::zero() - HFp::one(), HFp::zero()};
    HFp2 a1 = f2_pow(a, E1);
    HFp2 alpha = a1 * (a1 * a);
    HFp2 a0 = HFp2{alpha.a0, alpha.a1.neg()} * alpha;
    if (a0 == minus_one) return false;
    HFp2 x0 = a1 * a;
    if (alpha == minus_one) {
        *out = HFp2{HFp::zero(), HFp::one()} * x0;
    } else {
        HFp2 b = f2_pow(HFp2::one() + alpha, E2);
        *out = b * x0;
    }
    return out->sqr() == a;
}
static bool fp_lex_largest_host(const HFp& mont) {
    HFp c = mont.from_mont();
    uint64_t h[4];
    for (int i = 0; i < 4; i++) h[i] = (HFpParams::MOD[i] >> 1) | (i < 3 ? HFpParams::MOD[i + 1] << 63 : 0);
    for (int i = 3; i >= 0; i--)
        if (c.l[i] != h[i]) return c.l[i] > h[i];
    return false;
}
static bool fp_from_be(const uint8_t in[32], HFp* out) {
    uint64_t t[4];
    for (int i = 0; i < 4; i++) {
        uint64_t v = 0;
        for (int b = 0; b < 8; b++) v = (v << 8) | in[8 * (3 - i) + b];
        t[i] = v;
    }
    if (HFp::geq_mod(t)) return false;
    *out = HFp{{t[0], t[1], t[2], t[3]}}.to_mont();
    return true;
}
bool g2_decompress_host(const uint8_t in[64], Affine<HFp2>* out) {
    const unsigned flag = in[0] >> 6;
    *out = Affine<HFp2>::inf();
    if (flag == 1) {  // infinity: canonical only -- every other bit zero, as g1_decompress_host and gnark-crypto's SetBytes require
        if (in[0] & 0x3f) return false;
        for (int i = 1; i < 64; i++)
            if (in[i]) return false;
        return true;
    }
    if (flag == 0) return false;
    uint8_t b[64];
    memcpy(b, in, 64);
    b[0] &= 0x3f;
    HFp2 x;
    if (!fp_from_be(b, &x.a1) || !fp_from_be(b + 32, &x.a0)) return false;
    // twist: y^2 = x^3 + 3 / (9 + u)
    HFp nine = HFp::zero(), three = HFp::one() + HFp::one() + HFp::one();
    for (int i = 0; i < 3; i++) nine = nine + three;
    HFp2 bt = HFp2{three, HFp::zero()} * HFp2{nine, HFp::one()}.inv();
    HFp2 rhs = x.sqr() * x + bt, y;
    if (!f2_sqrt(rhs, &y)) return false;
    bool largest = y.a1.is_zero() ? fp_lex_largest_host(y.a0) : fp_lex_largest_host(y.a1);
    if (largest != (flag == 3)) y = y.neg();
    out->x = x;
    out->y = y;
    // subgroup check: r * P == infinity (G2 has a cofactor)
    uint32_t rk[8];
    memcpy(rk, HFrParams::MOD, 32);
    return scalar_mul(*out, rk).is_inf();
}

}  // namespace zkmi

using namespace zkmi;

extern "C" {

// kzg.SRS.ReadFrom on the bytes (or their hex text) of kzg.SRS.WriteTo: G2[0] | G2[1] (64 B compressed each) | u32 BE count | count x 32 B
// compressed G1.  The G1 points are decompressed on the device and registered as resident bases (window tables per table_window_bits as in
// zk_bn254_bases_register_cfg); handle / n_g1 / the two G2 points come back.  This is what replaces LoadSRS (backend/common.go:86-105).
int zk_bn254_kzg_srs_read(const void* data, size_t len, int is_hex, int table_window_bits, uint64_t* handle, size_t* n_g1, zk_g2_affine g2_out[2]) {
    if (!data || !handle) return set_err(ZK_ERR_ARG, "null pointer");
    SrsHeader H;  // the count and the total length are settled on the host, from the caller's bytes alone (text_host.hpp), before anything is sized by them
    {
        std::string e;
        const int rc = kzg_srs_header(data, len, is_hex, &H, &e);
        if (rc != ZK_OK) return set_err(rc, "%s", e.c_str());
    }
    const size_t nbytes = H.nbytes, n = H.n_g1;
    const uint8_t* head = H.g2;
    SlotGuard g;
    ZK_TRY(acquire_slot(&g.s));
    Slot* s = g.s;
    hipStream_t st = s->stream;
    ZK_TRY(s->reserve(len + nbytes + 2 * nbytes + 65536));
    int* d_status = (int*)s->alloc(64);
    ZK_HIP(hipMemsetAsync(d_status, 0, 4, st));
    uint8_t* d_bytes = (uint8_t*)s->alloc(nbytes + 16);
    if (is_hex) {
        void* d_text = s->alloc(len + 16);
        ZK_TRY(h2d_big(d_text, data, len, st));
        ZK_TRY(hex_decode_dev(s, st, d_text, nbytes, d_bytes, d_status));
    } else {
        ZK_TRY(h2d_big(d_bytes, data, nbytes, st));
    }
    Affine<HFp2> g2[2];
    for (int k = 0; k < 2; k++)
        if (!g2_decompress_host(head + 64 * k, &g2[k])) return set_err(ZK_ERR_ARG, "SRS: invalid G2 point %d", k);
    void* d_pts = s->alloc(n * 64 + 16);
    ZK_TRY(g1_decompress_dev(s, st, d_bytes + 132, n, d_pts, d_status));
    int h_status = 0;
    ZK_HIP(hipMemcpyAsync(&h_status, d_status, 4, hipMemcpyDeviceToHost, st));
    ZK_TRY(slot_sync(s, st));
    if (h_status & 1) return set_err(ZK_ERR_ARG, "SRS: invalid hex character");
    if (h_status & 4) return set_err(ZK_ERR_ARG, "SRS: invalid compressed G1 point (bad flags, x >= q, or no square root)");
    ZK_TRY(zk_bn254_bases_register_cfg(d_pts, n, 0, 1, table_window_bits, handle));
    if (n_g1) *n_g1 = n;
    if (g2_out) memcpy(g2_out, g2, 256);
    return ZK_OK;
}

// The two G2 points of an SRS image and nothing else: what plonk.Verify takes from the SRS (kzg.Verify's pairing check).  Host only -- no device is
// touched, so a process that only verifies (nargo verify) never starts the HIP runtime.  The header and the length are checked as in _read; the G1 points are not looked at.
int zk_bn254_kzg_srs_g2(const void* data, size_t len, int is_hex, zk_g2_affine g2_out[2]) {
    if (!data || !g2_out) return set_err(ZK_ERR_ARG, "null pointer");
    SrsHeader H;
    {
        std::string e;
        const int rc = kzg_srs_header(data, len, is_hex, &H, &e);
        if (rc != ZK_OK) return set_err(rc, "%s", e.c_str());
    }
    Affine<HFp2> g2[2];
    for (int k = 0; k < 2; k++)
        if (!g2_decompress_host(H.g2 + 64 * k, &g2[k])) return set_err(ZK_ERR_ARG, "SRS: invalid G2 point %d", k);
    memcpy(g2_out, g2, 256);
    return ZK_OK;
}

// kzg.SRS.WriteTo of a registered G1 base array + the two G2 points: bytes (or hex text) into out; *out_len = bytes written.
int zk_bn254_kzg_srs_write(uint64_t handle, const zk_g2_affine g2[2], int as_hex, void* out, size_t cap, size_t* out_len) {
    ZK_ON_ENTRY_OF(handle);
    if (!g2 || !out || !out_len) return set_err(ZK_ERR_ARG, "null pointer");
    const void* d_pts = nullptr;
    size_t n = 0;
    int is_g2 = 0;
    ZK_TRY(bases_ptr(handle, &d_pts, &n, &is_g2));
    if (is_g2) return set_err(ZK_ERR_ARG, "the SRS handle must be a G1 base array");
    const size_t nbytes = 132 + 32 * n, need = as_hex ? 2 * nbytes : nbytes;
    *out_len = need;
    if (cap < need) return set_err(ZK_ERR_ARG, "output holds %zu bytes, %zu needed", cap, need);
    SlotGuard g;
    ZK_TRY(acquire_slot(&g.s));
    Slot* s = g.s;
    hipStream_t st = s->stream;
    ZK_TRY(s->reserve(3 * nbytes + 65536));
    uint8_t* d_bytes = (uint8_t*)s->alloc(nbytes + 16);
    uint8_t head[132];
    Affine<HFp2> gg[2];
    memcpy(gg, g2, 256);
    // G2Affine.Bytes(): X.A1 | X.A0 big-endian, flags on the first byte
    for (int k = 0; k < 2; k++) {
        uint8_t* o = head + 64 * k;
        if (gg[k].is_inf()) { memset(o, 0, 64); o[0] = 0x40; continue; }
        for (int half = 0; half < 2; half++) {
            HFp c = (half ? gg[k].x.a0 : gg[k].x.a1).from_mont();
            for (int i = 0; i < 4; i++)
                for (int b = 0; b < 8; b++) o[32 * half + 31 - (8 * i + b)] = (uint8_t)(c.l[i] >> (8 * b));
        }
        bool largest = gg[k].y.a1.is_zero() ? fp_lex_largest_host(gg[k].y.a0) : fp_lex_largest_host(gg[k].y.a1);
        o[0] |= largest ? 0xC0 : 0x80;
    }
    head[128] = (uint8_t)(n >> 24); head[129] = (uint8_t)(n >> 16); head[130] = (uint8_t)(n >> 8); head[131] = (uint8_t)n;
    ZK_HIP(hipMemcpyAsync(d_bytes, head, 132, hipMemcpyHostToDevice, st));
    ZK_TRY(g1_compress_dev(s, st, d_pts, n, d_bytes + 132));
    if (as_hex) {
        void* d_text = s->alloc(2 * nbytes + 16);
        ZK_TRY(hex_encode_dev(s, st, d_bytes, nbytes, d_text));
        ZK_HIP(hipMemcpyAsync(out, d_text, 2 * nbytes, hipMemcpyDeviceToHost, st));
    } else {
        ZK_HIP(hipMemcpyAsync(out, d_bytes, nbytes, hipMemcpyDeviceToHost, st));
    }
    return slot_sync(s, st);
}

// ---- Groth16 keys (gnark v0.8.0 internal/backend/bn254/groth16/marshal.go  [UPSTREAM-RECALL]) -- what the reference's intended Groth16 FFI moves as hex:
// ProveWithPK(rawR1CS, encodedProvingKey) -> provingKey.ReadFrom  [REF gnark_backend_ffi/backend/groth16/r1cs.go:107-143], Preprocess -> both keys
// out [REF r1cs.go:214-266].  ProvingKey.WriteTo (compressed):
//   Domain.WriteTo 168 B | G1.Alpha, G1.Beta, G1.Delta 3 x 32 | G1.A, G1.B, G1.Z, G1.K each u32 count + 32 B per point | G2.Beta, G2.Delta 2 x 64
//   | G2.B u32 count + 64 B per point | nbWires u64 | NbInfinityA u64 | NbInfinityB u64 | InfinityA, InfinityB: nbWires bytes (0 / 1) each, no prefix
// A, B, G2.B are stored WITHOUT their points at infinity (that is what the bitmaps are for); the public-wire count is nbWires - len(K).
namespace {
void put_be(uint8_t* o, uint64_t v, int n) { for (int i = 0; i < n; i++) o[i] = (uint8_t)(v >> (8 * (n - 1 - i))); }
void domain_bytes(const Domain* d, uint8_t o[168]) {
    put_be(o, (uint64_t)1 << d->logn, 8);
    fr_to_be(d->card_inv, o + 8);
    fr_to_be(d->gen, o + 40);
    fr_to_be(d->gen_inv, o + 72);
    fr_to_be(d->coset, o + 104);
    fr_to_be(d->coset_inv, o + 136);
}
struct DevFree {
    std::vector<void*> ptrs;
    bool keep = false;
    int alloc(void** d, size_t bytes) {
        ZK_HIP(hipMalloc(d, bytes ? bytes : 16));
        ptrs.push_back(*d);
        return ZK_OK;
    }
    ~DevFree() { if (!keep) for (void* q : ptrs) (void)hipFree(q); }
};
}  // namespace

// groth16.ProvingKey.ReadFrom on the bytes (or hex text) of ProvingKey.WriteTo: every point is decompressed on the device (G1: one square root; G2:
// an Fp2 square root and the subgroup check), A / B / G2.B are expanded to the wire-indexed resident layout and the window tables are built as in
// zk_bn254_groth16_pk_load.  flags: bit 0 of zk_groth16_pk.flags (no window tables); table_window_bits as there.
int zk_bn254_groth16_pk_read(const void* data, size_t len, int is_hex, int flags, int table_window_bits, uint64_t* handle) {
    if (!data || !handle) return set_err(ZK_ERR_ARG, "null pointer");
    if (flags & ~1) return set_err(ZK_ERR_ARG, "only flag bit 0 (no window tables) applies to a key read from its wire format");
    struct Lap {
        std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
        void lap(const char* name) {
            const auto t1 = std::chrono::steady_clock::now();
            prof_host(name, std::chrono::duration<double, std::milli>(t1 - t0).count());
            t0 = t1;
        }
    } lap;
    Groth16KeyHeader H;  // the section table, the counts and the two bitmaps: read and cross-checked on the host from the caller's bytes alone (text_host.hpp)
    {
        std::string e;
        const int rc = groth16_pk_header(data, len, is_hex, &H, &e);
        if (rc != ZK_OK) return set_err(rc, "%s", e.c_str());
    }
    lap.lap("export.pk_read_header_host");
    const unsigned logN = H.logN;
    const size_t* cnt = H.cnt;
    const size_t* at = H.at;
    const size_t at_g2 = H.at_g2, at_bm = H.at_bitmaps;
    const uint64_t nw = H.n_wires, nia = H.nb_inf_a, nib = H.nb_inf_b;
    const std::vector<uint8_t>&ia = H.inf_a, &ib = H.inf_b;
    const uint8_t* dom_in = H.domain;
    uint8_t dom_ok[168];

    // two slots: the first one's stream carries the uploads (and its arena the text), the second one's the decompression -- two ORDINARY streams, because a lean
    // process (the export shim's) has no high-priority stream yet and hi() would hand back the slot's own: upload and decompression would take turns
    SlotsGuard<2> g;
    ZK_TRY(acquire_slots(2, g.s));
    Slot* s = g.s[0];
    hipStream_t st = s->stream;
    Domain* dom;
    ZK_TRY(get_domain(s, st, logN, 0, &dom));
    domain_bytes(dom, dom_ok);
    if (memcmp(dom_in, dom_ok, 168)) return set_err(ZK_ERR_ARG, "proving key: the domain is not gnark-crypto's radix-2 domain of that size");
    lap.lap("export.pk_read_header_domain");
    // Everything up to the bitmaps goes to the device (every section starts at a multiple of 4 bytes by construction) -- G2.B FIRST: its points are the expensive
    // ones to decompress (an Fp2 square root and the subgroup test each), so their kernel runs on the slot's second stream while the other 0.24 GB of a
    // 2^20-constraint key's text are still crossing PCIe on the first (round 5: 41 + 17 + 68 ms one after the other before).
    lap.lap("export.pk_read_slot");
    ZK_TRY(s->reserve((is_hex ? 2 * at_bm : 0) + at_bm + (cnt[4] + 2) * G2_DECOMPRESS_SCRATCH + 8 * 4096));
    lap.lap("export.pk_read_reserve");
    int* d_status = (int*)s->alloc(64);
    uint8_t* d_bytes = (uint8_t*)s->alloc(at_bm + 16);
    uint8_t* d_text = is_hex ? (uint8_t*)s->alloc(2 * at_bm + 16) : nullptr;
    hipStream_t sx = g.s[1]->stream;  // decompression
    ZK_HIP(hipMemsetAsync(d_status, 0, 4, st));
    auto upload = [&](size_t from, size_t to) -> int {  // bytes [from, to) of the key image -> d_bytes, on `st`
        if (to <= from) return ZK_OK;
        if (is_hex) {
            ZK_TRY(h2d_big(d_text + 2 * from, (const char*)data + 2 * from, 2 * (to - from), st));
            ZK_TRY(hex_decode_dev(s, st, d_text + 2 * from, to - from, d_bytes + from, d_status));
        } else {
            ZK_TRY(h2d_big(d_bytes + from, (const char*)data + from, to - from, st));
        }
        return ZK_OK;
    };
    hipEvent_t ev_g2 = nullptr, ev_rest = nullptr;
    struct Ev { hipEvent_t* e[2]; ~Ev() { for (auto p : e) if (*p) (void)hipEventDestroy(*p); } } ev_guard{{&ev_g2, &ev_rest}};
    ZK_HIP(hipEventCreateWithFlags(&ev_g2, hipEventDisableTiming));
    ZK_HIP(hipEventCreateWithFlags(&ev_rest, hipEventDisableTiming));
    DevFree tmp, own;  // tmp: the compact A / B / G2.B and the five single points; own: K and Z, adopted by the key
    void *d_a = nullptr, *d_b = nullptr, *d_b2 = nullptr, *d_k = nullptr, *d_z = nullptr, *d_single = nullptr;
    ZK_TRY(tmp.alloc(&d_a, cnt[0] * 64));
    ZK_TRY(tmp.alloc(&d_b, cnt[1] * 64));
    ZK_TRY(tmp.alloc(&d_b2, cnt[4] * 128));
    ZK_TRY(tmp.alloc(&d_single, 3 * 64 + 2 * 128));
    ZK_TRY(own.alloc(&d_z, cnt[2] * 64));
    ZK_TRY(own.alloc(&d_k, cnt[3] * 64));
    const size_t g2_end = at[4] + cnt[4] * 64;
    lap.lap("export.pk_read_allocs");
    {   // in quarters: the first points are being decompressed while the last ones are still on their way (an event may be re-recorded once the wait on its
        // previous recording has been enqueued)
        const size_t parts = cnt[4] >= ((size_t)1 << 16) ? 4 : 1, per = (cnt[4] + parts - 1) / parts;
        for (size_t q = 0; q < parts; q++) {
            const size_t p0 = q * per, p1 = p0 + per < cnt[4] ? p0 + per : cnt[4];
            if (p1 <= p0) break;
            ZK_TRY(upload(at[4] + p0 * 64, at[4] + p1 * 64));
            ZK_HIP(hipEventRecord(ev_g2, st));
            ZK_HIP(hipStreamWaitEvent(sx, ev_g2, 0));
            ZK_TRY(g2_decompress_dev(s, sx, d_bytes + at[4] + p0 * 64, p1 - p0, (uint8_t*)d_b2 + p0 * 128, d_status));
        }
    }
    lap.lap("export.pk_read_upload_g2_part");
    ZK_TRY(upload(0, at[4]));
    ZK_TRY(upload(g2_end, at_bm));
    ZK_HIP(hipEventRecord(ev_rest, st));
    ZK_HIP(hipStreamWaitEvent(sx, ev_rest, 0));
    lap.lap("export.pk_read_upload_rest");
    ZK_TRY(g1_decompress_dev(s, sx, d_bytes + 168, 3, d_single, d_status));
    ZK_TRY(g2_decompress_dev(s, sx, d_bytes + at_g2, 2, (uint8_t*)d_single + 192, d_status));
    void* g1_dst[4] = {d_a, d_b, d_z, d_k};
    for (int k = 0; k < 4; k++) ZK_TRY(g1_decompress_dev(s, sx, d_bytes + at[k], cnt[k], g1_dst[k], d_status));
    st = sx;  // the results are read back behind the decompression
    uint8_t single[3 * 64 + 2 * 128];
    int h_status = 0;
    ZK_HIP(hipMemcpyAsync(single, d_single, sizeof single, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipMemcpyAsync(&h_status, d_status, 4, hipMemcpyDeviceToHost, st));
    ZK_TRY(slot_sync(s, st));
    lap.lap("export.pk_read_decompress_wait");
    if (h_status & 1) return set_err(ZK_ERR_ARG, "proving key: invalid hex character");
    if (h_status & 4) return set_err(ZK_ERR_ARG, "proving key: invalid compressed G1 point (bad flags, x >= q, or no square root)");
    if (h_status & 8) return set_err(ZK_ERR_ARG, "proving key: invalid compressed G2 point (bad flags, coordinate >= q, or no square root)");
    if (h_status & 16) return set_err(ZK_ERR_ARG, "proving key: a G2 point outside the r-torsion subgroup");
    s->reset();
    for (int i = 0; i < 2; i++) {  // pk_load takes slots of its own
        release_slot(g.s[i]);
        g.s[i] = nullptr;
    }
    zk_groth16_pk pk;
    memset(&pk, 0, sizeof pk);
    pk.log_domain = logN;
    pk.n_wires = nw;
    pk.n_public = nw - cnt[3];
    pk.g1_alpha = (const zk_g1_affine*)single;
    pk.g1_beta = (const zk_g1_affine*)(single + 64);
    pk.g1_delta = (const zk_g1_affine*)(single + 128);
    pk.g2_beta = (const zk_g2_affine*)(single + 192);
    pk.g2_delta = (const zk_g2_affine*)(single + 320);
    pk.g1_a = (const zk_g1_affine*)d_a;
    pk.g1_b = (const zk_g1_affine*)d_b;
    pk.g1_k = (const zk_g1_affine*)d_k;
    pk.g1_z = (const zk_g1_affine*)d_z;
    pk.g2_b = (const zk_g2_affine*)d_b2;
    pk.bases_on_device = 1;
    pk.flags = flags;
    pk.infinity_a = ia.data();
    pk.infinity_b = ib.data();
    pk.nb_infinity_a = nia;
    pk.nb_infinity_b = nib;
    pk.table_window_bits = table_window_bits;
    ZK_TRY(zk_bn254_groth16_pk_load(&pk, handle));
    lap.lap("export.pk_read_load");
    ZK_TRY(groth16_pk_adopt(*handle));  // K and Z were allocated here for the key; A / B / G2.B are its own expanded arrays already
    own.keep = true;
    return ZK_OK;
}

// groth16.ProvingKey.WriteTo of a resident key: bytes (or hex text) into out; *out_len = bytes needed / written (out == NULL: size query).
int zk_bn254_groth16_pk_write(uint64_t handle, int as_hex, void* out, size_t cap, size_t* out_len) {
    ZK_ON_ENTRY_OF(handle);
    if (!out_len) return set_err(ZK_ERR_ARG, "null pointer");
    Groth16View v;
    ZK_TRY(groth16_pk_view(handle, &v));
    const size_t N = (size_t)1 << v.log_domain, nw = v.n_wires, nk = nw - v.n_public;
    if (v.nz != N - 1 && N > 1) return set_err(ZK_ERR_ARG, "a range-sharded slice of a key has no gnark wire format");
    SlotGuard g;
    ZK_TRY(acquire_slot(&g.s));
    Slot* s = g.s;
    hipStream_t st = s->stream;
    // InfinityA / InfinityB from the wire-indexed arrays
    ZK_TRY(s->reserve(2 * nw + 4096));
    uint8_t* d_flags = (uint8_t*)s->alloc(2 * nw + 16);
    std::vector<uint8_t> ia(nw ? nw : 1), ib(nw ? nw : 1);
    ZK_TRY(inf_flags_dev(s, st, 0, v.d_a, nw, d_flags));
    ZK_TRY(inf_flags_dev(s, st, 0, v.d_b, nw, d_flags + nw));
    if (nw) {
        ZK_HIP(hipMemcpyAsync(ia.data(), d_flags, nw, hipMemcpyDeviceToHost, st));
        ZK_HIP(hipMemcpyAsync(ib.data(), d_flags + nw, nw, hipMemcpyDeviceToHost, st));
    }
    ZK_TRY(slot_sync(s, st));
    std::vector<uint32_t> idx_a, idx_b;
    for (size_t i = 0; i < nw; i++) {
        if (!ia[i]) idx_a.push_back((uint32_t)i);
        if (!ib[i]) idx_b.push_back((uint32_t)i);
    }
    const size_t na = idx_a.size(), nb = idx_b.size();
    const size_t at_a = 168 + 96 + 4, at_b = at_a + 32 * na + 4, at_z = at_b + 32 * nb + 4, at_k = at_z + 32 * N + 4, at_g2 = at_k + 32 * nk, at_b2 = at_g2 + 128 + 4,
                 at_cnt = at_b2 + 64 * nb, at_bm = at_cnt + 24, nbytes = at_bm + 2 * nw, need = as_hex ? 2 * nbytes : nbytes;
    *out_len = need;
    if (!out) return ZK_OK;
    if (cap < need) return set_err(ZK_ERR_ARG, "output holds %zu bytes, %zu needed", cap, need);
    s->reset();
    const size_t padded = align_up(nbytes, 4);
    ZK_TRY(s->reserve(3 * padded + 4 * (na + nb) + 65536));
    uint8_t* d_bytes = (uint8_t*)s->alloc(padded + 16);
    uint32_t* d_ia = (uint32_t*)s->alloc(4 * na + 16);
    uint32_t* d_ib = (uint32_t*)s->alloc(4 * nb + 16);
    if (na) ZK_HIP(hipMemcpyAsync(d_ia, idx_a.data(), 4 * na, hipMemcpyHostToDevice, st));
    if (nb) ZK_HIP(hipMemcpyAsync(d_ib, idx_b.data(), 4 * nb, hipMemcpyHostToDevice, st));
    ZK_HIP(hipMemsetAsync(d_bytes + (padded - 4), 0, 4, st));
    // host-built pieces: the head (domain, three G1 points, count of A), the counts, the two G2 points, the trailer
    Domain* dom;
    ZK_TRY(get_domain(s, st, v.log_domain, 0, &dom));
    std::vector<uint8_t> head(at_a), mid(128 + 4), trailer(24 + 2 * nw);
    domain_bytes(dom, head.data());
    g1_compress(v.alpha, head.data() + 168);
    g1_compress(v.beta, head.data() + 200);
    g1_compress(v.delta, head.data() + 232);
    put_be(head.data() + 264, na, 4);
    uint8_t c_b[4], c_z[4], c_k[4];
    put_be(c_b, nb, 4);
    put_be(c_z, N, 4);
    put_be(c_k, nk, 4);
    g2_compress(v.beta2, mid.data());
    g2_compress(v.delta2, mid.data() + 64);
    put_be(mid.data() + 128, nb, 4);
    put_be(trailer.data(), nw, 8);
    put_be(trailer.data() + 8, nw - na, 8);
    put_be(trailer.data() + 16, nw - nb, 8);
    if (nw) {
        memcpy(trailer.data() + 24, ia.data(), nw);
        memcpy(trailer.data() + 24 + nw, ib.data(), nw);
    }
    ZK_HIP(hipMemcpyAsync(d_bytes, head.data(), at_a, hipMemcpyHostToDevice, st));
    ZK_HIP(hipMemcpyAsync(d_bytes + at_b - 4, c_b, 4, hipMemcpyHostToDevice, st));
    ZK_HIP(hipMemcpyAsync(d_bytes + at_z - 4, c_z, 4, hipMemcpyHostToDevice, st));
    ZK_HIP(hipMemcpyAsync(d_bytes + at_k - 4, c_k, 4, hipMemcpyHostToDevice, st));
    ZK_HIP(hipMemcpyAsync(d_bytes + at_g2, mid.data(), 132, hipMemcpyHostToDevice, st));
    ZK_HIP(hipMemcpyAsync(d_bytes + at_cnt, trailer.data(), trailer.size(), hipMemcpyHostToDevice, st));
    ZK_TRY(g1_compress_idx_dev(s, st, v.d_a, d_ia, na, d_bytes + at_a));
    ZK_TRY(g1_compress_idx_dev(s, st, v.d_b, d_ib, nb, d_bytes + at_b));
    ZK_TRY(g1_compress_dev(s, st, v.d_z, N, d_bytes + at_z));
    ZK_TRY(g1_compress_dev(s, st, v.d_k, nk, d_bytes + at_k));
    ZK_TRY(g2_compress_dev(s, st, v.d_b2, d_ib, nb, d_bytes + at_b2));
    if (as_hex) {
        void* d_text = s->alloc(2 * padded + 16);
        ZK_TRY(hex_encode_dev(s, st, d_bytes, padded, d_text));
        ZK_HIP(hipMemcpyAsync(out, d_text, 2 * nbytes, hipMemcpyDeviceToHost, st));
    } else {
        ZK_HIP(hipMemcpyAsync(out, d_bytes, nbytes, hipMemcpyDeviceToHost, st));
    }
    return slot_sync(s, st);  // the host staging vectors live until here
}

// groth16.VerifyingKey.WriteTo (compressed): [alpha]1, [beta]1, [beta]2, [gamma]2, [delta]1, [delta]2, u32 len(K), K  -- from what
// zk_bn254_groth16_setup returns (vk_g1 = [alpha]1 then the n_k = n_public points K; vk_g2 = [beta]2, [gamma]2, [delta]2) and the resident
// proving key ([beta]1, [delta]1).  Host only: 292 + 32 * n_k bytes.
int zk_bn254_groth16_vk_write(uint64_t pk_handle, const zk_g1_affine* vk_g1, size_t n_k, const zk_g2_affine vk_g2[3], int as_hex, void* out, size_t cap,
                              size_t* out_len) {
    ZK_ON_ENTRY_OF(pk_handle);
    if (!vk_g1 || !vk_g2 || !out_len) return set_err(ZK_ERR_ARG, "null pointer");
    Groth16View v;
    ZK_TRY(groth16_pk_view(pk_handle, &v));
    if (n_k != v.n_public) return set_err(ZK_ERR_LEN, "verifying key: %zu K points, the key has %zu public wires", n_k, v.n_public);
    const size_t nbytes = 292 + 32 * n_k, need = as_hex ? 2 * nbytes : nbytes;
    *out_len = need;
    if (!out) return ZK_OK;
    if (cap < need) return set_err(ZK_ERR_ARG, "output holds %zu bytes, %zu needed", cap, need);
    std::vector<uint8_t> b(nbytes);
    const Affine<HFp>* g1 = (const Affine<HFp>*)vk_g1;
    const Affine<HFp2>* g2 = (const Affine<HFp2>*)vk_g2;
    g1_compress(g1[0], b.data());
    g1_compress(v.beta, b.data() + 32);
    g2_compress(g2[0], b.data() + 64);
    g2_compress(g2[1], b.data() + 128);
    g1_compress(v.delta, b.data() + 192);
    g2_compress(g2[2], b.data() + 224);
    put_be(b.data() + 288, n_k, 4);
    for (size_t i = 0; i < n_k; i++) g1_compress(g1[1 + i], b.data() + 292 + 32 * i);
    if (!as_hex) { memcpy(out, b.data(), nbytes); return ZK_OK; }
    static const char* dg = "0123456789abcdef";
    char* o = (char*)out;
    for (size_t i = 0; i < nbytes; i++) { o[2 * i] = dg[b[i] >> 4]; o[2 * i + 1] = dg[b[i] & 15]; }
    return ZK_OK;
}


}  // extern "C"
