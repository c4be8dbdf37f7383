// SHA-256 (FIPS 180-4) for one lane: the same digests as proofio.hpp's Sha256, written so that the whole state stays in registers on the device.
// The message block is a 16-word shift register (no dynamically indexed array): bytes gather into a word, every fourth byte shifts the word in, every
// 64th compresses.  Every byte goes through put_byte, so each inlined update / put256 / final holds one copy of the compression.
#pragma once
#include <stdint.h>

#include "ff.hpp"

namespace zkmi {

struct Sha256Dev {
    uint32_t h[8];
    uint32_t w[16];
    uint32_t cur;
    uint64_t len;  // bytes absorbed

    ZK_HD void reset() {
        const uint32_t iv[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
#pragma unroll
        for (int i = 0; i < 8; i++) h[i] = iv[i];
        cur = 0;
        len = 0;
    }
    // continue from a midstate: the chaining value after `bytes` (a multiple of 64) bytes
    ZK_HD void resume(const uint32_t mid[8], uint64_t bytes) {
#pragma unroll
        for (int i = 0; i < 8; i++) h[i] = mid[i];
        cur = 0;
        len = bytes;
    }
    static ZK_HD uint32_t rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
    ZK_HD void compress() {
        const uint32_t K[64] = {
            0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be, 0x550c7dc3,
            0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da,
            0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, 0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13,
            0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070,
            0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208,
            0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};
        uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
#pragma unroll
        for (int i = 0; i < 64; i++) {
            if (i >= 16) {  // the schedule in place: w[i & 15] becomes W_i
                const uint32_t w15 = w[(i - 15) & 15], w2 = w[(i - 2) & 15];
                w[i & 15] += (rotr(w15, 7) ^ rotr(w15, 18) ^ (w15 >> 3)) + w[(i - 7) & 15] + (rotr(w2, 17) ^ rotr(w2, 19) ^ (w2 >> 10));
            }
            const uint32_t S1 = rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25), ch = (e & f) ^ (~e & g), t1 = hh + S1 + ch + K[i] + w[i & 15];
            const uint32_t S0 = rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22), mj = (a & b) ^ (a & c) ^ (b & c), t2 = S0 + mj;
            hh = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
        }
        h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
    }
    ZK_HD void put_byte(uint32_t byte) {
        cur = (cur << 8) | (byte & 0xff);
        len++;
        if ((len & 3) == 0) {
#pragma unroll
            for (int i = 0; i < 15; i++) w[i] = w[i + 1];
            w[15] = cur;
            cur = 0;
            if ((len & 63) == 0) compress();
        }
    }
    ZK_HD void update(const uint8_t* p, size_t n) {
#pragma unroll 1
        for (size_t i = 0; i < n; i++) put_byte(p[i]);
    }
    // a 256-bit integer given as 8 x u32 little-endian limbs, bound as its 32 big-endian bytes
    ZK_HD void put256(const uint32_t l[8]) {
        uint32_t t[8];
#pragma unroll
        for (int i = 0; i < 8; i++) t[i] = l[i];
        uint32_t x = t[7];
#pragma unroll 1
        for (int k = 0; k < 32; k++) {
            put_byte(x >> 24);
            x <<= 8;
            if ((k & 3) == 3) {  // next limb down
#pragma unroll
                for (int i = 7; i > 0; i--) t[i] = t[i - 1];
                x = t[7];
            }
        }
    }
    // the digest as 8 big-endian words (out[0] holds bytes 0..3)
    ZK_HD void final(uint32_t out[8]) {
        const uint64_t bits = len * 8;
        const uint32_t zeros = (uint32_t)((55 - (len & 63)) & 63), total = 1 + zeros + 8;
#pragma unroll 1
        for (uint32_t k = 0; k < total; k++) put_byte(k == 0 ? 0x80u : k <= zeros ? 0u : (uint32_t)(bits >> (8 * (total - 1 - k))));
#pragma unroll
        for (int i = 0; i < 8; i++) out[i] = h[i];
    }
};

// digest words -> the 256-bit big-endian integer they spell, as 8 x u32 little-endian limbs
ZK_HD void sha_words_to_limbs(const uint32_t d[8], uint32_t l[8]) {
#pragma unroll
    for (int i = 0; i < 8; i++) l[i] = d[7 - i];
}

// The coefficient rule of the batch verifiers (include/zkmi.h: r_i, rho_i, lambda_i): the low 128 bits of a digest read as a big-endian integer, forced
// non-zero.  l: that integer as limbs (sha_words_to_limbs on the device, the digest bytes read backwards on the host); out: the coefficient's four limbs
ZK_HD void batch_coeff(const uint32_t l[8], uint32_t out[4]) {
#pragma unroll
    for (int i = 0; i < 4; i++) out[i] = l[i];
    if ((out[0] | out[1] | out[2] | out[3]) == 0) out[0] = 1;
}

}  // namespace zkmi
