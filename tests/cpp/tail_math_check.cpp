// The arithmetic of the device proof tail (csrc/groth16_tail.hpp) run on the HOST, row by row in the order the kernel's four roles and its combine step use,
// against expectations computed elsewhere (tests/test_groth16_tail_cases_cpu.py writes the file: the pure-python bytes of tests/groth16_tail_cases.py).
// File: u64 n_rows, u64 n_partials | alpha, beta, delta (64 B each), beta2, delta2 (128 B each) | per row: n_partials x 768 B, r, s (32 B each), 128 B expected.
// Built as host code only; prints "ok <rows>" or the first mismatch.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "groth16_tail.hpp"
#include "host_ff.hpp"
#include "proofio.hpp"

using namespace zkmi;

template <class F>
static std::vector<Affine<F>> window_table(const Affine<F>& p) {  // [w * 255 + d - 1] = d * 2^(8w) * p, as fixed_base_table lays it out
    std::vector<XYZZ<F>> pts(32 * 255);
    XYZZ<F> base = XYZZ<F>::from_affine(p);
    for (int w = 0; w < 32; w++) {
        XYZZ<F> acc = XYZZ<F>::inf();
        for (int d = 1; d < 256; d++) {
            acc.add(base);
            pts[w * 255 + d - 1] = acc;
        }
        for (int i = 0; i < 8; i++) base.dbl();
    }
    // one inversion for all of them (no entry is the point at infinity: d * 2^(8w) < r)
    std::vector<F> pre(pts.size());
    F run = F::one();
    for (size_t i = 0; i < pts.size(); i++) {
        pre[i] = run;
        run = run * (pts[i].zz * pts[i].zzz);
    }
    F inv = run.inv();
    std::vector<Affine<F>> t(pts.size());
    for (size_t i = pts.size(); i-- > 0;) {
        const F zi = inv * pre[i];
        inv = inv * (pts[i].zz * pts[i].zzz);
        t[i] = Affine<F>{pts[i].x * (zi * pts[i].zzz), pts[i].y * (zi * pts[i].zz)};
    }
    return t;
}

static void tail_row(const TailKey& K, const uint64_t* rec, size_t n_partials, const Fr& r, const Fr& s, uint8_t out[128]) {
    // role 0 / 1
    XYZZ<Fp> a_alpha = tail_sum<Fp>(rec, n_partials, 0);
    a_alpha.madd(K.alpha.x, K.alpha.y);
    const XYZZ<Fp> s_a = tail_scaled(a_alpha, s);
    XYZZ<Fp> b_beta = tail_sum<Fp>(rec, n_partials, 16);
    b_beta.madd(K.beta.x, K.beta.y);
    const XYZZ<Fp> r_b = tail_scaled(b_beta, r);
    // role 2
    XYZZ<Fp2> bs = tail_sum<Fp2>(rec, n_partials, 64);
    bs.madd(K.beta2.x, K.beta2.y);
    tail_fixed_add(bs, K.t_delta2, s.from_mont());
    // role 3
    XYZZ<Fp> kz = tail_sum<Fp>(rec, n_partials, 32);
    kz.add(tail_sum<Fp>(rec, n_partials, 48));
    XYZZ<Fp> rd = XYZZ<Fp>::inf();
    tail_fixed_add(rd, K.t_delta, r.from_mont());
    tail_fixed_add(kz, K.t_delta, (r * s).from_mont());
    // combine
    XYZZ<Fp> ar = a_alpha;
    ar.add(rd);
    XYZZ<Fp> krs = kz;
    krs.add(s_a);
    krs.add(r_b);
    Affine<Fp> a_ar, a_krs;
    Affine<Fp2> a_bs;
    tail_to_affine(ar, bs, krs, &a_ar, &a_bs, &a_krs);
    Affine<HFp> h_ar, h_krs;
    Affine<HFp2> h_bs;
    memcpy(&h_ar, &a_ar, sizeof h_ar);
    memcpy(&h_krs, &a_krs, sizeof h_krs);
    memcpy(&h_bs, &a_bs, sizeof h_bs);
    g1_compress(h_ar, out);
    g2_compress(h_bs, out + 32);
    g1_compress(h_krs, out + 96);
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint64_t hdr[2];
    Affine<Fp> g1s[3];
    Affine<Fp2> g2s[2];
    if (fread(hdr, 8, 2, f) != 2 || fread(g1s, 64, 3, f) != 3 || fread(g2s, 128, 2, f) != 2) return 2;
    const size_t n = hdr[0], n_partials = hdr[1];
    const std::vector<Affine<Fp>> t1 = window_table(g1s[2]);
    const std::vector<Affine<Fp2>> t2 = window_table(g2s[1]);
    TailKey K;
    K.alpha = g1s[0]; K.beta = g1s[1]; K.beta2 = g2s[0];
    K.t_delta = t1.data();
    K.t_delta2 = t2.data();
    std::vector<uint64_t> rec(96 * n_partials);
    for (size_t i = 0; i < n; i++) {
        Fr r, s;
        uint8_t want[128], got[128];
        if (fread(rec.data(), 768, n_partials, f) != n_partials || fread(&r, 32, 1, f) != 1 || fread(&s, 32, 1, f) != 1 || fread(want, 128, 1, f) != 1) return 2;
        tail_row(K, rec.data(), n_partials, r, s, got);
        if (memcmp(got, want, 128) != 0) {
            const int part = memcmp(got, want, 32) ? 0 : memcmp(got + 32, want + 32, 64) ? 1 : 2;
            printf("MISMATCH row %zu element %s\n", i, part == 0 ? "Ar" : part == 1 ? "Bs" : "Krs");
            return 1;
        }
    }
    fclose(f);
    printf("ok %zu\n", n);
    return 0;
}
