// C++ host-side mirror of the gnark-crypto / gnark interfaces that libzkmi replaces (header-only, over the C ABI of zkmi.h).
// The reference's host language is Go (no toolchain in this image), so this is what a C++ caller -- or the cgo shim of
// INTEGRATION.md, line for line -- writes: same names, same argument meaning, same error behaviour as
//   gnark-crypto v0.9.1  ecc/bn254  (*G1Affine).MultiExp / (*G2Affine).MultiExp, ecc.MultiExpConfig      [REF gnark_backend_ffi/go.mod:5]
//   gnark-crypto v0.9.1  ecc/bn254/fr/fft  NewDomain, (*Domain).FFT / FFTInverse, BitReverse, Decimation
//   gnark-crypto v0.9.1  ecc/bn254/fr/iop  BuildRatioCopyConstraint (three entries, Lagrange regular), and its form for many witnesses
//   gnark v0.8.0         groth16.Prove (with the prover randomness as arguments)                          [REF gnark_backend_ffi/main.go:131]
//   the reference's      DeserializeFelts                                                                 [REF internal/backend/helpers.go:24-33]
// Go's `(value, error)` returns become `Error` return values (nil == ok()); nothing throws.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "zkmi.h"

namespace zkmi {

struct Error {
    int code = ZK_OK;
    std::string msg;
    bool ok() const { return code == ZK_OK; }
    explicit operator bool() const { return code != ZK_OK; }  // `if (err)` reads like Go's `if err != nil`
};
inline Error make_error(int rc) {
    if (rc == ZK_OK) return Error{};
    const char* m = zk_last_error();
    return Error{rc, m ? m : ""};
}

namespace fr {
typedef zk_fr Element;  // Montgomery, 4 x u64 little-endian limbs: gnark-crypto's memory image
typedef std::vector<Element> Vector;
// Device rows of polynomials, each opened at its own point (zk_bn254_fr_poly_open_rows_dev): d_values[v] = f_v(d_points[v]) and, where d_q is given, the len - 1
// coefficients of kzg.dividePolyByXminusA(f_v, f_v(a_v), a_v) at d_q + v * q_stride (d_q = d_f with q_stride = in_stride divides in place).
inline Error PolyOpenRows(const void* d_f, size_t in_stride, size_t len, size_t rows, const void* d_points, void* d_q, size_t q_stride, void* d_values,
                          void* stream = nullptr) {
    return make_error(zk_bn254_fr_poly_open_rows_dev(d_f, in_stride, len, rows, d_points, d_q, q_stride, d_values, stream));
}
}  // namespace fr

namespace ecc {
// ecc.MultiExpConfig{NbTasks int; ScalarsMont bool}
struct MultiExpConfig {
    int NbTasks = 0;
    bool ScalarsMont = false;  // upstream's zero value: the scalars' limbs are taken in REGULAR form (gnark v0.8.0's prover calls
                               // FromMont() on the wire values and on h, then passes MultiExpConfig{}); true: Montgomery fr.Elements
};
}  // namespace ecc

namespace bn254 {

struct G1Affine : zk_g1_affine {
    // func (p *G1Affine) MultiExp(points []G1Affine, scalars []fr.Element, config ecc.MultiExpConfig) (*G1Affine, error)
    // errors: "len(points) != len(scalars)" (ZK_ERR_LEN), "invalid config: config.NbTasks > 1024" (ZK_ERR_NB_TASKS)
    Error MultiExp(const std::vector<G1Affine>& points, const fr::Vector& scalars, const ecc::MultiExpConfig& config = ecc::MultiExpConfig()) {
        zk_msm_cfg c = {config.NbTasks, config.ScalarsMont ? 1 : 0, 0, 0};
        return make_error(zk_bn254_g1_msm(points.data(), points.size(), scalars.data(), scalars.size(), &c, this));
    }
    bool IsInfinity() const {
        for (int i = 0; i < 4; i++)
            if (x.l[i] | y.l[i]) return false;
        return true;
    }
};

// MultiExp for the rows of one matrix against bases[offset : offset + n] of a registered G1 base array (zk_bn254_msm_bases_rows, whose comment in zkmi.h says
// the rest): scalars holds rows * n elements, row after row; digests[v] is the point of row v, compressed (optional) its 32-byte G1Affine.Bytes() encoding.
// sparse: the scalars are wire-like (0 / 1 / small) -- the same digests from fewer sorted digits.
inline Error G1MultiExpRows(uint64_t bases, size_t offset, const fr::Vector& scalars, size_t n, std::vector<G1Affine>* digests,
                            const ecc::MultiExpConfig& config = ecc::MultiExpConfig(), bool sparse = false, std::vector<uint8_t>* compressed = nullptr) {
    if (n == 0 || scalars.size() % n) return Error{ZK_ERR_LEN, "scalars must hold whole rows of n elements"};
    const size_t rows = scalars.size() / n;
    zk_msm_cfg c = {config.NbTasks, config.ScalarsMont ? 1 : 0, 0, 0};
    digests->resize(rows);
    if (compressed) compressed->resize(rows * 32);
    static_assert(sizeof(G1Affine) == sizeof(zk_g1_affine), "digests are written back to back");
    return make_error(zk_bn254_msm_bases_rows(bases, offset, scalars.data(), n, rows, &c, sparse ? ZK_MSM_ROWS_SPARSE : 0u, digests->data(),
                                              compressed ? compressed->data() : nullptr));
}

struct G2Affine : zk_g2_affine {
    Error MultiExp(const std::vector<G2Affine>& points, const fr::Vector& scalars, const ecc::MultiExpConfig& config = ecc::MultiExpConfig()) {
        zk_msm_cfg c = {config.NbTasks, config.ScalarsMont ? 1 : 0, 0, 0};
        return make_error(zk_bn254_g2_msm(points.data(), points.size(), scalars.data(), scalars.size(), &c, this));
    }
};

}  // namespace bn254

namespace fft {

enum Decimation { DIT = ZK_DIT, DIF = ZK_DIF };  // same iota order as gnark-crypto

// fft.Domain: only the cardinality travels; the twiddle / coset tables are device-resident and cached per size inside libzkmi
class Domain {
public:
    uint64_t Cardinality = 1;
    // fft.NewDomain(m): next power of two >= m
    static Domain NewDomain(uint64_t m) {
        Domain d;
        while (d.Cardinality < m) d.Cardinality <<= 1;
        return d;
    }
    // (*Domain).FFT(a, decimation, coset...): in place; DIF natural -> bit-reversed, DIT bit-reversed -> natural
    Error FFT(fr::Vector& a, Decimation decimation, bool coset = false) const { return run(a, 0, decimation, coset); }
    // (*Domain).FFTInverse: same data movement with the inverse twiddles, scaled by 1/N (and the inverse coset table)
    Error FFTInverse(fr::Vector& a, Decimation decimation, bool coset = false) const { return run(a, 1, decimation, coset); }
    // the same on `rows` vectors of Cardinality elements each, row-major in a, in one launch per pass (zk_bn254_ntt_batch); no upstream counterpart
    Error FFTBatch(fr::Vector& a, size_t rows, Decimation decimation, bool coset = false) const { return run_batch(a, rows, 0, decimation, coset); }
    Error FFTInverseBatch(fr::Vector& a, size_t rows, Decimation decimation, bool coset = false) const { return run_batch(a, rows, 1, decimation, coset); }

private:
    uint32_t log_n() const {
        uint32_t l = 0;
        while ((uint64_t(1) << l) < Cardinality) l++;
        return l;
    }
    Error run_batch(fr::Vector& a, size_t rows, int inverse, Decimation decimation, bool coset) const {
        if (a.size() != rows * Cardinality) return Error{ZK_ERR_ARG, "len(a) != rows * domain.Cardinality"};
        if (rows == 0) return Error{};
        return make_error(zk_bn254_ntt_batch(a.data(), log_n(), rows, inverse, (int)decimation, coset ? 1 : 0));
    }
    Error run(fr::Vector& a, int inverse, Decimation decimation, bool coset) const {
        if (a.size() != Cardinality) return Error{ZK_ERR_ARG, "len(a) != domain.Cardinality"};
        uint32_t log_n = 0;
        while ((uint64_t(1) << log_n) < Cardinality) log_n++;
        return make_error(zk_bn254_ntt(a.data(), log_n, inverse, (int)decimation, coset ? 1 : 0));
    }
};

// fft.BitReverse(a): len(a) must be a power of two
inline Error BitReverse(fr::Vector& a) {
    uint32_t log_n = 0;
    while ((size_t(1) << log_n) < a.size()) log_n++;
    if ((size_t(1) << log_n) != a.size()) return Error{ZK_ERR_ARG, "len(a) is not a power of two"};
    return make_error(zk_bn254_bit_reverse(a.data(), log_n));
}

}  // namespace fft

namespace iop {

// iop.BuildRatioCopyConstraint(entries = {l, r, o}, permutation, beta, gamma, expectedForm = {Lagrange, Regular}, domain) for `rows` witnesses of one domain
// in one call (zk_bn254_iop_ratio_copy_batch): l, r, o hold rows x Cardinality values row-major, permutation the 3 x Cardinality positions (L | R | O) that
// every row shares, beta and gamma one challenge per row; z is resized to rows x Cardinality.  No upstream counterpart takes rows.
inline Error BuildRatioCopyConstraintBatch(const fr::Vector& l, const fr::Vector& r, const fr::Vector& o, size_t rows, const std::vector<uint32_t>& permutation,
                                           const fr::Vector& beta, const fr::Vector& gamma, const fft::Domain& domain, fr::Vector& z) {
    const uint64_t n = domain.Cardinality;
    uint32_t log_n = 0;
    while ((uint64_t(1) << log_n) < n) log_n++;
    if (l.size() != rows * n || r.size() != rows * n || o.size() != rows * n) return Error{ZK_ERR_ARG, "len(entry) != rows * domain.Cardinality"};
    if (permutation.size() != 3 * n) return Error{ZK_ERR_ARG, "len(permutation) != 3 * domain.Cardinality"};
    if (beta.size() != rows || gamma.size() != rows) return Error{ZK_ERR_ARG, "one beta and one gamma per row"};
    z.resize(rows * n);
    if (rows == 0) return Error{};
    return make_error(zk_bn254_iop_ratio_copy_batch(l.data(), r.data(), o.data(), log_n, rows, permutation.data(), beta.data(), gamma.data(), z.data()));
}
// the upstream call: one witness
inline Error BuildRatioCopyConstraint(const fr::Vector& l, const fr::Vector& r, const fr::Vector& o, const std::vector<uint32_t>& permutation, const fr::Element& beta,
                                      const fr::Element& gamma, const fft::Domain& domain, fr::Vector& z) {
    return BuildRatioCopyConstraintBatch(l, r, o, 1, permutation, fr::Vector(1, beta), fr::Vector(1, gamma), domain, z);
}

}  // namespace iop

namespace groth16 {

// groth16.ProvingKey resident in HBM (RAII over zk_bn254_groth16_pk_load / _free); keeps the geometry the prover validates against
class ProvingKey {
public:
    ProvingKey() = default;
    ProvingKey(const ProvingKey&) = delete;
    ProvingKey& operator=(const ProvingKey&) = delete;
    ~ProvingKey() {
        if (handle_) zk_bn254_groth16_pk_free(handle_);
    }
    // pk.infinity_a / infinity_b (gnark's InfinityA / InfinityB) select gnark's compact A / B / G2.B layout
    Error Load(const zk_groth16_pk& pk) {
        Error e = make_error(zk_bn254_groth16_pk_load(&pk, &handle_));
        if (!e.ok()) return e;
        return make_error(zk_bn254_groth16_pk_info(handle_, &n_wires_, &n_public_, &log_domain_, nullptr));
    }
    // (*ProvingKey).ReadFrom on the bytes of WriteTo (hex = true: the text the reference's ProveWithPK receives, backend/groth16/r1cs.go:107-128);
    // every point is decompressed on the device
    Error ReadFrom(const void* data, size_t len, bool hex = false) {
        Error e = make_error(zk_bn254_groth16_pk_read(data, len, hex ? 1 : 0, 0, 0, &handle_));
        if (!e.ok()) return e;
        return make_error(zk_bn254_groth16_pk_info(handle_, &n_wires_, &n_public_, &log_domain_, nullptr));
    }
    // (*ProvingKey).WriteTo: compressed points, A / B / G2.B without their points at infinity, then InfinityA / InfinityB
    Error WriteTo(std::vector<uint8_t>* out, bool hex = false) const {
        size_t need = 0;
        Error e = make_error(zk_bn254_groth16_pk_write(handle_, hex ? 1 : 0, nullptr, 0, &need));
        if (!e.ok()) return e;
        out->resize(need);
        return make_error(zk_bn254_groth16_pk_write(handle_, hex ? 1 : 0, out->data(), out->size(), &need));
    }
    uint64_t handle() const { return handle_; }
    size_t NbWires() const { return n_wires_; }
    size_t NbPublic() const { return n_public_; }
    uint64_t DomainCardinality() const { return uint64_t(1) << log_domain_; }

private:
    uint64_t handle_ = 0;
    size_t n_wires_ = 0, n_public_ = 0;
    uint32_t log_domain_ = 0;
};

struct Proof {
    uint8_t bytes[128];  // Proof.WriteTo: Ar | Bs | Krs, gnark's compressed encodings
};

// groth16.Prove after the solver: a, b, c = evaluations of the constraint system, w = wire values, (r, s) = the prover's randomness.
// All four vectors hold Montgomery fr.Elements (the solver's containers).  Length errors come back as ZK_ERR_LEN -- the library
// reads exactly NbWires() elements of w and at most DomainCardinality() of a, b, c, so nothing is read out of bounds.
inline Error Prove(const ProvingKey& pk, const fr::Vector& a, const fr::Vector& b, const fr::Vector& c, const fr::Vector& w, const fr::Element& r,
                   const fr::Element& s, Proof* proof) {
    if (a.size() != b.size() || a.size() != c.size()) return Error{ZK_ERR_LEN, "len(a), len(b), len(c) differ"};
    if (a.size() > pk.DomainCardinality()) return Error{ZK_ERR_LEN, "len(a) exceeds the domain cardinality"};
    if (w.size() != pk.NbWires()) return Error{ZK_ERR_LEN, "len(w) != number of wires of the proving key"};
    return make_error(zk_bn254_groth16_prove(pk.handle(), a.data(), b.data(), c.data(), a.size(), w.data(), w.size(), &r, &s, 0, proof->bytes));
}
// The same for many witnesses against one key in one call: a, b, c hold len(r) rows of n_constraints elements, w len(r) rows of NbWires(); proofs[i] is byte
// for byte what Prove writes for row i with r[i], s[i].
inline Error ProveBatch(const ProvingKey& pk, const fr::Vector& a, const fr::Vector& b, const fr::Vector& c, size_t n_constraints, const fr::Vector& w,
                        const fr::Vector& r, const fr::Vector& s, std::vector<Proof>* proofs) {
    const size_t n = r.size();
    if (s.size() != n) return Error{ZK_ERR_LEN, "len(r) != len(s)"};
    if (a.size() != n * n_constraints || b.size() != a.size() || c.size() != a.size()) return Error{ZK_ERR_LEN, "a, b, c must hold len(r) rows of n_constraints"};
    if (n_constraints > pk.DomainCardinality()) return Error{ZK_ERR_LEN, "n_constraints exceeds the domain cardinality"};
    if (w.size() != n * pk.NbWires()) return Error{ZK_ERR_LEN, "w must hold len(r) rows of the proving key's wires"};
    proofs->resize(n);
    static_assert(sizeof(Proof) == 128, "proofs are written back to back");
    return make_error(zk_bn254_groth16_prove_batch(pk.handle(), a.data(), b.data(), c.data(), n_constraints, w.data(), pk.NbWires(), r.data(), s.data(), n, 0,
                                                   n ? (*proofs)[0].bytes : nullptr));
}
// The second half of Prove for many rows in one device launch (zk_bn254_groth16_finalize_batch): partials holds len(r) rows of n_partials records of 96 limbs
// (the five un-normalised MSM sums A, B1, K, Z, G2.B of zk_bn254_groth16_msm5_*); proofs[i] is byte for byte what zk_bn254_groth16_finalize writes for row i.
inline Error FinalizeBatch(const ProvingKey& pk, const std::vector<uint64_t>& partials, size_t n_partials, const fr::Vector& r, const fr::Vector& s,
                           std::vector<Proof>* proofs) {
    const size_t n = r.size();
    if (s.size() != n) return Error{ZK_ERR_LEN, "len(r) != len(s)"};
    if (n_partials == 0) return Error{ZK_ERR_ARG, "n_partials must be at least 1"};
    if (partials.size() != n * n_partials * 96) return Error{ZK_ERR_LEN, "partials must hold len(r) rows of n_partials records of 96 limbs"};
    proofs->resize(n);
    static_assert(sizeof(Proof) == 128, "proofs are written back to back");
    return make_error(zk_bn254_groth16_finalize_batch(pk.handle(), partials.data(), n_partials, r.data(), s.data(), n, n ? (*proofs)[0].bytes : nullptr));
}

}  // namespace groth16

namespace kzg {

// kzg.SRS with the G1 side resident in HBM (RAII over the registered base array).  kzg.NewSRS / (*SRS).ReadFrom / WriteTo / kzg.Commit; the openings
// (Open, BatchOpenSinglePoint, FoldProof, Verify, BatchVerifySinglePoint, BatchVerifyMultiPoints) follow the class.
class SRS {
public:
    SRS() = default;
    SRS(const SRS&) = delete;
    SRS& operator=(const SRS&) = delete;
    ~SRS() {
        if (handle_) zk_bn254_bases_free(handle_);
    }
    // kzg.NewSRS(size, alpha): alpha^i * G1 generated on the device; alpha is a Montgomery fr.Element
    Error New(uint64_t size, const fr::Element& alpha) {
        void* d = nullptr;
        Error e = make_error(zk_dev_alloc(&d, size * 64));
        if (!e.ok()) return e;
        e = make_error(zk_bn254_kzg_new_srs_dev(d, size, &alpha, G2, nullptr));
        if (e.ok()) e = make_error(zk_bn254_bases_register_dev(d, size, 0, &handle_));
        zk_dev_free(d);
        if (e.ok()) size_ = size;
        return e;
    }
    // (*SRS).ReadFrom on the bytes of WriteTo (hex = true: the text of srs.hex); the G1 points are decompressed on the device
    Error ReadFrom(const void* data, size_t len, bool hex = false) {
        size_t n = 0;
        Error e = make_error(zk_bn254_kzg_srs_read(data, len, hex ? 1 : 0, 0, &handle_, &n, G2));
        if (e.ok()) size_ = n;
        return e;
    }
    Error WriteTo(std::vector<uint8_t>* out, bool hex = false) const {
        size_t need = (132 + 32 * size_) * (hex ? 2 : 1), n = 0;
        out->resize(need);
        return make_error(zk_bn254_kzg_srs_write(handle_, G2, hex ? 1 : 0, out->data(), out->size(), &n));
    }
    // kzg.Commit(p, srs) = MultiExp(srs.G1[:len(p)], p); p holds Montgomery fr.Elements
    Error Commit(const fr::Vector& p, zk_g1_affine* digest) const {
        if (p.size() > size_) return Error{ZK_ERR_LEN, "kzg: invalid polynomial size (larger than SRS or == 0)"};
        zk_msm_cfg c = {0, 1, 0, 0};
        return make_error(zk_bn254_msm_bases(handle_, 0, p.data(), p.size(), &c, digest));
    }
    // the three simultaneous commitments of plonk.Prove's rounds 1 and 3 in one call (zk_bn254_msm_bases_batch): digests[k] = Commit(*polys[k])
    Error CommitBatch(const std::vector<const fr::Vector*>& polys, zk_g1_affine* digests) const {
        std::vector<const zk_fr*> p;
        for (const fr::Vector* v : polys) {
            if (v->size() > size_ || v->size() != polys[0]->size()) return Error{ZK_ERR_LEN, "kzg: invalid polynomial size (larger than SRS, or the batch is ragged)"};
            p.push_back(v->data());
        }
        zk_msm_cfg c = {0, 1, 0, 0};
        return make_error(zk_bn254_msm_bases_batch(handle_, 0, p.data(), (uint32_t)p.size(), polys.empty() ? 0 : polys[0]->size(), &c, digests));
    }
    uint64_t handle() const { return handle_; }
    uint64_t Size() const { return size_; }
    zk_g2_affine G2[2] = {};

private:
    uint64_t handle_ = 0;
    uint64_t size_ = 0;
};

// kzg.OpeningProof{H, ClaimedValue} and kzg.BatchOpeningProof{H, ClaimedValues}
typedef zk_kzg_opening OpeningProof;
struct BatchOpeningProof {
    zk_g1_affine H = {};
    fr::Vector ClaimedValues;
};
typedef zk_g1_affine Digest;

// kzg.Commit for many polynomials of one length at once: polys holds rows * n Montgomery coefficients, row after row; digests[v] = Commit(row v)
inline Error CommitRows(const fr::Vector& polys, size_t n, const SRS& srs, std::vector<bn254::G1Affine>* digests, std::vector<uint8_t>* compressed = nullptr) {
    if (n > srs.Size()) return Error{ZK_ERR_LEN, "kzg: invalid polynomial size (larger than SRS or == 0)"};
    ecc::MultiExpConfig c;
    c.ScalarsMont = true;
    return bn254::G1MultiExpRows(srs.handle(), 0, polys, n, digests, c, false, compressed);
}

// kzg.Open(p, point, srs): ClaimedValue = p(point), H = Commit((p - p(point)) / (X - point)), on the device
inline Error Open(const fr::Vector& p, const fr::Element& point, const SRS& srs, OpeningProof* proof) {
    if (p.empty() || p.size() > srs.Size()) return Error{ZK_ERR_LEN, "kzg: invalid polynomial size (larger than SRS or == 0)"};
    const void* polys[1] = {p.data()};
    const size_t lens[1] = {p.size()};
    return make_error(zk_bn254_kzg_open(srs.handle(), polys, lens, &point, 1, 0, proof));
}
// kzg.BatchOpenSinglePoint(polynomials, digests, point, hf, srs) with hf = SHA-256
inline Error BatchOpenSinglePoint(const std::vector<fr::Vector>& polynomials, const std::vector<Digest>& digests, const fr::Element& point, const SRS& srs,
                                  BatchOpeningProof* proof) {
    if (polynomials.size() != digests.size()) return Error{ZK_ERR_ARG, "kzg: number of digests differs from the number of polynomials"};
    std::vector<const void*> polys;
    std::vector<size_t> lens;
    for (const fr::Vector& p : polynomials) {
        if (p.empty() || p.size() > srs.Size()) return Error{ZK_ERR_LEN, "kzg: invalid polynomial size (larger than SRS or == 0)"};
        polys.push_back(p.data());
        lens.push_back(p.size());
    }
    proof->ClaimedValues.resize(polynomials.size());
    return make_error(zk_bn254_kzg_batch_open_single_point(srs.handle(), polys.data(), lens.data(), digests.data(), polys.size(), &point, 0, &proof->H,
                                                           proof->ClaimedValues.data()));
}
// kzg.FoldProof(digests, batchOpeningProof, point, hf): the folded opening and the folded digest (host)
inline Error FoldProof(const std::vector<Digest>& digests, const BatchOpeningProof& batch, const fr::Element& point, OpeningProof* proof, Digest* digest) {
    if (digests.size() != batch.ClaimedValues.size()) return Error{ZK_ERR_ARG, "kzg: number of digests differs from the number of claimed values"};
    return make_error(zk_bn254_kzg_fold_proof(digests.data(), digests.size(), &batch.H, batch.ClaimedValues.data(), &point, proof, digest));
}
// kzg.Verify(commitment, proof, point, srs): nil when the opening holds, "can't verify opening proof" (upstream's ErrVerifyOpeningProof) otherwise (host)
inline Error Verify(const Digest& commitment, const OpeningProof& proof, const fr::Element& point, const SRS& srs) {
    int ok = 0;
    Error e = make_error(zk_bn254_kzg_verify(&commitment, &proof, &point, srs.G2, &ok));
    if (e.ok() && !ok) return Error{ZK_ERR_ARG, "can't verify opening proof"};
    return e;
}
// kzg.BatchVerifySinglePoint(digests, batchOpeningProof, point, hf, srs) (host)
inline Error BatchVerifySinglePoint(const std::vector<Digest>& digests, const BatchOpeningProof& batch, const fr::Element& point, const SRS& srs) {
    if (digests.size() != batch.ClaimedValues.size()) return Error{ZK_ERR_ARG, "kzg: number of digests differs from the number of claimed values"};
    int ok = 0;
    Error e = make_error(zk_bn254_kzg_batch_verify_single_point(digests.data(), digests.size(), &batch.H, batch.ClaimedValues.data(), &point, srs.G2, &ok));
    if (e.ok() && !ok) return Error{ZK_ERR_ARG, "can't verify opening proof"};
    return e;
}
// kzg.BatchVerifyMultiPoints(digests, proofs, points, srs) on the device.  Upstream answers for the whole batch; `accepted` (optional) receives a verdict per opening.
inline Error BatchVerifyMultiPoints(const std::vector<Digest>& digests, const std::vector<OpeningProof>& proofs, const fr::Vector& points, const SRS& srs,
                                    std::vector<uint8_t>* accepted = nullptr) {
    if (digests.size() != proofs.size() || digests.size() != points.size()) return Error{ZK_ERR_ARG, "kzg: number of digests, proofs and points differ"};
    if (digests.empty()) return Error{ZK_ERR_ARG, "kzg: no opening to verify"};
    std::vector<uint8_t> acc(digests.size());
    size_t n_ok = 0;
    Error e = make_error(zk_bn254_kzg_verify_batch(digests.data(), proofs.data(), points.data(), digests.size(), srs.G2, acc.data(), &n_ok));
    if (accepted) *accepted = acc;
    if (e.ok() && n_ok != digests.size()) return Error{ZK_ERR_ARG, "can't verify opening proof"};
    return e;
}

}  // namespace kzg

namespace plonk {

// plonk.ProvingKey resident in HBM; plonk.Setup / ReadFrom / WriteTo / plonk.Prove (the reference's live path: backend/plonk/plonk.go:21,67)
class ProvingKey {
public:
    ProvingKey() = default;
    ProvingKey(const ProvingKey&) = delete;
    ProvingKey& operator=(const ProvingKey&) = delete;
    ~ProvingKey() {
        if (handle_) zk_bn254_plonk_pk_free(handle_);
    }
    // plonk.Setup(spr, srs): the gates as BuildSparseR1CS emits them (backend/plonk/sparse_r1cs.go:44-107)
    Error Setup(const zk_plonk_circuit& spr, const kzg::SRS& srs) {
        n_vars_ = spr.n_vars;
        return make_error(zk_bn254_plonk_setup(&spr, srs.handle(), &handle_, &Vk));
    }
    // ProvingKey.ReadFrom on gnark's bytes (or their hex text) + the wire ids of the rebuilt spr
    Error ReadFrom(const void* data, size_t len, bool hex, size_t n_vars, const std::vector<uint32_t>& xa, const std::vector<uint32_t>& xb, const std::vector<uint32_t>& xc,
                   const kzg::SRS& srs) {
        if (xa.size() != xb.size() || xa.size() != xc.size()) return Error{ZK_ERR_LEN, "wire-id arrays differ in length"};
        n_vars_ = n_vars;
        return make_error(zk_bn254_plonk_pk_read(data, len, hex ? 1 : 0, n_vars, xa.size(), xa.data(), xb.data(), xc.data(), srs.handle(), &handle_));
    }
    Error WriteTo(std::vector<uint8_t>* out, bool hex = false) const {
        size_t n = 0;
        uint8_t dummy = 0;
        zk_bn254_plonk_pk_write(handle_, hex ? 1 : 0, &dummy, 0, &n);  // size query
        out->resize(n);
        return make_error(zk_bn254_plonk_pk_write(handle_, hex ? 1 : 0, out->data(), out->size(), &n));
    }
    uint64_t handle() const { return handle_; }
    size_t NbVariables() const { return n_vars_; }
    zk_plonk_vk Vk = {};

private:
    uint64_t handle_ = 0;
    size_t n_vars_ = 0;
};

struct Proof {
    uint8_t bytes[ZK_PLONK_PROOF_BYTES];  // Proof.WriteTo
};

// plonk.Prove after spr.Solve: solution = the values of all variables (public first), blinders = the nine fr.SetRandom draws of Blind(),
// challenges = nullptr (SHA-256 Fiat-Shamir as upstream) or five pinned values
inline Error Prove(const ProvingKey& pk, const fr::Vector& solution, const fr::Element blinders[9], Proof* proof, const fr::Element* challenges = nullptr) {
    if (solution.size() != pk.NbVariables()) return Error{ZK_ERR_LEN, "len(solution) != number of variables of the constraint system"};
    return make_error(zk_bn254_plonk_prove(pk.handle(), solution.data(), solution.size(), 0, blinders, challenges, proof->bytes));
}

// Round 3 of plonk.Prove -- the quotient -- for `rows` witnesses of one key in the launches of one (zk_bn254_plonk_quotient_batch_dev, whose comment in zkmi.h
// says the rest).  Everything lives on the device: row v of the blinded canonical l, r, o (n + 2 coefficients) and z (n + 3) at element v * in_stride, of the public
// inputs at v * pub_stride of `pub` (a solutions array with pub_stride = NbVariables() works), alpha / beta / gamma one element per row.  Row v's 3 (n + 2)
// coefficients go to d_h + v * out_stride and its verdict to d_status[v] (int32: 1 = not a polynomial, which fails neither the call nor the other rows).
struct QuotientRows {
    const void *l = nullptr, *r = nullptr, *o = nullptr, *z = nullptr;
    size_t in_stride = 0;
    const void* pub = nullptr;
    size_t pub_stride = 0;
    const void *alpha = nullptr, *beta = nullptr, *gamma = nullptr;
};
inline Error ComputeQuotientBatch(const ProvingKey& pk, const QuotientRows& in, size_t rows, void* d_h, size_t out_stride, void* d_status, void* stream = nullptr) {
    return make_error(zk_bn254_plonk_quotient_batch_dev(pk.handle(), in.l, in.r, in.o, in.z, in.in_stride, in.pub, in.pub_stride, rows, in.alpha, in.beta, in.gamma, d_h,
                                                        out_stride, d_status, stream));
}

// Rounds 4 and 5 of plonk.Prove for `rows` witnesses of one key (zk_bn254_plonk_linearize_batch_dev, zk_bn254_plonk_open_batch_dev; zkmi.h says the rest), all on
// the device.  Linearize: from the rows of round 3 (l, r, o, z at v * in_stride, h at v * h_stride) and alpha / beta / gamma / zeta per row to the eight values
// of the proof at d_values + 8 v and, v * out_stride apart, the quotient of z at omega zeta (n + 2), the linearised polynomial (n + 3), the folded quotient (n + 2).
struct LinearizeRows {
    const void *l = nullptr, *r = nullptr, *o = nullptr, *z = nullptr;
    size_t in_stride = 0;
    const void* h = nullptr;
    size_t h_stride = 0;
    const void *alpha = nullptr, *beta = nullptr, *gamma = nullptr, *zeta = nullptr;
};
struct LinearizedRows {
    void *values = nullptr, *zquot = nullptr, *lin = nullptr, *fh = nullptr;
    size_t out_stride = 0;
};
inline Error LinearizeBatch(const ProvingKey& pk, const LinearizeRows& in, size_t rows, const LinearizedRows& out, void* stream = nullptr) {
    return make_error(zk_bn254_plonk_linearize_batch_dev(pk.handle(), in.l, in.r, in.o, in.z, in.in_stride, in.h, in.h_stride, rows, in.alpha, in.beta, in.gamma, in.zeta,
                                                         out.values, out.zquot, out.lin, out.fh, out.out_stride, stream));
}
// Open: kzg.BatchOpenSinglePoint's quotient of (fh, lin, l, r, o, s1, s2) at zeta[v] under the challenge kzg_gamma[v]: n + 2 coefficients at d_q + v * out_stride,
// the folded value at d_value[v].
struct OpenRows {
    const void *fh = nullptr, *lin = nullptr, *l = nullptr, *r = nullptr, *o = nullptr;
    size_t in_stride = 0;
    const void *zeta = nullptr, *kzg_gamma = nullptr;
};
inline Error OpenBatch(const ProvingKey& pk, const OpenRows& in, size_t rows, void* d_q, size_t out_stride, void* d_value, void* stream = nullptr) {
    return make_error(zk_bn254_plonk_open_batch_dev(pk.handle(), in.fh, in.lin, in.l, in.r, in.o, in.in_stride, rows, in.zeta, in.kzg_gamma, d_q, out_stride, d_value,
                                                    stream));
}

// The digests those rounds end in (zk_bn254_plonk_commit_batch_dev), on the device: row v = the `len` Montgomery images at d_rows + v * row_stride, against the
// key's SRS (coefficients) or, with from_values, its Lagrange form (len = n + 2: the wire values, then the blinders b0, b1).  d_out: rows points (64 bytes each),
// d_compressed: rows x 32 bytes; one of the two may be null.
inline Error CommitBatch(const ProvingKey& pk, const void* d_rows, size_t row_stride, size_t len, size_t rows, bool from_values, void* d_out, void* d_compressed) {
    return make_error(zk_bn254_plonk_commit_batch_dev(pk.handle(), d_rows, row_stride, len, rows, from_values ? 1 : 0, d_out, d_compressed));
}

// plonk.Prove for `rows` witnesses of one key in one call (zk_bn254_plonk_prove_batch, whose comment in zkmi.h says the rest): solutions[v] and blinders[9 v ..)
// are row v's; challenges = nullptr (the transcript) or five pinned values per row.  proofs[v] is what Prove writes for row v; (*satisfied)[v] is false where the
// row's solution violates the circuit (its proof is then all zero), which fails neither the call nor the other rows.
inline Error ProveBatch(const ProvingKey& pk, const std::vector<fr::Vector>& solutions, const std::vector<fr::Element>& blinders, std::vector<Proof>* proofs,
                        std::vector<bool>* satisfied, const fr::Element* challenges = nullptr) {
    const size_t rows = solutions.size(), nv = pk.NbVariables();
    if (blinders.size() != 9 * rows) return Error{ZK_ERR_LEN, "nine blinders per solution"};
    fr::Vector flat(rows * nv);
    for (size_t v = 0; v < rows; v++) {
        if (solutions[v].size() != nv) return Error{ZK_ERR_LEN, "len(solution) != number of variables of the constraint system"};
        std::copy(solutions[v].begin(), solutions[v].end(), flat.begin() + v * nv);
    }
    proofs->assign(rows, Proof{});
    std::vector<int> status(rows, 0);
    if (rows == 0) {
        satisfied->clear();
        return Error{};
    }
    Error e = make_error(zk_bn254_plonk_prove_batch(pk.handle(), flat.data(), nv, nv, rows, 0, blinders.data(), challenges, 0, (*proofs)[0].bytes, status.data()));
    satisfied->assign(rows, false);
    for (size_t v = 0; v < rows; v++) (*satisfied)[v] = status[v] == 0;
    return e;
}

// plonk.Verify(proof, vk, publicWitness) on the host: vk = the bytes of VerifyingKey.WriteTo, srs supplies the two G2 points InitKZG attaches.
// *accepted <- the verdict; malformed encodings come back as errors (what upstream's ReadFrom returns).
inline Error Verify(const Proof& proof, const std::vector<uint8_t>& vk, const kzg::SRS& srs, const fr::Vector& public_witness, bool* accepted) {
    int ok = 0;
    Error e = make_error(zk_bn254_plonk_verify(proof.bytes, vk.data(), vk.size(), 0, srs.G2, public_witness.data(), public_witness.size(), &ok));
    *accepted = ok != 0;
    return e;
}

}  // namespace plonk

namespace groth16 {
// groth16.Verify(proof, vk, publicWitness) on the host: vk = the bytes of VerifyingKey.WriteTo; the public witness excludes the constant wire
inline Error Verify(const Proof& proof, const std::vector<uint8_t>& vk, const fr::Vector& public_witness, bool* accepted) {
    int ok = 0;
    Error e = make_error(zk_bn254_groth16_verify(proof.bytes, vk.data(), vk.size(), 0, public_witness.data(), public_witness.size(), &ok));
    *accepted = ok != 0;
    return e;
}
}  // namespace groth16

// DeserializeFelts(encodedFelts string): hex(u32 BE count || count x 32 B BE) -> Montgomery vector, decoded on the device into d_out
inline Error DeserializeFelts(const std::string& encoded, void* d_out, size_t capacity, size_t* n) {
    return make_error(zk_bn254_felts_decode_hex(encoded.data(), encoded.size(), d_out, capacity, n));
}

}  // namespace zkmi
