// ark_blst_amd.hpp — C++ host-side mirror of the trait surface nikkolasg/ark-blst exposes for the MSM path, on top
// of the C ABI (include/arkblst_amd.h).  The reference is Rust (no toolchain in this image), so this header is the
// compiled-language host side: same names, argument meaning and error behaviour as
//     impl ScalarMul        for G{1,2}Projective   /root/reference/src/g1.rs:593-600, src/g2.rs:573-580
//     impl VariableBaseMSM  for G{1,2}Projective   /root/reference/src/g1.rs:602-632, src/g2.rs:582-612
//     CurveGroup::normalize_batch                  /root/reference/src/g1.rs:537-543, src/g2.rs:517-523
//     ScalarMul::batch_mul (arkworks default)      one base, many scalars: mi_g{1,2}_batch_mul
//     ark_poly::Radix2EvaluationDomain<Scalar>     fft / ifft / coset_fft / coset_ifft: mi_fr_ntt
//     ark_poly::Radix2EvaluationDomain<Scalar>     fft / ifft over G1 points (monomial SRS <-> Lagrange-basis SRS): mi_g1_ntt
//     ark_poly::univariate::DensePolynomial<Scalar> evaluate, division by (X - z), KZG10::open: mi_fr_poly_open
//     ark_ff::batch_inversion / batch_inversion_and_mul, the grand product of a permutation argument: mi_fr_batch_inverse, mi_fr_scan
// Types are the reference's #[repr(transparent)] wrappers over the blst structs (src/g1.rs:55-56,436-437;
// src/scalar.rs:24-25), i.e. plain limb arrays.  Header-only; link with -larkblst_amd.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <stdexcept>
#include <variant>
#include <vector>

#include "../../include/arkblst_amd.h"

namespace ark_blst {

// Result<T, usize> of the reference: Ok(value) or Err(n).  Err(min(len)) on a length mismatch (arkworks' default),
// Err(0) for any GPU failure (src/g1.rs:628-630).
template <class T>
class Result {
public:
    static Result Ok(const T& v) { Result r; r.v_ = v; r.ok_ = true; return r; }
    static Result Err(size_t e) { Result r; r.e_ = e; r.ok_ = false; return r; }
    bool is_ok() const { return ok_; }
    bool is_err() const { return !ok_; }
    const T& unwrap() const {
        if (!ok_) throw std::runtime_error("called `Result::unwrap()` on an `Err` value");
        return v_;
    }
    size_t unwrap_err() const { return e_; }

private:
    T v_{};
    size_t e_ = 0;
    bool ok_ = false;
};

struct Scalar { uint64_t l[4]; };                   // blst_fr: Montgomery, R = 2^256   (src/scalar.rs:23-25)
struct BigInteger256 { uint64_t l[4]; };            // canonical little-endian integer  (PrimeField::BigInt)
using G1Affine = mi_g1_affine;                      // blst_p1_affine, all-zero = identity (src/g1.rs:54-56)
using G2Affine = mi_g2_affine;

// One process-wide context, created on first use — the reference rebuilds program and kernel on every call
// (src/gpu.rs:233-237) and panics if that fails (`.expect`, gpu.rs:235,237); here creation failure throws.
// Devices: GPU 0 by default, like the reference's `Device::all()[0]` (src/gpu.rs:233-234).  ARKBLST_AMD_DEVICES selects
// others: a comma-separated list of device ids ("0,1,2,3"), or "all".  The multi-device path (bases sharded contiguously,
// one persistent host thread per device) is opt-in: it has been rehearsed on one GPU listed several times and in
// multi-process form, not yet run on a multi-GPU node.
inline mi_ctx* context() {
    static mi_ctx* ctx = [] {
        mi_ctx* c = nullptr;
        std::vector<int> ids{0};
        bool all = false;
        if (const char* e = std::getenv("ARKBLST_AMD_DEVICES")) {
            std::string v(e);
            if (v == "all") {
                all = true;
            } else {
                ids.clear();
                size_t pos = 0;
                while (pos <= v.size()) {
                    size_t q = v.find(',', pos);
                    if (q == std::string::npos) q = v.size();
                    if (q > pos) ids.push_back(std::atoi(v.substr(pos, q - pos).c_str()));
                    pos = q + 1;
                }
                if (ids.empty()) ids.push_back(0);
            }
        }
        int rc = all ? mi_msm_init(&c, nullptr, 0) : mi_msm_init(&c, ids.data(), (int)ids.size());
        if (rc != MI_OK) throw std::runtime_error(std::string("Cannot initialize MI355X MSM context: ") + mi_msm_strerror(rc));
        // The trait call is stateless (`msm(&[G1Affine], &[Scalar])`, src/g1.rs:604) while a prover's base vectors are a fixed SRS: keep the
        // device form of the last two base vectors per group, so that the second call with the same slice runs the resident path
        // (include/arkblst_amd.h, mi_msm_set_base_cache).  The cache is keyed by a fingerprint of EVERY byte of the vector (round 6), computed
        // on helper threads under the GPU work and confirmed before the result leaves: the call stays a function of its arguments, also for a
        // caller that edits single points in place.  ARKBLST_AMD_BASE_CACHE=0 in the environment switches it off (read by mi_msm_init).
        mi_msm_set_base_cache(c, 2);
        return c;
    }();
    return ctx;
}

struct G1Projective {
    mi_g1 p;                                        // blst_p1 (src/g1.rs:435-437)
    using MulBase = G1Affine;                       // impl ScalarMul (src/g1.rs:593-600)
    static constexpr bool NEGATION_IS_CHEAP = true;

    static G1Projective zero() { G1Projective r; std::memset(&r.p, 0, sizeof r.p); return r; }
    bool is_zero() const { mi_fp z{}; return std::memcmp(&p.z, &z, sizeof z) == 0; }

    // fn msm(bases: &[Self::MulBase], scalars: &[Self::ScalarField]) -> Result<Self, usize>
    static Result<G1Projective> msm(const std::vector<G1Affine>& bases, const std::vector<Scalar>& scalars) {
        if (bases.size() != scalars.size()) return Result<G1Projective>::Err(std::min(bases.size(), scalars.size()));
        G1Projective out;
        int rc = mi_msm_g1(context(), bases.data(), reinterpret_cast<const uint8_t*>(scalars.data()), bases.size(),
                           MI_SCALAR_MONTGOMERY, &out.p);
        return rc == MI_OK ? Result<G1Projective>::Ok(out) : Result<G1Projective>::Err(0);
    }
    // fn msm_bigint(bases, bigints) — the form the reference's GPU impl builds first (src/g1.rs:624-627)
    // k commitments over the resident SRS in one call (set with mi_msm_g1_set_bases): two run at a time on the context
    static std::vector<G1Projective> msm_batch(const std::vector<std::vector<Scalar>>& polys) {
        std::vector<const uint8_t*> ptrs;
        size_t n = polys.empty() ? 0 : polys[0].size();
        for (auto& v : polys) {
            if (v.size() != n) throw std::runtime_error("msm_batch: scalar vectors of different length");
            ptrs.push_back(reinterpret_cast<const uint8_t*>(v.data()));
        }
        std::vector<G1Projective> out(polys.size());
        int rc = mi_msm_g1_batch(context(), ptrs.data(), ptrs.size(), n, MI_SCALAR_MONTGOMERY, reinterpret_cast<mi_g1*>(out.data()));
        if (rc != MI_OK) throw std::runtime_error(std::string("msm_batch: ") + mi_msm_last_error(context()));
        return out;
    }
    static Result<G1Projective> msm_bigint(const std::vector<G1Affine>& bases, const std::vector<BigInteger256>& bigints) {
        if (bases.size() != bigints.size()) return Result<G1Projective>::Err(std::min(bases.size(), bigints.size()));
        G1Projective out;
        int rc = mi_msm_g1(context(), bases.data(), reinterpret_cast<const uint8_t*>(bigints.data()), bases.size(),
                           MI_SCALAR_CANONICAL, &out.p);
        return rc == MI_OK ? Result<G1Projective>::Ok(out) : Result<G1Projective>::Err(0);
    }
    // fn normalize_batch(projective: &[Self]) -> Vec<Self::Affine>  (= ScalarMul::batch_convert_to_mul_base)
    static std::vector<G1Affine> normalize_batch(const std::vector<G1Projective>& projective) {
        std::vector<G1Affine> out(projective.size());
        if (projective.empty()) return out;
        static_assert(sizeof(G1Projective) == sizeof(mi_g1), "transparent wrapper");
        int rc = mi_g1_normalize_batch(context(), reinterpret_cast<const mi_g1*>(projective.data()), projective.size(), out.data());
        if (rc != MI_OK) throw std::runtime_error(std::string("normalize_batch: ") + mi_msm_last_error(context()));
        return out;
    }
    static std::vector<G1Affine> batch_convert_to_mul_base(const std::vector<G1Projective>& bases) { return normalize_batch(bases); }
    // ScalarMul::batch_mul / FixedBase::msm + normalize_batch: out[i] = scalars[i] * base, the arkworks default the reference inherits
    // (src/g1.rs:593-600) — here a table walk on the GPU (include/arkblst_amd.h, mi_g1_batch_mul)
    static std::vector<G1Affine> batch_mul(const G1Affine& base, const std::vector<Scalar>& scalars) {
        std::vector<G1Affine> out(scalars.size());
        if (scalars.empty()) return out;
        int rc = mi_g1_batch_mul(context(), &base, reinterpret_cast<const uint8_t*>(scalars.data()), scalars.size(), MI_SCALAR_MONTGOMERY, out.data());
        if (rc != MI_OK) throw std::runtime_error(std::string("batch_mul: ") + mi_msm_last_error(context()));
        return out;
    }
    // impl Valid: fn batch_check(batch) -> Result<(), SerializationError> (src/g1.rs:570-579: normalize_batch, then check() per affine point,
    // src/g1.rs:386-396).  true = every point is on the curve and in the prime-order subgroup (Ok(())), false = Err(InvalidData).
    static bool batch_check(const std::vector<G1Projective>& batch) {
        std::vector<G1Affine> aff = normalize_batch(batch);
        std::vector<uint8_t> st(aff.size());
        if (aff.empty()) return true;
        int rc = mi_g1_check_batch(context(), aff.data(), aff.size(), st.data());
        if (rc != MI_OK) throw std::runtime_error(std::string("batch_check: ") + mi_msm_last_error(context()));
        for (uint8_t s : st) if (s) return false;
        return true;
    }
    // iter::Sum (src/g1.rs:634-660)
    static G1Projective sum(const std::vector<G1Projective>& xs) {
        G1Projective r = zero();
        if (!xs.empty()) mi_g1_sum(reinterpret_cast<const mi_g1*>(xs.data()), xs.size(), &r.p);
        return r;
    }
};

struct G2Projective {
    mi_g2 p;                                        // blst_p2 (src/g2.rs:415-417)
    using MulBase = G2Affine;
    static constexpr bool NEGATION_IS_CHEAP = true;

    static G2Projective zero() { G2Projective r; std::memset(&r.p, 0, sizeof r.p); return r; }
    bool is_zero() const { mi_fp2 z{}; return std::memcmp(&p.z, &z, sizeof z) == 0; }

    static Result<G2Projective> msm(const std::vector<G2Affine>& bases, const std::vector<Scalar>& scalars) {
        if (bases.size() != scalars.size()) return Result<G2Projective>::Err(std::min(bases.size(), scalars.size()));
        G2Projective out;
        int rc = mi_msm_g2(context(), bases.data(), reinterpret_cast<const uint8_t*>(scalars.data()), bases.size(),
                           MI_SCALAR_MONTGOMERY, &out.p);
        return rc == MI_OK ? Result<G2Projective>::Ok(out) : Result<G2Projective>::Err(0);
    }
    static Result<G2Projective> msm_bigint(const std::vector<G2Affine>& bases, const std::vector<BigInteger256>& bigints) {
        if (bases.size() != bigints.size()) return Result<G2Projective>::Err(std::min(bases.size(), bigints.size()));
        G2Projective out;
        int rc = mi_msm_g2(context(), bases.data(), reinterpret_cast<const uint8_t*>(bigints.data()), bases.size(),
                           MI_SCALAR_CANONICAL, &out.p);
        return rc == MI_OK ? Result<G2Projective>::Ok(out) : Result<G2Projective>::Err(0);
    }
    static std::vector<G2Affine> normalize_batch(const std::vector<G2Projective>& projective) {
        std::vector<G2Affine> out(projective.size());
        if (projective.empty()) return out;
        int rc = mi_g2_normalize_batch(context(), reinterpret_cast<const mi_g2*>(projective.data()), projective.size(), out.data());
        if (rc != MI_OK) throw std::runtime_error(std::string("normalize_batch: ") + mi_msm_last_error(context()));
        return out;
    }
    static std::vector<G2Affine> batch_convert_to_mul_base(const std::vector<G2Projective>& bases) { return normalize_batch(bases); }
    // ScalarMul::batch_mul / FixedBase::msm + normalize_batch: out[i] = scalars[i] * base, the arkworks default the reference inherits
    // (src/g2.rs:573-580) — here a table walk on the GPU (include/arkblst_amd.h, mi_g2_batch_mul)
    static std::vector<G2Affine> batch_mul(const G2Affine& base, const std::vector<Scalar>& scalars) {
        std::vector<G2Affine> out(scalars.size());
        if (scalars.empty()) return out;
        int rc = mi_g2_batch_mul(context(), &base, reinterpret_cast<const uint8_t*>(scalars.data()), scalars.size(), MI_SCALAR_MONTGOMERY, out.data());
        if (rc != MI_OK) throw std::runtime_error(std::string("batch_mul: ") + mi_msm_last_error(context()));
        return out;
    }
    // impl Valid: batch_check (src/g2.rs:545-562, 366-376), as for G1
    static bool batch_check(const std::vector<G2Projective>& batch) {
        std::vector<G2Affine> aff = normalize_batch(batch);
        std::vector<uint8_t> st(aff.size());
        if (aff.empty()) return true;
        int rc = mi_g2_check_batch(context(), aff.data(), aff.size(), st.data());
        if (rc != MI_OK) throw std::runtime_error(std::string("batch_check: ") + mi_msm_last_error(context()));
        for (uint8_t s : st) if (s) return false;
        return true;
    }
    static G2Projective sum(const std::vector<G2Projective>& xs) {
        G2Projective r = zero();
        if (!xs.empty()) mi_g2_sum(reinterpret_cast<const mi_g2*>(xs.data()), xs.size(), &r.p);
        return r;
    }
};

// ark_poly::Radix2EvaluationDomain<Scalar> over the GPU transform (mi_fr_ntt).  The reference makes Scalar an FftField
// (the reference's src/scalar.rs:465-470: GENERATOR = 7, TWO_ADICITY = 32) and leaves the transforms to ark-poly's generic code, which has no
// trait method a field could override: a prover calls this type instead.  Vectors are `Scalar`s (Montgomery blst_fr), natural order.
struct Radix2EvaluationDomain {
    uint64_t size = 1;
    uint32_t log_size_of_group = 0;
    static constexpr uint32_t MAX_LOG_SIZE = 26;

    // fn new(num_coeffs: usize) -> Option<Self>: the next power of two; `false` above 2^26 elements
    static bool make(size_t num_coeffs, Radix2EvaluationDomain& out) {
        uint32_t log = 0;
        while (((size_t)1 << log) < num_coeffs) {
            if (++log > MAX_LOG_SIZE) return false;
        }
        out.size = (uint64_t)1 << log;
        out.log_size_of_group = log;
        return true;
    }
    static Scalar generator() { return Scalar{{0x0000000efffffff1ull, 0x17e363d300189c0full, 0xff9c57876f8457b0ull, 0x351332208fc5a8c4ull}}; }   // 7 R mod r

    std::vector<Scalar> fft(const std::vector<Scalar>& coeffs) const { return run(coeffs, 0, nullptr); }
    std::vector<Scalar> ifft(const std::vector<Scalar>& evals) const { return run(evals, 1, nullptr); }
    std::vector<Scalar> coset_fft(const std::vector<Scalar>& coeffs, const Scalar& offset = generator()) const { return run(coeffs, 0, &offset); }
    std::vector<Scalar> coset_ifft(const std::vector<Scalar>& evals, const Scalar& offset = generator()) const { return run(evals, 1, &offset); }

    // fft / ifft over DomainCoeff = G1Projective (the reference's src/g1.rs:215-226 makes it one), on affine points as the MSM takes its
    // bases (mi_g1_ntt, domains up to 2^24): ifft turns the monomial SRS [tau^j] G into the Lagrange-basis SRS [L_k(tau)] G.  The domain
    // must be the vector's size: ark-poly zero-pads a shorter one, and the zero of the group is the all-zero point the caller can append.
    std::vector<G1Affine> fft(const std::vector<G1Affine>& points) const { return run_g1(points, 0); }
    std::vector<G1Affine> ifft(const std::vector<G1Affine>& points) const { return run_g1(points, 1); }

private:
    std::vector<G1Affine> run_g1(const std::vector<G1Affine>& in, int inverse) const {
        if (in.size() != size) throw std::runtime_error("Radix2EvaluationDomain: the vector of points must have the domain's size");
        std::vector<G1Affine> out(in.size());
        int rc = mi_g1_ntt(context(), in.data(), log_size_of_group, inverse, out.data());
        if (rc != MI_OK) throw std::runtime_error(std::string("g1_ntt: ") + mi_msm_last_error(context()));
        return out;
    }
    // a shorter input is zero-padded to the domain (arkworks resizes it), a longer one is an error
    std::vector<Scalar> run(const std::vector<Scalar>& in, int inverse, const Scalar* offset) const {
        if (in.size() > size) throw std::runtime_error("Radix2EvaluationDomain: the input is longer than the domain");
        std::vector<Scalar> v(in);
        v.resize(size, Scalar{{0, 0, 0, 0}});
        int rc = mi_fr_ntt(context(), reinterpret_cast<const uint8_t*>(v.data()), log_size_of_group, 1, inverse, reinterpret_cast<const uint8_t*>(offset),
                           MI_SCALAR_MONTGOMERY, reinterpret_cast<uint8_t*>(v.data()));
        if (rc != MI_OK) throw std::runtime_error(std::string("fr_ntt: ") + mi_msm_last_error(context()));
        return v;
    }
};

// ark_poly::univariate::DensePolynomial<Scalar> where a KZG / Marlin / PLONK prover opens a commitment (mi_fr_poly_open): evaluate, and the
// division by (X - z) that ark-poly-commit's KZG10::compute_witness_polynomial runs on one CPU thread.  coeffs in ascending order, Montgomery blst_fr.
struct DensePolynomial {
    std::vector<Scalar> coeffs;
    static constexpr size_t MAX_COEFFS = (size_t)1 << 26;

    // fn evaluate(&self, point: &F) -> F
    Scalar evaluate(const Scalar& point) const {
        Scalar v{{0, 0, 0, 0}};
        if (coeffs.empty()) return v;   // the zero polynomial
        check(coeffs.size());
        int rc = mi_fr_poly_open(context(), reinterpret_cast<const uint8_t*>(coeffs.data()), coeffs.size(), 1, reinterpret_cast<const uint8_t*>(&point), 1,
                                 MI_SCALAR_MONTGOMERY, nullptr, reinterpret_cast<uint8_t*>(&v));
        if (rc != MI_OK) throw std::runtime_error(std::string("fr_poly_open: ") + mi_msm_last_error(context()));
        return v;
    }
    // (p(X) - p(z)) / (X - z), one coefficient shorter than p; *value = p(z) when asked for
    DensePolynomial divide_by_linear(const Scalar& point, Scalar* value = nullptr) const {
        DensePolynomial q;
        if (value) *value = Scalar{{0, 0, 0, 0}};
        if (coeffs.empty()) return q;
        check(coeffs.size());
        q.coeffs.resize(coeffs.size());
        int rc = mi_fr_poly_open(context(), reinterpret_cast<const uint8_t*>(coeffs.data()), coeffs.size(), 1, reinterpret_cast<const uint8_t*>(&point), 1,
                                 MI_SCALAR_MONTGOMERY, reinterpret_cast<uint8_t*>(q.coeffs.data()), reinterpret_cast<uint8_t*>(value));
        if (rc != MI_OK) throw std::runtime_error(std::string("fr_poly_open: ") + mi_msm_last_error(context()));
        q.coeffs.pop_back();   // the trailing zero that lets the device form feed the MSM over the same bases
        return q;
    }
    // KZG10::open on n coefficients in DEVICE memory over the n resident G1 bases of ctx (the SRS): divides on the device — into d_quotient, or
    // IN PLACE when it is nullptr: the coefficients are replaced by the quotient — and runs the MSM on the quotient as it is.
    // Returns the proof [q(tau)] G; *value = p(point).
    static G1Projective kzg10_open(mi_ctx* ctx, void* d_coeffs, size_t n, const Scalar& point, Scalar* value, void* d_quotient = nullptr) {
        if (n == 0) throw std::runtime_error("kzg10_open: no coefficients");
        check(n);
        void* d_q = d_quotient ? d_quotient : d_coeffs;
        G1Projective proof;
        int rc = mi_fr_poly_open_device(ctx, d_coeffs, n, 1, reinterpret_cast<const uint8_t*>(&point), 1, MI_SCALAR_MONTGOMERY, d_q, reinterpret_cast<uint8_t*>(value));
        if (rc == MI_OK) rc = mi_msm_g1_device(ctx, d_q, n, MI_SCALAR_MONTGOMERY, &proof.p);
        if (rc != MI_OK) throw std::runtime_error(std::string("kzg10_open: ") + mi_msm_last_error(ctx));
        return proof;
    }

private:
    static void check(size_t n) {
        if (n > MAX_COEFFS) throw std::runtime_error("DensePolynomial: more than 2^26 coefficients");
    }
};

// ark_ff::batch_inversion(&mut v): every non-zero element replaced by its inverse, zeros left as they are (mi_fr_batch_inverse; a vector of more
// than 2^26 elements goes through in pieces: the operation is element-wise).  Returns how many zeros there were.
inline size_t batch_inversion_and_mul(std::vector<Scalar>& v, const std::vector<Scalar>* coeffs);
inline size_t batch_inversion(std::vector<Scalar>& v) { return batch_inversion_and_mul(v, nullptr); }
// v[i] = coeffs[i] / v[i], zero where v[i] is zero: batch_inversion_and_mul with a multiplier per element, the element-wise quotient of two
// evaluation vectors (ark-poly's Evaluations / Evaluations)
inline size_t batch_inversion_and_mul(std::vector<Scalar>& v, const std::vector<Scalar>* coeffs) {
    if (coeffs && coeffs->size() != v.size()) throw std::runtime_error("batch_inversion_and_mul: the vectors differ in length");
    constexpr size_t STEP = (size_t)1 << 26;
    size_t zeros = 0;
    for (size_t lo = 0; lo < v.size(); lo += STEP) {
        const size_t cnt = std::min(STEP, v.size() - lo);
        size_t z = 0;
        uint8_t* p = reinterpret_cast<uint8_t*>(v.data() + lo);
        int rc = mi_fr_batch_inverse(context(), p, coeffs ? reinterpret_cast<const uint8_t*>(coeffs->data() + lo) : nullptr, cnt, MI_SCALAR_MONTGOMERY, p, &z);
        if (rc != MI_OK) throw std::runtime_error(std::string("fr_batch_inverse: ") + mi_msm_last_error(context()));
        zeros += z;
    }
    return zeros;
}
// The running product of a permutation argument on vectors in DEVICE memory: z[0] = 1, z[i+1] = z[i] num[i] / den[i], i < n, written to the n
// elements at d_out (which may be d_num or d_den): mi_fr_batch_inverse_device with the numerators, then the exclusive product scan in place.
// Returns the product of all n quotients (one for an argument that holds); *n_zero = zero denominators (their quotients count as zero).
inline Scalar grand_product(mi_ctx* ctx, const void* d_num, const void* d_den, size_t n, void* d_out, size_t* n_zero = nullptr) {
    if (n == 0) throw std::runtime_error("grand_product: no elements");
    Scalar total;
    int rc = mi_fr_batch_inverse_device(ctx, d_den, d_num, n, MI_SCALAR_MONTGOMERY, d_out, n_zero);
    if (rc == MI_OK) rc = mi_fr_scan_device(ctx, MI_FR_MUL, d_out, n, 1, 1, MI_SCALAR_MONTGOMERY, d_out, reinterpret_cast<uint8_t*>(&total));
    if (rc != MI_OK) throw std::runtime_error(std::string("grand_product: ") + mi_msm_last_error(ctx));
    return total;
}

// impl Pairing for Bls12 (/root/reference/src/pairing.rs:37-81): TargetField = Fp12, G1Prepared = G1Affine; G2 points are
// taken as plain affine points (the reference's G2Prepared is 68 precomputed lines; they are computed on the GPU instead).
using Fp12 = mi_fp12;
struct Bls12 {
    // fn multi_miller_loop(a: impl IntoIterator<G1Prepared>, b: impl IntoIterator<G2Prepared>) -> MillerLoopOutput
    // zip semantics: the shorter side decides (src/pairing.rs:55)
    static Fp12 multi_miller_loop(const std::vector<G1Affine>& a, const std::vector<G2Affine>& b) {
        Fp12 out;
        int rc = mi_multi_miller_loop(context(), a.data(), b.data(), std::min(a.size(), b.size()), &out);
        if (rc != MI_OK) throw std::runtime_error(std::string("multi_miller_loop: ") + mi_msm_last_error(context()));
        return out;
    }
    // fn final_exponentiation(f: MillerLoopOutput) -> Option<PairingOutput>: always Some (src/pairing.rs:76-80)
    static Fp12 final_exponentiation(const Fp12& f) {
        Fp12 out;
        mi_final_exponentiation(&f, &out);
        return out;
    }
    static Fp12 multi_pairing(const std::vector<G1Affine>& a, const std::vector<G2Affine>& b) {
        Fp12 out;
        int rc = mi_multi_pairing(context(), a.data(), b.data(), std::min(a.size(), b.size()), &out);
        if (rc != MI_OK) throw std::runtime_error(std::string("multi_pairing: ") + mi_msm_last_error(context()));
        return out;
    }
    static Fp12 pairing(const G1Affine& p, const G2Affine& q) { return multi_pairing({p}, {q}); }
};

}  // namespace ark_blst
