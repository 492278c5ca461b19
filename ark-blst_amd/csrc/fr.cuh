// BLS12-381 scalar field Fr on gfx950: 8 x 32-bit limbs, Montgomery radix R = 2^256 — blst_fr read as words, the in-memory form of the
// reference's `Scalar` (src/scalar.rs:23-25).  The field arithmetic of the NTT (ntt_kernels.cuh) and of mi_fr_vec_op_device, and the scalar
// prologue of the MSM's digit kernels and of the fixed-base walk (load_scalar).
// Every function takes operands below r and returns a value below r (fully reduced), so results compare bit for bit; the loads reduce
// whatever 256-bit value they are given.  One multiplication = 128 v_mad_u64_u32 (64 of the product, 64 of the reduction), straight-line.
// Compiles as plain C++ as well (tests/host/fr_host_check.cpp, fr_ntt_host.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include "fp28_consts.h"
#include "fr_consts.h"

#if defined(__HIPCC__)
#define FR_HD __host__ __device__ __forceinline__
#else
#define FR_HD inline
#endif

namespace fr {

struct Fr {
    uint32_t v[8];
};

constexpr unsigned FMT_CANONICAL = 0, FMT_MONTGOMERY = 1;   // MI_SCALAR_CANONICAL / MI_SCALAR_MONTGOMERY
constexpr unsigned FMT_RAW = 2;                             // a Montgomery value known to be below r (the passes' own intermediate vectors)

// a constant of fr_consts.h as a value (element by element: the tables are host constexpr arrays, usable in device code only as constants)
#define FR_CONST(NAME) (::fr::Fr{{frc::NAME[0], frc::NAME[1], frc::NAME[2], frc::NAME[3], frc::NAME[4], frc::NAME[5], frc::NAME[6], frc::NAME[7]}})
FR_HD Fr zero() {
    Fr r;
    for (int k = 0; k < 8; k++) r.v[k] = 0;
    return r;
}
FR_HD Fr one() { return FR_CONST(ONE); }
FR_HD bool is_zero(const Fr& a) {
    uint32_t o = 0;
    for (int k = 0; k < 8; k++) o |= a.v[k];
    return o == 0;
}
FR_HD bool equal(const Fr& a, const Fr& b) {
    uint32_t o = 0;
    for (int k = 0; k < 8; k++) o |= a.v[k] ^ b.v[k];
    return o == 0;
}

// t (8 limbs + the bit `top` above them) -> t - r when t >= r.  For t < 2r the result is below r.
FR_HD Fr cond_sub(const Fr& t, uint32_t top) {
    Fr d;
    uint64_t borrow = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 0; k < 8; k++) {
        const uint64_t x = (uint64_t)t.v[k] - fp28c::FR_MOD[k] - borrow;
        d.v[k] = (uint32_t)x;
        borrow = (x >> 32) & 1;
    }
    const bool ge = top != 0 || borrow == 0;
    Fr r;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 0; k < 8; k++) r.v[k] = ge ? d.v[k] : t.v[k];
    return r;
}

// any 256-bit value -> its residue below r: 2^256 / r < 3, so two conditional subtractions
FR_HD Fr reduce(const Fr& a) { return cond_sub(cond_sub(a, 0), 0); }

FR_HD Fr add(const Fr& a, const Fr& b) {   // a, b < r < 2^255: the sum fits 256 bits
    Fr t;
    uint64_t c = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 0; k < 8; k++) {
        c += (uint64_t)a.v[k] + b.v[k];
        t.v[k] = (uint32_t)c;
        c >>= 32;
    }
    return cond_sub(t, 0);
}

FR_HD Fr sub(const Fr& a, const Fr& b) {
    Fr d;
    uint64_t borrow = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 0; k < 8; k++) {
        const uint64_t x = (uint64_t)a.v[k] - b.v[k] - borrow;
        d.v[k] = (uint32_t)x;
        borrow = (x >> 32) & 1;
    }
    const uint32_t mask = borrow ? 0xffffffffu : 0u;   // a < b: add r back
    uint64_t c = 0;
    Fr r;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 0; k < 8; k++) {
        c += (uint64_t)d.v[k] + (fp28c::FR_MOD[k] & mask);
        r.v[k] = (uint32_t)c;
        c >>= 32;
    }
    return r;
}

// Montgomery product a b R^-1 mod r, operand scanning with the reduction interleaved (CIOS).  Every step is hi:lo = x * y + z + w on
// 32-bit words, which cannot overflow 64 bits: one v_mad_u64_u32 with a 64-bit addend.  a, b < r keep the running value below 2r < 2^256,
// so eight limbs and one conditional subtraction at the end suffice.
FR_HD Fr mul(const Fr& a, const Fr& b) {
    uint32_t t[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t t8 = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < 8; i++) {
        uint64_t c = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int j = 0; j < 8; j++) {
            c = (uint64_t)a.v[j] * b.v[i] + t[j] + c;
            t[j] = (uint32_t)c;
            c >>= 32;
        }
        c += t8;                                   // t < 2r + (2^32 - 1) r < 2^288: one limb and one bit above the eight
        const uint32_t hi = (uint32_t)c;
        const uint32_t hi2 = (uint32_t)(c >> 32);
        const uint32_t m = t[0] * fp28c::FR_INV32;
        c = (uint64_t)m * fp28c::FR_MOD[0] + t[0];
        c >>= 32;
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int j = 1; j < 8; j++) {
            c = (uint64_t)m * fp28c::FR_MOD[j] + t[j] + c;
            t[j - 1] = (uint32_t)c;
            c >>= 32;
        }
        c += hi;
        t[7] = (uint32_t)c;
        t8 = (uint32_t)(c >> 32) + hi2;
    }
    Fr r;
    for (int k = 0; k < 8; k++) r.v[k] = t[k];
    return cond_sub(r, t8);
}

FR_HD Fr to_mont(const Fr& a) { return mul(a, FR_CONST(R2)); }   // a < r
// Montgomery form -> canonical integer, a R^-1 mod r: the reduction half of mul alone (64 v_mad_u64_u32), for ANY 256-bit a.
// Device-side replacement for Scalar::into_bigint (/root/reference/src/scalar.rs:450-463,503-505).
FR_HD Fr from_mont(const Fr& a) {
    uint32_t t[9];
    for (int k = 0; k < 8; k++) t[k] = a.v[k];
    t[8] = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < 8; i++) {
        const uint32_t m = t[0] * fp28c::FR_INV32;
        uint64_t c = (uint64_t)m * fp28c::FR_MOD[0] + t[0];
        c >>= 32;
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int j = 1; j < 8; j++) {
            c += (uint64_t)m * fp28c::FR_MOD[j] + t[j];
            t[j - 1] = (uint32_t)c;
            c >>= 32;
        }
        c += t[8];
        t[7] = (uint32_t)c;
        t[8] = (uint32_t)(c >> 32);
    }
    Fr r;
    for (int k = 0; k < 8; k++) r.v[k] = t[k];
    return cond_sub(r, t[8]);   // t < 2r
}

// the caller's 32 bytes in scalar_fmt -> Montgomery form below r.  CANONICAL: any 256-bit integer, reduced modulo r (as load_scalar of the MSM
// reduces it).  MONTGOMERY: the value as it is, reduced modulo r.  RAW: taken on trust.
FR_HD Fr from_fmt(const Fr& w, unsigned fmt) {
    if (fmt == FMT_RAW) return w;
    const Fr x = reduce(w);
    return fmt == FMT_CANONICAL ? to_mont(x) : x;
}
FR_HD Fr to_fmt(const Fr& a, unsigned fmt) { return fmt == FMT_CANONICAL ? from_mont(a) : a; }

FR_HD Fr load_words(const uint32_t* p) {
    Fr r;
#if defined(__HIPCC__) && defined(__HIP_DEVICE_COMPILE__)
    const uint4 a = reinterpret_cast<const uint4*>(p)[0], b = reinterpret_cast<const uint4*>(p)[1];
    r.v[0] = a.x; r.v[1] = a.y; r.v[2] = a.z; r.v[3] = a.w; r.v[4] = b.x; r.v[5] = b.y; r.v[6] = b.z; r.v[7] = b.w;
#else
    for (int k = 0; k < 8; k++) r.v[k] = p[k];
#endif
    return r;
}
FR_HD void store_words(uint32_t* p, const Fr& a) {
#if defined(__HIPCC__) && defined(__HIP_DEVICE_COMPILE__)
    reinterpret_cast<uint4*>(p)[0] = make_uint4(a.v[0], a.v[1], a.v[2], a.v[3]);
    reinterpret_cast<uint4*>(p)[1] = make_uint4(a.v[4], a.v[5], a.v[6], a.v[7]);
#else
    for (int k = 0; k < 8; k++) p[k] = a.v[k];
#endif
}
// element i of a vector of 32-byte scalars (16-byte aligned) in `fmt`
FR_HD Fr load(const uint32_t* vec, size_t i, unsigned fmt) { return from_fmt(load_words(vec + i * 8), fmt); }
FR_HD void store(uint32_t* vec, size_t i, const Fr& a, unsigned fmt) { store_words(vec + i * 8, to_fmt(a, fmt)); }

FR_HD bool less(const Fr& a, const Fr& b) {   // as 256-bit integers
    uint64_t borrow = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 0; k < 8; k++) borrow = (((uint64_t)a.v[k] - b.v[k] - borrow) >> 32) & 1;
    return borrow != 0;
}

// Scalar i of an MSM or a fixed-base batch as the canonical integer s < r the digit recoding walks.
// fmt bit 0: the scalars are blst_fr Montgomery values (converted here); bit 1: sign fold (Plan::fold, host side).
// Canonical integers are expected below r, but any 256-bit value is accepted and reduced, so the signed recoding never carries out of
// the top window.  Without the fold s is recoded as it is — s P for ANY point P, the reference's semantics (blst's Pippenger,
// src/g1.rs:614-617, also for points that skipped Valid::check: Validate::No, src/g1.rs:425) — and `false` is returned.
// With the fold — only for resident bases that passed mi_msm_g{1,2}_validate_bases — a scalar above (r - 1) / 2 is replaced by
// r - s and `true` is returned: the caller inverts the sign of every digit (s P = (r - s)(-P) on the prime-order subgroup, and
// negating a point is free: NEGATION_IS_CHEAP, src/g1.rs:595).  The recoded values are then below 2^254, ceil(255 / c) windows
// always suffice and the signed recoding never carries out of the top window — for c = 15 and c = 17 (the divisors of 255) that
// removes the extra window whose single bucket collects a carry from 45 % of the points.
FR_HD bool load_scalar(uint32_t (&s)[8], const uint32_t* scalars, uint32_t i, unsigned fmt) {
    const Fr w = load_words(scalars + (size_t)i * 8);
    Fr x = (fmt & 1u) ? from_mont(w) : reduce(w);
    bool flip = false;
    if (fmt & 2u) {
        // s > (r - 1) / 2  <=>  2 s > r - 1  <=>  r - s < s, decided on d = -s = r - s (0 for s = 0, which never flips)
        const Fr d = sub(zero(), x);
        flip = less(d, x) && !is_zero(x);
        for (int k = 0; k < 8; k++) x.v[k] = flip ? d.v[k] : x.v[k];
    }
    for (int k = 0; k < 8; k++) s[k] = x.v[k];
    return flip;
}

// a^e for a 32-bit exponent (table entries: e < 2^26), left to right
FR_HD Fr pow_u32(const Fr& a, uint32_t e) {
    Fr r = one();
    bool any = false;
#if defined(__HIPCC__)
#pragma unroll 1
#endif
    for (int bit = 31; bit >= 0; bit--) {
        if (any) r = mul(r, r);
        if ((e >> bit) & 1u) {
            r = any ? mul(r, a) : a;
            any = true;
        }
    }
    return r;
}

// 1 / a = a^(r - 2) for a != 0 (host side: the inverse of a coset offset and of n, once per table)
inline Fr inverse(const Fr& a) {
    uint32_t e[8];   // r - 2
    uint64_t borrow = 2;
    for (int k = 0; k < 8; k++) {
        const uint64_t x = (uint64_t)fp28c::FR_MOD[k] - borrow;
        e[k] = (uint32_t)x;
        borrow = (x >> 32) & 1;
    }
    Fr r = one();
    for (int bit = 254; bit >= 0; bit--) {
        r = mul(r, r);
        if ((e[bit >> 5] >> (bit & 31)) & 1u) r = mul(r, a);
    }
    return r;
}

}  // namespace fr
