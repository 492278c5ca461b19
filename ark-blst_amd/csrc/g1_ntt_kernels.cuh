// Radix-2 NTT over G1 points (mi_g1_ntt): the butterfly whose multiply is a scalar multiplication on the curve.
//
// What ark_poly::Radix2EvaluationDomain<Scalar>::{fft, ifft} computes over a Vec<G1Projective> (the reference's G1Projective is a
// DomainCoeff<Scalar>: impl_add_sub_assign! / impl_mul_assign!(G1Projective, Scalar), src/g1.rs:215-226): a powers-of-tau SRS [tau^j] G
// becomes the Lagrange-basis SRS [L_k(tau)] G.  Natural order in and out, the root of unity of mi_fr_ntt.
//
// One butterfly level per launch, one lane per butterfly.  The levels are the passes of one level (b = 1) of ntt::make_pass — the
// self-sorting Stockham map of ntt_kernels.cuh, decimation in frequency: butterfly i < n / 2 of the level with s = 2^log_s, q = i mod s,
// p = i / s reads in[i] = a and in[i + n / 2] = b and writes
//     out[q + 2 s p] = a + b,      out[q + 2 s p + s] = [t] (a - b),   t = w^(s p)
// so the last level leaves the natural order and every twiddle of it is 1.  [t] is a left-to-right double-and-add over the non-adjacent form
// of the integer t (digits -1, 0, 1: 255 doublings and about 85 additions), ec::proj_dbl and the complete ec::proj_add: no branch rests on
// the inputs being points of the prime-order subgroup, infinity (0 : 1 : 0) needs no case of its own.  A butterfly with t = 1 does not multiply.
// t comes from the tables of mi_fr_ntt (ntt::twiddle: two halves joined by one fr::mul) and leaves Montgomery form in the lane.
//
// The factor 1 / n of the inverse direction rides on twiddles that are applied anyway.  Output k takes the difference branch at level l
// exactly when bit l of k is set, and q == 0 at level l says "sum branch at every level before": the butterflies with q == 0 multiply their
// difference by t / n instead of t, which scales every output k != 0 exactly once, at the lowest set bit of k.  That leaves the butterfly
// (q = 0, p = 0) of every level, whose t would have been 1, and output 0, the sum of the last level's butterfly 0, which one extra lane of
// that launch scales: log_n + 1 scalar multiplications more than the forward direction, where scaling the input or the output costs n.
//
// The first level reads the caller's affine points (all-zero = infinity), the levels between ping-pong between two vectors of projective
// points in the device limb form (three 16-word slots), the last level stores the reference's Jacobian form (X Z, Y Z^2, Z), which the
// product tree of normalize_batch turns into affine points with one inversion.
// About 300 B moved per butterfly against some 3000 field multiplications: compute-bound, nothing is tiled in LDS.
// Launch-bounds rule of curve_kernels.cuh: the kernel contains calls (the shared multiplier of ec::FpOps) and is built for two waves per
// SIMD — 256 registers, no AGPRs, no spills.  Two things keep it there: the sum of a butterfly leaves before the difference is formed
// (two points live, not three), and the point a ladder multiplies waits in LDS (Park) instead of in 42 registers.
// Everything but the kernel is plain C++: tests/host/g1_ntt_host.cpp runs the same functions as a serial loop over the lanes.
#pragma once
#include "ec.cuh"
#include "ntt_kernels.cuh"

namespace g1fft {

constexpr unsigned MAX_LOG_N = 24;
constexpr unsigned THREADS = 64;
constexpr int AFF_WORDS = 24, JAC_WORDS = 36, PROJ_WORDS = 48;   // mi_g1_affine, mi_g1, a projective point of a working vector

// ---------------------------------------------------------------------------------------------- recoding
// Non-adjacent form of an integer t < 2^255: t = sum_i (pos_i - neg_i) 2^i, i < 256, no two neighbouring digits non-zero.
// Digit i is bit i + 1 of 3 t minus bit i + 1 of t.
struct Digits {
    uint32_t pos[8], neg[8];
};
FR_HD Digits recode(const fr::Fr& t) {
    uint32_t x[9], x3[9];
    uint64_t c = 0;
    for (int k = 0; k < 8; k++) {
        x[k] = t.v[k];
        c += (uint64_t)t.v[k] + (uint32_t)((t.v[k] << 1) | (k ? t.v[k - 1] >> 31 : 0u));
        x3[k] = (uint32_t)c;
        c >>= 32;
    }
    x[8] = 0;
    x3[8] = (uint32_t)c + (t.v[7] >> 31);
    Digits d;
    for (int k = 0; k < 8; k++) {
        const uint32_t p0 = x3[k] & ~x[k], p1 = x3[k + 1] & ~x[k + 1], n0 = x[k] & ~x3[k], n1 = x[k + 1] & ~x3[k + 1];
        d.pos[k] = (p0 >> 1) | (p1 << 31);
        d.neg[k] = (n0 >> 1) | (n1 << 31);
    }
    return d;
}

// Where a lane parks the point it multiplies while the ladder runs: 42 limbs it reads once per addition and must not hold in registers
// beside the running sum, the digits and the addition's temporaries (256 registers, no spills).  Word k of the lane sits at w[k stride]:
// the kernel gives every lane a column of a 42 x 64 word block of LDS (neighbouring lanes, neighbouring banks), the host a plain array.
constexpr int PARK_WORDS = 3 * fp28::NL;
struct Park {
    uint32_t* w;
    uint32_t stride;
};
template <class F>
FP_HD void park_put(const Park& pk, const ec::Proj<F>& p) {
    for (int k = 0; k < fp28::NL; k++) {
        pk.w[(size_t)k * pk.stride] = p.x.l[k];
        pk.w[(size_t)(fp28::NL + k) * pk.stride] = p.y.l[k];
        pk.w[(size_t)(2 * fp28::NL + k) * pk.stride] = p.z.l[k];
    }
}
template <class F>
FP_HD ec::Proj<F> park_get(const Park& pk) {
    ec::Proj<F> p;
    for (int k = 0; k < fp28::NL; k++) {
        p.x.l[k] = pk.w[(size_t)k * pk.stride];
        p.y.l[k] = pk.w[(size_t)(fp28::NL + k) * pk.stride];
        p.z.l[k] = pk.w[(size_t)(2 * fp28::NL + k) * pk.stride];
    }
    return p;
}

// [t] p for the digits of t, left to right; p is parked (coordinates below 4p).
template <class F>
FP_HD ec::Proj<F> scalar_mul(const Park& pk, Digits dg) {
    ec::Proj<F> acc = ec::proj_inf<F>();
#if defined(__HIPCC__)
#pragma unroll 1
#endif
    for (int i = 255; i >= 0; i--) {
        ec::proj_dbl<F>(acc);
        const bool plus = (dg.pos[7] >> 31) != 0, minus = (dg.neg[7] >> 31) != 0;
        if (plus || minus) {
            ec::Proj<F> q = park_get<F>(pk);
            q.y = F::select(minus, q.y, F::template neg<4>(q.y));
            ec::proj_add<F>(acc, q);
        }
        for (int k = 7; k > 0; k--) {
            dg.pos[k] = (dg.pos[k] << 1) | (dg.pos[k - 1] >> 31);
            dg.neg[k] = (dg.neg[k] << 1) | (dg.neg[k - 1] >> 31);
        }
        dg.pos[0] <<= 1;
        dg.neg[0] <<= 1;
    }
    return acc;
}

// ---------------------------------------------------------------------------------------------- the level plan
// lanes of a level: its n / 2 butterflies, and for the last level of the inverse direction one more (output 0's factor 1 / n)
FR_HD bool last_level(const ntt::Pass& P) { return P.log_s + 1u == P.log_n; }
FR_HD uint32_t lanes(const ntt::Pass& P, int inverse) { return (1u << (P.log_n - 1u)) + (inverse && last_level(P) ? 1u : 0u); }

struct Fly {
    uint32_t src0, src1, dst0, dst1;
    uint32_t e;        // the twiddle is w^e
    bool first_sum;    // q == 0: no difference branch on the way here
};
FR_HD Fly fly_at(const ntt::Pass& P, uint32_t i) {
    const uint32_t q = i & ((1u << P.log_s) - 1u), p = i >> P.log_s;
    Fly f;
    f.src0 = i;
    f.src1 = i + (1u << (P.log_n - 1u));
    f.dst0 = q + ((2u * p) << P.log_s);
    f.dst1 = f.dst0 + (1u << P.log_s);
    f.e = p << P.log_s;
    f.first_sum = q == 0;
    return f;
}
// the integer a lane walks: w^e, times 1 / n where the butterfly carries the inverse's factor (P.f_lo: make_pass points it at 1 / n)
FR_HD fr::Fr fly_scalar(const ntt::Pass& P, const Fly& f, bool scaled) {
    fr::Fr t = f.e ? ntt::twiddle(P, f.e, P.log_s) : fr::one();
    if (scaled) t = fr::mul(t, fr::load_words(P.f_lo));
    return fr::from_mont(t);
}

// ---------------------------------------------------------------------------------------------- points in memory
FP_HD fp28::Fp load_slot(const uint32_t* p) {
    fp28::Fp r;
#if defined(__HIPCC__) && defined(__HIP_DEVICE_COMPILE__)
    const uint4* v = reinterpret_cast<const uint4*>(p);
    const uint4 a = v[0], b = v[1], c = v[2], d = v[3];
    r.l[0] = a.x; r.l[1] = a.y; r.l[2] = a.z; r.l[3] = a.w; r.l[4] = b.x; r.l[5] = b.y; r.l[6] = b.z; r.l[7] = b.w;
    r.l[8] = c.x; r.l[9] = c.y; r.l[10] = c.z; r.l[11] = c.w; r.l[12] = d.x; r.l[13] = d.y;
#else
    for (int k = 0; k < fp28::NL; k++) r.l[k] = p[k];
#endif
    return r;
}
FP_HD void store_slot(uint32_t* p, const fp28::Fp& a) {
#if defined(__HIPCC__) && defined(__HIP_DEVICE_COMPILE__)
    uint4* v = reinterpret_cast<uint4*>(p);
    v[0] = make_uint4(a.l[0], a.l[1], a.l[2], a.l[3]);
    v[1] = make_uint4(a.l[4], a.l[5], a.l[6], a.l[7]);
    v[2] = make_uint4(a.l[8], a.l[9], a.l[10], a.l[11]);
    v[3] = make_uint4(a.l[12], a.l[13], 0u, 0u);
#else
    for (int k = 0; k < fp28::NL; k++) p[k] = a.l[k];
    p[14] = p[15] = 0;
#endif
}
// What a level reads and writes.  The first level reads mi_g1_affine, the last writes mi_g1, everything between is PROJ_WORDS per point.
template <class F>
struct LevelIo {
    const uint32_t* src;
    uint32_t* dst;
    bool first, last;
    FP_HD ec::Proj<F> load(uint32_t idx) const {
        ec::Proj<F> r;
        if (first) {
            const uint32_t* p = src + (size_t)idx * AFF_WORDS;
            uint32_t x[12], y[12], any = 0;
            for (int k = 0; k < 12; k++) {
                x[k] = p[k];
                y[k] = p[12 + k];
                any |= x[k] | y[k];
            }
            r = ec::proj_from_affine<F>(fp28::fp_from_blst(x), fp28::fp_from_blst(y));
            const ec::Proj<F> inf = ec::proj_inf<F>();
            return ec::proj_select<F>(any == 0, r, inf);
        }
        const uint32_t* p = src + (size_t)idx * PROJ_WORDS;
        r.x = load_slot(p);
        r.y = load_slot(p + 16);
        r.z = load_slot(p + 32);
        return r;
    }
    FP_HD void store(uint32_t idx, const ec::Proj<F>& r) const {
        if (last) {   // (X Z, Y Z^2, Z); infinity (Z == 0) is all-zero
            uint32_t* o = dst + (size_t)idx * JAC_WORDS;
            uint32_t xw[12], yw[12], zw[12], any = 0;
            fp28::fp_to_blst(zw, r.z);
            fp28::fp_to_blst(xw, F::mul(r.x, r.z));
            fp28::fp_to_blst(yw, F::mul(r.y, F::sqr(r.z)));
            for (int k = 0; k < 12; k++) any |= zw[k];
            for (int k = 0; k < 12; k++) {
                o[k] = any ? xw[k] : 0u;
                o[12 + k] = any ? yw[k] : 0u;
                o[24 + k] = zw[k];
            }
            return;
        }
        uint32_t* o = dst + (size_t)idx * PROJ_WORDS;
        store_slot(o, r.x);
        store_slot(o + 16, r.y);
        store_slot(o + 32, r.z);
    }
};
template <class F>
FR_HD LevelIo<F> level_io(const ntt::Pass& P) {
    return LevelIo<F>{P.src, P.dst, P.log_s == 0, last_level(P)};
}

// ---------------------------------------------------------------------------------------------- one lane of a level
template <class F>
FP_HD void level_lane(const ntt::Pass& P, int inverse, uint32_t i, const Park& pk) {
    const LevelIo<F> io = level_io<F>(P);
    const bool only_sum = (i >> (P.log_n - 1u)) != 0;   // the extra lane of the inverse's last level: butterfly 0 again, for output 0
    const Fly f = fly_at(P, only_sum ? 0u : i);
    const bool scaled = inverse && f.first_sum;
    // the sum leaves before the difference is formed, and the difference reads its operands again: two points live at a time, not three
    if (!only_sum && !(scaled && last_level(P))) {
        ec::Proj<F> s = io.load(f.src0);
        ec::proj_add<F>(s, io.load(f.src1));
        io.store(f.dst0, s);
    }
    ec::Proj<F> d = io.load(f.src0);
    {
        ec::Proj<F> b = io.load(f.src1);
        b.y = F::select(only_sum, F::template neg<4>(b.y), b.y);
        ec::proj_add<F>(d, b);
    }
    if (scaled || f.e) {
        park_put<F>(pk, d);
        d = scalar_mul<F>(pk, recode(fly_scalar(P, f, scaled)));
    }
    io.store(only_sum ? f.dst0 : f.dst1, d);
}

#if defined(__HIPCC__)
__global__ void __launch_bounds__(THREADS, 2) k_g1_ntt_level(const ntt::Pass P, const int inverse) {
    __shared__ uint32_t park[PARK_WORDS * THREADS];
    const uint32_t i = blockIdx.x * THREADS + threadIdx.x;
    if (i >= lanes(P, inverse)) return;
    level_lane<ec::FpOps>(P, inverse, i, Park{park + threadIdx.x, THREADS});
}
#endif

}  // namespace g1fft
