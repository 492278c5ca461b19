// Fixed-base batch multiplication out[i] = s_i P (mi_g{1,2}_batch_mul, mi_g{1,2}_batch_mul_device): ark_ec FixedBase::msm followed by
// normalize_batch (src/g1.rs:593-600, src/g2.rs:573-580 leave both to the arkworks defaults, which run on the CPU).
// Host side of fixed_base_kernels.cuh: the context keeps the table of the last base per group; a call walks it in passes of
// fbm::PASS_POINTS scalars and normalises each pass with the product tree of normalize_batch.
#include "msm_curve.hpp"
#include "fixed_base_kernels.cuh"
#include "fixed_base_model.hpp"

namespace mi {
namespace {

// y^2 == x^3 + b on the host (host_curve.hpp): b = 4 for G1, 4 (1 + u) for G2
inline hostec::Fp fp_four() {
    const hostec::Fp two = hostec::Fp::one() + hostec::Fp::one();
    return two + two;
}
inline bool on_curve(const hostec::Fp& x, const hostec::Fp& y) { return y.sqr() == x.sqr() * x + fp_four(); }
inline bool on_curve(const hostec::Fp2& x, const hostec::Fp2& y) { return y.sqr() == x.sqr() * x + hostec::Fp2{fp_four(), fp_four()}; }

template <class C>
void launch_walk(hipStream_t s, const uint32_t* table, const uint32_t* scalars, size_t cnt, unsigned fmt, unsigned w, uint32_t W, uint32_t* jac) {
    const dim3 grid((uint32_t)((msmk::HotView<C>::LANES * cnt + 63) / 64));
    if constexpr (std::is_same<C, msmk::G2C>::value)
        hipLaunchKernelGGL((msmk::k_fb_walk_g2_coop<C>), grid, dim3(64), 0, s, table, scalars, (uint32_t)cnt, fmt, w, W, jac);
    else
        hipLaunchKernelGGL((msmk::k_fb_walk<C>), grid, dim3(64), 0, s, table, scalars, (uint32_t)cnt, fmt, w, W, jac);
}

// T[j][m - 1] = m 2^(w j) P for the finite curve point `base` (host memory, the reference's affine form) into tb.buf, all on the GPU
template <class C>
void build_table(DevState& d, FixedTable& tb, const void* base, unsigned w) {
    constexpr size_t PTB = (size_t)msmk::Geo<C>::PT_WORDS * 4, SLOTB = (size_t)msmk::Geo<C>::SLOT * 4, BKB = (size_t)msmk::Geo<C>::BK_WORDS * 4;
    const uint32_t W = fbm::windows(w);
    const size_t N = (size_t)fbm::entries(w);
    tb.valid = false;
    tb.buf.ensure_fit(N * PTB);
    const InvTree t(N);
    DevBuf raw, pt, ptflag, proj, flags, vals, pref, inv, top_raw;
    ScopedBufs guard{{&raw, &pt, &ptflag, &proj, &flags, &vals, &pref, &inv, &top_raw}};
    raw.ensure(aff_bytes<C>()); pt.ensure(PTB); ptflag.ensure(16);
    proj.ensure(N * BKB); flags.ensure(N);
    vals.ensure(t.total * SLOTB); pref.ensure(t.total * SLOTB); inv.ensure(t.total * SLOTB);
    top_raw.ensure(64 * sizeof(decltype(HostCurve<C>::J::inf().x)));
    hipStream_t s = d.stream;
    HIP_TRY(hipMemcpyAsync(raw.p, base, aff_bytes<C>(), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(msmk::k_ingest<C>, dim3(1), dim3(256), 0, s, (const uint32_t*)raw.p, (uint32_t*)pt.p, (uint8_t*)ptflag.p, 1u);
    hipLaunchKernelGGL(msmk::k_fb_bases<C>, dim3(1), dim3(64), 0, s, (const uint32_t*)pt.p, w, W, (uint32_t*)proj.p);
    for (uint32_t k = 0; k + 1 < w; k++)
        hipLaunchKernelGGL(msmk::k_fb_level<C>, dim3((uint32_t)((((size_t)W << k) + 255) / 256)), dim3(256), 0, s, (uint32_t*)proj.p, w, W, k);
    const uint32_t grid = (uint32_t)((N + 255) / 256);
    hipLaunchKernelGGL(msmk::k_fb_vals<C>, dim3(grid), dim3(256), 0, s, (const uint32_t*)proj.p, (uint32_t)N, (uint32_t*)vals.p, (uint8_t*)flags.p);
    HIP_TRY(hipGetLastError());
    invert_tree<C>(d, t, vals, pref, inv, top_raw);
    hipLaunchKernelGGL(msmk::k_table_affine<C>, dim3(grid), dim3(256), 0, s, (const uint32_t*)proj.p, (const uint32_t*)inv.p, (const uint8_t*)flags.p,
                       (uint32_t)N, (uint32_t*)tb.buf.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));   // the scratch above goes away
    tb.key.assign((const uint8_t*)base, (const uint8_t*)base + aff_bytes<C>());
    tb.w = w;
    tb.builds++;
    tb.valid = true;
}

template <class C, class Aff>
int batch_mul_impl(mi_ctx* ctx, const Aff* base, const uint8_t* scalars, bool on_device, size_t n, unsigned fmt, Aff* out) {
    using FE = decltype(HostCurve<C>::J::inf().x);
    static_assert(sizeof(Aff) == 2 * sizeof(FE), "affine layout");
    if (!ctx) return fail(ctx, MI_E_INVALID, "invalid argument");
    if (fmt != MI_SCALAR_CANONICAL && fmt != MI_SCALAR_MONTGOMERY) return fail(ctx, MI_E_INVALID, "unknown scalar_fmt");
    if (n == 0) return MI_OK;
    if (!base || !scalars || !out) return fail(ctx, MI_E_INVALID, "invalid argument");
    if (on_device && ctx->devs.size() != 1) return fail(ctx, MI_E_INVALID, "the *_device entry points need a single-device context");
    bool base_inf = true;
    for (size_t k = 0; k < sizeof(Aff); k++) base_inf = base_inf && reinterpret_cast<const uint8_t*>(base)[k] == 0;
    if (!base_inf) {
        FE xy[2];
        memcpy(xy, base, sizeof xy);
        if (!on_curve(xy[0], xy[1])) return fail(ctx, MI_E_INVALID, "base is neither a point of the curve nor the all-zero point at infinity");
    }
    LaneLock lk(ctx, true);
    return guarded(ctx, [&]() -> int {
        DevState& d = ctx->devs[0];
        const auto t0 = std::chrono::steady_clock::now();
        HIP_TRY(hipSetDevice(d.dev));
        if (on_device && (device_of_ptr(scalars, "d_scalars", 16) != d.dev || device_of_ptr(out, "d_out", 4) != d.dev))
            return fail(ctx, MI_E_INVALID, "device buffers must live on the context's device");
        mi_profile pr{};
        pr.n = n;
        if (base_inf) {   // s * infinity = infinity: every output is all-zero
            if (on_device) {
                for (size_t lo = 0; lo < n; lo += (size_t)1 << 24) {   // hipMemsetAsync sizes stay far below 2^32
                    const size_t cnt = std::min(n - lo, (size_t)1 << 24);
                    HIP_TRY(hipMemsetAsync((char*)out + lo * sizeof(Aff), 0, cnt * sizeof(Aff), d.stream));
                }
                HIP_TRY(hipStreamSynchronize(d.stream));
            } else {
                memset(out, 0, n * sizeof(Aff));
            }
            set_prof(ctx, pr);
            return MI_OK;
        }
        // ---- table: the one of the last base of this group when it still fits the request
        FixedTable& tb = ctx->fb[HostCurve<C>::IDX];
        const bool g2 = std::is_same<C, msmk::G2C>::value;
        const unsigned want = ctx->fb_forced_w ? ctx->fb_forced_w : fbm::choose_w(n, g2);
        const bool same = tb.valid && tb.key.size() == sizeof(Aff) && memcmp(tb.key.data(), base, sizeof(Aff)) == 0;
        // a forced w is taken literally; the built-in choice keeps a resident table that is at least as large (fewer additions, nothing to build)
        if (!(same && (ctx->fb_forced_w ? tb.w == want : tb.w >= want))) {
            const auto b0 = std::chrono::steady_clock::now();
            build_table<C>(d, tb, base, want);
            pr.ingest_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - b0).count();
        }
        const unsigned w = tb.w;
        const uint32_t W = fbm::windows(w);
        pr.window_bits = w;
        pr.num_windows = W;
        pr.work_items = (uint32_t)fbm::entries(w);
        // ---- passes: scalars in (host form: in chunks, the walk of a chunk under the copy of the next), walk, one batched inversion, points out
        const size_t pass = std::min(n, fbm::PASS_POINTS);
        d.fb_jac.ensure(pass * jac_bytes<C>());
        if (!on_device) d.scalars.ensure(pass * 32);
        for (size_t lo = 0; lo < n; lo += pass) {
            const size_t cnt = std::min(pass, n - lo);
            const uint32_t* d_sc = on_device ? (const uint32_t*)(scalars + lo * 32) : (const uint32_t*)d.scalars.p;
            double h2d = 0;
            pr.accumulate_ms += io_stream_pass(d, cnt, on_device ? nullptr : scalars + lo * 32, d.scalars.p, 32, nullptr, 0, [&](size_t clo, size_t ccnt) {
                launch_walk<C>(d.stream, (const uint32_t*)tb.buf.p, d_sc + clo * 8, ccnt, fmt, w, W, (uint32_t*)d.fb_jac.p + clo * msmk::Geo<C>::RAW_JAC);
            }, &h2d, (size_t)1 << 17);
            pr.h2d_ms += h2d;
            normalize_run<C>(ctx, d, nullptr, d.fb_jac.p, cnt, on_device ? nullptr : (void*)(out + lo), on_device ? (void*)(out + lo) : nullptr, false);
        }
        pr.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        set_prof(ctx, pr);
        return MI_OK;
    });
}

}  // namespace

int g1_batch_mul(mi_ctx* ctx, const mi_g1_affine* base, const uint8_t* scalars, bool on_device, size_t n, unsigned fmt, mi_g1_affine* out) {
    return batch_mul_impl<msmk::G1C>(ctx, base, scalars, on_device, n, fmt, out);
}
int g2_batch_mul(mi_ctx* ctx, const mi_g2_affine* base, const uint8_t* scalars, bool on_device, size_t n, unsigned fmt, mi_g2_affine* out) {
    return batch_mul_impl<msmk::G2C>(ctx, base, scalars, on_device, n, fmt, out);
}
int batch_mul_set_window_bits(mi_ctx* ctx, unsigned w) {
    if (!ctx || (w != 0 && (w < fbm::W_MIN || w > fbm::W_MAX))) return fail(ctx, MI_E_INVALID, "window_bits must be 0 or 8..16");
    LaneLock lk(ctx, true);
    ctx->fb_forced_w = w;
    return MI_OK;
}

}  // namespace mi
