// Radix-2 NTT over G1 points (mi_g1_ntt, mi_g1_ntt_device): ark_poly::Radix2EvaluationDomain<Scalar>::{fft, ifft} over a Vec<G1Projective>
// (the reference's G1Projective is a DomainCoeff<Scalar>, src/g1.rs:215-226; the transform itself is ark-poly's generic code on the CPU).
// Host side of g1_ntt_kernels.cuh: the twiddle tables are mi_fr_ntt's, the context keeps two working vectors of projective points; a call is
// one launch per butterfly level, ping-pong between the two, and one pass of normalize_batch's product tree over the last level's output.
#define MI_NTT_PLAN_ONLY   // ntt_kernels.cuh without its kernels: fr_ntt.hip owns those
#include "msm_curve.hpp"
#include "g1_ntt_kernels.cuh"

namespace mi {

int g1_ntt(mi_ctx* ctx, const void* in, bool on_device, unsigned log_n, int inverse, void* out) {
    if (!ctx) return fail(ctx, MI_E_INVALID, "invalid argument");
    if (inverse != 0 && inverse != 1) return fail(ctx, MI_E_INVALID, "inverse must be 0 or 1");
    if (log_n > g1fft::MAX_LOG_N) return fail(ctx, MI_E_INVALID, "log_n must be at most 24");
    if (!in || !out) return fail(ctx, MI_E_INVALID, "invalid argument");
    if (on_device && ctx->devs.size() != 1) return fail(ctx, MI_E_INVALID, "the *_device entry points need a single-device context");
    const size_t n = (size_t)1 << log_n, bytes = n * sizeof(mi_g1_affine);
    LaneLock lk(ctx, true);
    return guarded(ctx, [&]() -> int {
        DevState& d = ctx->devs[0];
        const auto t0 = std::chrono::steady_clock::now();
        HIP_TRY(hipSetDevice(d.dev));
        if (on_device) {
            if (device_of_ptr(in, "d_in", 16) != d.dev || device_of_ptr(out, "d_out", 16) != d.dev)
                return fail(ctx, MI_E_INVALID, "device buffers must live on the context's device");
            const uintptr_t x = (uintptr_t)in, y = (uintptr_t)out;
            if (in != out && x < y + bytes && y < x + bytes) return fail(ctx, MI_E_INVALID, "d_in and d_out must be the same vector or not overlap at all");
        }
        mi_profile pr{};
        pr.n = n;
        if (log_n == 0) {   // the transform of one point is the point
            if (!on_device) {
                memmove(out, in, bytes);
            } else if (in != out) {
                HIP_TRY(hipMemcpyAsync(out, in, bytes, hipMemcpyDeviceToDevice, d.stream));
                HIP_TRY(hipStreamSynchronize(d.stream));
            }
            pr.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            set_prof(ctx, pr);
            return MI_OK;
        }
        const FrTable& tw = fr_ntt_twiddles(ctx, d, log_n, inverse, &pr.ingest_ms);
        for (DevBuf& b : ctx->g1_ntt_work) b.ensure(n * g1fft::PROJ_WORDS * 4);
        const void* src0 = in;
        if (!on_device) {
            d.io_in.ensure(bytes);
            src0 = d.io_in.p;
        }
        // ---- levels: passes of one level each; the last one writes work[0], the ones before alternate backwards between work[1] and work[0]
        const ntt::Plan plan = ntt::make_plan(log_n, 1, false);
        pr.num_windows = plan.passes;
        {
            const IoPlan whole{1, n};
            IoDrain drain(d);
            io_feed(d, whole, n, 0, on_device ? nullptr : in, d.io_in.p, sizeof(mi_g1_affine));
            HIP_TRY(hipEventRecord(d.iev[0][0], d.stream));
            for (unsigned k = 0; k < plan.passes; k++) {
                const ntt::Pass P = ntt::make_pass(plan, k, fr::FMT_RAW, inverse, (const uint32_t*)tw.lo.p, (const uint32_t*)tw.hi.p, tw.h, nullptr, nullptr, 0,
                                                   (const uint32_t*)src0, (uint32_t*)ctx->g1_ntt_work[0].p, (uint32_t*)ctx->g1_ntt_work[1].p);
                const uint32_t lanes = g1fft::lanes(P, inverse);
                hipLaunchKernelGGL(g1fft::k_g1_ntt_level, dim3((lanes + g1fft::THREADS - 1) / g1fft::THREADS), dim3(g1fft::THREADS), 0, d.stream, P, inverse);
                HIP_TRY(hipGetLastError());
            }
            HIP_TRY(hipEventRecord(d.iev[1][0], d.stream));
            io_finish(d);
            pr.accumulate_ms = ev_ms(d.iev[0][0], d.iev[1][0]);
            pr.h2d_ms = on_device ? 0.0 : ev_ms(d.cev[0], d.cev[1]);
        }
        // ---- affine points out: one product tree over the whole vector, one inversion.  The host form's results leave in chunks: up to eight
        // from 2^17 points on, every chunk with its own level-0 kernels of the tree and its own copy (normalize_run)
        size_t min_chunk = 65536;
#if defined(MI_TEST_HOOKS)
        // switch of the test build (tests/test_gpu_g1_ntt.py): smaller chunks, so that 2^10 points of the host form leave in eight
        if (const char* e = getenv("MI_TEST_G1NTT_CHUNK")) min_chunk = (size_t)std::max(64, atoi(e));
#endif
        const auto n0 = std::chrono::steady_clock::now();
        normalize_run<msmk::G1C>(ctx, d, nullptr, ctx->g1_ntt_work[0].p, n, on_device ? nullptr : out, on_device ? out : nullptr, false, min_chunk);
        pr.work_items = (uint32_t)io_plan(n, !on_device, (size_t)msmk::NORM_K * msmk::NORM_K, min_chunk).K;
        const auto t1 = std::chrono::steady_clock::now();
        pr.reduce_ms = std::chrono::duration<double, std::milli>(t1 - n0).count();
        pr.total_ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
        set_prof(ctx, pr);
        return MI_OK;
    });
}

}  // namespace mi
