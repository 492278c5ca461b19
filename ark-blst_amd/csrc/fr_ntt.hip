// Radix-2 NTT over the scalar field (mi_fr_ntt, mi_fr_ntt_device) and element-wise Fr operations (mi_fr_vec_op_device): what
// ark_poly::Radix2EvaluationDomain<Scalar>::{fft, ifft, coset_fft, coset_ifft} computes on the CPU beside every MSM of an arkworks prover
// (the reference makes Scalar an FftField, src/scalar.rs:465-470, and leaves the transform to ark-poly's generic code).
// Host side of ntt_kernels.cuh: the context keeps the tables of powers of the last few (size, direction, offset) and one scratch vector;
// a call is a few passes that alternate between the caller's vectors and the scratch.
#include "internal.hpp"
#include "io_chunks.hpp"
#include "ntt_kernels.cuh"

namespace mi {
namespace {

using fr::Fr;

Fr fr_from_bytes(const uint8_t* p) {
    Fr r;
    memcpy(r.v, p, 32);
    return r;
}
void launch_powers(hipStream_t s, DevBuf& buf, size_t first, const Fr& base, const Fr& scale, uint32_t count) {
    hipLaunchKernelGGL(ntt::k_fr_powers, dim3((count + ntt::THREADS - 1) / ntt::THREADS), dim3(ntt::THREADS), 0, s, (uint32_t*)buf.p + first * 8, base, scale, count);
    HIP_TRY(hipGetLastError());
}

// the table of (coset, log_n, inverse, key), built on a miss (*built_ms gets the time) and stamped as the most recently used
FrTable& table_for(mi_ctx* ctx, DevState& d, bool coset, unsigned log_n, int inverse, const Fr& x, double* built_ms) {
    uint8_t key[32] = {};
    if (coset) memcpy(key, x.v, 32);
    for (FrTable& t : ctx->ntt_tables)
        if (t.coset == coset && t.log_n == log_n && t.inverse == inverse && memcmp(t.key, key, 32) == 0) {
            t.stamp = ++ctx->ntt_clock;
            return t;
        }
    const auto t0 = std::chrono::steady_clock::now();
    if (ctx->ntt_tables.size() >= FR_TABLES_KEPT) {   // the least recently used one leaves
        size_t old = 0;
        for (size_t k = 1; k < ctx->ntt_tables.size(); k++)
            if (ctx->ntt_tables[k].stamp < ctx->ntt_tables[old].stamp) old = k;
        ctx->ntt_tables[old].lo.release();
        ctx->ntt_tables[old].hi.release();
        ctx->ntt_tables.erase(ctx->ntt_tables.begin() + (long)old);
    }
    FrTable t;
    t.coset = coset;
    t.log_n = log_n;
    t.inverse = inverse;
    memcpy(t.key, key, 32);
    const ntt::TableSpec sp = ntt::table_spec(coset, log_n, inverse, x);
    t.h = sp.h;
    try {
        t.lo.ensure(((size_t)sp.n_lo + 1) * 32);
        t.hi.ensure((size_t)sp.n_hi * 32);
        launch_powers(d.stream, t.lo, 0, sp.base, sp.scale, sp.n_lo);
        launch_powers(d.stream, t.lo, sp.n_lo, fr::one(), sp.ninv, 1);   // 1 / n behind the powers (the constant factor of a plain inverse)
        launch_powers(d.stream, t.hi, 0, sp.hi_base, fr::one(), sp.n_hi);
        HIP_TRY(hipStreamSynchronize(d.stream));
    } catch (...) {
        t.lo.release();
        t.hi.release();
        throw;
    }
    t.stamp = ++ctx->ntt_clock;
    ctx->ntt_tables.push_back(t);
    *built_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return ctx->ntt_tables.back();
}

bool ranges_overlap(const void* a, const void* b, size_t bytes) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + bytes && y < x + bytes;
}

int ntt_impl(mi_ctx* ctx, const uint8_t* in, bool on_device, unsigned log_n, size_t batch, int inverse, const uint8_t* coset_offset, unsigned fmt, uint8_t* out) {
    if (!ctx) return fail(ctx, MI_E_INVALID, "invalid argument");
    if (fmt != MI_SCALAR_CANONICAL && fmt != MI_SCALAR_MONTGOMERY) return fail(ctx, MI_E_INVALID, "unknown scalar_fmt");
    if (inverse != 0 && inverse != 1) return fail(ctx, MI_E_INVALID, "inverse must be 0 or 1");
    if (log_n > ntt::MAX_LOG_N) return fail(ctx, MI_E_INVALID, "log_n must be at most 26");
    if (batch == 0 || batch > (SIZE_MAX >> (log_n + 6))) return fail(ctx, MI_E_INVALID, "batch must be at least 1 and batch * 2^log_n * 32 must fit size_t");
    if (!in || !out) return fail(ctx, MI_E_INVALID, "invalid argument");
    Fr g = fr::one();
    if (coset_offset) {
        g = fr::from_fmt(fr_from_bytes(coset_offset), fmt);
        if (fr::is_zero(g)) return fail(ctx, MI_E_INVALID, "the coset offset must not be zero");
    }
    if (on_device && ctx->devs.size() != 1) return fail(ctx, MI_E_INVALID, "the *_device entry points need a single-device context");
    const size_t total = batch << log_n, bytes = total * 32;
    LaneLock lk(ctx, true);
    return guarded(ctx, [&]() -> int {
        DevState& d = ctx->devs[0];
        const auto t0 = std::chrono::steady_clock::now();
        HIP_TRY(hipSetDevice(d.dev));
        if (on_device) {
            if (device_of_ptr(in, "d_in", 16) != d.dev || device_of_ptr(out, "d_out", 16) != d.dev)
                return fail(ctx, MI_E_INVALID, "device buffers must live on the context's device");
            if (in != out && ranges_overlap(in, out, bytes)) return fail(ctx, MI_E_INVALID, "d_in and d_out must be the same vector or not overlap at all");
        }
        mi_profile pr{};
        pr.n = total;
        // ---- tables
        const FrTable* cs = nullptr;
        if (coset_offset) cs = &table_for(ctx, d, true, log_n, inverse, g, &pr.ingest_ms);
        const FrTable& tw = table_for(ctx, d, false, log_n, inverse, g, &pr.ingest_ms);
        if (coset_offset)   // building the twiddles may have evicted or moved the entry above: look it up again (a hit)
            cs = &table_for(ctx, d, true, log_n, inverse, g, &pr.ingest_ms);
        // ---- plan
        unsigned cap = ntt::MAX_LEVELS;
#if defined(MI_TEST_HOOKS)
        // switch of the test build (tests/test_gpu_fr_ntt.py): fewer levels per pass, so that small sizes run the multi-pass structure
        if (const char* e = getenv("MI_TEST_NTT_TILE_BITS")) cap = (unsigned)std::min<int>((int)ntt::MAX_LEVELS, std::max(1, atoi(e)));
#endif
        const uint8_t *src0 = in;
        uint8_t* dst_last = out;
        if (!on_device) {
            d.io_in.ensure(bytes);
            d.io_out.ensure(bytes);
            src0 = (const uint8_t*)d.io_in.p;
            dst_last = (uint8_t*)d.io_out.p;
        }
        const ntt::Plan plan = ntt::make_plan(log_n, cap, src0 == dst_last);
        pr.num_windows = plan.passes;
        pr.window_bits = plan.widest;
        if (plan.passes > 1) ctx->ntt_scratch.ensure(bytes);
        // ---- passes: the last one writes the output, the ones before alternate backwards between the scratch vector and the output
        const IoPlan whole{1, total};
        IoDrain drain(d);
        io_feed(d, whole, total, 0, on_device ? nullptr : in, d.io_in.p, 32);
        HIP_TRY(hipEventRecord(d.iev[0][0], d.stream));
        for (unsigned k = 0; k < plan.passes; k++) {
            const ntt::Pass P = ntt::make_pass(plan, k, fmt, inverse, (const uint32_t*)tw.lo.p, (const uint32_t*)tw.hi.p, tw.h, cs ? (const uint32_t*)cs->lo.p : nullptr,
                                               cs ? (const uint32_t*)cs->hi.p : nullptr, cs ? cs->h : 0, (const uint32_t*)src0, (uint32_t*)dst_last,
                                               (uint32_t*)ctx->ntt_scratch.p);
            const uint64_t blocks = (uint64_t)batch * ntt::tiles_per_vector(P);
            for (uint64_t b0 = 0; b0 < blocks; b0 += (uint64_t)1 << 30) {
                const uint32_t cnt = (uint32_t)std::min<uint64_t>(blocks - b0, (uint64_t)1 << 30);
                hipLaunchKernelGGL(ntt::k_ntt_pass, dim3(cnt), dim3(ntt::THREADS), 0, d.stream, P, b0);
            }
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipEventRecord(d.iev[1][0], d.stream));
        const IoOut res{on_device ? nullptr : (void*)out, d.io_out.p, 32};
        io_drain_chunk(d, whole, total, 0, d.iev[1][0], &res, 1);
        io_finish(d);
        pr.accumulate_ms = ev_ms(d.iev[0][0], d.iev[1][0]);
        pr.h2d_ms = on_device ? 0.0 : ev_ms(d.cev[0], d.cev[1]);
        pr.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        set_prof(ctx, pr);
        return MI_OK;
    });
}

}  // namespace

const FrTable& fr_ntt_twiddles(mi_ctx* ctx, DevState& d, unsigned log_n, int inverse, double* built_ms) {
    return table_for(ctx, d, false, log_n, inverse, fr::one(), built_ms);
}

int fr_ntt(mi_ctx* ctx, const uint8_t* in, bool on_device, unsigned log_n, size_t batch, int inverse, const uint8_t* coset_offset, unsigned fmt, uint8_t* out) {
    return ntt_impl(ctx, in, on_device, log_n, batch, inverse, coset_offset, fmt, out);
}

int fr_vec_op(mi_ctx* ctx, int op, const void* d_a, const void* d_b, size_t n, unsigned fmt, void* d_out) {
    if (!ctx) return fail(ctx, MI_E_INVALID, "invalid argument");
    if (op != MI_FR_MUL && op != MI_FR_ADD && op != MI_FR_SUB) return fail(ctx, MI_E_INVALID, "unknown op");
    if (fmt != MI_SCALAR_CANONICAL && fmt != MI_SCALAR_MONTGOMERY) return fail(ctx, MI_E_INVALID, "unknown scalar_fmt");
    if (n > (SIZE_MAX >> 6)) return fail(ctx, MI_E_INVALID, "n * 32 must fit size_t");
    if (n == 0) return MI_OK;
    if (!d_a || !d_b || !d_out) return fail(ctx, MI_E_INVALID, "invalid argument");
    if (ctx->devs.size() != 1) return fail(ctx, MI_E_INVALID, "the *_device entry points need a single-device context");
    LaneLock lk(ctx, true);
    return guarded(ctx, [&]() -> int {
        DevState& d = ctx->devs[0];
        HIP_TRY(hipSetDevice(d.dev));
        if (device_of_ptr(d_a, "d_a", 16) != d.dev || device_of_ptr(d_b, "d_b", 16) != d.dev || device_of_ptr(d_out, "d_out", 16) != d.dev)
            return fail(ctx, MI_E_INVALID, "device buffers must live on the context's device");
        for (const void* x : {d_a, d_b})
            if (x != d_out && ranges_overlap(x, d_out, n * 32)) return fail(ctx, MI_E_INVALID, "d_out must be one of the inputs or not overlap them at all");
        const uint32_t grid = (uint32_t)std::min<size_t>((n + ntt::THREADS - 1) / ntt::THREADS, (size_t)1 << 16);
        hipLaunchKernelGGL(ntt::k_fr_vec_op, dim3(grid), dim3(ntt::THREADS), 0, d.stream, (const uint32_t*)d_a, (const uint32_t*)d_b, (uint32_t*)d_out, n, op,
                           fmt);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(d.stream));
        return MI_OK;
    });
}

}  // namespace mi
