// Opening polynomials over the scalar field at a point (mi_fr_poly_open, mi_fr_poly_open_device): p(z) and the witness polynomial
// (p(X) - p(z)) / (X - z) — ark_poly's DensePolynomial::evaluate and its division by a linear factor, which ark-poly-commit's
// KZG10::compute_witness_polynomial runs on one CPU thread between the commitment and the proof's MSM.
// Host side of poly_kernels.cuh: the level plan, the table of powers of every point (a few dozen multiplications on the host, one upload per
// call), the context's scratch vector of tile totals, and one launch per level and sweep.
#include "internal.hpp"
#include "io_chunks.hpp"
#include "poly_kernels.cuh"

namespace mi {
namespace {

using fr::Fr;

bool ranges_overlap(const void* a, const void* b, size_t bytes) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + bytes && y < x + bytes;
}

template <unsigned K>
void launch_sweep(hipStream_t s, const poly::Level& P, size_t batch, bool down) {
    const uint64_t blocks = poly::blocks_of(P, batch);
    for (uint64_t b0 = 0; b0 < blocks; b0 += (uint64_t)1 << 30) {
        const uint32_t cnt = (uint32_t)std::min<uint64_t>(blocks - b0, (uint64_t)1 << 30);
        if (down) hipLaunchKernelGGL(poly::k_poly_down<K>, dim3(cnt), dim3(poly::THREADS), 0, s, P, b0);
        else hipLaunchKernelGGL(poly::k_poly_up<K>, dim3(cnt), dim3(poly::THREADS), 0, s, P, b0);
    }
    HIP_TRY(hipGetLastError());
}
void launch_sweep(hipStream_t s, const poly::Level& P, size_t batch, bool down) {
#if defined(MI_TEST_HOOKS)
    if (poly::lane_bits(P.tile_bits) == 0) return launch_sweep<1>(s, P, batch, down);   // reduced tiles: one element per lane
#endif
    launch_sweep<poly::LANE_ELEMS>(s, P, batch, down);
}

int poly_impl(mi_ctx* ctx, const uint8_t* coeffs, bool on_device, size_t n, size_t batch, const uint8_t* points, size_t n_points, unsigned fmt,
              uint8_t* quotients, uint8_t* values) {
    if (!ctx || !coeffs || !points) return fail(ctx, MI_E_INVALID, "invalid argument");
    if (!quotients && !values) return fail(ctx, MI_E_INVALID, "quotients and values must not both be NULL");
    if (fmt != MI_SCALAR_CANONICAL && fmt != MI_SCALAR_MONTGOMERY) return fail(ctx, MI_E_INVALID, "unknown scalar_fmt");
    if (batch == 0) return fail(ctx, MI_E_INVALID, "batch must be at least 1");
    if (n_points != 1 && n_points != batch) return fail(ctx, MI_E_INVALID, "n_points must be 1 or batch");
    if (n > poly::MAX_N) return fail(ctx, MI_E_INVALID, "n must be at most 2^26");
    // (the table of powers and the values take up to (POW_SLOTS + 1) x 32 B per polynomial: bounded by the same test)
    if (batch > (SIZE_MAX >> 6) / std::max<size_t>(n, poly::POW_SLOTS + 1)) return fail(ctx, MI_E_INVALID, "batch * n * 32 must fit size_t");
    if (on_device && ctx->devs.size() != 1) return fail(ctx, MI_E_INVALID, "the *_device entry points need a single-device context");
    const size_t total = batch * n, bytes = total * 32;
    LaneLock lk(ctx, true);
    return guarded(ctx, [&]() -> int {
        DevState& d = ctx->devs[0];
        const auto t0 = std::chrono::steady_clock::now();
        HIP_TRY(hipSetDevice(d.dev));
        if (on_device) {
            if (device_of_ptr(coeffs, "d_coeffs", 16) != d.dev || (quotients && device_of_ptr(quotients, "d_quotients", 16) != d.dev))
                return fail(ctx, MI_E_INVALID, "device buffers must live on the context's device");
            if (quotients && quotients != coeffs && ranges_overlap(coeffs, quotients, bytes))
                return fail(ctx, MI_E_INVALID, "d_coeffs and d_quotients must be the same vectors or not overlap at all");
        }
        mi_profile pr{};
        pr.n = total;
        unsigned tile_bits = poly::TILE_BITS;
#if defined(MI_TEST_HOOKS)
        // switch of the test build (tests/test_gpu_fr_poly.py): smaller tiles, so that small sizes run two, three and more levels
        if (const char* e = getenv("MI_TEST_POLY_TILE_BITS")) tile_bits = (unsigned)std::min<int>((int)poly::TILE_BITS, std::max<int>((int)poly::MIN_TILE_BITS, atoi(e)));
#endif
        if (n == 0) {   // the zero polynomial: every value is zero, there is no quotient element
            if (values) memset(values, 0, batch * 32);
            pr.window_bits = tile_bits;
            pr.num_windows = 1;
            set_prof(ctx, pr);
            return MI_OK;
        }
        const poly::Plan plan = poly::make_plan(n, batch, tile_bits);
        pr.window_bits = plan.tile_bits;
        pr.num_windows = plan.levels;
        // ---- the powers z^(2^s) of every point, and room for the values behind them: pinned host staging <-> one device buffer
        const size_t pow_bytes = n_points * poly::POW_SLOTS * 32, aux_bytes = pow_bytes + batch * 32;
        d.ensure_host(aux_bytes);
        ctx->poly_aux.ensure(aux_bytes);
        ctx->poly_scratch.ensure((size_t)plan.scratch * 32);
        uint32_t* h_pows = static_cast<uint32_t*>(d.h_pairs);
        for (size_t k = 0; k < n_points; k++) {
            Fr w;
            memcpy(w.v, points + k * 32, 32);
            poly::point_powers(h_pows + k * poly::POW_SLOTS * 8, plan, fr::from_fmt(w, fmt));
        }
        const uint32_t* d_pows = static_cast<const uint32_t*>(ctx->poly_aux.p);
        uint32_t* d_vals = values ? reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(ctx->poly_aux.p) + pow_bytes) : nullptr;
        uint32_t* scratch = static_cast<uint32_t*>(ctx->poly_scratch.p);
        const uint8_t* src = coeffs;
        uint8_t* dst = quotients;
        if (!on_device) {
            d.io_in.ensure(bytes);
            src = static_cast<const uint8_t*>(d.io_in.p);
            if (quotients) {
                d.io_out.ensure(bytes);
                dst = static_cast<uint8_t*>(d.io_out.p);
            }
        }
        const IoPlan whole{1, total};
        IoDrain drain(d);
        io_feed(d, whole, total, 0, on_device ? nullptr : coeffs, d.io_in.p, 32);
        HIP_TRY(hipMemcpyAsync(ctx->poly_aux.p, h_pows, pow_bytes, hipMemcpyHostToDevice, d.stream));
        HIP_TRY(hipEventRecord(d.iev[0][0], d.stream));
        const bool per_poly = n_points > 1;
        const uint32_t* in = reinterpret_cast<const uint32_t*>(src);
        if (dst) {   // divide (and evaluate): totals of every level but the top, then the suffixes from the top down
            for (unsigned l = 0; l + 1 < plan.levels; l++) launch_sweep(d.stream, poly::make_up(plan, l, fmt, in, scratch, d_pows, per_poly, nullptr), batch, false);
            for (unsigned l = plan.levels; l-- > 0;)
                launch_sweep(d.stream, poly::make_down(plan, l, fmt, in, reinterpret_cast<uint32_t*>(dst), scratch, d_pows, per_poly, d_vals), batch, true);
        } else {     // evaluate only: the totals of every level; the top level's are the values
            for (unsigned l = 0; l < plan.levels; l++) launch_sweep(d.stream, poly::make_up(plan, l, fmt, in, scratch, d_pows, per_poly, d_vals), batch, false);
        }
        HIP_TRY(hipEventRecord(d.iev[1][0], d.stream));
        uint8_t* h_vals = static_cast<uint8_t*>(d.h_pairs) + pow_bytes;
        if (values) HIP_TRY(hipMemcpyAsync(h_vals, d_vals, batch * 32, hipMemcpyDeviceToHost, d.stream));
        const IoOut res{on_device || !quotients ? nullptr : (void*)quotients, d.io_out.p, 32};
        io_drain_chunk(d, whole, total, 0, d.iev[1][0], &res, 1);
        io_finish(d);
        if (values) memcpy(values, h_vals, batch * 32);
        pr.accumulate_ms = ev_ms(d.iev[0][0], d.iev[1][0]);
        pr.h2d_ms = on_device ? 0.0 : ev_ms(d.cev[0], d.cev[1]);
        pr.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        set_prof(ctx, pr);
        return MI_OK;
    });
}

}  // namespace

int fr_poly_open(mi_ctx* ctx, const uint8_t* coeffs, bool on_device, size_t n, size_t batch, const uint8_t* points, size_t n_points, unsigned fmt,
                 uint8_t* quotients, uint8_t* values) {
    return poly_impl(ctx, coeffs, on_device, n, batch, points, n_points, fmt, quotients, values);
}

}  // namespace mi
