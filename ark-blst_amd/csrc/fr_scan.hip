// Batched inversion and running products / sums over the scalar field (mi_fr_batch_inverse, mi_fr_scan and their *_device forms):
// ark_ff::batch_inversion / batch_inversion_and_mul and the serial loop of a grand product or a running sum, which a prover with a permutation or
// lookup argument runs on the CPU between its NTTs and its MSMs.
// Host side of scan_kernels.cuh: the level plan, the context's scratch vector of tile totals (shared with mi_fr_poly_open: the calls take the
// context exclusively), and one launch per level and sweep.  No launch of a call waits for the host: the one inversion runs on the device.
#include "internal.hpp"
#include "io_chunks.hpp"
#include "scan_kernels.cuh"

namespace mi {
namespace {

using fr::Fr;

bool ranges_overlap(const void* a, const void* b, size_t bytes) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + bytes && y < x + bytes;
}

enum Sweep { SCAN_UP, SCAN_DOWN, INV_DOWN };

template <int OP, unsigned K>
void launch_sweep(hipStream_t s, const scan::Level& P, size_t batch, Sweep w, bool top) {
    const uint64_t blocks = scan::blocks_of(P, batch);
    for (uint64_t b0 = 0; b0 < blocks; b0 += (uint64_t)1 << 30) {
        const uint32_t cnt = (uint32_t)std::min<uint64_t>(blocks - b0, (uint64_t)1 << 30);
        if (w == SCAN_UP) hipLaunchKernelGGL((scan::k_scan_up<OP, K>), dim3(cnt), dim3(scan::THREADS), 0, s, P, b0);
        else if (w == SCAN_DOWN) hipLaunchKernelGGL((scan::k_scan_down<OP, K>), dim3(cnt), dim3(scan::THREADS), 0, s, P, b0);
        else if (OP == scan::OP_MUL) {
            if (top) hipLaunchKernelGGL((scan::k_inv_down<K, true>), dim3(cnt), dim3(scan::THREADS), 0, s, P, b0);
            else hipLaunchKernelGGL((scan::k_inv_down<K, false>), dim3(cnt), dim3(scan::THREADS), 0, s, P, b0);
        }
    }
    HIP_TRY(hipGetLastError());
}
template <int OP>
void launch_sweep(hipStream_t s, const scan::Level& P, size_t batch, Sweep w, bool top = false) {
#if defined(MI_TEST_HOOKS)
    if (poly::lane_bits(P.tile_bits) == 0) return launch_sweep<OP, 1>(s, P, batch, w, top);   // reduced tiles: one element per lane
#endif
    launch_sweep<OP, scan::LANE_ELEMS>(s, P, batch, w, top);
}

unsigned plan_tile_bits() {
    unsigned tile_bits = scan::TILE_BITS;
#if defined(MI_TEST_HOOKS)
    // switch of the test build (tests/test_gpu_fr_scan.py): smaller tiles, so that small sizes run two, three and more levels
    if (const char* e = getenv("MI_TEST_SCAN_TILE_BITS")) tile_bits = (unsigned)std::min<int>((int)scan::TILE_BITS, std::max<int>((int)scan::MIN_TILE_BITS, atoi(e)));
#endif
    return tile_bits;
}

// what the two calls keep in the context's aux buffer: the zero counter, then the totals
constexpr size_t AUX_HEAD = 32;

int inverse_impl(mi_ctx* ctx, const uint8_t* a, const uint8_t* num, bool on_device, size_t n, unsigned fmt, uint8_t* out, size_t* n_zero) {
    if (!ctx) return fail(ctx, MI_E_INVALID, "invalid argument");
    if (n > 0 && (!a || !out)) return fail(ctx, MI_E_INVALID, "a and out must not be NULL");
    if (fmt != MI_SCALAR_CANONICAL && fmt != MI_SCALAR_MONTGOMERY) return fail(ctx, MI_E_INVALID, "unknown scalar_fmt");
    if (n > scan::MAX_N) return fail(ctx, MI_E_INVALID, "n must be at most 2^26");
    if (on_device && ctx->devs.size() != 1) return fail(ctx, MI_E_INVALID, "the *_device entry points need a single-device context");
    const size_t bytes = n * 32;
    LaneLock lk(ctx, true);
    return guarded(ctx, [&]() -> int {
        DevState& d = ctx->devs[0];
        const auto t0 = std::chrono::steady_clock::now();
        HIP_TRY(hipSetDevice(d.dev));
        if (on_device && n) {
            if (device_of_ptr(a, "d_a", 16) != d.dev || device_of_ptr(out, "d_out", 16) != d.dev || (num && device_of_ptr(num, "d_num", 16) != d.dev))
                return fail(ctx, MI_E_INVALID, "device buffers must live on the context's device");
            if ((out != a && ranges_overlap(a, out, bytes)) || (num && out != num && ranges_overlap(num, out, bytes)))
                return fail(ctx, MI_E_INVALID, "d_out must be one of the input vectors or overlap none of them");
        }
        mi_profile pr{};
        pr.n = n;
        const unsigned tile_bits = plan_tile_bits();
        if (n == 0) {
            if (n_zero) *n_zero = 0;
            pr.window_bits = tile_bits;
            pr.num_windows = 1;
            set_prof(ctx, pr);
            return MI_OK;
        }
        const scan::Plan plan = poly::make_plan(n, 1, tile_bits);
        pr.window_bits = plan.tile_bits;
        pr.num_windows = plan.levels;
        d.ensure_host(AUX_HEAD);
        ctx->poly_aux.ensure(AUX_HEAD);
        ctx->poly_scratch.ensure((size_t)plan.scratch * 32);
        unsigned long long* d_zeros = static_cast<unsigned long long*>(ctx->poly_aux.p);
        uint32_t* scratch = static_cast<uint32_t*>(ctx->poly_scratch.p);
        const uint8_t *src = a, *src_num = num;
        uint8_t* dst = out;
        IoDrain drain(d);
        if (!on_device) {   // a -> io_in; num -> io_out, where the results replace it
            d.io_in.ensure(bytes);
            d.io_out.ensure(bytes);
            src = static_cast<const uint8_t*>(d.io_in.p);
            dst = static_cast<uint8_t*>(d.io_out.p);
            HIP_TRY(hipEventRecord(d.cev[0], d.copy_stream));
            HIP_TRY(hipMemcpyAsync(d.io_in.p, a, bytes, hipMemcpyHostToDevice, d.copy_stream));
            if (num) {
                HIP_TRY(hipMemcpyAsync(d.io_out.p, num, bytes, hipMemcpyHostToDevice, d.copy_stream));
                src_num = dst;
            }
            HIP_TRY(hipEventRecord(d.cev[1], d.copy_stream));
            HIP_TRY(hipStreamWaitEvent(d.stream, d.cev[1], 0));
        }
        HIP_TRY(hipMemsetAsync(d_zeros, 0, AUX_HEAD, d.stream));
        HIP_TRY(hipEventRecord(d.iev[0][0], d.stream));
        const uint32_t* in = reinterpret_cast<const uint32_t*>(src);
        for (unsigned l = 0; l + 1 < plan.levels; l++) launch_sweep<scan::OP_MUL>(d.stream, scan::make_up(plan, l, fmt, in, scratch, nullptr, true), 1, SCAN_UP);
        for (unsigned l = plan.levels; l-- > 0;)
            launch_sweep<scan::OP_MUL>(d.stream, scan::make_inv_down(plan, l, fmt, in, reinterpret_cast<const uint32_t*>(src_num), reinterpret_cast<uint32_t*>(dst), scratch, d_zeros),
                                       1, INV_DOWN, l + 1 == plan.levels);
        HIP_TRY(hipEventRecord(d.iev[1][0], d.stream));
        HIP_TRY(hipMemcpyAsync(d.h_pairs, d_zeros, sizeof(unsigned long long), hipMemcpyDeviceToHost, d.stream));
        const IoPlan whole{1, n};
        const IoOut res{on_device ? nullptr : (void*)out, d.io_out.p, 32};
        io_drain_chunk(d, whole, n, 0, d.iev[1][0], &res, 1);
        io_finish(d);
        if (n_zero) *n_zero = (size_t) * static_cast<const unsigned long long*>(d.h_pairs);
        pr.accumulate_ms = ev_ms(d.iev[0][0], d.iev[1][0]);
        pr.h2d_ms = on_device ? 0.0 : ev_ms(d.cev[0], d.cev[1]);
        pr.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        set_prof(ctx, pr);
        return MI_OK;
    });
}

template <int OP>
void scan_launches(hipStream_t s, const scan::Plan& plan, size_t batch, unsigned fmt, const uint32_t* in, uint32_t* out, uint32_t* scratch, uint32_t* d_vals,
                   bool exclusive) {
    if (out) {   // totals of every level but the top, then the prefixes from the top down
        for (unsigned l = 0; l + 1 < plan.levels; l++) launch_sweep<OP>(s, scan::make_up(plan, l, fmt, in, scratch, nullptr, false), batch, SCAN_UP);
        for (unsigned l = plan.levels; l-- > 0;) launch_sweep<OP>(s, scan::make_scan_down(plan, l, fmt, in, out, scratch, d_vals, exclusive), batch, SCAN_DOWN);
    } else {     // a reduction: the totals of every level; the top level's are the vectors' totals
        for (unsigned l = 0; l < plan.levels; l++) launch_sweep<OP>(s, scan::make_up(plan, l, fmt, in, scratch, d_vals, false), batch, SCAN_UP);
    }
}

int scan_impl(mi_ctx* ctx, int op, const uint8_t* in_, bool on_device, size_t n, size_t batch, int exclusive, unsigned fmt, uint8_t* out, uint8_t* totals) {
    if (!ctx) return fail(ctx, MI_E_INVALID, "invalid argument");
    if (op != MI_FR_MUL && op != MI_FR_ADD) return fail(ctx, MI_E_INVALID, "op must be MI_FR_MUL or MI_FR_ADD");
    if (exclusive != 0 && exclusive != 1) return fail(ctx, MI_E_INVALID, "exclusive must be 0 or 1");
    if (fmt != MI_SCALAR_CANONICAL && fmt != MI_SCALAR_MONTGOMERY) return fail(ctx, MI_E_INVALID, "unknown scalar_fmt");
    if (batch == 0) return fail(ctx, MI_E_INVALID, "batch must be at least 1");
    if (n > 0 && !in_) return fail(ctx, MI_E_INVALID, "in must not be NULL");
    if (!out && !totals) return fail(ctx, MI_E_INVALID, "out and totals must not both be NULL");
    if (n > scan::MAX_N) return fail(ctx, MI_E_INVALID, "n must be at most 2^26");
    // (the levels above the data take at most n elements per vector, the totals one more; the head of the aux buffer one more in all)
    if (batch > ((SIZE_MAX >> 5) - 2) / std::max<size_t>(n, 1)) return fail(ctx, MI_E_INVALID, "batch * n * 32 must fit size_t");
    if (on_device && ctx->devs.size() != 1) return fail(ctx, MI_E_INVALID, "the *_device entry points need a single-device context");
    const size_t total = batch * n, bytes = total * 32;
    LaneLock lk(ctx, true);
    return guarded(ctx, [&]() -> int {
        DevState& d = ctx->devs[0];
        const auto t0 = std::chrono::steady_clock::now();
        HIP_TRY(hipSetDevice(d.dev));
        if (on_device && n) {
            if (device_of_ptr(in_, "d_in", 16) != d.dev || (out && device_of_ptr(out, "d_out", 16) != d.dev))
                return fail(ctx, MI_E_INVALID, "device buffers must live on the context's device");
            if (out && out != in_ && ranges_overlap(in_, out, bytes)) return fail(ctx, MI_E_INVALID, "d_in and d_out must be the same vectors or not overlap at all");
        }
        mi_profile pr{};
        pr.n = total;
        const unsigned tile_bits = plan_tile_bits();
        if (n == 0) {   // the empty product is one, the empty sum is zero; there is no output element
            const Fr id = fr::to_fmt(op == MI_FR_MUL ? fr::one() : fr::zero(), fmt);
            if (totals)
                for (size_t b = 0; b < batch; b++) memcpy(totals + b * 32, id.v, 32);
            pr.window_bits = tile_bits;
            pr.num_windows = 1;
            set_prof(ctx, pr);
            return MI_OK;
        }
        const scan::Plan plan = poly::make_plan(n, batch, tile_bits);
        pr.window_bits = plan.tile_bits;
        pr.num_windows = plan.levels;
        const size_t aux_bytes = AUX_HEAD + batch * 32;
        d.ensure_host(aux_bytes);
        ctx->poly_aux.ensure(aux_bytes);
        ctx->poly_scratch.ensure((size_t)plan.scratch * 32);
        uint32_t* d_vals = totals ? reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(ctx->poly_aux.p) + AUX_HEAD) : nullptr;
        uint32_t* scratch = static_cast<uint32_t*>(ctx->poly_scratch.p);
        const uint8_t* src = in_;
        uint8_t* dst = out;
        if (!on_device) {
            d.io_in.ensure(bytes);
            src = static_cast<const uint8_t*>(d.io_in.p);
            if (out) {
                d.io_out.ensure(bytes);
                dst = static_cast<uint8_t*>(d.io_out.p);
            }
        }
        const IoPlan whole{1, total};
        IoDrain drain(d);
        io_feed(d, whole, total, 0, on_device ? nullptr : in_, d.io_in.p, 32);
        HIP_TRY(hipEventRecord(d.iev[0][0], d.stream));
        const uint32_t* in = reinterpret_cast<const uint32_t*>(src);
        if (op == MI_FR_MUL) scan_launches<scan::OP_MUL>(d.stream, plan, batch, fmt, in, reinterpret_cast<uint32_t*>(dst), scratch, d_vals, exclusive != 0);
        else scan_launches<scan::OP_ADD>(d.stream, plan, batch, fmt, in, reinterpret_cast<uint32_t*>(dst), scratch, d_vals, exclusive != 0);
        HIP_TRY(hipEventRecord(d.iev[1][0], d.stream));
        uint8_t* h_vals = static_cast<uint8_t*>(d.h_pairs) + AUX_HEAD;
        if (totals) HIP_TRY(hipMemcpyAsync(h_vals, d_vals, batch * 32, hipMemcpyDeviceToHost, d.stream));
        const IoOut res{on_device || !out ? nullptr : (void*)out, d.io_out.p, 32};
        io_drain_chunk(d, whole, total, 0, d.iev[1][0], &res, 1);
        io_finish(d);
        if (totals) memcpy(totals, h_vals, batch * 32);
        pr.accumulate_ms = ev_ms(d.iev[0][0], d.iev[1][0]);
        pr.h2d_ms = on_device ? 0.0 : ev_ms(d.cev[0], d.cev[1]);
        pr.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        set_prof(ctx, pr);
        return MI_OK;
    });
}

}  // namespace

int fr_batch_inverse(mi_ctx* ctx, const uint8_t* a, const uint8_t* num, bool on_device, size_t n, unsigned fmt, uint8_t* out, size_t* n_zero) {
    return inverse_impl(ctx, a, num, on_device, n, fmt, out, n_zero);
}
int fr_scan(mi_ctx* ctx, int op, const uint8_t* in, bool on_device, size_t n, size_t batch, int exclusive, unsigned fmt, uint8_t* out, uint8_t* totals) {
    return scan_impl(ctx, op, in, on_device, n, batch, exclusive, fmt, out, totals);
}

}  // namespace mi
