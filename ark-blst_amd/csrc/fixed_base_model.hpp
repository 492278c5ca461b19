// Table geometry and window-size model of the fixed-base batch multiplication (mi_g{1,2}_batch_mul, fixed_base.hip): host-only, no HIP in
// here, so that tests/host/fixed_base_model.cpp compiles it with a plain C++ compiler and checks it without a GPU.
//
// out[i] = s_i P walks a table T[j][m - 1] = m 2^(w j) P, j < W, 1 <= m <= 2^(w-1): one mixed addition per non-zero signed w-bit digit of s_i.
// A larger w means fewer additions per scalar and a larger table, which costs more to build and no longer fits an XCD's L2.
#pragma once
#include <cstddef>
#include <cstdint>

namespace mi {
namespace fbm {

constexpr unsigned W_MIN = 8, W_MAX = 16;   // window sizes mi_batch_mul_set_window_bits accepts (besides 0)

// Digit windows of the unfolded signed recoding of an integer below r < 2^255: the rule of num_windows(c, false) (common.hpp).  A top window
// of a full w bits can carry out, so one more window when w divides 255 (w = 15 in the supported range).
constexpr uint32_t windows(unsigned w) { return (255 + w - 1) / w + (255 % w == 0 ? 1u : 0u); }
constexpr uint64_t entries(unsigned w) { return (uint64_t)windows(w) << (w - 1); }
// bytes of the resident table: 128 B per G1 entry, 256 B per G2 entry (the device form k_accumulate gathers from)
constexpr uint64_t table_bytes(unsigned w, bool g2) { return entries(w) * (g2 ? 256u : 128u); }
// the documented cap (include/arkblst_amd.h): the largest table, w = 16
constexpr uint64_t table_cap(bool g2) { return g2 ? (uint64_t)128 << 20 : (uint64_t)64 << 20; }

// Scalars per pass of a call: bounds the scratch (one Jacobian point of 144 / 288 B per scalar and the product tree over them)
constexpr size_t PASS_POINTS = (size_t)1 << 20;

// ---- time model, microseconds.  Constants fitted to profiles/fixed_base_w_scan.json (MI355X; w in {8, 10, 12, 13, 16} forced at n = 2^16 and
// 2^20, both groups): table builds of 3.5 - 5.0 ms (G1) and 8.8 - 14.1 ms (G2), walk kernels at 7.4 - 7.6e9 (G1) and 2.35 - 2.49e9 (G2) mixed
// additions per second.  The window sizes between the scanned ones are interpolated, and big_table_us is a step the scan only brackets
// (between the 1.6 MiB table of w = 10 and the 5.5 MiB one of w = 12): those two are still GUESSES.
struct Cost {
    double dbl_us;        // one doubling of the serial chain that makes the window bases 2^(w j) P (one lane, nothing beside it): the build's
                          // floor, ~3.4 ms (G1) / ~8.4 ms (G2) whatever w is
    double fixed_us;      // launches, the two host round trips of the batch inversion, small allocations
    double big_table_us;  // allocating and freeing scratch and table once the table passes 2 MiB (measured: +0.9 ms from w = 12 on; w = 11 GUESSED)
    double entry_us;      // per table entry: its complete addition, its share of the inversion, ~1 KB (G1) through HBM
    double adds_per_us;   // mixed additions per microsecond of the walk kernel while the table fits an XCD's L2 (4 MiB); k_accumulate<G1C>
                          // ran 7570 - 7700 in the same process
    double far_factor;    // ... as a fraction of it when the gathers go to the Infinity Cache instead (64 MiB G1 table: 0.975, 128 MiB G2: 0.945)
    double lane_add_us;   // one lane's time per mixed addition when the call does not fill the wave slots (n = 2^16: 0.18 ms for 16 windows)
};
constexpr Cost cost(bool g2) {
    return g2 ? Cost{34.0, 600.0, 1500.0, 0.0050, 2470.0, 0.96, 28.0} : Cost{13.5, 300.0, 900.0, 0.0006, 7550.0, 0.98, 11.0};
}

inline double build_us(unsigned w, bool g2) {
    const Cost c = cost(g2);
    return (double)(w * (windows(w) - 1)) * c.dbl_us + c.fixed_us + (table_bytes(w, g2) > ((uint64_t)2 << 20) ? c.big_table_us : 0.0) +
           (double)entries(w) * c.entry_us;
}
inline double walk_us(size_t n, unsigned w, bool g2) {
    const Cost c = cost(g2);
    const double rate = c.adds_per_us * (table_bytes(w, g2) <= ((uint64_t)4 << 20) ? 1.0 : c.far_factor);
    const double busy = (double)n * (double)windows(w) / rate, floor_us = (double)windows(w) * c.lane_add_us;
    return busy > floor_us ? busy : floor_us;
}
// a first call: table build plus n W additions (the normalisation of the n sums does not depend on w)
inline double call_us(size_t n, unsigned w, bool g2) { return build_us(w, g2) + walk_us(n, w, g2); }

// The built-in choice: the cheapest FIRST call (measured at 2^16 G1 scalars: 4.2 ms at w = 10 against 5.4 ms at w = 16; at 2^20: 8.1 ms at w = 16
// against 8.8 ms at w = 10 and 13).  Small n gets a table that fits an XCD's L2; in steady state — the table resident — w = 16 is the fastest
// at every scanned size (2^16 G1: 0.55 against 0.66 ms), so a caller that keeps one base for many small calls forces it with the setter.
inline unsigned choose_w(size_t n, bool g2) {
    unsigned best = W_MIN;
    double best_us = call_us(n, W_MIN, g2);
    for (unsigned w = W_MIN + 1; w <= W_MAX; w++) {
        const double us = call_us(n, w, g2);
        if (us < best_us) { best = w; best_us = us; }
    }
    return best;
}

}  // namespace fbm
}  // namespace mi
