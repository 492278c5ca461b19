// Host build (g++) of csrc/poly_kernels.cuh: the level plan, the tables of powers, the index maps and the per-lane steps of mi_fr_poly_open, run
// as a serial loop over the workgroups and their lanes exactly as k_poly_up and k_poly_down run them (totals, barrier, scan steps with a barrier
// each, second pass), against the Python reference (tests/test_fr_poly_cpu.py).  Stand-alone program, also built under AddressSanitizer + UBSan:
// every vector has exactly the size the library allocates, so an index that leaves its tile, its level or its table is reported there.
//   fr_poly_host <in> <out>
//   in:  u32 cases; per case u32 tile_bits, n, batch, n_points, fmt, mode (bit 0 in place, bit 1 quotients wanted, bit 2 values wanted);
//        n_points x 32 bytes; batch x n x 32 bytes
//   out: per case u32 levels, tile_bits; batch x n x 32 bytes of quotients (if wanted); batch x 32 bytes of values (if wanted)
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../ark-blst_amd/csrc/poly_kernels.cuh"

namespace {
template <unsigned K>
void run_tile(const poly::Level& P, uint64_t block, bool down) {
    const poly::TileAt t = poly::tile_at(P, block);
    const uint32_t kb = K == 1 ? 0 : poly::LANE_BITS, lanes = 1u << (P.tile_bits - kb);
    const fr::Fr z = poly::power(t, P.s0), cin = down ? poly::carry_in(P, t) : fr::zero();
    std::vector<uint32_t> st[2] = {std::vector<uint32_t>(8 * poly::THREADS), std::vector<uint32_t>(8 * poly::THREADS)};
    struct Held { fr::Fr p[K]; };
    std::vector<Held> held(lanes);
    std::vector<fr::Fr> x(lanes);
    for (uint32_t lane = 0; lane < lanes; lane++) {
        x[lane] = poly::lane_total<K>(P, t, lane, lanes, held[lane].p, z, poly::power(t, P.s0 + kb), down ? &cin : nullptr);
        poly::scan_put(st[0].data(), lane, x[lane]);
    }
    uint32_t buf = 0;
    for (uint32_t j = 0; (1u << j) < lanes; j++) {
        for (uint32_t lane = 0; lane < lanes; lane++) {
            x[lane] = poly::scan_step(st[buf].data(), lane, lanes, 1u << j, poly::power(t, P.s0 + kb + j), x[lane]);
            poly::scan_put(st[buf ^ 1u].data(), lane, x[lane]);
        }
        buf ^= 1u;
    }
    if (!down) {
        poly::put_total(P, t, x[0]);
        return;
    }
    poly::put_value(P, t, x[0]);
    for (uint32_t lane = 0; lane < lanes; lane++) poly::lane_finish<K>(P, t, lane, held[lane].p, z, poly::lane_carry(st[buf].data(), lane, lanes, cin));
}
void run_sweep(const poly::Level& P, uint64_t batch, bool down) {
    for (uint64_t b = 0; b < poly::blocks_of(P, batch); b++) {
        if (poly::lane_bits(P.tile_bits) == 0) run_tile<1>(P, b, down);
        else run_tile<poly::LANE_ELEMS>(P, b, down);
    }
}
bool get(FILE* f, void* p, size_t bytes) { return bytes == 0 || fread(p, bytes, 1, f) == 1; }
bool put(FILE* f, const void* p, size_t bytes) { return bytes == 0 || fwrite(p, bytes, 1, f) == 1; }
}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    FILE* g = fopen(argv[2], "wb");
    if (!f || !g) return 2;
    uint32_t cases = 0;
    if (!get(f, &cases, 4)) return 2;
    for (uint32_t c = 0; c < cases; c++) {
        uint32_t hd[6];
        if (!get(f, hd, sizeof hd)) return 2;
        const unsigned tile_bits = hd[0], fmt = hd[4];
        const size_t n = hd[1], batch = hd[2], n_points = hd[3], total = batch * n;
        const bool in_place = hd[5] & 1u, want_q = hd[5] & 2u, want_v = hd[5] & 4u;
        if (n > poly::MAX_N || batch == 0 || (n_points != 1 && n_points != batch) || (!want_q && !want_v) || (in_place && !want_q)) return 2;
        std::vector<uint32_t> points(n_points * 8), in(total * 8), other(want_q && !in_place ? total * 8 : 0), vals(want_v ? batch * 8 : 0);
        if (!get(f, points.data(), n_points * 32) || !get(f, in.data(), total * 32)) return 2;
        uint32_t* out = !want_q ? nullptr : in_place ? in.data() : other.data();
        uint32_t res[2] = {1, tile_bits};
        if (n) {
            const poly::Plan plan = poly::make_plan(n, batch, tile_bits);
            if (plan.levels > poly::MAX_LEVELS || plan.tile_bits * plan.levels > poly::POW_SLOTS) return 4;
            res[0] = plan.levels;
            res[1] = plan.tile_bits;
            std::vector<uint32_t> pows(n_points * poly::POW_SLOTS * 8), scratch(plan.scratch * 8);
            for (size_t k = 0; k < n_points; k++) {
                fr::Fr w;
                memcpy(w.v, &points[k * 8], 32);
                poly::point_powers(&pows[k * poly::POW_SLOTS * 8], plan, fr::from_fmt(w, fmt));
            }
            const bool per_poly = n_points > 1;
            uint32_t* v = want_v ? vals.data() : nullptr;
            if (out) {
                for (unsigned l = 0; l + 1 < plan.levels; l++) run_sweep(poly::make_up(plan, l, fmt, in.data(), scratch.data(), pows.data(), per_poly, nullptr), batch, false);
                for (unsigned l = plan.levels; l-- > 0;)
                    run_sweep(poly::make_down(plan, l, fmt, in.data(), out, scratch.data(), pows.data(), per_poly, v), batch, true);
            } else {
                for (unsigned l = 0; l < plan.levels; l++) run_sweep(poly::make_up(plan, l, fmt, in.data(), scratch.data(), pows.data(), per_poly, v), batch, false);
            }
        }
        if (!put(g, res, 8) || (out && !put(g, out, total * 32)) || !put(g, vals.data(), vals.size() * 4)) return 2;
    }
    fclose(f);
    fclose(g);
    return 0;
}
