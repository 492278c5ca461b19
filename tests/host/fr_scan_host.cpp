// Host build (g++) of csrc/scan_kernels.cuh: the level plan, the index maps and the per-lane steps of mi_fr_scan and mi_fr_batch_inverse, run as a
// serial loop over the workgroups and their lanes exactly as k_scan_up, k_scan_down and k_inv_down run them (totals, barrier, scan steps with a
// barrier each, second pass), against the Python reference (tests/test_fr_scan_cpu.py).  Stand-alone program, also built under AddressSanitizer +
// UBSan: every vector has exactly the size the library allocates, so an index that leaves its tile, its level or the scratch is reported there.
//   fr_scan_host <in> <out>
//   in:  u32 cases; per case u32 kind (0 scan, 1 inverse), tile_bits, n, batch, fmt, op, exclusive, mode; batch x n x 32 bytes; inverse with
//        numerators: n x 32 bytes more
//        mode, scan:    bit 0 in place, bit 1 out wanted, bit 2 totals wanted
//        mode, inverse: bit 0 in place over a, bit 3 numerators given, bit 4 in place over the numerators
//   out: per case u32 levels, tile_bits; inverse: u64 zeros; batch x n x 32 bytes of out (if wanted); batch x 32 bytes of totals (if wanted)
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../ark-blst_amd/csrc/scan_kernels.cuh"

namespace {
using fr::Fr;

template <int OP, unsigned K>
void scan_tile(const scan::Level& P, uint64_t block, bool down) {
    const scan::TileAt t = scan::tile_at(P, block);
    const uint32_t lanes = 1u << (P.tile_bits - (K == 1 ? 0 : scan::LANE_BITS));
    std::vector<uint32_t> st[2] = {std::vector<uint32_t>(8 * scan::THREADS), std::vector<uint32_t>(down ? 8 * scan::THREADS : 0)};
    struct Held { Fr p[K]; };
    std::vector<Held> held(lanes);
    std::vector<Fr> x(lanes);
    for (uint32_t lane = 0; lane < lanes; lane++) {
        uint32_t zmask;
        x[lane] = scan::lane_total<OP, K>(P, t, lane, held[lane].p, zmask);
        scan::scan_put(st[0].data(), lane, x[lane]);
    }
    if (!down) {   // the reduction: one copy of the planes
        for (uint32_t h = lanes >> 1; h; h >>= 1)
            for (uint32_t lane = 0; lane < h; lane++) {
                x[lane] = scan::reduce_step<OP>(st[0].data(), lane, h, x[lane]);
                scan::scan_put(st[0].data(), lane, x[lane]);
            }
        scan::put_total(P, t, x[0]);
        return;
    }
    uint32_t buf = 0;
    for (uint32_t d = 1; d < lanes; d <<= 1) {
        for (uint32_t lane = 0; lane < lanes; lane++) {
            x[lane] = scan::prefix_step<OP>(st[buf].data(), lane, d, x[lane]);
            scan::scan_put(st[buf ^ 1u].data(), lane, x[lane]);
        }
        buf ^= 1u;
    }
    scan::put_value(P, t, x[lanes - 1]);
    const Fr cin = scan::carry_in<OP>(P, t);
    for (uint32_t lane = 0; lane < lanes; lane++) scan::lane_finish<OP, K>(P, t, lane, held[lane].p, scan::lane_carry<OP>(st[buf].data(), lane, cin));
}

template <unsigned K>
void inv_tile(const scan::Level& P, uint64_t block, bool top) {
    const scan::TileAt t = scan::tile_at(P, block);
    const uint32_t lanes = 1u << (P.tile_bits - (K == 1 ? 0 : scan::LANE_BITS));
    std::vector<uint32_t> st[2][2];
    for (auto& b : st)
        for (auto& v : b) v.resize(8 * scan::THREADS);
    struct Held { Fr e[K]; uint32_t zmask; };
    std::vector<Held> held(lanes);
    std::vector<Fr> pre(lanes), suf(lanes);
    for (uint32_t lane = 0; lane < lanes; lane++) {
        pre[lane] = suf[lane] = scan::lane_total<scan::OP_MUL, K>(P, t, lane, held[lane].e, held[lane].zmask);
        scan::scan_put(st[0][0].data(), lane, pre[lane]);
        scan::scan_put(st[0][1].data(), lane, pre[lane]);
    }
    uint32_t buf = 0;
    for (uint32_t d = 1; d < lanes; d <<= 1) {
        for (uint32_t lane = 0; lane < lanes; lane++) {
            pre[lane] = scan::prefix_step<scan::OP_MUL>(st[buf][0].data(), lane, d, pre[lane]);
            suf[lane] = scan::suffix_step<scan::OP_MUL>(st[buf][1].data(), lane, lanes, d, suf[lane]);
            scan::scan_put(st[buf ^ 1u][0].data(), lane, pre[lane]);
            scan::scan_put(st[buf ^ 1u][1].data(), lane, suf[lane]);
        }
        buf ^= 1u;
    }
    uint32_t* spare = st[buf ^ 1u][0].data();
    if (top) scan::scan_put(spare, 0, scan::inverse(pre[lanes - 1]));
    const Fr inv = top ? scan::scan_get(spare, 0) : fr::load_words(P.carry + (size_t)t.block * 8);
    for (uint32_t lane = 0; lane < lanes; lane++) {
        if (P.zeros) *P.zeros += scan::zeros_of(held[lane].zmask);
        scan::lane_invert<K>(P, t, lane, lanes, held[lane].e, held[lane].zmask, inv, st[buf][0].data(), st[buf][1].data());
    }
}

template <int OP>
void scan_sweep(const scan::Level& P, uint64_t batch, bool down) {
    for (uint64_t b = 0; b < scan::blocks_of(P, batch); b++) {
        if (poly::lane_bits(P.tile_bits) == 0) scan_tile<OP, 1>(P, b, down);
        else scan_tile<OP, scan::LANE_ELEMS>(P, b, down);
    }
}
void inv_sweep(const scan::Level& P, bool top) {
    for (uint64_t b = 0; b < scan::blocks_of(P, 1); b++) {
        if (poly::lane_bits(P.tile_bits) == 0) inv_tile<1>(P, b, top);
        else inv_tile<scan::LANE_ELEMS>(P, b, top);
    }
}
template <int OP>
void run_scan(const scan::Plan& plan, uint64_t batch, unsigned fmt, const uint32_t* in, uint32_t* out, uint32_t* scratch, uint32_t* vals, bool exclusive) {
    if (out) {
        for (unsigned l = 0; l + 1 < plan.levels; l++) scan_sweep<OP>(scan::make_up(plan, l, fmt, in, scratch, nullptr, false), batch, false);
        for (unsigned l = plan.levels; l-- > 0;) scan_sweep<OP>(scan::make_scan_down(plan, l, fmt, in, out, scratch, vals, exclusive), batch, true);
    } else {
        for (unsigned l = 0; l < plan.levels; l++) scan_sweep<OP>(scan::make_up(plan, l, fmt, in, scratch, vals, false), batch, false);
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
        uint32_t hd[8];
        if (!get(f, hd, sizeof hd)) return 2;
        const bool invert = hd[0] == 1;
        const unsigned tile_bits = hd[1], fmt = hd[4], op = hd[5], exclusive = hd[6], mode = hd[7];
        const size_t n = hd[2], batch = hd[3], total = batch * n;
        if (hd[0] > 1 || n > scan::MAX_N || batch == 0 || fmt > 1 || op > 1 || exclusive > 1 || (invert && batch != 1)) return 2;
        uint32_t res[2] = {1, tile_bits};
        if (invert) {
            const bool over_a = mode & 1u, with_num = mode & 8u, over_num = mode & 16u;
            if ((over_a && over_num) || (over_num && !with_num)) return 2;
            std::vector<uint32_t> a(n * 8), num(with_num ? n * 8 : 0), other(over_a || over_num ? 0 : n * 8);
            if (!get(f, a.data(), n * 32) || !get(f, num.data(), num.size() * 4)) return 2;
            uint32_t* out = over_a ? a.data() : over_num ? num.data() : other.data();
            unsigned long long zeros = 0;
            if (n) {
                const scan::Plan plan = poly::make_plan(n, 1, tile_bits);
                if (plan.levels > poly::MAX_LEVELS) return 4;
                res[0] = plan.levels;
                res[1] = plan.tile_bits;
                std::vector<uint32_t> scratch(plan.scratch * 8);
                for (unsigned l = 0; l + 1 < plan.levels; l++) scan_sweep<scan::OP_MUL>(scan::make_up(plan, l, fmt, a.data(), scratch.data(), nullptr, true), 1, false);
                for (unsigned l = plan.levels; l-- > 0;)
                    inv_sweep(scan::make_inv_down(plan, l, fmt, a.data(), with_num ? num.data() : nullptr, out, scratch.data(), &zeros), l + 1 == plan.levels);
            }
            const uint64_t z64 = zeros;
            if (!put(g, res, 8) || !put(g, &z64, 8) || !put(g, out, n * 32)) return 2;
            continue;
        }
        const bool in_place = mode & 1u, want_out = mode & 2u, want_tot = mode & 4u;
        if ((!want_out && !want_tot) || (in_place && !want_out)) return 2;
        std::vector<uint32_t> in(total * 8), other(want_out && !in_place ? total * 8 : 0), vals(want_tot ? batch * 8 : 0);
        if (!get(f, in.data(), total * 32)) return 2;
        uint32_t* out = !want_out ? nullptr : in_place ? in.data() : other.data();
        if (n) {
            const scan::Plan plan = poly::make_plan(n, batch, tile_bits);
            if (plan.levels > poly::MAX_LEVELS) return 4;
            res[0] = plan.levels;
            res[1] = plan.tile_bits;
            std::vector<uint32_t> scratch(plan.scratch * 8);
            uint32_t* v = want_tot ? vals.data() : nullptr;
            if (op == scan::OP_MUL) run_scan<scan::OP_MUL>(plan, batch, fmt, in.data(), out, scratch.data(), v, exclusive);
            else run_scan<scan::OP_ADD>(plan, batch, fmt, in.data(), out, scratch.data(), v, exclusive);
        } else {
            for (size_t b = 0; b < vals.size() / 8; b++) fr::store(vals.data(), b, op == scan::OP_MUL ? fr::one() : fr::zero(), fmt);
        }
        if (!put(g, res, 8) || (out && !put(g, out, total * 32)) || !put(g, vals.data(), vals.size() * 4)) return 2;
    }
    fclose(f);
    fclose(g);
    return 0;
}
