// Host build (g++) of csrc/ntt_kernels.cuh: the pass plan, the tables of powers and the per-pass index maps and butterflies of the NTT, run
// as a serial loop over the workgroups and their lanes exactly as k_ntt_pass runs them (load, barrier, levels, barrier, store), against the
// Python reference (tests/test_fr_ntt_cpu.py).  Stand-alone program, also built under AddressSanitizer + UBSan: an index of a pass that
// leaves its tile, its vector or its table is reported there.   fr_ntt_host <in> <out>
//   in:  u32 cases; per case u32 log_n, cap, batch, inverse, has_offset, fmt, in_place; 32-byte offset; batch x 2^log_n x 32 bytes
//   out: per case u32 passes, widest; batch x 2^log_n x 32 bytes
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../ark-blst_amd/csrc/ntt_kernels.cuh"

namespace {
struct Tables {
    std::vector<uint32_t> lo, hi;
    unsigned h = 0;
};
Tables build(bool coset, unsigned log_n, int inverse, const fr::Fr& x) {
    const ntt::TableSpec sp = ntt::table_spec(coset, log_n, inverse, x);
    Tables t;
    t.h = sp.h;
    t.lo.resize(((size_t)sp.n_lo + 1) * 8);   // exactly the device allocation: a read past it is an error here as well
    t.hi.resize((size_t)sp.n_hi * 8);
    for (uint32_t i = 0; i < sp.n_lo; i++) fr::store_words(&t.lo[(size_t)i * 8], ntt::power_entry(sp.base, sp.scale, i));
    fr::store_words(&t.lo[(size_t)sp.n_lo * 8], ntt::power_entry(fr::one(), sp.ninv, 0));
    for (uint32_t i = 0; i < sp.n_hi; i++) fr::store_words(&t.hi[(size_t)i * 8], ntt::power_entry(sp.hi_base, fr::one(), i));
    return t;
}
bool get(FILE* f, void* p, size_t bytes) { return bytes == 0 || fread(p, bytes, 1, f) == 1; }
}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    FILE* g = fopen(argv[2], "wb");
    if (!f || !g) return 2;
    uint32_t cases = 0;
    if (!get(f, &cases, 4)) return 2;
    for (uint32_t c = 0; c < cases; c++) {
        uint32_t hd[7];
        uint32_t off[8];
        if (!get(f, hd, sizeof hd) || !get(f, off, 32)) return 2;
        const unsigned log_n = hd[0], cap = hd[1], fmt = hd[5];
        const size_t batch = hd[2], total = batch << log_n;
        const int inverse = (int)hd[3];
        const bool has_offset = hd[4] != 0, in_place = hd[6] != 0;
        if (log_n > ntt::MAX_LOG_N) return 2;
        std::vector<uint32_t> in(total * 8), other(in_place ? 0 : total * 8), scratch;
        if (!get(f, in.data(), total * 32)) return 2;
        uint32_t* out = in_place ? in.data() : other.data();
        fr::Fr x = fr::one();
        if (has_offset) {
            fr::Fr w;
            memcpy(w.v, off, 32);
            x = fr::from_fmt(w, fmt);
            if (fr::is_zero(x)) return 3;
        }
        const Tables tw = build(false, log_n, inverse, x), cs = has_offset ? build(true, log_n, inverse, x) : Tables{};
        const ntt::Plan plan = ntt::make_plan(log_n, cap, in_place);
        if (plan.passes > 1) scratch.resize(total * 8);
        std::vector<uint32_t> lds(8 * ntt::TILE);
        for (unsigned k = 0; k < plan.passes; k++) {
            const ntt::Pass P = ntt::make_pass(plan, k, fmt, inverse, tw.lo.data(), tw.hi.data(), tw.h, has_offset ? cs.lo.data() : nullptr,
                                               has_offset ? cs.hi.data() : nullptr, cs.h, in.data(), out, scratch.data());
            if (P.b > ntt::MAX_LEVELS || P.b + P.log_ct > ntt::TILE_BITS || (P.src == P.dst && plan.passes != 1)) return 4;
            const uint64_t blocks = (uint64_t)batch * ntt::tiles_per_vector(P);
            for (uint64_t blk = 0; blk < blocks; blk++) {
                for (uint32_t t = 0; t < ntt::THREADS; t++) ntt::pass_load(P, blk, t, ntt::THREADS, lds.data());
                for (uint32_t l = 0; l < P.b; l++)
                    for (uint32_t t = 0; t < ntt::THREADS; t++) ntt::pass_level(P, blk, l, t, ntt::THREADS, lds.data());
                for (uint32_t t = 0; t < ntt::THREADS; t++) ntt::pass_store(P, blk, t, ntt::THREADS, lds.data());
            }
        }
        const uint32_t res[2] = {plan.passes, plan.widest};
        if (fwrite(res, 8, 1, g) != 1 || (total && fwrite(out, total * 32, 1, g) != 1)) return 2;
    }
    fclose(f);
    fclose(g);
    return 0;
}
