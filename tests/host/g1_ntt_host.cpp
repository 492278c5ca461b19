// Host build (g++) of csrc/g1_ntt_kernels.cuh: the digit recoding of a twiddle, and the level plan, index map, twiddle lookup, butterfly body
// and point I/O of the NTT over G1 points run as a serial loop over the lanes of every level exactly as k_g1_ntt_level runs them, over
// ec.cuh's host arithmetic.  Stand-alone program, also built under AddressSanitizer + UBSan (tests/test_g1_ntt_cpu.py).
//   g1_ntt_host recode <in> <out>      in: u32 count; count x 32 B integers below 2^255     out: count x (32 B pos, 32 B neg)
//   g1_ntt_host transform <in> <out>   in: u32 cases; per case u32 log_n, inverse; 2^log_n x 96 B affine points (all-zero = infinity)
//                                      out: per case 2^log_n x 144 B Jacobian points as the last level stores them (log_n = 0: the 96 B copied)
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../ark-blst_amd/csrc/g1_ntt_kernels.cuh"

namespace {
bool get(FILE* f, void* p, size_t bytes) { return bytes == 0 || fread(p, bytes, 1, f) == 1; }

int run_recode(FILE* f, FILE* g) {
    uint32_t count = 0;
    if (!get(f, &count, 4)) return 2;
    for (uint32_t c = 0; c < count; c++) {
        fr::Fr t;
        if (!get(f, t.v, 32)) return 2;
        const g1fft::Digits d = g1fft::recode(t);
        if (fwrite(d.pos, 32, 1, g) != 1 || fwrite(d.neg, 32, 1, g) != 1) return 2;
    }
    return 0;
}

int run_transform(FILE* f, FILE* g) {
    uint32_t cases = 0;
    if (!get(f, &cases, 4)) return 2;
    for (uint32_t c = 0; c < cases; c++) {
        uint32_t hd[2];
        if (!get(f, hd, sizeof hd)) return 2;
        const unsigned log_n = hd[0];
        const int inverse = (int)hd[1];
        if (log_n > 12 || (inverse != 0 && inverse != 1)) return 2;
        const size_t n = (size_t)1 << log_n;
        std::vector<uint32_t> in(n * g1fft::AFF_WORDS);
        if (!get(f, in.data(), in.size() * 4)) return 2;
        if (log_n == 0) {
            if (fwrite(in.data(), in.size() * 4, 1, g) != 1) return 2;
            continue;
        }
        // the tables of mi_fr_ntt, exactly the device allocation: a read past them is an error here as well
        const ntt::TableSpec sp = ntt::table_spec(false, log_n, inverse, fr::one());
        std::vector<uint32_t> lo(((size_t)sp.n_lo + 1) * 8), hi((size_t)sp.n_hi * 8);
        for (uint32_t i = 0; i < sp.n_lo; i++) fr::store_words(&lo[(size_t)i * 8], ntt::power_entry(sp.base, sp.scale, i));
        fr::store_words(&lo[(size_t)sp.n_lo * 8], ntt::power_entry(fr::one(), sp.ninv, 0));
        for (uint32_t i = 0; i < sp.n_hi; i++) fr::store_words(&hi[(size_t)i * 8], ntt::power_entry(sp.hi_base, fr::one(), i));
        // the last level writes n x JAC_WORDS into the vector the levels before it used for n x PROJ_WORDS, as the library does
        std::vector<uint32_t> work0(n * g1fft::PROJ_WORDS), work1(n * g1fft::PROJ_WORDS);
        const ntt::Plan plan = ntt::make_plan(log_n, 1, false);
        if (plan.passes != log_n) return 4;
        for (unsigned k = 0; k < plan.passes; k++) {
            const ntt::Pass P = ntt::make_pass(plan, k, fr::FMT_RAW, inverse, lo.data(), hi.data(), sp.h, nullptr, nullptr, 0, in.data(), work0.data(), work1.data());
            if (P.b != 1 || P.log_s != k || P.src == P.dst || (k + 1 == plan.passes && P.dst != work0.data())) return 4;
            uint32_t park[g1fft::PARK_WORDS];
            for (uint32_t i = 0; i < g1fft::lanes(P, inverse); i++) g1fft::level_lane<ec::FpOps>(P, inverse, i, g1fft::Park{park, 1});
        }
        if (fwrite(work0.data(), n * g1fft::JAC_WORDS * 4, 1, g) != 1) return 2;
    }
    return 0;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc != 4) return 2;
    FILE* f = fopen(argv[2], "rb");
    FILE* g = fopen(argv[3], "wb");
    if (!f || !g) return 2;
    const int rc = strcmp(argv[1], "recode") == 0 ? run_recode(f, g) : strcmp(argv[1], "transform") == 0 ? run_transform(f, g) : 2;
    fclose(f);
    fclose(g);
    return rc;
}
