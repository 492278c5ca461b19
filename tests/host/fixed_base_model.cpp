// Stand-alone check of the window-size model of the fixed-base batch multiplication (ark-blst_amd/csrc/fixed_base_model.hpp): host only.
//   fixed_base_model            checks the geometry and the choice for EVERY n from 1 to 2^26, both groups; prints "fixed-base model OK"
//   fixed_base_model choose N G prints the chosen w for n = N, G = 0 (G1) / 1 (G2)
#include <cstdio>
#include <cstdlib>
#include "../../ark-blst_amd/csrc/fixed_base_model.hpp"

using namespace mi::fbm;

int main(int argc, char** argv) {
    if (argc == 4) {
        printf("%u\n", choose_w((size_t)strtoull(argv[2], nullptr, 10), atoi(argv[3]) != 0));
        return 0;
    }
    if (W_MIN > 8 || W_MAX < 16) { printf("the supported range must include 8 and 16\n"); return 1; }
    for (unsigned w = W_MIN; w <= W_MAX; w++) {
        const unsigned W = windows(w);
        // a scalar below r < 2^255 plus the carry of the signed recoding: the top window must keep one spare bit, and no window is wasted
        if (W * w < 256 || (W - 1) * w > 255) { printf("w = %u: %u windows do not fit 255 bits plus the carry\n", w, W); return 1; }
        if (entries(w) != ((unsigned long long)W << (w - 1))) return 1;
        for (int g2 = 0; g2 < 2; g2++)
            if (table_bytes(w, g2) > table_cap(g2)) { printf("w = %u: table above the documented cap\n", w); return 1; }
    }
    for (int g2 = 0; g2 < 2; g2++) {
        unsigned prev = 0;
        for (size_t n = 1; n <= ((size_t)1 << 26); n++) {
            const unsigned w = choose_w(n, g2);
            if (w < W_MIN || w > W_MAX || table_bytes(w, g2) > table_cap(g2)) { printf("n = %zu: w = %u out of range\n", n, w); return 1; }
            if (w < prev) { printf("group %d: w falls from %u to %u at n = %zu\n", g2 + 1, prev, w, n); return 1; }
            if (w != prev) printf("group %d: w = %u from n = %zu\n", g2 + 1, w, n);
            prev = w;
        }
        if (table_bytes(choose_w(1000, g2), g2) > ((unsigned long long)4 << 20)) { printf("small n pays for a large table\n"); return 1; }
    }
    printf("fixed-base model OK\n");
    return 0;
}
