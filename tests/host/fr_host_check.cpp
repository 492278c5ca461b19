// Host build (g++) of csrc/fr.cuh: the Fr arithmetic of the NTT on a CPU-only box, against Python integers (tests/test_fr_ntt_cpu.py).
// Stand-alone program, also built under AddressSanitizer + UBSan.   fr_host_check <in> <out>
//   in:  u64 count, then count pairs (a, b) of 32-byte words (any 256-bit values)
//   out: per pair ten 32-byte words: for fmt = canonical, Montgomery: store(load(a) * load(b)), store(.. + ..), store(.. - ..);
//        then to_mont(reduce(a)), from_mont(reduce(a)), load(a) as canonical, load(a) as Montgomery
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../ark-blst_amd/csrc/fr.cuh"

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint64_t count = 0;
    if (fread(&count, 8, 1, f) != 1) return 2;
    std::vector<uint32_t> in(count * 16), out(count * 80);
    if (count && fread(in.data(), 64, count, f) != count) return 2;
    fclose(f);
    for (uint64_t i = 0; i < count; i++) {
        const uint32_t *a = &in[i * 16], *b = a + 8;
        uint32_t* o = &out[i * 80];
        for (unsigned fmt = 0; fmt < 2; fmt++) {
            const fr::Fr x = fr::load(a, 0, fmt), y = fr::load(b, 0, fmt);
            fr::store(o, 3 * fmt + 0, fr::mul(x, y), fmt);
            fr::store(o, 3 * fmt + 1, fr::add(x, y), fmt);
            fr::store(o, 3 * fmt + 2, fr::sub(x, y), fmt);
        }
        const fr::Fr ra = fr::reduce(fr::load_words(a));
        fr::store_words(o + 48, fr::to_mont(ra));
        fr::store_words(o + 56, fr::from_mont(ra));
        fr::store_words(o + 64, fr::load(a, 0, fr::FMT_CANONICAL));
        fr::store_words(o + 72, fr::load(a, 0, fr::FMT_MONTGOMERY));
    }
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    if (count && fwrite(out.data(), 320, count, f) != count) return 2;
    fclose(f);
    return 0;
}
