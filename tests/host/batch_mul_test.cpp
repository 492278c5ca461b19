// The C++ host mirror's batch_mul (ark-blst_amd/host/ark_blst_amd.hpp: ScalarMul::batch_mul of the arkworks trait surface) against
// expected points the Python test wrote:  batch_mul_test DIR  reads DIR/{g1,g2}_base.bin, _scalars_mont.bin, _expected.bin.
#include <cstdio>
#include <fstream>
#include <iterator>
#include <string>
#include "../../ark-blst_amd/host/ark_blst_amd.hpp"

static std::vector<char> slurp(const std::string& path) {
    std::ifstream f(path, std::ios::binary);
    return std::vector<char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

template <class P, class Aff>
static bool run(const std::string& dir, const char* g) {
    const std::vector<char> base = slurp(dir + "/" + g + "_base.bin"), sc = slurp(dir + "/" + g + "_scalars_mont.bin"),
                            want = slurp(dir + "/" + g + "_expected.bin");
    if (base.size() != sizeof(Aff) || sc.empty() || sc.size() % 32 || want.size() != sc.size() / 32 * sizeof(Aff)) return false;
    Aff b;
    std::memcpy(&b, base.data(), sizeof b);
    std::vector<ark_blst::Scalar> scalars(sc.size() / 32);
    std::memcpy(scalars.data(), sc.data(), sc.size());
    const std::vector<Aff> got = P::batch_mul(b, scalars);
    if (got.size() != scalars.size() || std::memcmp(got.data(), want.data(), want.size()) != 0) return false;
    if (!P::batch_mul(b, {}).empty()) return false;
    printf("%s batch_mul OK\n", g);
    return true;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string dir = argv[1];
    if (!run<ark_blst::G1Projective, ark_blst::G1Affine>(dir, "g1")) { printf("g1 batch_mul FAILED\n"); return 1; }
    if (!run<ark_blst::G2Projective, ark_blst::G2Affine>(dir, "g2")) { printf("g2 batch_mul FAILED\n"); return 1; }
    return 0;
}
