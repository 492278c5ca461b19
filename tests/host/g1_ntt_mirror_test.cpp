// The C++ host mirror's Radix2EvaluationDomain::fft / ifft over std::vector<G1Affine> (ark-blst_amd/host/ark_blst_amd.hpp) against points the
// Python test wrote:  g1_ntt_mirror_test DIR  reads DIR/in.bin (2^k affine points), DIR/fft.bin and DIR/ifft.bin (their transforms).
#include <cstdio>
#include <fstream>
#include <iterator>
#include <string>
#include "../../ark-blst_amd/host/ark_blst_amd.hpp"

static std::vector<ark_blst::G1Affine> points(const std::string& path) {
    std::ifstream f(path, std::ios::binary);
    const std::vector<char> b((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    std::vector<ark_blst::G1Affine> v(b.size() / sizeof(ark_blst::G1Affine));
    std::memcpy(v.data(), b.data(), v.size() * sizeof(ark_blst::G1Affine));
    return v;
}
static bool same(const std::vector<ark_blst::G1Affine>& a, const std::vector<ark_blst::G1Affine>& b) {
    return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(ark_blst::G1Affine)) == 0;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string dir = argv[1];
    const std::vector<ark_blst::G1Affine> in = points(dir + "/in.bin"), fwd = points(dir + "/fft.bin"), inv = points(dir + "/ifft.bin");
    if (in.empty() || fwd.size() != in.size() || inv.size() != in.size()) return 2;
    ark_blst::Radix2EvaluationDomain dom;
    if (!ark_blst::Radix2EvaluationDomain::make(in.size(), dom) || dom.size != in.size()) return 2;
    if (!same(dom.fft(in), fwd)) { printf("fft FAILED\n"); return 1; }
    if (!same(dom.ifft(in), inv)) { printf("ifft FAILED\n"); return 1; }
    if (!same(dom.ifft(dom.fft(in)), in)) { printf("round trip FAILED\n"); return 1; }
    bool threw = false;
    try {
        dom.fft(std::vector<ark_blst::G1Affine>(in.begin(), in.end() - 1));   // not the domain's size
    } catch (const std::runtime_error&) {
        threw = true;
    }
    if (!threw) { printf("size check FAILED\n"); return 1; }
    printf("g1 fft OK\n");
    return 0;
}
