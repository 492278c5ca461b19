// The C++ host mirror's DensePolynomial (ark-blst_amd/host/ark_blst_amd.hpp: evaluate and the division by X - z of the arkworks surface)
// against values the Python test wrote:  poly_open_test DIR  reads DIR/coeffs.bin, point.bin, quotient.bin (one coefficient fewer), value.bin.
#include <cstdio>
#include <fstream>
#include <iterator>
#include <string>
#include "../../ark-blst_amd/host/ark_blst_amd.hpp"

static std::vector<char> slurp(const std::string& path) {
    std::ifstream f(path, std::ios::binary);
    return std::vector<char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string dir = argv[1];
    const std::vector<char> co = slurp(dir + "/coeffs.bin"), pt = slurp(dir + "/point.bin"), wq = slurp(dir + "/quotient.bin"), wv = slurp(dir + "/value.bin");
    if (co.empty() || co.size() % 32 || pt.size() != 32 || wq.size() + 32 != co.size() || wv.size() != 32) return 2;
    ark_blst::DensePolynomial p;
    p.coeffs.resize(co.size() / 32);
    std::memcpy(p.coeffs.data(), co.data(), co.size());
    ark_blst::Scalar z, v;
    std::memcpy(&z, pt.data(), 32);
    v = p.evaluate(z);
    if (std::memcmp(&v, wv.data(), 32) != 0) { printf("evaluate FAILED\n"); return 1; }
    std::memset(&v, 0xff, sizeof v);
    const ark_blst::DensePolynomial q = p.divide_by_linear(z, &v);
    if (q.coeffs.size() + 1 != p.coeffs.size() || std::memcmp(q.coeffs.data(), wq.data(), wq.size()) != 0 || std::memcmp(&v, wv.data(), 32) != 0) {
        printf("divide_by_linear FAILED\n");
        return 1;
    }
    const ark_blst::DensePolynomial none;   // the zero polynomial: value zero, empty quotient, no call
    v = none.evaluate(z);
    const ark_blst::Scalar zero{{0, 0, 0, 0}};
    if (std::memcmp(&v, &zero, 32) != 0 || !none.divide_by_linear(z).coeffs.empty()) { printf("zero polynomial FAILED\n"); return 1; }
    printf("DensePolynomial OK\n");
    return 0;
}
