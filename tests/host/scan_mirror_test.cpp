// The C++ host mirror's batch_inversion, batch_inversion_and_mul and grand_product (ark-blst_amd/host/ark_blst_amd.hpp) against values the Python
// test wrote:  scan_mirror_test DIR  reads DIR/v.bin, coeffs.bin, inverse.bin, quotient.bin, z.bin (the exclusive running product of the
// quotients) and total.bin; v has zeros.bin (u64) zero elements.
#include <hip/hip_runtime_api.h>
#include <cstdio>
#include <fstream>
#include <iterator>
#include <string>
#include "../../ark-blst_amd/host/ark_blst_amd.hpp"

static std::vector<char> slurp(const std::string& path) {
    std::ifstream f(path, std::ios::binary);
    return std::vector<char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}
static std::vector<ark_blst::Scalar> scalars(const std::vector<char>& b) {
    std::vector<ark_blst::Scalar> v(b.size() / 32);
    std::memcpy(v.data(), b.data(), v.size() * 32);
    return v;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string dir = argv[1];
    const std::vector<char> bv = slurp(dir + "/v.bin"), bc = slurp(dir + "/coeffs.bin"), wi = slurp(dir + "/inverse.bin"), wq = slurp(dir + "/quotient.bin"),
                            wz = slurp(dir + "/z.bin"), wt = slurp(dir + "/total.bin"), bz = slurp(dir + "/zeros.bin");
    const size_t bytes = bv.size(), n = bytes / 32;
    if (!n || bytes % 32 || bc.size() != bytes || wi.size() != bytes || wq.size() != bytes || wz.size() != bytes || wt.size() != 32 || bz.size() != 8) return 2;
    uint64_t zeros = 0;
    std::memcpy(&zeros, bz.data(), 8);
    std::vector<ark_blst::Scalar> v = scalars(bv);
    const std::vector<ark_blst::Scalar> coeffs = scalars(bc);
    if (ark_blst::batch_inversion(v) != zeros || std::memcmp(v.data(), wi.data(), bytes) != 0) { printf("batch_inversion FAILED\n"); return 1; }
    v = scalars(bv);
    if (ark_blst::batch_inversion_and_mul(v, &coeffs) != zeros || std::memcmp(v.data(), wq.data(), bytes) != 0) { printf("batch_inversion_and_mul FAILED\n"); return 1; }
    std::vector<ark_blst::Scalar> none;
    if (ark_blst::batch_inversion(none) != 0) { printf("empty vector FAILED\n"); return 1; }
    // the grand product of coeffs / v on the context's device, written over the denominators
    mi_ctx* ctx = ark_blst::context();
    void *d_num = nullptr, *d_den = nullptr;
    if (hipSetDevice(mi_msm_device_id(ctx, 0)) != hipSuccess || hipMalloc(&d_num, bytes) != hipSuccess || hipMalloc(&d_den, bytes) != hipSuccess) return 3;
    if (hipMemcpy(d_num, bc.data(), bytes, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(d_den, bv.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) return 3;
    size_t nz = 99;
    const ark_blst::Scalar total = ark_blst::grand_product(ctx, d_num, d_den, n, d_den, &nz);
    std::vector<char> z(bytes);
    if (hipMemcpy(z.data(), d_den, bytes, hipMemcpyDeviceToHost) != hipSuccess) return 3;
    (void)hipFree(d_num);
    (void)hipFree(d_den);
    if (nz != zeros || std::memcmp(&total, wt.data(), 32) != 0 || std::memcmp(z.data(), wz.data(), bytes) != 0) { printf("grand_product FAILED\n"); return 1; }
    printf("batch_inversion OK\n");
    return 0;
}
