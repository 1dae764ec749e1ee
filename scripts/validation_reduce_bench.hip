// Stand-alone timing of k_validate_reduce (hp_vpinns_amd/csrc/kernels_validate.hip) behind profiles/validation.md: one workgroup
// against the fixed-order several-workgroup grid at 10^4 and 10^5 points, with and without exact gradients.  hipEvents around 200
// back-to-back launches after 20 warm-up launches, median of 5 repeats; every launch's six numbers are compared bitwise with the
// first launch's and to 1e-12 with a host sum.  Build (from the repository root):
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -o validation_reduce_bench scripts/validation_reduce_bench.hip hp_vpinns_amd/csrc/kernels_validate.hip
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../hp_vpinns_amd/csrc/hpv_internal.h"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 2; } } while (0)

int main() {
    const int sizes[] = {10000, 40401, 100000};
    std::mt19937_64 rng(7);
    std::normal_distribution<double> nd;
    hipStream_t s;
    CK(hipStreamCreate(&s));
    int bad = 0;
    for (int n : sizes) {
        std::vector<double> OUT((size_t)3 * n), u(n), du((size_t)2 * n);
        for (auto& v : OUT) v = nd(rng);
        for (auto& v : u) v = nd(rng);
        for (auto& v : du) v = nd(rng);
        double *dOUT, *du_, *ddu, *dbuf;
        unsigned int* dtick;
        CK(hipMalloc(&dOUT, OUT.size() * 8)); CK(hipMalloc(&du_, u.size() * 8)); CK(hipMalloc(&ddu, du.size() * 8));
        CK(hipMalloc(&dbuf, (6 + 5 * HPV_VAL_MAX_BLOCKS) * 8)); CK(hipMalloc(&dtick, 8));
        CK(hipMemcpy(dOUT, OUT.data(), OUT.size() * 8, hipMemcpyHostToDevice));
        CK(hipMemcpy(du_, u.data(), u.size() * 8, hipMemcpyHostToDevice));
        CK(hipMemcpy(ddu, du.data(), du.size() * 8, hipMemcpyHostToDevice));
        CK(hipMemset(dtick, 0, 8));
        for (int with_du = 0; with_du < 2; ++with_du) {
            double want[6] = {0, 0, 0, 0, 0, (double)n};
            for (int p = 0; p < n; ++p) {
                const double e = OUT[p] - u[p];
                want[0] += e * e; want[1] += u[p] * u[p]; want[2] = std::max(want[2], std::fabs(e));
                for (int c = 0; c < 2 && with_du; ++c) {
                    const double g = OUT[(size_t)(1 + c) * n + p] - du[(size_t)c * n + p];
                    want[3] += g * g; want[4] += du[(size_t)c * n + p] * du[(size_t)c * n + p];
                }
            }
            const int grids[2] = {1, validate_reduce_blocks(n)};
            for (int blocks : grids) {
                ValArgs a{dOUT, n, du_, with_du ? ddu : nullptr, n, 2, dbuf + 6, dtick, dbuf, nullptr, nullptr, 0};
                double first[6], got[6];
                std::vector<double> us;
                hipEvent_t e0, e1;
                CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
                for (int rep = 0; rep < 6; ++rep) {      // rep 0: warm-up
                    const int K = rep ? 200 : 20;
                    CK(hipEventRecord(e0, s));
                    for (int k = 0; k < K; ++k) launch_validate_reduce(a, blocks, s);
                    CK(hipEventRecord(e1, s));
                    CK(hipStreamSynchronize(s));
                    CK(hipGetLastError());
                    float ms = 0;
                    CK(hipEventElapsedTime(&ms, e0, e1));
                    if (rep) us.push_back(1e3 * ms / K);
                    CK(hipMemcpy(got, dbuf, 48, hipMemcpyDeviceToHost));
                    if (!rep) memcpy(first, got, 48);
                    if (memcmp(first, got, 48)) { printf("NOT REPRODUCIBLE n=%d blocks=%d\n", n, blocks); bad = 1; }
                }
                for (int k = 0; k < 6; ++k) {
                    const double tol = (k == 2 || k == 5) ? 0.0 : 1e-12 * want[k];
                    if (std::fabs(got[k] - want[k]) > tol) { printf("WRONG n=%d blocks=%d k=%d %.17g %.17g\n", n, blocks, k, got[k], want[k]); bad = 1; }
                }
                std::sort(us.begin(), us.end());
                printf("n=%6d du=%d workgroups=%2d  us per launch incl. launch gap: median %.2f  min %.2f  max %.2f\n", n, with_du, blocks,
                       us[2], us[0], us[4]);
                CK(hipEventDestroy(e0)); CK(hipEventDestroy(e1));
            }
        }
        CK(hipFree(dOUT)); CK(hipFree(du_)); CK(hipFree(ddu)); CK(hipFree(dbuf)); CK(hipFree(dtick));
    }
    printf(bad ? "FAILED\n" : "all results reproducible and equal to the host sums\n");
    return bad;
}
