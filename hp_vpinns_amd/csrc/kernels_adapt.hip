// Per-element refinement indicators for gfx950 (hpv_element_indicators): ONE launch, one workgroup per owned element, that turns the
// full channel list at the element's quadrature points and its block of projected residuals R into five numbers
//   0 loss_e  = sumR2 / (nax_e * nay_e)            the term the training pass sums into lossv
//   1 eta2_e  = J_e * sum_q w_x[i] w_y[j] r_q^2     r the strong residual (hpv_residual.h, the expression k_residual_points uses)
//   2 sumR2_e = sum of R^2 over the active nay_e x nax_e block
//   3 topx_e  = sum of R^2 over the highest active x index (r == nax_e - 1)
//   4 topy_e  = the same for the highest active y / t index (k == nay_e - 1); 0 in 1-D
// Zero-weight padding points of a padded rule contribute exactly 0 through their weight.
//
// Reproducibility (bitwise, call to call): the summation order is a function of (qx, qy, ntx, nty) alone.
//   thread:     its points q = tid, tid + 256, .. and its residual entries o = tid, tid + 256, .., each in that order;
//   wave:       the fixed butterfly of hpv_lane.h (group_sum<64>: VALU only, the same tree in every lane, all 64 lanes active --
//               no thread leaves before the reduction);
//   workgroup:  the four wave results through LDS, added by thread 0 in wave order.
// No atomics; the five results leave through ordinary vector stores.
#include "hpv_internal.h"
#include "hpv_lane.h"
#include "hpv_residual.h"

#define IND_THREADS 256

template <int PDE>
__global__ void __launch_bounds__(IND_THREADS) k_elem_indicators(IndArgs a) {
    __shared__ double red[4][IND_THREADS / 64];
    const long e = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int qx = a.qx, NQ = a.qx * a.qy, ntx = a.ntx, NR = a.ntx * a.nty;
    const double* __restrict__ OUT = a.OUT;
    const double* __restrict__ f = a.f;
    const double* __restrict__ wx = a.wx;
    const double* __restrict__ wy = a.wy;
    const double* __restrict__ R = a.R + e * NR;
    const double eps = PDE == HPV_PDE_ADVDIFF ? *a.eps_ptr : 0.0;
    const long base = e * NQ;
    // v[0] sum w r^2, v[1] sum R^2, v[2] top x, v[3] top y
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    for (int q = tid; q < NQ; q += IND_THREADS) {
        const int j = q / qx, i = q - j * qx;
        const long p = base + q;
        const double r = strong_residual<PDE>(OUT, a.N, p, f ? f[p] : 0.0, a.V, eps);
        v[0] += wx[i] * wy[j] * (r * r);
    }
    const int nax = a.nact ? a.nact[e] : ntx;
    const int nay = a.nacty ? a.nacty[e] : a.nty;
    for (int o = tid; o < NR; o += IND_THREADS) {
        const int k = o / ntx, r = o - k * ntx;
        if (r < nax && k < nay) {
            const double u = R[o], u2 = u * u;
            v[1] += u2;
            if (r == nax - 1) v[2] += u2;
            if (PDE != HPV_PDE_POISSON1D && k == nay - 1) v[3] += u2;
        }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        v[c] = group_sum<64>(v[c]);
        if (lane == 0) red[c][w] = v[c];
    }
    __syncthreads();
    if (tid != 0) return;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        double t = red[c][0];
        for (int i = 1; i < IND_THREADS / 64; ++i) t += red[c][i];
        v[c] = t;
    }
    double* dst = a.out + e * HPV_IND_N;
    dst[0] = v[1] / (double)(nax * nay);
    dst[1] = a.jac[e] * v[0];
    dst[2] = v[1];
    dst[3] = v[2];
    dst[4] = v[3];
}

void launch_elem_indicators(int pde, const IndArgs& a, long n_elem, hipStream_t s) {
    if (n_elem < 1) return;
    const dim3 grid((unsigned)n_elem), block(IND_THREADS);
    if (pde == HPV_PDE_POISSON1D) hipLaunchKernelGGL(k_elem_indicators<HPV_PDE_POISSON1D>, grid, block, 0, s, a);
    else if (pde == HPV_PDE_POISSON2D) hipLaunchKernelGGL(k_elem_indicators<HPV_PDE_POISSON2D>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(k_elem_indicators<HPV_PDE_ADVDIFF>, grid, block, 0, s, a);
}
