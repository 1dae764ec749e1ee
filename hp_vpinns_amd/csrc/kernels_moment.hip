// Integral constraints on the linear classes (hpv_set_moments): up to HPV_MAX_MOMENTS weighted moments of u over the handle's Nq
// quadrature points and a quadratic penalty on each,
//
//     I_k   = sum_q m_k[q] u_q^p_k          p_k in {1, 2}
//     pen_k = w_k (I_k - c_k)^2             loss += sum_k pen_k
//     GBAR[u][q] += 2 w_k (I_k - c_k) p_k u_q^(p_k - 1) m_k[q]
//
// with m_k a ready-made measure plane (density x quadrature weight x Jacobian, the host's business) in the layout of the operator
// planes.  Mean and mass constraints, the normalisation and the deflation integrals of an eigenvalue problem are all this term.
//
// Three launches between the projection kernel and the reverse launch of pass_linear (the first two in a forward-only pass):
//   k_moment_part    one 256-thread workgroup per element, all terms: each thread sums its points in index order, the block sum is
//                    the fixed tree of the projection kernels (block_sum256, hpv_lane.h) -> part[k][e]
//   k_moment_close   ONE workgroup: I_k as the same fixed-order sum over e, then I_k, pen_k and 2 w_k (I_k - c_k) -> res; pen_k also
//                    -> loss_e[n_elem + k], where k_finalize adds it with the element losses (the pass's n_loss is n_elem + K).  On a
//                    handle with trainable coefficients k_finalize reads d lossv / d c_m in rows of n_loss entries, so the close step
//                    also lays k_project_id's [n_coef][n_elem] out again as [n_coef][n_elem + K] with zero tails
//   k_moment_adj     pointwise on the first Nq entries of GBAR's value channel (merged data points behind them are left alone)
// The close step is a launch of its own and not folded into the adjoint kernel: folded, each of its Nq / 256 workgroups would read
// all K * n_elem partials again, and a forward-only pass needs the stand-alone kernel anyway.
// No atomics; every sum runs in a fixed order, so the results are the same bits from call to call.  A zero-weight padding point has
// m_k = 0 exactly: it adds 0 to I_k and receives exactly 0.
#include "hpv_internal.h"
#include "hpv_lane.h"

__global__ void __launch_bounds__(256) k_moment_part(MomentArgs a) {
    __shared__ double red[4];
    const long e = blockIdx.x;
    const long base = e * a.NQ;
    for (int k = 0; k < a.K; ++k) {
        const double* m = a.m + (long)k * a.Nq + base;
        const bool sq = a.power[k] == 2;
        double acc = 0.0;
        for (int q = threadIdx.x; q < a.NQ; q += 256) {
            const double u = a.OUT[base + q];
            acc += m[q] * (sq ? u * u : u);
        }
        acc = block_sum256(acc, red);
        if (threadIdx.x == 0) a.part[(long)k * a.n_elem + e] = acc;
    }
}

__global__ void __launch_bounds__(256) k_moment_close(MomentArgs a) {
    __shared__ double red[4];
    for (int k = 0; k < a.K; ++k) {
        const double* p = a.part + (long)k * a.n_elem;
        double acc = 0.0;
        for (long e = threadIdx.x; e < a.n_elem; e += 256) acc += p[e];
        acc = block_sum256(acc, red);
        if (threadIdx.x == 0) {
            const double d = acc - a.target[k];
            const double pen = a.weight[k] * d * d;
            a.res[k] = acc;
            a.res[HPV_MAX_MOMENTS + k] = pen;
            a.res[2 * HPV_MAX_MOMENTS + k] = 2.0 * a.weight[k] * d;
            a.loss_e[a.n_elem + k] = pen;
        }
    }
    if (!a.dcoef_dst) return;
    const long row = a.n_elem + a.K;
    for (long idx = threadIdx.x; idx < a.n_coef * row; idx += 256) {
        const long m = idx / row, e = idx - m * row;
        a.dcoef_dst[idx] = e < a.n_elem ? a.dcoef_src[m * a.n_elem + e] : 0.0;
    }
}

__global__ void __launch_bounds__(256) k_moment_adj(MomentArgs a) {
    const long q = (long)blockIdx.x * 256 + threadIdx.x;
    if (q >= a.Nq) return;
    const double u = a.OUT[q];
    double g = a.GBAR[q];
    for (int k = 0; k < a.K; ++k) {
        const double s = a.res[2 * HPV_MAX_MOMENTS + k];
        g += (a.power[k] == 2 ? s * (2.0 * u) : s) * a.m[(long)k * a.Nq + q];
    }
    a.GBAR[q] = g;
}

void launch_moments(const MomentArgs& a, bool adjoint, hipStream_t s) {
    if (a.K <= 0 || a.n_elem <= 0) return;
    hipLaunchKernelGGL(k_moment_part, dim3((unsigned)a.n_elem), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_moment_close, dim3(1), dim3(256), 0, s, a);
    if (adjoint) hipLaunchKernelGGL(k_moment_adj, dim3((unsigned)((a.Nq + 255) / 256)), dim3(256), 0, s, a);
}
