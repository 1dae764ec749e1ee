// The strong residual of the three problems from the FULL channel list [u, u_x, (u_y | u_t), u_xx, (u_yy | u_tt)] stored as [C][N]:
// one definition for k_residual_points (kernels_validate.hip) and k_elem_indicators (kernels_adapt.hip), so the two cannot drift.
//   Poisson-1D  r = -u_xx - f   (P1:150-155)      Poisson-2D  r = u_xx + u_yy - f   (P2:187-194)
//   AdvDiff     r = u_t + V u_x - epsilon u_xx - f   (P3:247-253)
#pragma once
#include "hpv_internal.h"

template <int PDE>
__device__ __forceinline__ double strong_residual(const double* __restrict__ OUT, long N, long p, double fp, double V, double eps) {
    if constexpr (PDE == HPV_PDE_POISSON1D) return -OUT[2 * N + p] - fp;
    else if constexpr (PDE == HPV_PDE_POISSON2D) return OUT[3 * N + p] + OUT[4 * N + p] - fp;
    else return OUT[2 * N + p] + V * OUT[N + p] - eps * OUT[3 * N + p] - fp;
}
