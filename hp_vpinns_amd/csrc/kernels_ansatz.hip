// Exact Dirichlet conditions by ansatz (hpv_set_ansatz): the trial function is  u = G + D N  with N the network, G a lift of the
// boundary (and initial) data and D a function that vanishes where the condition holds.  On the channels a batch carries -- u alone
// (boundary / data and value-only validation batches) or u, u_x[, u_y] -- the ansatz is a pointwise linear map of the network's
// channels, and its adjoint the transposed map of the channel adjoints:
//     u   = G   + D N                              Nbar   = D ubar + D_x uxbar + D_y uybar
//     u_x = G_x + D_x N + D N_x   (same for y)     N_xbar = D uxbar        N_ybar = D uybar
// k_ansatz_fwd rewrites OUT in place behind a forward launch, k_ansatz_adj rewrites GBAR in place in front of a reverse launch.  The
// adjoint needs the planes only (the map is linear in N): nothing is stashed.  One lane per point, plane-contiguous accesses (lane i
// at base + 8 i of every plane: coalesced), no reductions and no atomics -- bitwise reproducible.  Per point, 2-D with all channels:
// 3 channel values and 6 plane values read, 3 channel values written (the adjoint reads 3 plane values).
#include <algorithm>

#include "hpv_internal.h"

// OUT: [nch][N] channel planes, the points [off, off + n) are transformed; planes: [2 * (1 + dim)][n] = (G, G_x[, G_y], D, D_x[, D_y]);
// nch: the channels the batch carries, 1 (u alone) or 1 + dim
__global__ void __launch_bounds__(256) k_ansatz_fwd(double* __restrict__ OUT, long N, long off, long n, int dim, int nch,
                                                   const double* __restrict__ planes) {
    const long stride = (long)gridDim.x * blockDim.x;
    const double* __restrict__ Gp = planes;
    const double* __restrict__ Dp = planes + (long)(1 + dim) * n;
    for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += stride) {
        const double Nv = OUT[off + p], D = Dp[p];
        OUT[off + p] = Gp[p] + D * Nv;
        if (nch > 1)
            for (int c = 1; c <= dim; ++c) {
                const long ch = (long)c * N + off + p, pl = (long)c * n + p;
                OUT[ch] = Gp[pl] + Dp[pl] * Nv + D * OUT[ch];
            }
    }
}

// GBAR: [nch][N] channel adjoints (ubar, uxbar[, uybar]) of the points [off, off + n) -> (Nbar, N_xbar[, N_ybar]) in place
__global__ void __launch_bounds__(256) k_ansatz_adj(double* __restrict__ GBAR, long N, long off, long n, int dim, int nch,
                                                   const double* __restrict__ planes) {
    const long stride = (long)gridDim.x * blockDim.x;
    const double* __restrict__ Dp = planes + (long)(1 + dim) * n;
    for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += stride) {
        const double D = Dp[p];
        double nb = D * GBAR[off + p];
        if (nch > 1)
            for (int c = 1; c <= dim; ++c) {
                const long ch = (long)c * N + off + p;
                const double gb = GBAR[ch];
                nb += Dp[(long)c * n + p] * gb;
                GBAR[ch] = D * gb;
            }
        GBAR[off + p] = nb;
    }
}

// memory-bound: at most 2048 workgroups, the grid-stride loop takes the rest
static int ansatz_blocks(long n) { return (int)std::min<long>((n + 255) / 256, 2048); }

void launch_ansatz_fwd(double* OUT, long N, long off, long n, int dim, int nch, const double* planes, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_ansatz_fwd, dim3(ansatz_blocks(n)), dim3(256), 0, s, OUT, N, off, n, dim, nch, planes);
}

void launch_ansatz_adj(double* GBAR, long N, long off, long n, int dim, int nch, const double* planes, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_ansatz_adj, dim3(ansatz_blocks(n)), dim3(256), 0, s, GBAR, N, off, n, dim, nch, planes);
}
