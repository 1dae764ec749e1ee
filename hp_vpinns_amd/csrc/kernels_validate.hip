// Device-side validation for gfx950: the error norms of the network against an exact solution on a stored point set, and the strong
// residual at arbitrary points -- what VPINN.predict plus numpy do on the host in the reference (P1:197-199, P2:255-257: u_pred on
// the test grid; P2:187-194, P3:247-253: net_f).  The forward launches are the existing per-layer kernels; new here are
//   k_validate_reduce   {sum (u^-u)^2, sum u^2, max |u^-u|, sum |grad u^ - grad u|^2, sum |grad u|^2, n} in ONE launch, fp64, written
//                       to a result slot or appended to a device-side history (no host round trip between training iterations);
//   k_residual_points   the strong residual from the full channel list of hpv_eval_points.
//
// Reproducibility of the reduction (bitwise, run to run and rank to rank): the summation order is a function of n alone.
//   thread:     its points p = g, g + T, g + 2T, .. in that order (g the global thread index, T = blocks * 256);
//   wave:       the fixed butterfly of hpv_lane.h (group_reduce<64>: VALU only, the same tree in every lane, all 64 lanes active);
//   workgroup:  its four wave results in wave order (thread 0);
//   grid:       one workgroup below HPV_VAL_BLOCK_POINTS points.  Above, every workgroup stores its five partials, takes a ticket
//               (integer atomic), and the workgroup that draws the LAST ticket combines the partials in WORKGROUP-INDEX order: lane b
//               of its first wave loads workgroup b's partial, then the same fixed butterfly.  Which workgroup that is does not enter
//               the result.  No floating-point atomics anywhere.
#include "hpv_internal.h"
#include "hpv_lane.h"
#include "hpv_residual.h"

#define VAL_THREADS 256
#define HPV_VAL_BLOCK_POINTS 2048      // points per workgroup before another one is added (8 per thread)

namespace {

struct OpMax { __device__ __forceinline__ double operator()(double a, double b) const { return fmax(a, b); } };

__device__ __forceinline__ void val_store(double* p, double v) {
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(p), (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double val_load(const double* p) {
    return __longlong_as_double((long long)__hip_atomic_load(reinterpret_cast<const unsigned long long*>(p), __ATOMIC_RELAXED,
                                                             __HIP_MEMORY_SCOPE_AGENT));
}

}  // namespace

__global__ void __launch_bounds__(VAL_THREADS) k_validate_reduce(ValArgs a) {
    __shared__ double red[5][VAL_THREADS / 64];
    __shared__ int s_last;
    const double* __restrict__ OUT = a.OUT;
    const double* __restrict__ u = a.u;
    const double* __restrict__ du = a.du;
    const long N = a.N;
    const int n = a.n, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int nblk = gridDim.x;
    // v[0] sum (u^-u)^2, v[1] sum u^2, v[2] max |u^-u|, v[3] sum |grad u^ - grad u|^2, v[4] sum |grad u|^2
    double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (long p = (long)blockIdx.x * VAL_THREADS + tid; p < n; p += (long)nblk * VAL_THREADS) {
        const double ue = u[p], e = OUT[p] - ue;
        v[0] += e * e;
        v[1] += ue * ue;
        v[2] = fmax(v[2], fabs(e));
        if (du) {
            for (int c = 0; c < a.dim; ++c) {
                const double ge = du[(long)c * n + p], g = OUT[(long)(1 + c) * N + p] - ge;
                v[3] += g * g;
                v[4] += ge * ge;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        v[k] = (k == 2) ? group_reduce<64>(v[k], OpMax()) : group_sum<64>(v[k]);
        if (lane == 0) red[k][w] = v[k];
    }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            double r = red[k][0];
            for (int i = 1; i < VAL_THREADS / 64; ++i) r = (k == 2) ? fmax(r, red[k][i]) : r + red[k][i];
            v[k] = r;
        }
    }
    if (nblk > 1) {
        if (tid == 0) {
            for (int k = 0; k < 5; ++k) val_store(a.part + 5 * blockIdx.x + k, v[k]);
            __threadfence();
            s_last = atomicAdd(a.ticket, 1u) == (unsigned int)nblk - 1u;
        }
        __syncthreads();
        if (!s_last || w != 0) return;
        __threadfence();
        // the partials in workgroup-index order: lane b holds workgroup b's (0 beyond the grid: the neutral element of both operations,
        // every term is >= 0), then the fixed butterfly
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const double pk = lane < nblk ? val_load(a.part + 5 * lane + k) : 0.0;
            v[k] = (k == 2) ? group_reduce<64>(pk, OpMax()) : group_sum<64>(pk);
        }
        if (lane == 0) *a.ticket = 0u;
    }
    if (tid != 0) return;
    double* dst = a.out;
    if (a.hist) {
        const int i = *a.hist_idx;
        *a.hist_idx = i + 1;
        if (i >= a.hist_cap) return;
        dst = a.hist + 6 * (long)i;
    }
    for (int k = 0; k < 5; ++k) dst[k] = v[k];
    dst[5] = (double)n;
}

int validate_reduce_blocks(int n) {
    const int b = (n + HPV_VAL_BLOCK_POINTS - 1) / HPV_VAL_BLOCK_POINTS;
    return b < 1 ? 1 : (b > HPV_VAL_MAX_BLOCKS ? HPV_VAL_MAX_BLOCKS : b);
}

void launch_validate_reduce(const ValArgs& a, int blocks, hipStream_t s) {
    if (blocks < 1) blocks = 1;
    if (blocks > HPV_VAL_MAX_BLOCKS) blocks = HPV_VAL_MAX_BLOCKS;
    hipLaunchKernelGGL(k_validate_reduce, dim3(blocks), dim3(VAL_THREADS), 0, s, a);
}

// Strong residual at foreign points from the FULL channel list (1-D: u, u_x, u_xx; 2-D: u, u_x, u_y | u_t, u_xx, u_yy | u_tt), with
// the formulas of k_pinn_residual (kernels_generic.hip; include/hpvpinn.h at hpv_set_collocation):
//   Poisson-1D  r = -u_xx - f   (P1:150-155)      Poisson-2D  r = u_xx + u_yy - f   (P2:187-194)
//   AdvDiff     r = u_t + V u_x - epsilon u_xx - f, epsilon read from the device parameters   (P3:247-253)
template <int PDE>
__global__ void __launch_bounds__(256) k_residual_points(const double* __restrict__ OUT, long N, const double* __restrict__ f,
                                                         const double* __restrict__ eps_ptr, double V, int n, double* __restrict__ r) {
    const double eps = PDE == HPV_PDE_ADVDIFF ? *eps_ptr : 0.0;
    for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (long)gridDim.x * blockDim.x) {
        const double fp = f ? f[p] : 0.0;
        r[p] = strong_residual<PDE>(OUT, N, p, fp, V, eps);      // (hpv_residual.h: shared with k_elem_indicators)
    }
}

void launch_residual_points(int pde, const double* OUT, long N, const double* f, const double* eps_ptr, double V, int n, double* r,
                            hipStream_t s) {
    int b = (n + 255) / 256;
    const dim3 grid(b < 1 ? 1 : (b > 1024 ? 1024 : b)), block(256);
    if (pde == HPV_PDE_POISSON1D) hipLaunchKernelGGL(k_residual_points<HPV_PDE_POISSON1D>, grid, block, 0, s, OUT, N, f, eps_ptr, V, n, r);
    else if (pde == HPV_PDE_POISSON2D) hipLaunchKernelGGL(k_residual_points<HPV_PDE_POISSON2D>, grid, block, 0, s, OUT, N, f, eps_ptr, V, n, r);
    else hipLaunchKernelGGL(k_residual_points<HPV_PDE_ADVDIFF>, grid, block, 0, s, OUT, N, f, eps_ptr, V, n, r);
}
