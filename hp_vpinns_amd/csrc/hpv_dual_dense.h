// The dual-norm loss with a DENSE inverse Gram factor per element (hpv_set_residual_gram): the sibling of hpv_dual_norm.h for the
// inner products whose Gram matrix is no Kronecker sum -- the physical H^1 product of a mapped element, the energy product
// (sym(K) grad v, grad w) of a variable or full-tensor kappa.  The host factors G_e = L L^T once per element and ships W_e = L^{-1}:
//
//     loss_e = |W_e R_e|^2 = R_e^T G_e^{-1} R_e           d loss_e / d R = 2 W_e^T (W_e R_e)
//
// W_e is [NR][NR] row-major in the full index k * ntx + r (the index of U in LDS), lower triangular, exactly zero in the rows and
// columns of inactive functions (the host has checked all of it: hpv_set_residual_gram).  It is read from global memory twice per
// pass, the second time from cache; it is NOT staged in LDS (NR^2 doubles: 51 KB at 10 x 8 functions, for a matrix read twice).
//     forward   y = W_e U: wave w takes the rows i = w, w + 4, ..; its 64 lanes stride over the columns j <= i (consecutive doubles
//               of one row), the wave sum is the fixed butterfly of the callers' block sum, lane 0 writes y[i].  An inactive row is
//               skipped: y[i] = 0.  Lane 0 keeps the wave's share of sum y_i^2 in row order for the caller's block sum.
//     adjoint   U[j] = 2 sum_{i >= j} W_e[i][j] y[i]: one thread per column j (consecutive lanes read consecutive doubles of every
//               row), the sum in index order in that thread; 0 on an inactive entry.  Ends with the barrier the adjoint contractions need.
// No atomics, every sum in a fixed order: the same bits from call to call.
// Scratch: y, NR doubles.  It aliases the kernels' G region [3][qy][qx|1] (dead after the first contraction) where that holds it and
// is appended behind `red` otherwise -- many functions on few points, e.g. 5 x 4 functions on 2 x 2 points: 20 > 3 * 2 * 3; in 1-D
// every ntx > 3 (qx | 1) -- the rule of hpv_dual_norm.h with another size.
#pragma once
#include <cstddef>
#ifdef __HIPCC__
#define HPV_DENSE_HD __host__ __device__
#else
#define HPV_DENSE_HD
#endif

HPV_DENSE_HD static inline bool hpv_dual_dense_aliases_g(int qx, int qy, int ntx, int nty) {
    return (size_t)ntx * nty <= (size_t)3 * qy * (qx | 1);
}

#ifdef __HIPCC__
// U complete on entry (the caller's barrier); W: this element's factor; returns this thread's share of loss_e and leaves y in the
// scratch.  The caller's block sum (two barriers) stands between this and hpv_dual_dense_adjoint.
__device__ __forceinline__ double hpv_dual_dense_forward(const double* __restrict__ W, int ntx, int NR, int nax, int nay,
                                                         const double* U, double* y) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double sq = 0.0;
    for (int i = wave; i < NR; i += 4) {
        const int k = i / ntx, r = i - k * ntx;
        double v = 0.0;
        if (r < nax && k < nay) {      // (uniform over the wave)
            const double* wi = W + (size_t)i * NR;
            for (int j = lane; j <= i; j += 64) v += wi[j] * U[j];
            for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        }
        if (lane == 0) {
            y[i] = v;
            sq += v * v;
        }
    }
    return sq;
}

// y complete on entry (the barriers of the caller's block sum); U <- d loss_e / d R, 0 on inactive entries; ends with a barrier
__device__ __forceinline__ void hpv_dual_dense_adjoint(const double* __restrict__ W, int ntx, int NR, int nax, int nay, double* U,
                                                       const double* y) {
    for (int j = threadIdx.x; j < NR; j += 256) {
        const int k = j / ntx, r = j - k * ntx;
        double v = 0.0;
        if (r < nax && k < nay) {
            const double* wj = W + j;
            for (int i = j; i < NR; ++i) v += wj[(size_t)i * NR] * y[i];
        }
        U[j] = 2.0 * v;
    }
    __syncthreads();
}
#endif
