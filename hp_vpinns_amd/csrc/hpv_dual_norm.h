// The dual-norm (Riesz) residual loss of the variable-coefficient class (hpv_set_residual_norm): one device function pair, used by
// k_project_lin_dual, k_project_nl_dual and k_project_id<.., true> between their forward and their adjoint contractions.
//
//     loss_e = R_e^T G_e^{-1} R_e,      G_e the Gram matrix of the element's ACTIVE test functions in  (grad v, grad w) + mass (v, w)
//
// With K, M the 1-D stiffness and mass matrices of phi_n = P_{n+1} - P_{n-1} on the reference interval and K S = M S Lambda,
// S^T M S = I (one pair per active count: S of n functions is not a sub-block of S of n + 1), on half widths Jx, Jy
//
//     G_e^{-1} = (S_y (x) S_x) diag(1 / d) (S_y (x) S_x)^T,      d[a][b] = (Jy/Jx) lam_x[b] + (Jx/Jy) lam_y[a] + mass Jx Jy
//
// (1-D: S_y = 1, lam_y = 0, Jy = 1, which is d[b] = lam_x[b] / Jx + mass Jx).  With U the masked residual block [nty][ntx] in LDS:
//     forward   A = U S_x;   Rh = S_y^T A;   w = Rh / d;   the thread's share of sum Rh w;   U <- W = 2 w
//     adjoint   A = S_y W;   U <- A S_x^T on the active block, 0 outside            (= d loss_e / d R: the adjoint phase runs with sc = 1)
// Every sum runs in index order in one thread; the caller adds the shares up with its fixed tree.  Loops run over the active counts.
// Scratch: S_x [ntx][ntx|1], S_y [nty][nty|1], lam_x [ntx], lam_y [nty], A [nty][ntx|1] -- rows padded to an odd length, so that the
// lane-per-row reads of the last product (lane r reads S_x[r][b]) fall on distinct banks; everywhere else the lanes of a wave read
// consecutive doubles of one row or the same double.  The kernels' G region [3][qy][qx|1] is dead after the first contraction: the
// scratch aliases it where it is large enough and is appended behind `red` otherwise (hpv_dual_aliases_g).
// Tables (one device buffer): S_x stack [ntx][ntx][ntx] (count n at [n - 1]: its leading n x n block, zero-padded), lam_x stack
// [ntx][ntx], S_y stack [nty][nty][nty], lam_y stack [nty][nty].
// Inner products whose Gram matrix is no Kronecker sum (mapped elements, a kappa-weighted energy product): hpv_dual_dense.h.
#pragma once
#include <cstddef>
#ifdef __HIPCC__
#define HPV_DUAL_HD __host__ __device__
#else
#define HPV_DUAL_HD
#endif

HPV_DUAL_HD static inline size_t hpv_dual_scratch_doubles(int ntx, int nty) {
    return (size_t)ntx * (ntx | 1) + (size_t)nty * (nty | 1) + (size_t)ntx + nty + (size_t)nty * (ntx | 1);
}
HPV_DUAL_HD static inline bool hpv_dual_aliases_g(int qx, int qy, int ntx, int nty) {
    return hpv_dual_scratch_doubles(ntx, nty) <= (size_t)3 * qy * (qx | 1);
}
static inline size_t hpv_dual_table_doubles(int ntx, int nty) {
    return (size_t)ntx * ntx * ntx + (size_t)ntx * ntx + (size_t)nty * nty * nty + (size_t)nty * nty;
}

#ifdef __HIPCC__
struct DualScratch {
    double *Sx, *Sy, *lx, *ly, *A;
    int sxs, sys, as;
};

__device__ __forceinline__ DualScratch hpv_dual_scratch(double* W, int ntx, int nty) {
    DualScratch s;
    s.sxs = ntx | 1; s.sys = nty | 1; s.as = ntx | 1;
    s.Sx = W;
    s.Sy = s.Sx + ntx * s.sxs;
    s.lx = s.Sy + nty * s.sys;
    s.ly = s.lx + ntx;
    s.A = s.ly + nty;
    return s;
}

// U complete and the G region dead on entry (the caller's barrier); returns this thread's share of loss_e; leaves W = 2 w in U.
// The caller's block sum (two barriers) stands between this and hpv_dual_adjoint.
__device__ __forceinline__ double hpv_dual_forward(const double* __restrict__ tab, double mass, int ntx, int nty, int nax, int nay,
                                                   double Jx, double Jy, double* U, const DualScratch& s) {
    const int tid = threadIdx.x;
    const double* gSx = tab + (size_t)(nax - 1) * ntx * ntx;
    const double* glx = tab + (size_t)ntx * ntx * ntx + (size_t)(nax - 1) * ntx;
    const double* ty = tab + (size_t)ntx * ntx * ntx + (size_t)ntx * ntx;
    const double* gSy = ty + (size_t)(nay - 1) * nty * nty;
    const double* gly = ty + (size_t)nty * nty * nty + (size_t)(nay - 1) * nty;
    const int nb = nax * nay;
    for (int idx = tid; idx < nax * nax; idx += 256) {
        const int r = idx / nax, b = idx - r * nax;
        s.Sx[r * s.sxs + b] = gSx[r * ntx + b];
    }
    for (int idx = tid; idx < nay * nay; idx += 256) {
        const int k = idx / nay, a = idx - k * nay;
        s.Sy[k * s.sys + a] = gSy[k * nty + a];
    }
    for (int idx = tid; idx < nax; idx += 256) s.lx[idx] = glx[idx];
    for (int idx = tid; idx < nay; idx += 256) s.ly[idx] = gly[idx];
    __syncthreads();
    // ---- A[k][b] = sum_r U[k][r] Sx[r][b] ----
    for (int idx = tid; idx < nb; idx += 256) {
        const int k = idx / nax, b = idx - k * nax;
        const double* u = U + k * ntx;
        double acc = 0.0;
        for (int r = 0; r < nax; ++r) acc += u[r] * s.Sx[r * s.sxs + b];
        s.A[k * s.as + b] = acc;
    }
    __syncthreads();
    // ---- Rh[a][b] = sum_k Sy[k][a] A[k][b];  w = Rh / d;  W = 2 w ----
    const double cx = Jy / Jx, cy = Jx / Jy, cm = mass * (Jx * Jy);
    double sq = 0.0;
    for (int idx = tid; idx < nb; idx += 256) {
        const int a = idx / nax, b = idx - a * nax;
        double acc = 0.0;
        for (int k = 0; k < nay; ++k) acc += s.Sy[k * s.sys + a] * s.A[k * s.as + b];
        const double d = (cx * s.lx[b] + cy * s.ly[a]) + cm;
        const double w = acc / d;
        sq += acc * w;
        U[a * ntx + b] = 2.0 * w;
    }
    return sq;
}

// U <- d loss_e / d R on the active block, 0 outside; ends with a barrier (U before the adjoint contractions)
__device__ __forceinline__ void hpv_dual_adjoint(int ntx, int nty, int nax, int nay, double* U, const DualScratch& s) {
    const int tid = threadIdx.x;
    const int nb = nax * nay;
    // ---- A[k][b] = sum_a Sy[k][a] W[a][b] ----
    for (int idx = tid; idx < nb; idx += 256) {
        const int k = idx / nax, b = idx - k * nax;
        double acc = 0.0;
        for (int a = 0; a < nay; ++a) acc += s.Sy[k * s.sys + a] * U[a * ntx + b];
        s.A[k * s.as + b] = acc;
    }
    __syncthreads();
    // ---- U[k][r] = sum_b A[k][b] Sx[r][b] ----
    for (int idx = tid; idx < ntx * nty; idx += 256) {
        const int k = idx / ntx, r = idx - k * ntx;
        double v = 0.0;
        if (r < nax && k < nay) {
            const double* ak = s.A + k * s.as;
            const double* sr = s.Sx + r * s.sxs;
            for (int b = 0; b < nax; ++b) v += ak[b] * sr[b];
        }
        U[idx] = v;
    }
    __syncthreads();
}
#endif
