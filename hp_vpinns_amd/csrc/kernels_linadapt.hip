// k_lin_indicators: the refinement indicators of the variable-coefficient class (HPV_PDE_LINEAR1D / _LINEAR2D; hpv_linear_indicators),
// the sibling of k_elem_indicators (kernels_adapt.hip) for handles whose strong residual needs derivatives of the diffusion planes:
//
//     r = kx u_xx + (d kx/dx) u_x + ky u_yy + (d ky/dy) u_y + bx u_x + by u_y + s u + N(u, grad u) - f      (1-D: k u'' + k' u' + b u' + s u + N - f)
//
// with N the expression of k_project_nl (kernels_nonlin.hip).  The planes are nodal values on the element's tensor rule, so the
// derivative of their interpolant at the element's own points is one small matrix product with the rule's differentiation matrix on
// the reference interval (hpv_set_strong_form), scaled by the element's half width:
//     dkx[j][i] = (sum_m Dx[i][m] kx[j][m]) / Jx[e]          dky[j][i] = (sum_m Dy[j][m] ky[m][i]) / Jy[e].
// Exact for a plane that is a polynomial of degree < q on the element, spectrally accurate for a smooth one, and correct inside every
// element for a piecewise-constant one whose jumps lie on element edges (no value of a neighbour is read).
// With trainable coefficients (hpv_set_trainable) every plane is base_p + sum_m c_m D_m,p as k_project_id (kernels_ident.hip) forms
// it: c read from device memory at the launch, m in index order, a (m, p) plane outside dmask[m] never read.  A nonlinear term outside
// `mask` is not evaluated and its plane not read: an exp nobody asked for is never computed.
//
// One 256-thread workgroup per owned element, run-time shapes.  LDS (hpv_linadapt_lds_bytes; rows padded to an odd number of doubles):
//     KX [qy][qx|1]   KY [qy][qx|1] (2-D only)   DX [qx][qx|1]   DY [qy][qy|1] (2-D only)   red [4][4]
// Lanes run along i first.  In the dkx sum lanes of one j read DX[i][m] down a column -- row stride odd, so the 32 lanes of a half
// wave hit 32 different bank pairs -- and KX[j][m] as a broadcast; in the dky sum DY[j][m] is a broadcast and KY[m][i] runs along a
// row.  Rows of different j are an odd stride apart as well.
// The five columns are those of k_elem_indicators, 0 and 2-4 from R exactly as there; column 1 is J_e sum_q w_x[i] w_y[j] r_q^2, and
// r itself goes to r_out when the caller asks.  A zero-weight padding point contributes exactly 0 through its weight.
//
// Reproducibility (bitwise, call to call), the rule of k_elem_indicators: a thread takes its points q = tid, tid + 256, .. and its
// entries of R in index order; every inner sum runs in index order in one thread; the wave sum is group_sum<64> with all 64 lanes
// active (no thread leaves before it); the four wave sums are added by thread 0 in wave order.  No atomics, ordinary vector stores.
//
// k_div_indicators<DIM, TENSOR>: the sibling for the strong residual in DIVERGENCE form (hpv_set_strong_form_div), which needs no second
// derivative of anything -- not of the network, not of an element map, not of the ansatz functions G and D:
//
//     r_ref[j][i] = (1/Jx) sum_m Dx[i][m] G1[j][m] + (1/Jy) sum_m Dy[j][m] G2[m][i] + G0[j][i] + N[j][i] - f[j][i]        r = m r_ref
//     G1 = kxx u_x + kxy u_y    G2 = kyx u_x + kyy u_y    (diagonal handles: kx u_x, ky u_y; 1-D: k u')    G0 = bx u_x + by u_y + s u
//
// the flux planes of project_lin_body (kernels_linop.hip) from the effective planes, their nodal interpolant differentiated by the
// rule's matrices.  On unit (mapped) elements the planes hold the fold -- K_eff = adj(A) K, everything else times det A -- so G1, G2
// are the Piola-transformed fluxes, r_ref is det A times the physical residual and m = inv_det[q] = 1 / det A; on boxes m = 1.
// Column 1 is J_e sum_q w_x[i] w_y[j] m_q r_ref_q^2 = int r^2 dx; columns 0, 2 - 4 and the reduction are k_lin_indicators' own.
// OUT holds THREE channels (two in 1-D): u, u_x[, u_y] as the forward-only pass that hpv_linear_indicators has just run left them in
// the quadrature batch -- after k_ansatz_fwd where the handle has an ansatz -- so nothing is launched between that pass and this kernel.
// Planes: 7 + 5 in tensor mode, 5 + 5 on diagonal 2-D handles, 3 + 4 in 1-D (eff_plane, as above).
// LDS (hpv_div_lds_bytes; the sizes of k_lin_indicators' layout):  G1 [qy][qx|1]   G2 [qy][qx|1] (2-D only)   DX   DY (2-D only)   red [4][4]
// Stage 1: a thread forms G1, G2 at its points q = tid, tid + 256, ..; barrier.  Stage 2: at the same points the two products in index
// order -- DX[i][m] down a column at odd stride and G1[j][m] a broadcast, DY[j][m] a broadcast and G2[m][i] along a row -- then G0, N,
// f and the weighted square.  Plain fp64 FMAs: 4 q^3 flops per element, the fixed order is worth more than the matrix pipe here.
#include "hpv_internal.h"
#include "hpv_lane.h"

#define LIND_THREADS 256

namespace {

__device__ __forceinline__ int odd(int n) { return n | 1; }

// plane p (operator planes first, then the nonlinear ones) at point q of this element: base + sum_m c_m D_m,p, m in index order
template <int NP>
__device__ __forceinline__ double eff_plane(const LinIndArgs& a, const double* dirs, int p, double v, int q) {
    for (int m = 0; m < a.n_coef; ++m)
        if (a.dmask[m] >> p & 1) v += a.c[m] * dirs[((long)m * NP + p) * a.cs + q];
    return v;
}

template <int DIM>
__global__ void __launch_bounds__(LIND_THREADS) k_lin_indicators(LinIndArgs a) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    constexpr int K = DIM == 2 ? 5 : 3, M = DIM == 2 ? 5 : 4, NP = K + M;
    const long e = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int qx = a.qx, qy = a.qy, NQ = qx * qy, ntx = a.ntx, NR = a.ntx * a.nty;
    const int ks = odd(qx), xs = odd(qx), ys = odd(qy);
    double* KX = sm;                                       // [qy][ks]
    double* KY = KX + qy * ks;                             // [qy][ks]   (2-D only)
    double* DX = KY + (DIM == 2 ? qy * ks : 0);            // [qx][xs]
    double* DY = DX + qx * xs;                             // [qy][ys]   (2-D only)
    double* red = DY + (DIM == 2 ? qy * ys : 0);           // [4][4]
    const long base = e * NQ, N = a.N, cs = a.cs;
    const double* __restrict__ OUT = a.OUT;
    const double* cf = a.coef + base;
    const double* nl = a.nl ? a.nl + base : nullptr;
    const double* dirs = a.dirs ? a.dirs + base : nullptr;
    const int mask = a.mask;

    // ---- stage the differentiation matrices and the effective diffusion planes ----
    for (int idx = tid; idx < qx * qx; idx += LIND_THREADS) {
        const int i = idx / qx, m = idx - i * qx;
        DX[i * xs + m] = a.Dx[idx];
    }
    if (DIM == 2)
        for (int idx = tid; idx < qy * qy; idx += LIND_THREADS) {
            const int j = idx / qy, m = idx - j * qy;
            DY[j * ys + m] = a.Dy[idx];
        }
    for (int q = tid; q < NQ; q += LIND_THREADS) {
        const int j = q / qx, i = q - j * qx;
        KX[j * ks + i] = eff_plane<NP>(a, dirs, 0, cf[q], q);
        if (DIM == 2) KY[j * ks + i] = eff_plane<NP>(a, dirs, 1, cf[cs + q], q);
    }
    __syncthreads();

    // ---- the strong residual at the thread's points ----
    const double rJx = 1.0 / a.Jx[e], rJy = DIM == 2 ? 1.0 / a.Jy[e] : 0.0;
    // v[0] sum w r^2, v[1] sum R^2, v[2] top x, v[3] top y
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    for (int q = tid; q < NQ; q += LIND_THREADS) {
        const int j = q / qx, i = q - j * qx;
        const long p = base + q;
        const double u = OUT[p], ux = OUT[N + p];
        double dkx = 0.0;
        {
            const double* d = DX + i * xs;
            const double* k = KX + j * ks;
            for (int m = 0; m < qx; ++m) dkx += d[m] * k[m];
        }
        dkx *= rJx;
        double r, ga = 0.0;
        if (DIM == 2) {
            const double uy = OUT[2 * N + p], uxx = OUT[3 * N + p], uyy = OUT[4 * N + p];
            double dky = 0.0;
            {
                const double* d = DY + j * ys;
                const double* k = KY + i;
                for (int m = 0; m < qy; ++m) dky += d[m] * k[m * ks];
            }
            dky *= rJy;
            const double bx = eff_plane<NP>(a, dirs, 2, cf[2 * cs + q], q), by = eff_plane<NP>(a, dirs, 3, cf[3 * cs + q], q);
            const double s = eff_plane<NP>(a, dirs, 4, cf[4 * cs + q], q);
            r = (KX[j * ks + i] * uxx + dkx * ux) + (KY[j * ks + i] * uyy + dky * uy) + ((bx * ux + by * uy) + s * u);
            if (mask & HPV_NL_ADVECTION)
                ga = eff_plane<NP>(a, dirs, K + 3, nl[3 * cs + q], q) * ux + eff_plane<NP>(a, dirs, K + 4, nl[4 * cs + q], q) * uy;
        } else {
            const double uxx = OUT[2 * N + p];
            const double b = eff_plane<NP>(a, dirs, 1, cf[cs + q], q), s = eff_plane<NP>(a, dirs, 2, cf[2 * cs + q], q);
            r = (KX[i] * uxx + dkx * ux) + (b * ux + s * u);
            if (mask & HPV_NL_ADVECTION) ga = eff_plane<NP>(a, dirs, K + 3, nl[3 * cs + q], q) * ux;
        }
        // N of k_project_nl: a term outside the mask is not touched
        double n = 0.0;
        if (mask & HPV_NL_QUADRATIC) n = eff_plane<NP>(a, dirs, K, nl[q], q) * (u * u);
        if (mask & HPV_NL_CUBIC) n += eff_plane<NP>(a, dirs, K + 1, nl[cs + q], q) * ((u * u) * u);
        if (mask & HPV_NL_EXP) n += eff_plane<NP>(a, dirs, K + 2, nl[2 * cs + q], q) * exp(u);
        if (mask & HPV_NL_ADVECTION) n += u * ga;
        r = (r + n) - (a.f ? a.f[p] : 0.0);
        if (a.r_out) a.r_out[p] = r;
        v[0] += a.wx[i] * a.wy[j] * (r * r);
    }

    // ---- the block of projected residuals, as k_elem_indicators reads it ----
    const double* __restrict__ R = a.R + e * NR;
    const int nax = a.nact ? a.nact[e] : ntx;
    const int nay = a.nacty ? a.nacty[e] : a.nty;
    for (int o = tid; o < NR; o += LIND_THREADS) {
        const int k = o / ntx, r = o - k * ntx;
        if (r < nax && k < nay) {
            const double t = R[o], t2 = t * t;
            v[1] += t2;
            if (r == nax - 1) v[2] += t2;
            if (DIM == 2 && k == nay - 1) v[3] += t2;
        }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        v[c] = group_sum<64>(v[c]);
        if (lane == 0) red[c * 4 + w] = v[c];
    }
    __syncthreads();
    if (tid != 0) return;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        double t = red[c * 4];
        for (int i = 1; i < LIND_THREADS / 64; ++i) t += red[c * 4 + i];
        v[c] = t;
    }
    double* dst = a.out + e * HPV_IND_N;
    dst[0] = a.loss_e ? a.loss_e[e] : v[1] / (double)(nax * nay);      // (dual norm: what the forward-only pass wrote)
    dst[1] = a.J[e] * v[0];
    dst[2] = v[1];
    dst[3] = v[2];
    dst[4] = v[3];
}

// QUASI (hpv_set_quasilinear): stage 1 multiplies both flux planes by mu = P(u) B(|grad u|^2) of project_nl_body (kernels_nonlin.hip) at
// the point -- the channels are physical on mapped elements too, so nothing else changes; false is the kernel as it always was.  Only
// this form carries the multiplier: k_lin_indicators would need the derivative of mu along the element.
template <int DIM, bool TENSOR, bool QUASI = false>
__global__ void __launch_bounds__(LIND_THREADS) k_div_indicators(LinIndArgs a) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    constexpr int K = TENSOR ? 7 : DIM == 2 ? 5 : 3, M = DIM == 2 ? 5 : 4, NP = K + M;
    constexpr int PB = TENSOR ? 4 : DIM == 2 ? 2 : 1;      // the first of the planes bx, by, s (1-D: b, s)
    const long e = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int qx = a.qx, qy = a.qy, NQ = qx * qy, ntx = a.ntx, NR = a.ntx * a.nty;
    const int ks = odd(qx), xs = odd(qx), ys = odd(qy);
    double* G1 = sm;                                       // [qy][ks]
    double* G2 = G1 + qy * ks;                             // [qy][ks]   (2-D only)
    double* DX = G2 + (DIM == 2 ? qy * ks : 0);            // [qx][xs]
    double* DY = DX + qx * xs;                             // [qy][ys]   (2-D only)
    double* red = DY + (DIM == 2 ? qy * ys : 0);           // [4][4]
    const long base = e * NQ, N = a.N, cs = a.cs;
    const double* __restrict__ OUT = a.OUT;
    const double* cf = a.coef + base;
    const double* nl = a.nl ? a.nl + base : nullptr;
    const double* dirs = a.dirs ? a.dirs + base : nullptr;
    const int mask = a.mask;

    // ---- stage 1: the differentiation matrices and the flux planes ----
    for (int idx = tid; idx < qx * qx; idx += LIND_THREADS) {
        const int i = idx / qx, m = idx - i * qx;
        DX[i * xs + m] = a.Dx[idx];
    }
    if (DIM == 2)
        for (int idx = tid; idx < qy * qy; idx += LIND_THREADS) {
            const int j = idx / qy, m = idx - j * qy;
            DY[j * ys + m] = a.Dy[idx];
        }
    for (int q = tid; q < NQ; q += LIND_THREADS) {
        const int j = q / qx, i = q - j * qx;
        const long p = base + q;
        const double ux = OUT[N + p];
        double mu = 1.0;
        if constexpr (QUASI) {
            const double u = OUT[p], uy = DIM == 2 ? OUT[2 * N + p] : 0.0;
            const double* qp = a.qp + p;
            double P = 1.0, B = 1.0;
            if (mask & HPV_NL_DIFF_U) P = (qp[0] + qp[cs] * u) + qp[2 * cs] * (u * u);
            if (mask & HPV_NL_DIFF_GRAD) B = pow(qp[3 * cs] + (ux * ux + uy * uy), a.qr);
            mu = P * B;
        }
        if constexpr (TENSOR) {
            const double uy = OUT[2 * N + p];
            const double kxx = eff_plane<NP>(a, dirs, 0, cf[q], q), kxy = eff_plane<NP>(a, dirs, 1, cf[cs + q], q);
            const double kyx = eff_plane<NP>(a, dirs, 2, cf[2 * cs + q], q), kyy = eff_plane<NP>(a, dirs, 3, cf[3 * cs + q], q);
            G1[j * ks + i] = QUASI ? mu * (kxx * ux + kxy * uy) : kxx * ux + kxy * uy;
            G2[j * ks + i] = QUASI ? mu * (kyx * ux + kyy * uy) : kyx * ux + kyy * uy;
        } else if (DIM == 2) {
            G1[j * ks + i] = QUASI ? mu * (eff_plane<NP>(a, dirs, 0, cf[q], q) * ux) : eff_plane<NP>(a, dirs, 0, cf[q], q) * ux;
            G2[j * ks + i] = QUASI ? mu * (eff_plane<NP>(a, dirs, 1, cf[cs + q], q) * OUT[2 * N + p]) : eff_plane<NP>(a, dirs, 1, cf[cs + q], q) * OUT[2 * N + p];
        } else {
            G1[i] = QUASI ? mu * (eff_plane<NP>(a, dirs, 0, cf[q], q) * ux) : eff_plane<NP>(a, dirs, 0, cf[q], q) * ux;
        }
    }
    __syncthreads();

    // ---- stage 2: the divergence of the interpolant, the lower-order terms, the weighted square ----
    const double rJx = 1.0 / a.Jx[e], rJy = DIM == 2 ? 1.0 / a.Jy[e] : 0.0;
    // v[0] sum w m r_ref^2, v[1] sum R^2, v[2] top x, v[3] top y
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    for (int q = tid; q < NQ; q += LIND_THREADS) {
        const int j = q / qx, i = q - j * qx;
        const long p = base + q;
        const double u = OUT[p], ux = OUT[N + p], uy = DIM == 2 ? OUT[2 * N + p] : 0.0;
        double d1 = 0.0, d2 = 0.0;
        {
            const double* d = DX + i * xs;
            const double* g = G1 + j * ks;
            for (int m = 0; m < qx; ++m) d1 += d[m] * g[m];
        }
        if (DIM == 2) {
            const double* d = DY + j * ys;
            const double* g = G2 + i;
            for (int m = 0; m < qy; ++m) d2 += d[m] * g[m * ks];
        }
        const double b0 = eff_plane<NP>(a, dirs, PB, cf[PB * cs + q], q);
        double g0, ga = 0.0;
        if (DIM == 2) {
            const double by = eff_plane<NP>(a, dirs, PB + 1, cf[(PB + 1) * cs + q], q), s = eff_plane<NP>(a, dirs, PB + 2, cf[(PB + 2) * cs + q], q);
            g0 = (b0 * ux + by * uy) + s * u;
            if (mask & HPV_NL_ADVECTION)
                ga = eff_plane<NP>(a, dirs, K + 3, nl[3 * cs + q], q) * ux + eff_plane<NP>(a, dirs, K + 4, nl[4 * cs + q], q) * uy;
        } else {
            g0 = b0 * ux + eff_plane<NP>(a, dirs, PB + 1, cf[(PB + 1) * cs + q], q) * u;
            if (mask & HPV_NL_ADVECTION) ga = eff_plane<NP>(a, dirs, K + 3, nl[3 * cs + q], q) * ux;
        }
        // N of k_project_nl: a term outside the mask is not touched
        double n = 0.0;
        if (mask & HPV_NL_QUADRATIC) n = eff_plane<NP>(a, dirs, K, nl[q], q) * (u * u);
        if (mask & HPV_NL_CUBIC) n += eff_plane<NP>(a, dirs, K + 1, nl[cs + q], q) * ((u * u) * u);
        if (mask & HPV_NL_EXP) n += eff_plane<NP>(a, dirs, K + 2, nl[2 * cs + q], q) * exp(u);
        if (mask & HPV_NL_ADVECTION) n += u * ga;
        const double rr = (((rJx * d1 + rJy * d2) + g0) + n) - (a.f ? a.f[p] : 0.0);
        const double mq = a.inv_det ? a.inv_det[p] : 1.0;
        if (a.r_out) a.r_out[p] = mq * rr;
        v[0] += a.wx[i] * a.wy[j] * (mq * (rr * rr));
    }

    // ---- the block of projected residuals and the reduction, as in k_lin_indicators ----
    const double* __restrict__ R = a.R + e * NR;
    const int nax = a.nact ? a.nact[e] : ntx;
    const int nay = a.nacty ? a.nacty[e] : a.nty;
    for (int o = tid; o < NR; o += LIND_THREADS) {
        const int k = o / ntx, r = o - k * ntx;
        if (r < nax && k < nay) {
            const double t = R[o], t2 = t * t;
            v[1] += t2;
            if (r == nax - 1) v[2] += t2;
            if (DIM == 2 && k == nay - 1) v[3] += t2;
        }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        v[c] = group_sum<64>(v[c]);
        if (lane == 0) red[c * 4 + w] = v[c];
    }
    __syncthreads();
    if (tid != 0) return;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        double t = red[c * 4];
        for (int i = 1; i < LIND_THREADS / 64; ++i) t += red[c * 4 + i];
        v[c] = t;
    }
    double* dst = a.out + e * HPV_IND_N;
    dst[0] = a.loss_e ? a.loss_e[e] : v[1] / (double)(nax * nay);      // (dual norm: what the forward-only pass wrote)
    dst[1] = a.J[e] * v[0];
    dst[2] = v[1];
    dst[3] = v[2];
    dst[4] = v[3];
}

}  // namespace

size_t hpv_linadapt_lds_bytes(int dim, int qx, int qy) {
    const size_t ks = (size_t)(qx | 1), ys = (size_t)(qy | 1);
    const size_t planes = (size_t)(dim == 2 ? 2 : 1) * qy * ks, mats = (size_t)qx * ks + (dim == 2 ? (size_t)qy * ys : 0);
    return (planes + mats + 16) * sizeof(double);
}

void launch_lin_indicators(const LinIndArgs& a, long n_elem, hipStream_t s) {
    if (n_elem < 1) return;
    const size_t lds = hpv_linadapt_lds_bytes(a.dim, a.qx, a.qy);
    const dim3 grid((unsigned)n_elem), block(LIND_THREADS);
    if (a.dim == 2) hipLaunchKernelGGL(k_lin_indicators<2>, grid, block, lds, s, a);
    else hipLaunchKernelGGL(k_lin_indicators<1>, grid, block, lds, s, a);
}

// the layout of k_div_indicators has the sizes of k_lin_indicators' (two flux planes where that one keeps two diffusion planes)
size_t hpv_div_lds_bytes(int dim, int qx, int qy) { return hpv_linadapt_lds_bytes(dim, qx, qy); }

void launch_div_indicators(const LinIndArgs& a, long n_elem, hipStream_t s) {
    if (n_elem < 1) return;
    const size_t lds = hpv_div_lds_bytes(a.dim, a.qx, a.qy);
    const dim3 grid((unsigned)n_elem), block(LIND_THREADS);
    if (a.mask & (HPV_NL_DIFF_U | HPV_NL_DIFF_GRAD)) {      // (hpv_set_quasilinear)
        if (a.dim == 1) hipLaunchKernelGGL((k_div_indicators<1, false, true>), grid, block, lds, s, a);
        else if (a.tensor) hipLaunchKernelGGL((k_div_indicators<2, true, true>), grid, block, lds, s, a);
        else hipLaunchKernelGGL((k_div_indicators<2, false, true>), grid, block, lds, s, a);
        return;
    }
    if (a.dim == 1) hipLaunchKernelGGL((k_div_indicators<1, false>), grid, block, lds, s, a);
    else if (a.tensor) hipLaunchKernelGGL((k_div_indicators<2, true>), grid, block, lds, s, a);
    else hipLaunchKernelGGL((k_div_indicators<2, false>), grid, block, lds, s, a);
}
