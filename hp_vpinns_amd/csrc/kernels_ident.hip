// k_project_id: k_project_nl (kernels_nonlin.hip) with trainable coefficients on the same handles (hpv_create_ex, hpv_set_trainable)
//
//     plane_p(x_q) = base_p(x_q) + sum_m c_m D_m,p(x_q)          c = theta[P .. P + n_coef),  1 <= n_coef <= HPV_MAX_COEF
//
// p runs over the operator planes (k, b, s | kx, ky, bx, by, s) followed by the nonlinear planes (a2, a3, ae, g | a2, a3, ae, gx, gy);
// base is what hpv_set_operator / hpv_set_nonlinear hold, D_m the direction scalar m owns.  The integrands G_0, G_1, G_2, the tables,
// c_t, masking, F, R, loss_e, the two forward and the two adjoint contractions and the chain rule at the point are k_project_nl's,
// with its arithmetic, on the effective planes.  What is new:
//   staging   c is read from device memory at every launch (it changes inside the captured graphs); every thread forms the
//             effective planes of its points in registers, m = 0 .. in index order (a run-time loop over the coefficients).
//   adjoint   with Gbar_0, Gbar_1, Gbar_2 known at the point the effective planes are formed AGAIN (no LDS beyond k_project_lin's:
//             hpv_linop_lds_bytes), and the same loads of D_m,p feed the point's share of
//                 d lossv / d c_m = sum_q [ (D_s u + D_bx u_x + D_by u_y + D_a2 u^2 + D_a3 u^3 + D_ae e^u + u (D_gx u_x + D_gy u_y)) Gbar_0
//                                           + D_kx u_x Gbar_1 + D_ky u_y Gbar_2 ],
//             one accumulator per coefficient, in registers (selected through a loop over the compile-time HPV_MAX_COEF: a
//             run-time index would send the array to scratch memory).
//   reduce    each accumulator through the fixed-order block sum of the siblings -> dcoef_e[m * n_elem + e]; k_finalize adds the
//             elements up in index order.  No atomics: the same bits from call to call.
// Masks: a (m, p) plane that is zero at every owned point is outside dmask[m] (host side) and never read; a nonlinear term is
// evaluated when its base plane or any direction touches it (`mask`); the host keeps a base plane (zeros where hpv_set_nonlinear
// gave none) for every such term.  All of these branches are uniform over the grid.  A zero-weight padding point has Gbar_t = 0:
// whatever finite value its weights take, it adds exactly 0 to every accumulator and every GBAR entry.
// Registers: profiles/identification.md (no scratch, no VGPR spill; some kernel arguments are parked in VGPR lanes).
#include "hpv_internal.h"
#include "hpv_dual_norm.h"
#include "hpv_dual_dense.h"

namespace {

__device__ __forceinline__ int odd(int n) { return n | 1; }

// sum over the 256 threads, fixed order: butterfly inside each wave, the four wave sums added in wave order; every thread gets it
__device__ __forceinline__ double id_block_sum(double v, double* red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[w] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// N and dN/du at one point from the effective planes (nl_point of kernels_nonlin.hip, operation for operation); ex = exp(u) where
// the term is active
__device__ __forceinline__ void id_nl_point(int mask, double a2, double a3, double ae, double ex, double u, double ga, double& Nv, double& dNu) {
    double n = 0.0, d = 0.0;
    if (mask & HPV_NL_QUADRATIC) {
        n = a2 * (u * u);
        d = 2.0 * (a2 * u);
    }
    if (mask & HPV_NL_CUBIC) {
        const double uu = u * u;
        n += a3 * (uu * u);
        d += 3.0 * (a3 * uu);
    }
    if (mask & HPV_NL_EXP) {
        const double t = ae * ex;
        n += t;
        d += t;
    }
    if (mask & HPV_NL_ADVECTION) {
        n += u * ga;
        d += ga;
    }
    Nv = n;
    dNu = d;
}

// The effective planes of point q: pl[p] = base_p + sum_m c_m D_m,p, m in index order.  K operator planes, then M nonlinear ones.
// WITH_GRAD: acc[m] += sum_p D_m,p w[p] from the same loads (w: the weight of plane p in d lossv / d c_m at this point).
template <int K, int M, bool WITH_GRAD>
__device__ __forceinline__ void id_planes(const IdProjArgs& b, const double* cf, const double* nl, const double* dirs, long cs, int q,
                                          double (&pl)[K + M], const double (&w)[K + M], double (&acc)[HPV_MAX_COEF]) {
#pragma unroll
    for (int p = 0; p < K; ++p) pl[p] = cf[p * cs + q];
#pragma unroll
    for (int p = 0; p < M; ++p) pl[K + p] = (b.mask >> (p < 3 ? p : 3) & 1) ? nl[p * cs + q] : 0.0;
#pragma unroll 1
    for (int m = 0; m < b.n_coef; ++m) {      // (a run-time loop: one copy of the plane loop; the accumulators are selected below)
        const double* D = dirs + (long)m * (K + M) * cs + q;
        const double cm = b.c[m];
        const int dm = b.dmask[m];
        double am = 0.0;
#pragma unroll
        for (int p = 0; p < K + M; ++p)
        {
            if (dm >> p & 1) {
                const double d = *D;
                pl[p] += cm * d;
                if (WITH_GRAD) am += d * w[p];
            }
            D += cs;
        }
        if (WITH_GRAD) {
#pragma unroll
            for (int k = 0; k < HPV_MAX_COEF; ++k)      // (a compile-time index keeps acc in registers)
                if (k == m) acc[k] += am;
        }
    }
}

// DUAL: 1 the dual-norm loss of hpv_dual_norm.h between the two halves (hpv_set_residual_norm), 2 that of hpv_dual_dense.h
// (hpv_set_residual_gram: a dense inverse Gram factor per element); 0 is the kernel as it always was
// TENSOR: a full diffusion tensor per point (hpv_set_operator_tensor; DIM == 2 only): the operator planes are (kxx, kxy, kyx, kyy, bx,
// by, s), each base + sum_m c_m D_m like the others; G1 = kxx u_x + kxy u_y, G2 = kyx u_x + kyy u_y, and d lossv / d c_m weighs
// D_kxx with u_x Gbar_1, D_kxy with u_y Gbar_1, D_kyx with u_x Gbar_2, D_kyy with u_y Gbar_2
template <int DIM, int DUAL, bool TENSOR = false>
__global__ void __launch_bounds__(256) k_project_id(IdProjArgs b) {
    static_assert(!TENSOR || DIM == 2, "the tensor operator is 2-D");
    extern __shared__ __attribute__((aligned(16))) double sm[];
    constexpr int K = TENSOR ? 7 : DIM == 2 ? 5 : 3, M = DIM == 2 ? 5 : 4;
    const LinProjArgs& a = b.lin;
    const long e = blockIdx.x;
    const int qx = a.qx, qy = a.qy, ntx = a.ntx, nty = a.nty, nt = DIM + 1;
    const int NQ = qx * qy, NR = ntx * nty;
    const int gs = odd(qx), ts = odd(ntx), xs = odd(qx), ys = odd(qy);
    double* G = sm;                            // [nt][qy][gs]
    double* T = G + 3 * qy * gs;               // [nt][qy][ts]   T_t, later S_t
    double* U = T + 3 * qy * ts;               // [nty][ntx]
    double* X = U + NR;                        // [2][ntx][xs]   w phi, w phi' of the x direction
    double* Y = X + 2 * ntx * xs;              // [2][nty][ys]
    double* red = Y + 2 * nty * ys;            // [4]
    const int tid = threadIdx.x;
    const long base = e * NQ, N = a.N;
    const long cs = a.coef_stride;
    const double* cf = a.coef + base;
    const double* nl = b.nl + base;                    // planes a2, a3, ae, gx, (gy), the stride of the operator's
    const int mask = b.mask;
    const double* dirs = b.dirs + base;                // [n_coef][K + M] planes of the same stride

    double acc[HPV_MAX_COEF];                          // this thread's share of d lossv / d c_m
#pragma unroll
    for (int m = 0; m < HPV_MAX_COEF; ++m) acc[m] = 0.0;

    // ---- stage the tables and the three integrands ----
    for (int idx = tid; idx < 2 * ntx * qx; idx += 256) {
        const int row = idx / qx, i = idx - row * qx;       // row = d * ntx + r: the first two planes of wtx are contiguous
        X[row * xs + i] = a.wtx[idx];
    }
    for (int idx = tid; idx < 2 * nty * qy; idx += 256) {
        const int row = idx / qy, j = idx - row * qy;
        Y[row * ys + j] = a.wty[idx];
    }
    for (int q = tid; q < NQ; q += 256) {
        const int j = q / qx, i = q - j * qx;
        const double u = a.OUT[base + q], ux = a.OUT[N + base + q];
        const double ex = (mask & HPV_NL_EXP) ? exp(u) : 0.0;
        double pl[K + M], Nv, dNu;
        const double w0[K + M] = {};
        id_planes<K, M, false>(b, cf, nl, dirs, cs, q, pl, w0, acc);
        if constexpr (TENSOR) {
            const double uy = a.OUT[2 * N + base + q];
            const double bx = pl[4], by = pl[5], s = pl[6];
            const double ga = (mask & HPV_NL_ADVECTION) ? pl[K + 3] * ux + pl[K + 4] * uy : 0.0;
            id_nl_point(mask, pl[K], pl[K + 1], pl[K + 2], ex, u, ga, Nv, dNu);
            G[j * gs + i] = ((bx * ux + by * uy) + s * u) + Nv;
            G[(qy + j) * gs + i] = pl[0] * ux + pl[1] * uy;
            G[(2 * qy + j) * gs + i] = pl[2] * ux + pl[3] * uy;
        } else if constexpr (DIM == 2) {
            const double uy = a.OUT[2 * N + base + q];
            const double kx = pl[0], ky = pl[1], bx = pl[2], by = pl[3], s = pl[4];
            const double ga = (mask & HPV_NL_ADVECTION) ? pl[K + 3] * ux + pl[K + 4] * uy : 0.0;
            id_nl_point(mask, pl[K], pl[K + 1], pl[K + 2], ex, u, ga, Nv, dNu);
            G[j * gs + i] = ((bx * ux + by * uy) + s * u) + Nv;
            G[(qy + j) * gs + i] = kx * ux;
            G[(2 * qy + j) * gs + i] = ky * uy;
        } else {
            const double k = pl[0], bv = pl[1], s = pl[2];
            const double ga = (mask & HPV_NL_ADVECTION) ? pl[K + 3] * ux : 0.0;
            id_nl_point(mask, pl[K], pl[K + 1], pl[K + 2], ex, u, ga, Nv, dNu);
            G[j * gs + i] = (bv * ux + s * u) + Nv;
            G[(qy + j) * gs + i] = k * ux;
        }
    }
    __syncthreads();

    // ---- T_t[j][r] = sum_i WTX[dx_t][r][i] G_t[j][i],  dx = (0, 1, 0) ----
    for (int idx = tid; idx < nt * qy * ntx; idx += 256) {
        const int tj = idx / ntx, r = idx - tj * ntx, t = tj / qy;
        const double* ax = X + ((t == 1 ? ntx : 0) + r) * xs;
        const double* g = G + tj * gs;
        double s = 0.0;
        for (int i = 0; i < qx; ++i) s += ax[i] * g[i];
        T[tj * ts + r] = s;
    }
    __syncthreads();

    // ---- U[k][r] = sum_t c_t sum_j WTY[dy_t][k][j] T_t[j][r] - F,  dy = (0, 0, 1); masked; loss ----
    const double J = a.J[e];
    const double c0 = J, c1 = -(J / a.Jx[e]), c2 = DIM == 2 ? -(J / a.Jy[e]) : 0.0;
    const int nax = a.nact ? a.nact[e] : ntx;
    const int nay = a.nacty ? a.nacty[e] : nty;
    const double NRa = (double)(nax * nay);
    double sq = 0.0;
    for (int idx = tid; idx < NR; idx += 256) {
        const int k = idx / ntx, r = idx - k * ntx;
        double v = 0.0;
        if (r < nax && k < nay) {
            const double* y0 = Y + k * ys;
            const double* y1 = Y + (nty + k) * ys;
            double a0 = 0.0, a1 = 0.0, a2 = 0.0;
            for (int j = 0; j < qy; ++j) {
                a0 += y0[j] * T[j * ts + r];
                a1 += y0[j] * T[(qy + j) * ts + r];
            }
            if (DIM == 2)
                for (int j = 0; j < qy; ++j) a2 += y1[j] * T[(2 * qy + j) * ts + r];
            v = ((c0 * a0 + c1 * a1) + c2 * a2) - (a.F ? a.F[e * NR + idx] : 0.0);
        }
        U[idx] = v;
        a.R[e * NR + idx] = v;
        if constexpr (DUAL == 0) sq += v * v;
    }
    DualScratch ds{};
    const double* We = nullptr;           // (DUAL == 2) this element's factor and the scratch of y = W_e U
    double* yd = nullptr;
    if constexpr (DUAL == 2) {
        We = a.dual + (size_t)e * NR * NR;
        yd = hpv_dual_dense_aliases_g(qx, qy, ntx, nty) ? G : red + 4;
        __syncthreads();                  // U is complete (G has been dead since T was)
        sq = hpv_dual_dense_forward(We, ntx, NR, nax, nay, U, yd);
    } else if constexpr (DUAL == 1) {
        ds = hpv_dual_scratch(hpv_dual_aliases_g(qx, qy, ntx, nty) ? G : red + 4, ntx, nty);
        __syncthreads();                  // U is complete (G has been dead since T was)
        sq = hpv_dual_forward(a.dual, a.dual_mass, ntx, nty, nax, nay, a.Jx[e], DIM == 2 ? a.Jy[e] : 1.0, U, ds);
    }
    sq = id_block_sum(sq, red);           // (its barriers also order U before the adjoint and T's readers before S's writers)
    if (tid == 0) a.loss_e[e] = DUAL != 0 ? sq : sq / NRa;
    if (!a.do_adjoint) return;
    if constexpr (DUAL == 1) hpv_dual_adjoint(ntx, nty, nax, nay, U, ds);      // U <- d loss_e / d R: sc = 1 below
    if constexpr (DUAL == 2) hpv_dual_dense_adjoint(We, ntx, NR, nax, nay, U, yd);

    // ---- S_t[j][r] = c_t sum_k WTY[dy_t][k][j] Rbar[k][r],  Rbar = (2 / n_active) R ----
    const double sc = DUAL != 0 ? 1.0 : 2.0 / NRa;
    for (int idx = tid; idx < nt * qy * ntx; idx += 256) {
        const int tj = idx / ntx, r = idx - tj * ntx, t = tj / qy, j = tj - t * qy;
        const double* y = Y + (t == 2 ? nty * ys : 0) + j;
        double s = 0.0;
        for (int k = 0; k < nty; ++k) s += y[k * ys] * U[k * ntx + r];
        T[tj * ts + r] = (t == 0 ? c0 : t == 1 ? c1 : c2) * (sc * s);
    }
    __syncthreads();

    // ---- Gbar_t[j][i] = sum_r WTX[dx_t][r][i] S_t[j][r]; the effective planes again, with the point's share of d lossv / d c_m;
    //      the chain rule at the point; the adjoints of the channels ----
    for (int q = tid; q < NQ; q += 256) {
        const int j = q / qx, i = q - j * qx;
        const double* s0 = T + j * ts;
        const double* s1 = T + (qy + j) * ts;
        const double* s2 = T + (2 * qy + j) * ts;
        double g0 = 0.0, g1 = 0.0, g2 = 0.0;
        for (int r = 0; r < ntx; ++r) {
            const double x0 = X[r * xs + i], x1 = X[(ntx + r) * xs + i];
            g0 += x0 * s0[r];
            g1 += x1 * s1[r];
            if (DIM == 2) g2 += x0 * s2[r];
        }
        const double u = a.OUT[base + q], ux = a.OUT[N + base + q];
        const double ex = (mask & HPV_NL_EXP) ? exp(u) : 0.0;
        const double ug0 = u * g0, uug0 = u * ug0;
        double pl[K + M], Nv, dNu;
        if constexpr (TENSOR) {
            const double uy = a.OUT[2 * N + base + q];
            // the weight of each plane in d lossv / d c_m: (kxx, kxy, kyx, kyy, bx, by, s | a2, a3, ae, gx, gy)
            const double w[K + M] = {ux * g1, uy * g1, ux * g2, uy * g2, ux * g0, uy * g0, ug0, uug0, u * uug0, ex * g0, ux * ug0, uy * ug0};
            id_planes<K, M, true>(b, cf, nl, dirs, cs, q, pl, w, acc);
            const double s = pl[6];
            double bx = pl[4], by = pl[5], ga = 0.0;
            if (mask & HPV_NL_ADVECTION) {
                const double gx = pl[K + 3], gy = pl[K + 4];
                ga = gx * ux + gy * uy;
                bx += gx * u;
                by += gy * u;
            }
            id_nl_point(mask, pl[K], pl[K + 1], pl[K + 2], ex, u, ga, Nv, dNu);
            a.GBAR[base + q] = (s + dNu) * g0;
            a.GBAR[N + base + q] = (pl[0] * g1 + pl[2] * g2) + bx * g0;
            a.GBAR[2 * N + base + q] = (pl[1] * g1 + pl[3] * g2) + by * g0;
        } else if constexpr (DIM == 2) {
            const double uy = a.OUT[2 * N + base + q];
            // the weight of each plane in d lossv / d c_m: (kx, ky, bx, by, s | a2, a3, ae, gx, gy)
            const double w[K + M] = {ux * g1, uy * g2, ux * g0, uy * g0, ug0, uug0, u * uug0, ex * g0, ux * ug0, uy * ug0};
            id_planes<K, M, true>(b, cf, nl, dirs, cs, q, pl, w, acc);
            const double kx = pl[0], ky = pl[1], s = pl[4];
            double bx = pl[2], by = pl[3], ga = 0.0;
            if (mask & HPV_NL_ADVECTION) {
                const double gx = pl[K + 3], gy = pl[K + 4];
                ga = gx * ux + gy * uy;
                bx += gx * u;
                by += gy * u;
            }
            id_nl_point(mask, pl[K], pl[K + 1], pl[K + 2], ex, u, ga, Nv, dNu);
            a.GBAR[base + q] = (s + dNu) * g0;
            a.GBAR[N + base + q] = kx * g1 + bx * g0;
            a.GBAR[2 * N + base + q] = ky * g2 + by * g0;
        } else {
            // (k, b, s | a2, a3, ae, g)
            const double w[K + M] = {ux * g1, ux * g0, ug0, uug0, u * uug0, ex * g0, ux * ug0};
            id_planes<K, M, true>(b, cf, nl, dirs, cs, q, pl, w, acc);
            const double k = pl[0], s = pl[2];
            double bv = pl[1], ga = 0.0;
            if (mask & HPV_NL_ADVECTION) {
                const double g = pl[K + 3];
                ga = g * ux;
                bv += g * u;
            }
            id_nl_point(mask, pl[K], pl[K + 1], pl[K + 2], ex, u, ga, Nv, dNu);
            a.GBAR[base + q] = (s + dNu) * g0;
            a.GBAR[N + base + q] = k * g1 + bv * g0;
        }
    }

    // ---- d lossv / d c_m of this element: the block sum of the siblings, one coefficient after the other ----
#pragma unroll
    for (int m = 0; m < HPV_MAX_COEF; ++m)
        if (m < b.n_coef) {
            const double t = id_block_sum(acc[m], red);
            if (tid == 0) b.dcoef_e[(long)m * gridDim.x + e] = t;
        }
}

}  // namespace

void launch_project_id(const IdProjArgs& a, long n_elem, hipStream_t s) {
    if (n_elem <= 0) return;
    const size_t lds = hpv_linop_lds_bytes(a.lin.qx, a.lin.qy, a.lin.ntx, a.lin.nty);      // (nothing is added to k_project_lin's layout)
    const dim3 grid((unsigned)n_elem), block(256);
    if (a.lin.dual_dense) {      // (hpv_set_residual_gram)
        const size_t ldsd = hpv_dual_dense_lds_bytes(a.lin.qx, a.lin.qy, a.lin.ntx, a.lin.nty);
        if (a.lin.tensor) hipLaunchKernelGGL((k_project_id<2, 2, true>), grid, block, ldsd, s, a);
        else if (a.lin.dim == 2) hipLaunchKernelGGL((k_project_id<2, 2>), grid, block, ldsd, s, a);
        else hipLaunchKernelGGL((k_project_id<1, 2>), grid, block, ldsd, s, a);
        return;
    }
    if (a.lin.tensor) {      // (hpv_set_operator_tensor: 2-D only, the host has made sure)
        if (a.lin.dual) hipLaunchKernelGGL((k_project_id<2, 1, true>), grid, block, hpv_dual_lds_bytes(a.lin.qx, a.lin.qy, a.lin.ntx, a.lin.nty), s, a);
        else hipLaunchKernelGGL((k_project_id<2, 0, true>), grid, block, lds, s, a);
    } else if (a.lin.dual) {
        const size_t ldsd = hpv_dual_lds_bytes(a.lin.qx, a.lin.qy, a.lin.ntx, a.lin.nty);
        if (a.lin.dim == 2) hipLaunchKernelGGL((k_project_id<2, 1>), grid, block, ldsd, s, a);
        else hipLaunchKernelGGL((k_project_id<1, 1>), grid, block, ldsd, s, a);
    } else if (a.lin.dim == 2) hipLaunchKernelGGL((k_project_id<2, 0>), grid, block, lds, s, a);
    else hipLaunchKernelGGL((k_project_id<1, 0>), grid, block, lds, s, a);
}
