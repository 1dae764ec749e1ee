// k_project_lin: the projection of the variable-coefficient convection-diffusion-reaction class (HPV_PDE_LINEAR1D / _LINEAR2D)
//
//     L u = d/dx(kx u_x) + d/dy(ky u_y) + bx u_x + by u_y + s u = f        (1-D: (k u')' + b u' + s u = f)
//
// with kx, ky, bx, by, s given per quadrature point.  Once integrated by parts against test functions that vanish on the element's
// boundary, the residual of element e is
//
//     R[k][r] = -(J/Jx) sum_q kx u_x phi_r' phi_k  - (J/Jy) sum_q ky u_y phi_r phi_k'  +  J sum_q (bx u_x + by u_y + s u) phi_r phi_k  -  F[k][r]
//
// (the tables on the device are w * phi, derivatives with respect to the reference coordinate).  That is three integrand terms
//     t = 0: G0 = bx u_x + by u_y + s u   tables (0, 0)   c0 = J
//     t = 1: G1 = kx u_x                  tables (1, 0)   c1 = -(J/Jx)
//     t = 2: G2 = ky u_y                  tables (0, 1)   c2 = -(J/Jy)                (2-D only)
// with per-POINT coefficients -- more than ProjDesc / TermDesc (two terms, one constant per handle) can say, and nothing the
// whole-iteration kernels should pay registers for.  So the class has a projection kernel of its own, between the forward and the
// reverse layer kernels every network shape already has for the channel set u, u_x, u_y.
//
// One 256-thread workgroup per element, run-time shapes, sum-factorised like k_project:
//     T_t[j][r] = sum_i WTX[dx_t][r][i] G_t[j][i]          U[k][r] = sum_t c_t sum_j WTY[dy_t][k][j] T_t[j][r] - F[k][r]
// and, for the adjoint, with Rbar = (2 / n_active) R on the active block,
//     S_t[j][r] = c_t sum_k WTY[dy_t][k][j] Rbar[k][r]     Gbar_t[j][i] = sum_r WTX[dx_t][r][i] S_t[j][r]
//     GBAR[u] = s Gbar_0     GBAR[u_x] = kx Gbar_1 + bx Gbar_0     GBAR[u_y] = ky Gbar_2 + by Gbar_0.
// Every sum runs in index order in one thread, the block sum of R^2 is a fixed tree: no atomics, the same bits from call to call.
// A zero-weight padding point has all-zero table columns: it adds exactly 0 to T and receives Gbar = 0.
// LDS rows are padded to an odd number of doubles, so a lane-per-row access never lands on a power-of-two multiple of the banks.
// Out of scope: the strong form of the class (it takes derivatives of kx, ky).  hpv_set_collocation*, hpv_residual_points and
// hpv_element_indicators are refused on these handles; the strong residual at the elements' own quadrature points, for refinement
// indicators, is an opt-in with a kernel of its own (hpv_set_strong_form, k_lin_indicators, kernels_linadapt.hip).
#include "hpv_internal.h"
#include "hpv_lane.h"
#include "hpv_dual_norm.h"
#include "hpv_dual_dense.h"

namespace {

__device__ __forceinline__ int odd(int n) { return n | 1; }

// sum over the 256 threads, fixed order: butterfly inside each wave, the four wave sums added in wave order; every thread gets it
// (block_sum256 of hpv_lane.h, which k_moment_part shares)
__device__ __forceinline__ double lin_block_sum(double v, double* red) { return block_sum256(v, red); }

// DUAL: 1 the dual-norm loss of hpv_dual_norm.h between the two halves (hpv_set_residual_norm), 2 that of hpv_dual_dense.h
// (hpv_set_residual_gram: a dense inverse Gram factor per element); 0 is the kernel as it always was
// TENSOR: a full diffusion tensor per point (hpv_set_operator_tensor; 2-D only): seven planes (kxx, kxy, kyx, kyy, bx, by, s),
//     G1 = kxx u_x + kxy u_y     G2 = kyx u_x + kyy u_y     GBAR[u_x] = kxx Gbar_1 + kyx Gbar_2 + bx Gbar_0     GBAR[u_y] = kxy Gbar_1 + kyy Gbar_2 + by Gbar_0
// -- still three integrands, so tables, contractions and LDS are untouched; false is the kernel as it always was
template <int DUAL, bool TENSOR = false>
__device__ __forceinline__ void project_lin_body(const LinProjArgs& a) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const long e = blockIdx.x;
    const int qx = a.qx, qy = a.qy, ntx = a.ntx, nty = a.nty, nt = a.dim + 1;
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
        if constexpr (TENSOR) {
            const double uy = a.OUT[2 * N + base + q];
            const double kxx = cf[q], kxy = cf[cs + q], kyx = cf[2 * cs + q], kyy = cf[3 * cs + q];
            const double bx = cf[4 * cs + q], by = cf[5 * cs + q], s = cf[6 * cs + q];
            G[j * gs + i] = (bx * ux + by * uy) + s * u;
            G[(qy + j) * gs + i] = kxx * ux + kxy * uy;
            G[(2 * qy + j) * gs + i] = kyx * ux + kyy * uy;
        } else if (a.dim == 2) {
            const double uy = a.OUT[2 * N + base + q];
            const double kx = cf[q], ky = cf[cs + q], bx = cf[2 * cs + q], by = cf[3 * cs + q], s = cf[4 * cs + q];
            G[j * gs + i] = (bx * ux + by * uy) + s * u;
            G[(qy + j) * gs + i] = kx * ux;
            G[(2 * qy + j) * gs + i] = ky * uy;
        } else {
            const double k = cf[q], b = cf[cs + q], s = cf[2 * cs + q];
            G[j * gs + i] = b * ux + s * u;
            G[(qy + j) * gs + i] = k * ux;
        }
    }
    __syncthreads();

    // ---- T_t[j][r] = sum_i WTX[dx_t][r][i] G_t[j][i],  dx = (0, 1, 0) ----
    for (int idx = tid; idx < nt * qy * ntx; idx += 256) {
        const int tj = idx / ntx, r = idx - tj * ntx, t = tj / qy;
        const double* ax = X + ((t == 1 ? ntx : 0) + r) * xs;
        const double* g = G + tj * gs;
        double acc = 0.0;
        for (int i = 0; i < qx; ++i) acc += ax[i] * g[i];
        T[tj * ts + r] = acc;
    }
    __syncthreads();

    // ---- U[k][r] = sum_t c_t sum_j WTY[dy_t][k][j] T_t[j][r] - F,  dy = (0, 0, 1); masked; loss ----
    const double J = a.J[e];
    const double c0 = J, c1 = -(J / a.Jx[e]), c2 = a.dim == 2 ? -(J / a.Jy[e]) : 0.0;
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
            if (a.dim == 2)
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
        sq = hpv_dual_forward(a.dual, a.dual_mass, ntx, nty, nax, nay, a.Jx[e], a.dim == 2 ? a.Jy[e] : 1.0, U, ds);
    }
    sq = lin_block_sum(sq, red);          // (its barriers also order U before the adjoint and T's readers before S's writers)
    if (tid == 0) a.loss_e[e] = DUAL != 0 ? sq : sq / NRa;
    if (!a.do_adjoint) return;
    if constexpr (DUAL == 1) hpv_dual_adjoint(ntx, nty, nax, nay, U, ds);      // U <- d loss_e / d R: sc = 1 below
    if constexpr (DUAL == 2) hpv_dual_dense_adjoint(We, ntx, NR, nax, nay, U, yd);

    // ---- S_t[j][r] = c_t sum_k WTY[dy_t][k][j] Rbar[k][r],  Rbar = (2 / n_active) R ----
    const double sc = DUAL != 0 ? 1.0 : 2.0 / NRa;
    for (int idx = tid; idx < nt * qy * ntx; idx += 256) {
        const int tj = idx / ntx, r = idx - tj * ntx, t = tj / qy, j = tj - t * qy;
        const double* y = Y + (t == 2 ? nty * ys : 0) + j;
        double acc = 0.0;
        for (int k = 0; k < nty; ++k) acc += y[k * ys] * U[k * ntx + r];
        T[tj * ts + r] = (t == 0 ? c0 : t == 1 ? c1 : c2) * (sc * acc);
    }
    __syncthreads();

    // ---- Gbar_t[j][i] = sum_r WTX[dx_t][r][i] S_t[j][r]; the adjoints of the channels ----
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
            if (a.dim == 2) g2 += x0 * s2[r];
        }
        if constexpr (TENSOR) {
            const double kxx = cf[q], kxy = cf[cs + q], kyx = cf[2 * cs + q], kyy = cf[3 * cs + q];
            const double bx = cf[4 * cs + q], by = cf[5 * cs + q], s = cf[6 * cs + q];
            a.GBAR[base + q] = s * g0;
            a.GBAR[N + base + q] = (kxx * g1 + kyx * g2) + bx * g0;
            a.GBAR[2 * N + base + q] = (kxy * g1 + kyy * g2) + by * g0;
        } else if (a.dim == 2) {
            const double kx = cf[q], ky = cf[cs + q], bx = cf[2 * cs + q], by = cf[3 * cs + q], s = cf[4 * cs + q];
            a.GBAR[base + q] = s * g0;
            a.GBAR[N + base + q] = kx * g1 + bx * g0;
            a.GBAR[2 * N + base + q] = ky * g2 + by * g0;
        } else {
            const double k = cf[q], b = cf[cs + q], s = cf[2 * cs + q];
            a.GBAR[base + q] = s * g0;
            a.GBAR[N + base + q] = k * g1 + b * g0;
        }
    }
}

}  // namespace

__global__ void __launch_bounds__(256) k_project_lin(LinProjArgs a) { project_lin_body<0>(a); }
__global__ void __launch_bounds__(256) k_project_lin_dual(LinProjArgs a) { project_lin_body<1>(a); }
__global__ void __launch_bounds__(256) k_project_lin_tensor(LinProjArgs a) { project_lin_body<0, true>(a); }
__global__ void __launch_bounds__(256) k_project_lin_tensor_dual(LinProjArgs a) { project_lin_body<1, true>(a); }
__global__ void __launch_bounds__(256) k_project_lin_dense(LinProjArgs a) { project_lin_body<2>(a); }
__global__ void __launch_bounds__(256) k_project_lin_tensor_dense(LinProjArgs a) { project_lin_body<2, true>(a); }

size_t hpv_linop_lds_bytes(int qx, int qy, int ntx, int nty) {
    const size_t gs = (size_t)(qx | 1), ts = (size_t)(ntx | 1), ys = (size_t)(qy | 1);
    return (3 * qy * gs + 3 * qy * ts + (size_t)ntx * nty + 2 * ntx * gs + 2 * nty * ys + 4) * sizeof(double);
}

// the same layout, with the scratch of hpv_dual_norm.h appended where the G region cannot hold it
size_t hpv_dual_lds_bytes(int qx, int qy, int ntx, int nty) {
    return hpv_linop_lds_bytes(qx, qy, ntx, nty) + (hpv_dual_aliases_g(qx, qy, ntx, nty) ? 0 : hpv_dual_scratch_doubles(ntx, nty) * sizeof(double));
}

// the same layout, with y of hpv_dual_dense.h (NR doubles) appended where the G region cannot hold it
size_t hpv_dual_dense_lds_bytes(int qx, int qy, int ntx, int nty) {
    return hpv_linop_lds_bytes(qx, qy, ntx, nty) + (hpv_dual_dense_aliases_g(qx, qy, ntx, nty) ? 0 : (size_t)ntx * nty * sizeof(double));
}

void launch_project_lin(const LinProjArgs& a, long n_elem, hipStream_t s) {
    if (n_elem <= 0) return;
    const dim3 grid((unsigned)n_elem), block(256);
    if (a.dual_dense) {      // (hpv_set_residual_gram)
        const size_t ldsd = hpv_dual_dense_lds_bytes(a.qx, a.qy, a.ntx, a.nty);
        if (a.tensor) hipLaunchKernelGGL(k_project_lin_tensor_dense, grid, block, ldsd, s, a);
        else hipLaunchKernelGGL(k_project_lin_dense, grid, block, ldsd, s, a);
        return;
    }
    const size_t lds = a.dual ? hpv_dual_lds_bytes(a.qx, a.qy, a.ntx, a.nty) : hpv_linop_lds_bytes(a.qx, a.qy, a.ntx, a.nty);
    if (a.tensor) {      // (hpv_set_operator_tensor: 2-D only, the host has made sure)
        if (a.dual) hipLaunchKernelGGL(k_project_lin_tensor_dual, grid, block, lds, s, a);
        else hipLaunchKernelGGL(k_project_lin_tensor, grid, block, lds, s, a);
    } else if (a.dual) hipLaunchKernelGGL(k_project_lin_dual, grid, block, lds, s, a);
    else hipLaunchKernelGGL(k_project_lin, grid, block, lds, s, a);
}
