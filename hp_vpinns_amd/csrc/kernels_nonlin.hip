// k_project_nl: k_project_lin (kernels_linop.hip) with a pointwise nonlinear term on the same handles (HPV_PDE_LINEAR1D / _LINEAR2D)
//
//     L u + N(x; u, grad u) = f          N = a2 u^2 + a3 u^3 + ae exp(u) + u (gx u_x + gy u_y)        (1-D: ... + g u u_x)
//
// with L the operator of hpv_set_operator, its sign convention unchanged, and a2, a3, ae, gx, gy given per quadrature point
// (hpv_set_nonlinear).  N is projected against phi_r phi_k without integration by parts, so it joins the first integrand:
//     t = 0: G0 = (bx u_x + by u_y + s u) + N   tables (0, 0)   c0 = J
//     t = 1: G1 = kx u_x                        tables (1, 0)   c1 = -(J/Jx)
//     t = 2: G2 = ky u_y                        tables (0, 1)   c2 = -(J/Jy)                (2-D only)
// The projection stays linear in its integrands: tables, c_t, masking, F, R and loss_e are those of k_project_lin, and so are the two
// forward and the two adjoint contractions.  The nonlinearity is undone by the chain rule at the point, after the adjoint ones:
//     dN/du     = 2 a2 u + 3 a3 u^2 + ae exp(u) + gx u_x + gy u_y
//     GBAR[u]   = (s + dN/du) Gbar_0
//     GBAR[u_x] = kx Gbar_1 + (bx + gx u) Gbar_0
//     GBAR[u_y] = ky Gbar_2 + (by + gy u) Gbar_0.
// Special cases: space-time viscous Burgers u_t + u u_x - nu u_xx = 0 is kx = -nu, ky = 0, by = 1, gx = 1 on a 2-D handle with
// y = t (the AdvDiff special case with V replaced by u); Bratu u'' + lambda e^u = 0 is k = 1, ae = lambda; Allen-Cahn
// eps^2 lap u + u - u^3 = f is k = eps^2, s = 1, a3 = -1.
// Quasilinear diffusion (hpv_set_quasilinear; the QUASI instantiations, k_project_nl*_q): the flux is scaled by a multiplier at the point,
//     div(mu K grad u) + ..      mu = P(u) B(s)      P = m0 + m1 u + m2 u^2      B = (delta + s)^r      s = |grad u|^2 = u_x^2 [+ u_y^2]
// with m0, m1, m2, delta given per quadrature point and r one scalar per handle.  With F1, F2 the flux values above (kx u_x, ky u_y;
// kxx u_x + kxy u_y, kyx u_x + kyy u_y with a full tensor; k u' in 1-D) the integrands are G1 = mu F1, G2 = mu F2, and the chain rule
// after the adjoint contractions gains, with h = F1 Gbar_1 + F2 Gbar_2, mu_u = (m1 + 2 m2 u) B and mu_s = r P (delta + s)^(r-1),
//     GBAR[u]   += mu_u h       GBAR[u_x] = mu (kxx Gbar_1 + kyx Gbar_2) + .. + 2 u_x mu_s h       GBAR[u_y] likewise with u_y.
// u_x, u_y are physical derivatives on mapped elements too (the fold puts the geometry into K_eff), so s is the physical |grad u|^2.
// B costs one pow per point and phase, (delta + s)^(r-1) = B / (delta + s) one division; mu is recomputed in the adjoint phase from the
// channels re-read from OUT, as exp(u) is.  HPV_NL_DIFF_U / HPV_NL_DIFF_GRAD select the factors: without DIFF_GRAD pow is never called
// and delta never read, without DIFF_U m0, m1, m2 are never read.  P(u) > 0 is not checked; delta > 0 is the host's duty wherever
// r != 0, at padding points as well (their mu is then finite, multiplied by 0 forward and by Gbar = 0 backward).
// Out of scope: a diffusion coefficient outside that family (exp-type k(u)), solution-dependent anisotropy, trainable coefficients
// together with the multiplier; the strong form at arbitrary points (trainable coefficients:
// k_project_id, kernels_ident.hip; hpv_set_collocation*, hpv_residual_points and hpv_element_indicators stay refused as for the linear
// class; the strong residual at the elements' own points, for refinement: hpv_set_strong_form, k_lin_indicators, kernels_linadapt.hip;
// with the multiplier only the divergence form, k_div_indicators).
//
// Term mask (HPV_NL_*): a plane that is zero at every owned point is left out of the mask on the host, and its term is not evaluated
// at all -- the branch is uniform over the grid, an exp nobody asked for is never computed and 0 * inf cannot arise.  exp(u) is
// evaluated once per point and phase and serves N and dN/du; there is no guard against its overflow.
// The channels and exp(u) are NOT kept in LDS across the two contraction phases: the adjoint phase reads u, u_x, u_y from OUT again
// (L2-resident, 3 coalesced loads per point) and recomputes the one exp, so the kernel's LDS footprint is k_project_lin's to the byte
// and as many workgroups share a CU (profiles/nonlinear_terms.md).
// One 256-thread workgroup per element, run-time shapes, odd-padded LDS rows, every sum in index order in one thread, the block sum
// a fixed tree: no atomics, the same bits from call to call.  A zero-weight padding point has all-zero table columns: whatever finite
// value N takes there is multiplied by 0 in T, and its Gbar_0 = 0 makes every GBAR entry above 0.
#include "hpv_internal.h"
#include "hpv_dual_norm.h"
#include "hpv_dual_dense.h"

namespace {

__device__ __forceinline__ int odd(int n) { return n | 1; }

// sum over the 256 threads, fixed order: butterfly inside each wave, the four wave sums added in wave order; every thread gets it
__device__ __forceinline__ double nl_block_sum(double v, double* red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[w] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// N and dN/du at one point; ga = gx u_x + gy u_y (0 without the advection term).  Terms outside the mask are not touched.
__device__ __forceinline__ void nl_point(int mask, const double* nl, long cs, double u, double ga, double& Nv, double& dNu) {
    double n = 0.0, d = 0.0;
    if (mask & HPV_NL_QUADRATIC) {
        const double a2 = nl[0];
        n = a2 * (u * u);
        d = 2.0 * (a2 * u);
    }
    if (mask & HPV_NL_CUBIC) {
        const double a3 = nl[cs], uu = u * u;
        n += a3 * (uu * u);
        d += 3.0 * (a3 * uu);
    }
    if (mask & HPV_NL_EXP) {
        const double t = nl[2 * cs] * exp(u);
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

// mu = P(u) B(s) at one point and its partials mu_u, mu_s; qp the planes m0, m1, m2, delta at the point.  A factor outside the mask is 1
// and its planes are not touched.
__device__ __forceinline__ void quasi_point(int mask, const double* qp, long cs, double r, double u, double s, double& mu, double& mu_u, double& mu_s) {
    double P = 1.0, dP = 0.0, B = 1.0, dB = 0.0;
    if (mask & HPV_NL_DIFF_U) {
        const double m0 = qp[0], m1 = qp[cs], m2 = qp[2 * cs];
        P = (m0 + m1 * u) + m2 * (u * u);
        dP = m1 + 2.0 * (m2 * u);
    }
    if (mask & HPV_NL_DIFF_GRAD) {
        const double t = qp[3 * cs] + s;
        B = pow(t, r);
        dB = r * (B / t);
    }
    mu = P * B;
    mu_u = dP * B;
    mu_s = P * dB;
}

// DUAL: 1 the dual-norm loss of hpv_dual_norm.h between the two halves (hpv_set_residual_norm), 2 that of hpv_dual_dense.h
// (hpv_set_residual_gram: a dense inverse Gram factor per element); 0 is the kernel as it always was
// TENSOR: a full diffusion tensor per point (hpv_set_operator_tensor; 2-D only), as in project_lin_body: the operator has seven planes
// (kxx, kxy, kyx, kyy, bx, by, s), G1 = kxx u_x + kxy u_y, G2 = kyx u_x + kyy u_y; the nonlinear planes and N are untouched
// QUASI: the multiplier mu on the two flux integrands (hpv_set_quasilinear; the file header); false is the kernel as it always was
template <int DUAL, bool TENSOR = false, bool QUASI = false>
__device__ __forceinline__ void project_nl_body(const NlProjArgs& b) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const LinProjArgs& a = b.lin;
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
    const double* nl = QUASI && !b.nl ? nullptr : b.nl + base;      // planes a2, a3, ae, gx, (gy), the stride of the operator's (QUASI: none
    const int mask = b.mask;                                        //  where the mask holds no pointwise term -- nl_point reads nothing then)
    const double* qp = QUASI ? b.qp + base : nullptr;               // planes m0, m1, m2, delta, the same stride
    const double qr = b.qr;
    const bool adv = mask & HPV_NL_ADVECTION;

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
        double Nv, dNu;
        if constexpr (TENSOR) {
            const double uy = a.OUT[2 * N + base + q];
            const double kxx = cf[q], kxy = cf[cs + q], kyx = cf[2 * cs + q], kyy = cf[3 * cs + q];
            const double bx = cf[4 * cs + q], by = cf[5 * cs + q], s = cf[6 * cs + q];
            const double ga = adv ? nl[3 * cs + q] * ux + nl[4 * cs + q] * uy : 0.0;
            nl_point(mask, nl + q, cs, u, ga, Nv, dNu);
            G[j * gs + i] = ((bx * ux + by * uy) + s * u) + Nv;
            double f1 = kxx * ux + kxy * uy, f2 = kyx * ux + kyy * uy;
            if constexpr (QUASI) {
                double mu, mu_u, mu_s;
                quasi_point(mask, qp + q, cs, qr, u, ux * ux + uy * uy, mu, mu_u, mu_s);
                f1 *= mu;
                f2 *= mu;
            }
            G[(qy + j) * gs + i] = f1;
            G[(2 * qy + j) * gs + i] = f2;
        } else if (a.dim == 2) {
            const double uy = a.OUT[2 * N + base + q];
            const double kx = cf[q], ky = cf[cs + q], bx = cf[2 * cs + q], by = cf[3 * cs + q], s = cf[4 * cs + q];
            const double ga = adv ? nl[3 * cs + q] * ux + nl[4 * cs + q] * uy : 0.0;
            nl_point(mask, nl + q, cs, u, ga, Nv, dNu);
            G[j * gs + i] = ((bx * ux + by * uy) + s * u) + Nv;
            double f1 = kx * ux, f2 = ky * uy;
            if constexpr (QUASI) {
                double mu, mu_u, mu_s;
                quasi_point(mask, qp + q, cs, qr, u, ux * ux + uy * uy, mu, mu_u, mu_s);
                f1 *= mu;
                f2 *= mu;
            }
            G[(qy + j) * gs + i] = f1;
            G[(2 * qy + j) * gs + i] = f2;
        } else {
            const double k = cf[q], bb = cf[cs + q], s = cf[2 * cs + q];
            const double ga = adv ? nl[3 * cs + q] * ux : 0.0;
            nl_point(mask, nl + q, cs, u, ga, Nv, dNu);
            G[j * gs + i] = (bb * ux + s * u) + Nv;
            double f1 = k * ux;
            if constexpr (QUASI) {
                double mu, mu_u, mu_s;
                quasi_point(mask, qp + q, cs, qr, u, ux * ux, mu, mu_u, mu_s);
                f1 *= mu;
            }
            G[(qy + j) * gs + i] = f1;
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
    sq = nl_block_sum(sq, red);           // (its barriers also order U before the adjoint and T's readers before S's writers)
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

    // ---- Gbar_t[j][i] = sum_r WTX[dx_t][r][i] S_t[j][r]; the chain rule at the point; the adjoints of the channels ----
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
        const double u = a.OUT[base + q], ux = a.OUT[N + base + q];
        double Nv, dNu;
        if constexpr (TENSOR) {
            const double uy = a.OUT[2 * N + base + q];
            const double kxx = cf[q], kxy = cf[cs + q], kyx = cf[2 * cs + q], kyy = cf[3 * cs + q], s = cf[6 * cs + q];
            double bx = cf[4 * cs + q], by = cf[5 * cs + q], ga = 0.0;
            if (adv) {
                const double gx = nl[3 * cs + q], gy = nl[4 * cs + q];
                ga = gx * ux + gy * uy;
                bx += gx * u;
                by += gy * u;
            }
            nl_point(mask, nl + q, cs, u, ga, Nv, dNu);
            if constexpr (QUASI) {
                double mu, mu_u, mu_s;
                quasi_point(mask, qp + q, cs, qr, u, ux * ux + uy * uy, mu, mu_u, mu_s);
                const double h = (kxx * ux + kxy * uy) * g1 + (kyx * ux + kyy * uy) * g2;
                a.GBAR[base + q] = (s + dNu) * g0 + mu_u * h;
                a.GBAR[N + base + q] = (mu * (kxx * g1 + kyx * g2) + bx * g0) + 2.0 * ux * (mu_s * h);
                a.GBAR[2 * N + base + q] = (mu * (kxy * g1 + kyy * g2) + by * g0) + 2.0 * uy * (mu_s * h);
            } else {
                a.GBAR[base + q] = (s + dNu) * g0;
                a.GBAR[N + base + q] = (kxx * g1 + kyx * g2) + bx * g0;
                a.GBAR[2 * N + base + q] = (kxy * g1 + kyy * g2) + by * g0;
            }
        } else if (a.dim == 2) {
            const double uy = a.OUT[2 * N + base + q];
            const double kx = cf[q], ky = cf[cs + q], s = cf[4 * cs + q];
            double bx = cf[2 * cs + q], by = cf[3 * cs + q], ga = 0.0;
            if (adv) {
                const double gx = nl[3 * cs + q], gy = nl[4 * cs + q];
                ga = gx * ux + gy * uy;
                bx += gx * u;
                by += gy * u;
            }
            nl_point(mask, nl + q, cs, u, ga, Nv, dNu);
            if constexpr (QUASI) {
                double mu, mu_u, mu_s;
                quasi_point(mask, qp + q, cs, qr, u, ux * ux + uy * uy, mu, mu_u, mu_s);
                const double h = (kx * ux) * g1 + (ky * uy) * g2;
                a.GBAR[base + q] = (s + dNu) * g0 + mu_u * h;
                a.GBAR[N + base + q] = (mu * (kx * g1) + bx * g0) + 2.0 * ux * (mu_s * h);
                a.GBAR[2 * N + base + q] = (mu * (ky * g2) + by * g0) + 2.0 * uy * (mu_s * h);
            } else {
                a.GBAR[base + q] = (s + dNu) * g0;
                a.GBAR[N + base + q] = kx * g1 + bx * g0;
                a.GBAR[2 * N + base + q] = ky * g2 + by * g0;
            }
        } else {
            const double k = cf[q], s = cf[2 * cs + q];
            double bb = cf[cs + q], ga = 0.0;
            if (adv) {
                const double g = nl[3 * cs + q];
                ga = g * ux;
                bb += g * u;
            }
            nl_point(mask, nl + q, cs, u, ga, Nv, dNu);
            if constexpr (QUASI) {
                double mu, mu_u, mu_s;
                quasi_point(mask, qp + q, cs, qr, u, ux * ux, mu, mu_u, mu_s);
                const double h = (k * ux) * g1;
                a.GBAR[base + q] = (s + dNu) * g0 + mu_u * h;
                a.GBAR[N + base + q] = (mu * (k * g1) + bb * g0) + 2.0 * ux * (mu_s * h);
            } else {
                a.GBAR[base + q] = (s + dNu) * g0;
                a.GBAR[N + base + q] = k * g1 + bb * g0;
            }
        }
    }
}

}  // namespace

__global__ void __launch_bounds__(256) k_project_nl(NlProjArgs b) { project_nl_body<0>(b); }
__global__ void __launch_bounds__(256) k_project_nl_dual(NlProjArgs b) { project_nl_body<1>(b); }
__global__ void __launch_bounds__(256) k_project_nl_tensor(NlProjArgs b) { project_nl_body<0, true>(b); }
__global__ void __launch_bounds__(256) k_project_nl_tensor_dual(NlProjArgs b) { project_nl_body<1, true>(b); }
__global__ void __launch_bounds__(256) k_project_nl_dense(NlProjArgs b) { project_nl_body<2>(b); }
__global__ void __launch_bounds__(256) k_project_nl_tensor_dense(NlProjArgs b) { project_nl_body<2, true>(b); }
// (hpv_set_quasilinear: the same six with the multiplier on the flux)
__global__ void __launch_bounds__(256) k_project_nl_q(NlProjArgs b) { project_nl_body<0, false, true>(b); }
__global__ void __launch_bounds__(256) k_project_nl_dual_q(NlProjArgs b) { project_nl_body<1, false, true>(b); }
__global__ void __launch_bounds__(256) k_project_nl_tensor_q(NlProjArgs b) { project_nl_body<0, true, true>(b); }
__global__ void __launch_bounds__(256) k_project_nl_tensor_dual_q(NlProjArgs b) { project_nl_body<1, true, true>(b); }
__global__ void __launch_bounds__(256) k_project_nl_dense_q(NlProjArgs b) { project_nl_body<2, false, true>(b); }
__global__ void __launch_bounds__(256) k_project_nl_tensor_dense_q(NlProjArgs b) { project_nl_body<2, true, true>(b); }

// (the channels are re-read from OUT in the adjoint phase, so nothing is added to k_project_lin's layout)
size_t hpv_nonlin_lds_bytes(int qx, int qy, int ntx, int nty) { return hpv_linop_lds_bytes(qx, qy, ntx, nty); }

void launch_project_nl(const NlProjArgs& a, long n_elem, hipStream_t s) {
    if (n_elem <= 0) return;
    const dim3 grid((unsigned)n_elem), block(256);
    const bool quasi = a.mask & (HPV_NL_DIFF_U | HPV_NL_DIFF_GRAD);      // (hpv_set_quasilinear: the _q instantiations, the same LDS)
    if (a.lin.dual_dense) {      // (hpv_set_residual_gram)
        const size_t ldsd = hpv_dual_dense_lds_bytes(a.lin.qx, a.lin.qy, a.lin.ntx, a.lin.nty);
        if (a.lin.tensor) hipLaunchKernelGGL(quasi ? k_project_nl_tensor_dense_q : k_project_nl_tensor_dense, grid, block, ldsd, s, a);
        else hipLaunchKernelGGL(quasi ? k_project_nl_dense_q : k_project_nl_dense, grid, block, ldsd, s, a);
        return;
    }
    const size_t lds = a.lin.dual ? hpv_dual_lds_bytes(a.lin.qx, a.lin.qy, a.lin.ntx, a.lin.nty) : hpv_nonlin_lds_bytes(a.lin.qx, a.lin.qy, a.lin.ntx, a.lin.nty);
    if (a.lin.tensor) {      // (hpv_set_operator_tensor: 2-D only, the host has made sure)
        if (a.lin.dual) hipLaunchKernelGGL(quasi ? k_project_nl_tensor_dual_q : k_project_nl_tensor_dual, grid, block, lds, s, a);
        else hipLaunchKernelGGL(quasi ? k_project_nl_tensor_q : k_project_nl_tensor, grid, block, lds, s, a);
    } else if (a.lin.dual) hipLaunchKernelGGL(quasi ? k_project_nl_dual_q : k_project_nl_dual, grid, block, lds, s, a);
    else hipLaunchKernelGGL(quasi ? k_project_nl_q : k_project_nl, grid, block, lds, s, a);
}
