// Internal descriptors shared by the host orchestration (hpv_api.hip, hpv_pass.hip, hpv_exchange.hip, hpv_bench.hip) and the kernels.
// Everything here is plain-old-data passed to kernels by value (kernarg segment).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/hpvpinn.h"

#define HPV_MAXC 5    // value + up to 2 first tangents + up to 2 second tangents
#define HPV_MAXH 64   // widest layer the generic kernels handle
#define HPV_MAXT 2    // integrand terms per variational form

// Network + Taylor-channel layout.  Channel order everywhere: [value | d/dc for c in T1 | d2/dc2 for c in T2].
struct NetDesc {
    int d;                       // input dimension (1 or 2)
    int nl;                      // number of affine layers = n_layers - 1
    int width[HPV_MAX_LAYERS];   // layer widths, width[0] = d, width[nl] = 1
    int woff[HPV_MAX_LAYERS];    // offset of W_l (row-major [in][out]) in theta
    int boff[HPV_MAX_LAYERS];    // offset of b_l in theta
    int act;                     // HPV_ACT_*
    int nT1, nT2;                // number of first / second tangent channels
    int t1dim[2];                // input coordinate of each first tangent
    int t2idx[2];                // index INTO the T1 list of each second tangent
    // MIXED second tangent (round 6; nT1 == 2 && nT2 == 1 only): the one second-order channel is  t2w[0] d2/dc0^2 + t2w[1] d2/dc1^2
    // -- second-order Taylor channels propagate LINEARLY (z_cc -> s'' z_c^2 + s' z_cc -> W), so a weighted sum of them is itself one
    // channel: Poisson-2D var_form 0 integrates u_xx + u_yy (P2:91) and needs 4 channels instead of 5 in the forward, the tangent
    // recompute and the reverse pass.  {1, 0} = the plain second tangent of coordinate t2idx[0] = 0 (AdvDiff var_form 0, P3:163).
    double t2w[2];
    int C;                       // 1 + nT1 + nT2
    int nslot;                   // saved slots per hidden layer: A, A1, ZC[nT1], ZCC[nT2]
    long actoff[HPV_MAX_LAYERS]; // hidden layer l block starts at actoff[l] * N doubles in ACT
    int P;                       // number of network parameters (without epsilon)
};

// One integrand term: U[k][r] += mult * coef[e] * sum_q WTX[dx][r][i] WTY[dy][k][j] G[q],
// G = sum_ch (a0[ch] + eps * a1[ch]) OUT[ch][q],  mult = eps if eps_mult else 1.
struct TermDesc {
    int dx, dy;      // derivative order (0,1,2) of the test-function table per direction
    int eps_mult;    // the term carries the trainable epsilon as a factor (P3:171)
    double a0[HPV_MAXC];
    double a1[HPV_MAXC];
};

struct ProjDesc {
    int nterms;
    TermDesc t[HPV_MAXT];
    int qx, qy, ntx, nty;
    int C;
    int has_eps;     // theta carries a trailing trainable epsilon
    int edge;        // Poisson-1D var_form 3 boundary term (P1:90)
    // p-refinement of the 1-D driver (P1:66-67, 268-281: F_ext_total[e] may be shorter in some elements): number of ACTIVE test
    // functions per owned element (device pointer, nullptr = all ntx); the residual rows beyond it are zero and the element's
    // mean runs over the active ones.  The general projections (k_project, project_element_wg) and the 1-D tile kernel honour
    // it; of the specialised 2-D kernels only k_iter_fused does (with `nacty` below), the others are bypassed when it is set.
    const int* nact;
    // p-refinement of the 2-D drivers (P2:72-73, P3:112-113: Ntest_elementx = N_testfcn[0][ex], Ntest_elementy = N_testfcn[1][ey]):
    // the second direction's count per owned element (device pointer; nullptr = all nty -- always so in 1-D).  Set together with
    // `nact`, which then holds the x counts: element e keeps the residuals (k, r) with r < nact[e] and k < nacty[e], and its mean
    // runs over nact[e] * nacty[e] of them.  Honoured by the general projections and by k_iter_fused (kernels_fused.hip).
    const int* nacty;
};

// All arguments of one projection launch (plain pointers; passed by value in the kernarg segment).
struct ProjArgs {
    ProjDesc pd;
    const double* OUT;
    double* GBAR;
    double* R;
    const double* F;
    const double* coef;
    long coef_stride;
    const double* wtx;
    const double* wty;
    const double* eps_ptr;
    double* loss_e;
    double* deps_e;
    long N;
    int do_adjoint;
    const double* edge_u;
    const double* edge_dphi;
    const double* edge_coef;
    double* edge_gbar;
};

static inline size_t hpv_proj_lds_bytes(const ProjDesc& pd) {
    size_t nq = (size_t)pd.qx * pd.qy, nr = (size_t)pd.ntx * pd.nty;
    return (nq + (size_t)pd.qy * pd.ntx + nr + (size_t)pd.nterms * nr + (size_t)pd.nterms * pd.nty * pd.qx + 256) *
           sizeof(double);
}

// All arguments of the linear-problem projection launch (k_project_lin, kernels_linop.hip): the variable-coefficient class
//   d/dx(kx u_x) + d/dy(ky u_y) + bx u_x + by u_y + s u = f   with per-quadrature-point coefficients.
struct LinProjArgs {
    const double* OUT;       // [1 + dim][N] channels u, u_x, (u_y) of the quadrature batch
    double* GBAR;            // [1 + dim][N] their adjoints (written when do_adjoint)
    const double* coef;      // planes (k, b, s) in 1-D, (kx, ky, bx, by, s) in 2-D; element-major over the owned elements, q = j * qx + i
    long coef_stride;        // doubles between two planes (= n_owned * qx * qy)
    const double* F;         // [n_elem][nty][ntx], or nullptr (zero)
    double* R;               // [n_elem][nty][ntx]
    double* loss_e;          // [n_elem]
    const double* wtx;       // [3][ntx][qx] weighted tables (w phi, w phi', w phi''); the first two are read
    const double* wty;       // [3][nty][qy]
    const double *J, *Jx, *Jy;   // [n_elem] |J_e| and the half widths per direction (Jy: 2-D only)
    const int* nact;         // [n_elem] active counts per direction, or nullptr (all)
    const int* nacty;
    long N;
    int qx, qy, ntx, nty, dim;
    int do_adjoint;
    const double* dual;      // the tables of the dual-norm loss (hpv_set_residual_norm; layout: hpv_dual_norm.h), or nullptr: mean(R^2)
    double dual_mass;        // the weight of the L2 part of its inner product
    int tensor;              // 2-D, hpv_set_operator_tensor: coef holds seven planes (kxx, kxy, kyx, kyy, bx, by, s) and the TENSOR
                             // instantiations run: G1 = kxx u_x + kxy u_y, G2 = kyx u_x + kyy u_y (0: the planes above, the kernels as ever)
    int dual_dense;          // hpv_set_residual_gram: `dual` holds the inverse Gram factors W_e [n_elem][NR][NR] (hpv_dual_dense.h) and the
                             // _dense instantiations run (0: `dual` holds the eigen tables, or is nullptr)
};
size_t hpv_linop_lds_bytes(int qx, int qy, int ntx, int nty);
size_t hpv_dual_lds_bytes(int qx, int qy, int ntx, int nty);      // k_project_lin_dual, _nl_dual, _id<.., 1>: says whether the scratch is appended
size_t hpv_dual_dense_lds_bytes(int qx, int qy, int ntx, int nty);      // k_project_lin_dense, _nl_dense, _id<.., 2>: the same for the NR doubles of y
void launch_project_lin(const LinProjArgs& a, long n_elem, hipStream_t s);

// The same launch with a pointwise nonlinear term (k_project_nl, kernels_nonlin.hip; hpv_set_nonlinear):
//   L u + a2 u^2 + a3 u^3 + ae exp(u) + u (gx u_x + gy u_y) = f.   A term outside `mask` is not evaluated and its plane not read.
// Quasilinear diffusion (hpv_set_quasilinear): div(mu K grad u) with mu = P(u) B(|grad u|^2), P = m0 + m1 u + m2 u^2, B = (delta + s)^r;
// the bits HPV_NL_DIFF_U / _DIFF_GRAD say which factor is not identically 1, and either one selects the _q instantiations.
enum { HPV_NL_QUADRATIC = 1, HPV_NL_CUBIC = 2, HPV_NL_EXP = 4, HPV_NL_ADVECTION = 8, HPV_NL_DIFF_U = 16, HPV_NL_DIFF_GRAD = 32 };
struct NlProjArgs {
    LinProjArgs lin;
    const double* nl;        // planes (a2, a3, ae, g) in 1-D, (a2, a3, ae, gx, gy) in 2-D; layout and stride of lin.coef; may be nullptr
                             // where the mask holds none of the four pointwise terms
    int mask;                // HPV_NL_* of the planes that are not zero everywhere (never 0: such a handle launches k_project_lin)
    const double* qp;        // planes (m0, m1, m2, delta) of the multiplier, layout and stride of lin.coef; nullptr without a DIFF bit
    double qr;               // the exponent r of B
};
size_t hpv_nonlin_lds_bytes(int qx, int qy, int ntx, int nty);
void launch_project_nl(const NlProjArgs& a, long n_elem, hipStream_t s);

// The same launch with trainable coefficients (k_project_id, kernels_ident.hip; hpv_create_ex / hpv_set_trainable): every plane is
//   base_p + sum_m c_m D_m,p,   p over the operator planes followed by the nonlinear ones,   c = theta[P .. P + n_coef)
// and the kernel also reduces d lossv / d c_m per element.
#define HPV_ID_PLANES 12     // 7 + 5 with a full diffusion tensor; 5 + 5 in 2-D otherwise (3 + 4 in 1-D)
struct IdProjArgs {
    LinProjArgs lin;
    const double* nl;        // base planes of the nonlinear term (zeros where hpv_set_nonlinear gave none)
    int mask;                // HPV_NL_* of the terms that are evaluated: the base's and every term a direction touches
    const double* dirs;      // [n_coef][K + M][coef_stride] directions, the layout of lin.coef (K = 7 where lin.tensor)
    const double* c;         // theta + P on the device: read at every launch
    int n_coef;
    const int* dmask;        // [n_coef] on the device; bit p: plane p of direction m is not zero everywhere (the others are never read)
    double* dcoef_e;         // [n_coef][n_elem] partials of d lossv / d c_m (written when lin.do_adjoint; n_elem = the grid)
};
void launch_project_id(const IdProjArgs& a, long n_elem, hipStream_t s);

// Integral constraints (hpv_set_moments; kernels_moment.hip): K weighted moments I_k = sum_q m_k[q] u_q^p_k of the value channel and a
// penalty w_k (I_k - c_k)^2 on each, between the projection kernel and the reverse launch of a linear handle's pass.
struct MomentArgs {
    const double* OUT;       // the quadrature batch's channels; the value channel's first Nq entries are read
    double* GBAR;            // ... their adjoints; the same entries take the += (adjoint launches only)
    const double* m;         // [K][Nq] measure planes, the layout of LinProjArgs::coef
    long Nq, n_elem;
    int NQ, K;               // points per element, active terms (1 .. HPV_MAX_MOMENTS)
    int power[HPV_MAX_MOMENTS];
    double target[HPV_MAX_MOMENTS], weight[HPV_MAX_MOMENTS];
    double* part;            // [K][n_elem] per-element partial sums
    double* res;             // [3][HPV_MAX_MOMENTS] I_k | pen_k | 2 w_k (I_k - c_k) of this pass
    double* loss_e;          // pen_k -> loss_e[n_elem + k]
    int n_coef;              // trainable coefficients: dcoef_src [n_coef][n_elem] is laid out again as dcoef_dst [n_coef][n_elem + K],
    const double* dcoef_src; // zero tails, for k_finalize (whose rows are n_loss = n_elem + K long); dcoef_dst == nullptr: nothing to do
    double* dcoef_dst;
};
// k_moment_part, k_moment_close and, where adjoint, k_moment_adj
void launch_moments(const MomentArgs& a, bool adjoint, hipStream_t s);

struct AdamArgs {
    double *theta, *m, *v, *state;   // theta == nullptr: no update
    double lr, b1, b2, eps;
    // loss history: every training iteration appends {lossv, w*lossb, mean sq, epsilon} of ITS forward pass (= the loss
    // and the trainable coefficient after the previous update) at hist[4 * (*hist_idx)++]; entries beyond hist_cap are dropped
    double* hist;
    int* hist_idx;
    int hist_cap;
    // sticky failure flag of the handle (a SPLIT-mode element barrier timed out, kernels_fused.hip): while it is set -- or the
    // pad slot of the all-reduced buffer says some rank's is -- no update is applied (theta, m, v, beta powers, history untouched)
    int* xerr;
    // number of updates applied through this handle since it was created (thread 0 of the kernel that applies one adds 1);
    // the host reads it after a failed run to learn how many of the requested iterations took place (hpv_updates_applied)
    unsigned long long* n_upd;
};
#define HPV_HIST_CAP 4096

#ifdef __HIPCC__
// One TF1-Adam update of one parameter (P1:103-104; eps OUTSIDE the bias correction).  ONE definition for every place an update
// is applied (k_finalize, k_adam, k_p2p_exchange, the one-workgroup tail of k_iter_tile) or merely FORMED (the prologue of
// k_iter_fused computes with the updated parameter of the deferred update, k_finalize behind it stores it): all of them must
// produce the same bits, in every translation unit, under every compiler release -- so the operation sequence is pinned:
// floating-point contraction is OFF inside (each *, +, -, /, sqrt rounds on its own; no fma is formed here or there by the
// optimiser).  Advisor, round 5: under the default -ffp-contract the two compilations were free to fuse a*b + c differently.
__device__ __forceinline__ double hpv_adam_lr_t(double lr, double b1p, double b2p) {
#pragma clang fp contract(off)
    return lr * sqrt(1.0 - b2p) / (1.0 - b1p);
}
__device__ __forceinline__ void hpv_adam_one_lr(double lr_t, double b1, double b2, double eps, double g, double m0, double v0,
                                                double t0, double& m1, double& v1, double& t1) {
#pragma clang fp contract(off)
    const double gm = (1.0 - b1) * g, gv = (1.0 - b2) * g;
    m1 = b1 * m0 + gm;
    v1 = b2 * v0 + gv * g;
    t1 = t0 - lr_t * m1 / (sqrt(v1) + eps);
}
__device__ __forceinline__ void hpv_adam_one(double lr, double b1, double b2, double eps, double b1p, double b2p, double g, double m0,
                                             double v0, double t0, double& m1, double& v1, double& t1) {
    hpv_adam_one_lr(hpv_adam_lr_t(lr, b1p, b2p), b1, b2, eps, g, m0, v0, t0, m1, v1, t1);
}
#endif

// One-shot exchange of the packed buffer between the ranks of one node (multi-GPU path without a collective library
// in the iteration): every rank owns a mailbox [2 parities][world][n] doubles + arrival counters [2][world], mapped
// into every peer through hipIpc; see k_p2p_exchange (kernels_generic.hip).
#define HPV_P2P_MAX 8
struct P2PArgs {
    double* inbox[HPV_P2P_MAX];                 // inbox[r] = rank r's mailbox as mapped here (own rank: the local pointer)
    unsigned long long* flag[HPV_P2P_MAX];      // flag[r]  = rank r's arrival counters
    unsigned long long* counter;                // exchanges done so far (local)
    int* err;                                   // set to 1 when a peer did not arrive in time (sticky; the exchange then is a no-op)
    int world, rank, n;
    unsigned long long timeout_ticks;           // wait budget in s_memrealtime ticks (100 MHz)
};
#define HPV_P2P_POISON 0xFFFFFFFFFFFFFFFFULL     // arrival-counter value a rank publishes after giving up

// ---- kernel launchers (kernels_generic.hip) ----
void launch_mlp_fwd_generic(const NetDesc& nd, const double* theta, const double* X, double* ACT, double* OUT, long N,
                            int save_act, hipStream_t s);
void launch_mlp_bwd_generic(const NetDesc& nd, const double* theta, const double* X, const double* ACT,
                            const double* GBAR, double* GPART, int rows, long N, hipStream_t s);
int mlp_bwd_generic_rows(long N);
void launch_project(const ProjArgs& pa, long n_elem, hipStream_t s);
int data_loss_parts(int n);
void launch_data_loss(const double* U, const double* Ud, double* GBAR, double scale_grad, double* part, int n,
                      hipStream_t s);
// the flux term of a pass (k_flux_loss) as the finalize step sees it; all-zero: the handle has no flux data
struct FluxFin {
    const double* GPART;     // [rows][P] gradient rows of the flux batch's reverse pass (nullptr: forward-only pass)
    int rows;
    const double* part;      // [n_part] partial sums of r^2 (nullptr: no flux term)
    int n_part;
    double w;                // w_f
    int n;                   // n_f
    double* ms;              // the plain mean of r^2 (hpv_read_flux_loss)
};
int flux_loss_parts(int n);
void launch_flux_loss(const double* OUT, long N, int dim, const double* coef, const double* g, double* GBAR,
                      double scale_grad, double* part, int n, hipStream_t s);
// the ansatz u = G + D N on the points [off, off + n) of a batch's channel planes [nch][N] (kernels_ansatz.hip; hpv_set_ansatz): OUT in
// place behind a forward launch, GBAR in place in front of a reverse launch.  planes: [2 * (1 + dim)][n] = (G, G_x[, G_y], D, D_x[, D_y]);
// nch: the channels the batch carries, 1 (u alone) or 1 + dim
void launch_ansatz_fwd(double* OUT, long N, long off, long n, int dim, int nch, const double* planes, hipStream_t s);
void launch_ansatz_adj(double* GBAR, long N, long off, long n, int dim, int nch, const double* planes, hipStream_t s);
// All arguments of the finalize launch (k_finalize); a field left at its zero value is an argument that is not there.
struct GradRows { const double* GPART; int rows; };   // [rows][P] partial gradients of one batch's reverse pass (nullptr: not a source)
struct FinalizeArgs {
    GradRows g[3];           // quadrature (PINN scheme: collocation) batch, the data batch of its own, the element-edge batch
    const double* loss_e;    // [n_loss] loss partials: per element (and row split) / per block of k_pinn_residual
    long n_loss;
    const double* deps_e;    // [n_loss] partials of d loss / d epsilon (nullptr: none)
    int n_coef;              // trainable coefficients of a linear handle behind the network (hpv_create_ex); 0: none
    const double* dcoef_e;   // [n_coef][n_loss] partials of d loss / d c_m (k_project_id)
    const double* data_part; // [n_data_part] partial sums of the data term
    int n_data_part;
    double lossb_weight;
    int n_data;
    int P, has_eps;
    double* RB;              // the packed buffer [grad (P) | (d eps) | (d c_0 ..) | lossv | w*lossb | mean square | pad]
    int write_grad;          // reverse-mode pass: the gradient rows are summed
    AdamArgs adam;           // the TF1-Adam update applied behind the sums (theta == nullptr: none; ignored without write_grad)
    const int* xerr;         // the handle's sticky failure flag (nullptr: no kernel of the pass can set it)
    unsigned int* xiter_bump;// launch counter of the shared-element kernels' exchange, advanced here (nullptr: none ran)
    int pending_adam;        // `adam` is the PREVIOUS iteration's deferred update: stored before RB takes this pass's sums
    FluxFin fx;              // the flux term
};
void launch_finalize(const FinalizeArgs& a, hipStream_t s);
void launch_adam(const AdamArgs& ad, const double* RB, int P, int Ptot, hipStream_t s);
void launch_p2p_exchange(const P2PArgs& pp, double* RB, const AdamArgs* adam_or_null, int P, int Ptot, hipStream_t s);
int adam_state_doubles(int P);
void launch_debug_act(int act, const double* x, int n, double* a, double* a1, double* ref, hipStream_t s);
void launch_gll_rule(int Q, double* x, double* w, hipStream_t s);
void launch_test_tables(int ntest, int q, const double* xi, double* tab, hipStream_t s);
bool launch_project_tp(const ProjArgs& pa, long n_elem, hipStream_t s);
int pinn_residual_parts(int n);
// All arguments of the strong-form residual launch (k_pinn_residual, kernels_generic.hip).
struct PinnArgs {
    const double* OUT;       // [C][N] channels of the collocation batch
    const double* f;         // [n] right-hand side at the points
    double* GBAR;            // [C][N] adjoints, every row written (write_gbar)
    double* part;            // [pinn_residual_parts(n)] per-block sums of r^2 / n_total
    double* deps_part;       // [pinn_residual_parts(n)] per-block sums of d lossp / d epsilon (AdvDiff only)
    const double* eps_ptr;   // theta + P on the device (AdvDiff only)
    double V;                // advection speed (AdvDiff only)
    long N;
    int n;                   // points of THIS shard
    long n_total;            // points of all shards: the mean runs over them
    int write_gbar;
};
void launch_pinn_residual(int pde, const PinnArgs& a, hipStream_t s);
bool launch_project_wg(const ProjArgs& pa, long n_elem, hipStream_t s, double* upart = nullptr);
int project_row_split(const ProjDesc& pd, long n_elem, int backend_generic);   // workgroups per element of the row-split projection

// ---- device-side validation (kernels_validate.hip) ----
// All arguments of the error-norm reduction over a validation set: {sum (u^ - u)^2, sum u^2, max |u^ - u|, sum |grad u^ - grad u|^2,
// sum |grad u|^2, n} -- six doubles written at `out`, or appended to the device-side history at hist[6 * (*hist_idx)++] (entries
// beyond hist_cap are dropped, the index still counts them) when `hist` is given.
struct ValArgs {
    const double* OUT;       // [C][N] channels of the validation batch: u^, then d/dx, d/dy (d/dt) when du is given
    long N;
    const double* u;         // [n] exact values
    const double* du;        // [dim][n] exact gradients, or nullptr (the two gradient sums are then 0)
    int n, dim;
    double* part;            // [HPV_VAL_MAX_BLOCKS][5] per-workgroup partial results (several workgroups only)
    unsigned int* ticket;    // arrival counter of the workgroups, left at 0 by every launch
    double* out;             // [6]
    double* hist;            // [hist_cap][6], or nullptr
    int* hist_idx;
    int hist_cap;
};
#define HPV_VAL_MAX_BLOCKS 64
int validate_reduce_blocks(int n);       // the workgroups the reduction runs with at n points (a function of n alone: fixed summation order)
void launch_validate_reduce(const ValArgs& a, int blocks, hipStream_t s);
// strong residual from the full channel list [u, u_x, (u_y | u_t), u_xx, (u_yy | u_tt)] at n foreign points (formulas: hpv_set_collocation)
void launch_residual_points(int pde, const double* OUT, long N, const double* f_or_null, const double* eps_ptr, double V, int n,
                            double* r, hipStream_t s);

// ---- L-BFGS stage (kernels_lbfgs.hip; hpv_lbfgs_step) ----
// The device-resident state of the optimiser: every vector has P entries and stays on the device; only `scal` travels.  The ring
// holds n_hist <= m pairs (s_i, y_i) at the slots head, head + 1, .. (mod m), oldest first.
#define HPV_LBFGS_MAX_HISTORY 64
#define HPV_LBFGS_YS_MIN 1e-10    // a pair with y . s at or below this is skipped (the curvature test of the reference implementation)
struct LbfgsArgs {
    int P, m;
    double *S, *Y;           // [m][P] the rings of steps s = t d and gradient differences y
    double* rho;             // [m] 1 / (y_i . s_i)
    double* h_diag;          // [1] (y . s) / (y . y) of the newest pair; 1 while there is none
    int* ring;               // [4] head, n_hist, pairs skipped so far, unused
    double* g;               // [P] gradient at theta0 (the accepted iterate): g_prev of the next pair
    double* d;               // [P] search direction
    double* theta0;          // [P] the accepted iterate
    double* theta;           // [P] the handle's live parameters (what a pass reads)
    double* scal;            // [8]: k_lbfgs_direction writes [0..3] = g . d, max|g|, sum|g|, max|d|;
                             //      k_lbfgs_probe writes [4..7] = loss, g_new . d, max|g_new|, 0
};
void launch_lbfgs_direction(const LbfgsArgs& a, hipStream_t s);
void launch_lbfgs_trial(const LbfgsArgs& a, double t, hipStream_t s);
// RB = [grad (P) | lossv | w*lossb | ..] of the pass just run; the gradient is copied to g_keep [P] (a: nothing to project on --
// the call's first evaluation -- when with_d == 0; g . d is then 0)
void launch_lbfgs_probe(const LbfgsArgs& a, const double* RB, double* g_keep, int with_d, hipStream_t s);
void launch_lbfgs_push(const LbfgsArgs& a, double t, const double* g_new, hipStream_t s);

// ---- per-element refinement indicators (kernels_adapt.hip; hpv_element_indicators) ----
struct IndArgs {
    const double* OUT;       // [5 | 3][N] the full channel list at the quadrature batch's points (element-major, q = j * qx + i)
    long N;
    const double* f;         // [n_elem * qx * qy] right-hand side at those points, or nullptr (zero)
    const double* eps_ptr;   // theta + P on the device (AdvDiff only)
    double V;
    const double* wx;        // [qx] raw 1-D weights
    const double* wy;        // [qy] (1-D problems: one entry, 1.0)
    int qx, qy;
    const double* jac;       // [n_elem] |J_e|
    const double* R;         // [n_elem][nty][ntx] residuals of the most recent pass
    int ntx, nty;
    const int* nact;         // [n_elem] active counts per direction, or nullptr (all)
    const int* nacty;
    double* out;             // [n_elem][HPV_IND_N]
};
void launch_elem_indicators(int pde, const IndArgs& a, long n_elem, hipStream_t s);

// ---- the same for the linear problems (kernels_linadapt.hip; hpv_set_strong_form, hpv_linear_indicators) ----
struct LinIndArgs {
    const double* OUT;       // [5 | 3][N] the full channel list at the quadrature batch's points (element-major, q = j * qx + i)
    long N;
    const double* f;         // [n_elem * qx * qy] right-hand side at those points, or nullptr (zero)
    const double* coef;      // the operator planes of LinProjArgs
    long cs;                 // doubles between two planes (= n_owned * qx * qy)
    const double* nl;        // base planes of the nonlinear term (NlProjArgs / IdProjArgs), or nullptr when mask == 0
    int mask;                // HPV_NL_* of the terms that are evaluated
    const double* dirs;      // [n_coef][K + M][cs] directions of the trainable coefficients, or nullptr
    const double* c;         // theta + P on the device: read at the launch
    int n_coef;              // 0: the base planes are the effective ones
    const int* dmask;        // [n_coef] on the device; bit p: plane p of direction m is not zero everywhere (the others are never read)
    const double* Dx;        // [qx][qx] differentiation matrix of the rule's x nodes on the reference interval, row-major
    const double* Dy;        // [qy][qy] (2-D only)
    const double* wx;        // [qx] raw 1-D weights
    const double* wy;        // [qy] (1-D problems: one entry, 1.0)
    const double *J, *Jx, *Jy;   // [n_elem] |J_e| and the half widths per direction (Jy: 2-D only)
    const double* R;         // [n_elem][nty][ntx] residuals of the most recent pass
    const int* nact;         // [n_elem] active counts per direction, or nullptr (all)
    const int* nacty;
    double* out;             // [n_elem][HPV_IND_N]
    double* r_out;           // [n_elem * qx * qy] the strong residual at every point, or nullptr (not wanted)
    int qx, qy, ntx, nty, dim;
    const double* loss_e;    // [n_elem] the dual-norm loss the forward-only pass wrote (column 0 under hpv_set_residual_norm), or nullptr
    // k_div_indicators only (hpv_set_strong_form_div): OUT is then [3 | 2][N] = u, u_x[, u_y] of the quadrature batch after the pass
    const double* inv_det;   // [n_elem * qx * qy] 1 / det A at every point of the unit (mapped) elements, or nullptr (boxes: 1)
    int tensor;              // coef holds seven planes (hpv_set_operator_tensor)
    const double* qp;        // planes (m0, m1, m2, delta) of the flux multiplier (hpv_set_quasilinear; NlProjArgs), stride cs, or nullptr:
    double qr;               // then mask holds neither HPV_NL_DIFF_U nor _DIFF_GRAD.  qr: the exponent of B
};
size_t hpv_linadapt_lds_bytes(int dim, int qx, int qy);
void launch_lin_indicators(const LinIndArgs& a, long n_elem, hipStream_t s);
size_t hpv_div_lds_bytes(int dim, int qx, int qy);
void launch_div_indicators(const LinIndArgs& a, long n_elem, hipStream_t s);
