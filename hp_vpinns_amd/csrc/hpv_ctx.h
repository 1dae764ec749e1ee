// Shared by the host-side translation units of libhpvpinn.so (hpv_api.hip: handle, set-up, batches, the C-ABI's entry points;
// hpv_pass.hip: the pass engine -- passes, exchange, sequences of iterations; hpv_exchange.hip: the multi-GPU exchanges;
// hpv_bench.hip: timing / benchmark / debug hooks): the handle itself and the few helpers and entry points they share.
#pragma once
#include <dlfcn.h>
#include <unistd.h>
#include <rccl/rccl.h>   // types and prototypes only: the library is dlopen'ed on first multi-GPU use (no link-time dependency)

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "hpv_internal.h"
#include "hpv_mfma.h"
#include "hpv_project_wg.h"

struct Batch {
    long N = 0;
    NetDesc nd{};
    double* X = nullptr;     // [d][N]
    double* ACT = nullptr;   // saved slots of every hidden layer
    double* OUT = nullptr;   // [C][N]
    double* GBAR = nullptr;  // [C][N]
    double* GPART = nullptr; // [rows][P] partial parameter gradients
    int rows = 0;
    size_t act_doubles = 0;
    HpvMfma* m = nullptr;    // the MFMA layer kernels' object for exactly this batch (nullptr: generic kernels); goes with it (free_batch)
};

struct TimerClass {
    std::vector<hipEvent_t> ev;  // start/stop pairs
    size_t used = 0;
    double total_ms = 0.0;
    long launches = 0;
};

struct hpv_ctx {
    hpv_config cfg{};
    std::string err;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    int dim = 1;
    int P = 0, Ptot = 0, has_eps = 0;
    NetDesc nd_var{}, nd_val{};
    ProjDesc pd{};
    int backend = HPV_BACKEND_GENERIC;
    // quadrature / tables (host copies + device weighted tables)
    std::vector<double> xi, wx, yi, wy;
    int qx = 0, qy = 1, ntx = 0, nty = 1;
    double *d_wtx = nullptr, *d_wty = nullptr, *d_edge_dphi = nullptr;
    bool have_quad = false, have_tables = false, have_elems = false, have_params = false;
    // elements
    int nex = 0, ney = 1, e_begin = 0, e_end = 0;
    int ne_tot = 0;                // elements of the whole mesh: nex * ney of a grid, the rows of a box list (hpv_set_element_boxes)
    long n_elem = 0;
    double *d_coef = nullptr, *d_edge_coef = nullptr, *d_F = nullptr, *d_R = nullptr, *d_loss_e = nullptr,
           *d_deps_e = nullptr;
    std::vector<double> F_all;
    bool have_F = false;
    std::vector<int> nact_all;     // active test functions per element of the whole grid (empty: all); see hpv_set_active_tests
    int* d_nact = nullptr;         // ... of the owned elements
    std::vector<int> nacty_all;    // 2-D: the second direction's counts (nact_all then holds the x counts); see hpv_set_active_tests_2d
    int* d_nacty = nullptr;
    Batch var, data, edge, pred;
    // host copies of the point sets; the device batches are (re)assembled lazily (assemble_batches)
    std::vector<double> Xq_host;   // [dim][Nq] quadrature points of the owned elements
    std::vector<double> Xd_host;   // [n_data][dim] boundary / data points
    long Nq = 0;
    bool batch_dirty = true;
    bool merged = false;           // MFMA path: data points ride as extra tiles of the quadrature batch
    long data_off = 0;             // first data point inside the merged batch
    double* d_udata = nullptr;
    double* d_data_part = nullptr;
    int n_data = 0;
    // flux term (hpv_set_flux_data): lossf = w_f * mean((a u + b . grad u - g)^2) at points of its own -- a batch under nd_grad
    // (N = n_flux rounded up to a 16-point tile), k_flux_loss between its forward and its reverse launch
    Batch flux;
    int n_flux = 0;
    double w_flux = 0.0;
    double *d_flux_coef = nullptr, *d_flux_g = nullptr;   // [1 + dim][n_flux] rows a, b_0 ..; [n_flux]
    double* d_flux_part = nullptr;                        // [64] partial sums of r^2, then [1] the plain mean of the most recent pass
    // parameters / optimizer
    double *d_theta = nullptr, *d_m = nullptr, *d_v = nullptr, *d_state = nullptr, *d_RB = nullptr;
    double* d_hist = nullptr;   // [HPV_HIST_CAP][4] loss / epsilon history (AdamArgs)
    int* d_hist_idx = nullptr;
    unsigned long long* d_nupd = nullptr;   // updates applied so far (AdamArgs::n_upd)
    bool shared_elem_ok = true; // hpv_set_shared_element_kernels
    long long nupd_host = 0;    // updates ENQUEUED so far (equals *d_nupd once the stream is idle unless a run failed)
    int n_fallbacks = 0;        // runs finished on the barrier-free structures after an exchange timeout (after_exchange_timeout)
    int* d_xerr = nullptr;      // sticky failure flag: a SPLIT-mode element barrier timed out (kernels_fused.hip); see sync_check
    // hpv_eval_channels reports the REFERENCE's channel list (nd_eval); where the training pass runs on fewer channels (Poisson-2D
    // var_form 0: u_xx + u_yy as one mixed second tangent, NetDesc::t2w) a forward-only object + output buffer are created on demand
    NetDesc nd_eval{};
    bool eval_differs = false;
    HpvMfma* mfma_eval = nullptr;
    double* d_eval_out = nullptr;
    long eval_N = 0;
    // strong-form PINN branch (scheme == PINNs): collocation batch with the channels of the problem's residual (k_pinn_residual) -- 1-D
    // u, u_x, u_xx; 2-D u, u_x, u_y and the Laplacian as one mixed second tangent; AdvDiff u, u_x, u_t, u_xx
    NetDesc nd_pinn{};
    Batch colloc;
    double *d_fcol = nullptr, *d_col_part = nullptr;      // d_col_part: [64] r^2 partials, then [64] d epsilon partials
    int n_col = 0;
    long n_col_total = 0;      // collocation points of ALL shards (the mean of P2:124 runs over them)
    double* d_jac = nullptr;   // |J_e| of the owned elements (RHS assembly, hpv_assemble_rhs)
    // linear problems (HPV_PDE_LINEAR1D / _LINEAR2D; hpv_set_operator): the coefficient planes [3 | 5][Nq] at the owned quadrature
    // points and the half widths [2][n_elem] = (Jx | Jy) of the owned elements; k_project_lin (kernels_linop.hip) reads both
    bool linear = false;
    bool have_lin = false;     // the planes belong to the current elements
    double *d_lin = nullptr, *d_jxy = nullptr;
    // hpv_set_operator_tensor: d_lin holds seven planes (kxx, kxy, kyx, kyy, bx, by, s) and the TENSOR instantiations of the three
    // projection kernels run (2-D only); the operator call made last decides.  hpv_set_element_points: the elements are unit elements
    // (J = Jx = Jy = 1) at the caller's points -- the host has folded the element maps into the planes
    bool lin_tensor = false;
    bool unit_elems = false;
    // the nonlinear term of such a handle (hpv_set_nonlinear): planes [4 | 5][Nq], the HPV_NL_* mask of the planes that are not zero
    // everywhere (0: no term, k_project_lin runs), and whether new elements have orphaned a term that has not been set again or removed
    double* d_nl = nullptr;
    int nl_mask = 0;
    bool nl_stale = false;
    // the flux multiplier of such a handle (hpv_set_quasilinear): planes [4][Nq] = m0, m1, m2, delta, the exponent, the bits
    // HPV_NL_DIFF_U | _DIFF_GRAD of the factors that are not identically 1 (0: no multiplier, the planes are freed; the launch ORs
    // them into nl_mask, and either one selects k_project_nl's _q instantiations), and the same orphan rule as nl_stale
    double* d_qp = nullptr;
    double q_exp = 0.0;
    int q_mask = 0;
    bool q_stale = false;
    // the integral constraints of such a handle (hpv_set_moments): n_mom terms (0: none, everything below is freed and the handle launches
    // what it launched before), their powers, targets and weights, the measure planes [n_mom][Nq], the per-element partials
    // [n_mom][n_elem], the results [3][HPV_MAX_MOMENTS] of the last pass (MomentArgs::res), with trainable coefficients the rows
    // [n_coef][n_elem + n_mom] k_finalize reads in place of d_dcoef_e, and the same orphan rule as nl_stale
    int n_mom = 0;
    int mom_power[HPV_MAX_MOMENTS] = {};
    double mom_target[HPV_MAX_MOMENTS] = {}, mom_weight[HPV_MAX_MOMENTS] = {};
    double *d_mom = nullptr, *d_mom_part = nullptr, *d_mom_res = nullptr, *d_mom_dcoef = nullptr;
    bool mom_stale = false;
    // the dual-norm loss of such a handle (hpv_set_residual_norm): the eigen tables of the test functions' Gram matrices (layout:
    // hpv_dual_norm.h; nullptr: mean(R^2)), the weight of the L2 part, and whether hpv_set_tables has dropped tables that have not
    // been given again (the tables belong to the test-function tables; a pass then refuses)
    double* d_dual = nullptr;
    double dual_mass = 0.0;
    bool dual_stale = false;
    // the same loss through dense factors (hpv_set_residual_gram): W_e = L_e^{-1} [n_elem][NR][NR] of the owned elements (layout:
    // hpv_dual_dense.h; nullptr: not set), and whether new tables, elements or counts have dropped factors that have not been given
    // again (they belong to the elements AND the test functions; a pass then refuses).  At most one of d_dual, d_gram is set.
    double* d_gram = nullptr;
    bool gram_stale = false;
    // trainable coefficients of such a handle (hpv_create_ex, hpv_set_trainable): n_coef slots behind the network in theta, their
    // directions [n_coef][K + M][Nq], the per-direction masks of the planes that are not zero everywhere (host and device copy), the
    // HPV_NL_* terms the directions touch, the partials [n_coef][n_elem] of d lossv / d c_m, and -- where hpv_set_nonlinear gave no
    // planes but a direction touches a term -- zero base planes [M][Nq] for k_project_id to read
    int n_coef = 0;
    bool have_dirs = false;    // the directions belong to the current elements
    double *d_dirs = nullptr, *d_dcoef_e = nullptr, *d_nl_zero = nullptr;
    int dir_mask[HPV_MAX_COEF] = {};
    int* d_dir_mask = nullptr;
    int dir_nl_mask = 0;
    // exact Dirichlet conditions by ansatz u = G + D N (hpv_set_ansatz): per point set (HPV_ANSATZ_QUAD, _DATA, _FLUX, _VALID) the planes
    // [2 * (1 + dim)][n] = (G, G_x[, G_y], D, D_x[, D_y]) at its points.  ans_on: the set has planes (an empty set's are no allocation);
    // the point-set calls drop their own.  A handle with any of them keeps its data points in a batch of their own (assemble_batches)
    bool ans_on[4] = {};
    double* d_ans[4] = {};
    long ans_n[4] = {};
    // per-element refinement indicators (hpv_element_indicators): the raw 1-D weights [qx | qy] (uploaded with the quadrature), a
    // forward-only object of the full channel set on the quadrature batch's own X and its buffers; re-created when Nq (sizes d_ind_f),
    // the batch size var.N (sizes d_ind_out and the object) or the owned element count (sizes d_ind) changes
    double* d_wq = nullptr;
    HpvMfma* mfma_ind = nullptr;
    double *d_ind_out = nullptr, *d_ind_f = nullptr, *d_ind = nullptr;
    long ind_Nq = -1, ind_N = -1, ind_ne = -1;
    // the strong form of a linear handle (hpv_set_strong_form): the differentiation matrices [qx*qx | qy*qy] of the current rule
    // (nullptr: not set -- hpv_linear_indicators refuses); they go with the rule (hpv_set_quadrature), nothing a pass reads.
    // d_ind_r: the strong residual at the owned points for a caller who asks, sized by Nq (ind_r_n)
    double* d_sf = nullptr;
    // the same in divergence form (hpv_set_strong_form_div; at most one of d_sf, d_sfd is set): the matrices, and on unit elements
    // 1 / det A at the owned points [n_elem * qx * qy] (nullptr on boxes).  Both belong to the rule AND the elements: a new rule,
    // new boxes or new points drop them and set sfd_stale, and hpv_linear_indicators answers -3 until they are handed over again
    double *d_sfd = nullptr, *d_inv_det = nullptr;
    bool sfd_stale = false;
    double* d_ind_r = nullptr;
    long ind_r_n = -1;
    // device-side validation (hpv_eval_points .. hpv_step_validate): forward-only batches at the caller's points
    NetDesc nd_full{};         // the full channel list: u, every first and every second input derivative (hpv_eval_points)
    NetDesc nd_grad{};         // u and the first derivatives (validation against exact gradients)
    Batch evalp;               // batch of hpv_eval_points / hpv_residual_points, re-created when n changes
    double *d_res_f = nullptr, *d_res_r = nullptr;      // [evalp.N] right-hand side and residual of hpv_residual_points
    Batch valb;                // the stored validation set (nd_val, or nd_grad with exact gradients)
    int n_val = 0;
    double *d_val_u = nullptr, *d_val_du = nullptr;     // exact values [n], exact gradients [dim][n] (nullptr: none given)
    double* d_val_buf = nullptr;   // [6] result of hpv_validate | [HPV_HIST_CAP][6] history | [HPV_VAL_MAX_BLOCKS][5] partials
    int* d_val_idx = nullptr;      // [0] history index, [1] the reduction's ticket counter
    // L-BFGS stage (hpv_lbfgs_step; hpv_lbfgs.hip): one allocation d_lb = [theta0 | g | d | three gradient slots of the line search |
    // S[m] | Y[m]] (Ptot each) | rho[m] | h_diag | scal[8], the ring's counters d_lb_ring[4], the capacity lb_m the buffers were made
    // for (0: none yet) and the iterations taken since the history was last dropped (the first one steps along -g with its own length)
    double* d_lb = nullptr;
    int* d_lb_ring = nullptr;
    int lb_m = 0;
    long long lb_iters = 0;
    // in-library exchange of the packed buffer between the ranks of a node (hpv_p2p_*)
    P2PArgs pp{};
    bool p2p_on = false;
    int pass_structure = -1;   // see hpv_pass_structure
    char variant[320] = "";    // see hpv_kernel_variant
    double* d_inbox = nullptr;
    unsigned long long* d_flag = nullptr;
    unsigned long long* d_p2p_counter = nullptr;
    int* d_p2p_err = nullptr;
    void* p2p_maps[2 * HPV_P2P_MAX] = {};
    // in-library RCCL all-reduce of the packed buffer (hpv_rccl_*): the multi-GPU default
    ncclComm_t rccl_comm = nullptr;
    bool rccl_on = false;
    int rccl_world = 1, rccl_rank = 0;
    // hpv_rccl_abandon (the ONE entry point that may be called from another thread while a call is inside the library): the
    // caller has given up waiting for a blocking hpv_rccl_connect / hpv_rccl_selftest that runs on a helper thread.  The
    // abandoned call then never touches the handle again: a communicator that comes up late is destroyed, rccl_on stays false
    std::atomic<int> rccl_abandoned{0};
    double* d_upart = nullptr; // partial residual sums of the row-split projection (few tall elements)
    int proj_split = 1;        // workgroups per element there; loss_e / deps_e hold n_elem * proj_split entries
    long n_red_alloc = 0;      // entries loss_e / deps_e were allocated with (>= every launch structure's count)
    long n_loss_entries = 0;   // entries the most recent pass wrote (what the finalize kernel sums)
    // timing
    bool timing = false;
    TimerClass timers[3];
    // whole-iteration hipGraph (forward + projection + backward || boundary branch -> finalize -> Adam)
    hipStream_t stream2 = nullptr;       // side stream: the boundary/data branch runs beside the main branch
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    bool side_active = false;            // true only while capturing
    bool use_graph = true;
    // the multi-GPU iteration in two launches (in-library RCCL exchange): inside a sequence of training iterations the TF1-Adam
    // update of iteration i is DEFERRED -- k_iter_fused of iteration i + 1 computes with the updated parameters (prologue), k_finalize
    // behind it stores them -- and the last one of the sequence is applied by k_adam (flush_adam): nothing is pending at an API boundary
    bool defer_ok = true;        // HPV_NO_DEFERRED_ADAM=1 turns it off (A/B, tests)
    bool defer_adam = false;     // a sequence is being enqueued / captured
    bool adam_pending = false;   // RB holds a reduced gradient whose update has not been applied
    hipGraphExec_t g_stepK = nullptr;    // HPV_GRAPH_ITERS iterations per replay (fewer inter-graph gaps)
    hipGraphExec_t g_rem[8] = {};        // g_rem[r]: r iterations (the remainder of a call), captured at first use
};

namespace hpvd {
extern std::string g_create_error;          // last hpv_create() error (hpv_last_error(NULL))
int fail(hpv_ctx* h, int code, const char* fmt, ...);
int upload(hpv_ctx* h, double* dst, const double* src, size_t n);
void drop_graph(hpv_ctx* h);                 // captured iteration graphs (hpv_api.hip)
int check_ready(hpv_ctx* h);                 // everything of the variational scheme is set; (re)assembles the device batches (hpv_api.hip)
int assemble_data_batch(hpv_ctx* h);
// the ansatz of a point set (hpv_set_ansatz)
inline bool has_ansatz(const hpv_ctx* h) { return h->ans_on[0] || h->ans_on[1] || h->ans_on[2] || h->ans_on[3]; }
void drop_moments(hpv_ctx* h);               // the constraint terms and their buffers go (the caller has made sure no enqueued launch reads them)
void drop_ansatz(hpv_ctx* h, int which);     // the planes of one set go (the caller has made sure no enqueued launch reads them)
int ansatz_ready(hpv_ctx* h, int which);     // -3, naming the set, where a handle with an ansatz has points of that set and no planes for them
void ansatz_fwd(hpv_ctx* h, int which, Batch& b, long n);      // k_ansatz_fwd on the first n points of b.OUT (no-op without planes)
void ansatz_adj(hpv_ctx* h, int which, Batch& b, long n);      // k_ansatz_adj on b.GBAR
// the pass engine (hpv_pass.hip)
void run_fwd(hpv_ctx* h, Batch& b, int save_act);       // forward launch over a batch
void enqueue_adam(hpv_ctx* h);
int launch_check(hpv_ctx* h, const char* what);
int enqueue_pass(hpv_ctx* h, bool backward, bool fuse_adam = false, bool pend = false);
int enqueue_pass_x(hpv_ctx* h, bool backward, bool fuse_adam);      // ... with the multi-GPU exchange behind it
int enqueue_iterations(hpv_ctx* h, int n_iters);
// the pass over the quadrature batch as the MFMA launch functions take it (hpv_time_iteration_kernel launches one stand-alone)
MfmaDataTerm pass_data_term(hpv_ctx* h, bool backward);
ProjArgs pass_proj_args(hpv_ctx* h, bool backward, bool edge = false);
MfmaPass pass_mfma(hpv_ctx* h, const MfmaDataTerm& dt, const ProjArgs& pa);
int lbfgs_drop(hpv_ctx* h);                  // the L-BFGS history goes: new parameters were handed in (hpv_lbfgs.hip)
void p2p_release(hpv_ctx* h);                // hpv_exchange.hip
void rccl_release(hpv_ctx* h);
int p2p_check(hpv_ctx* h);
// one ncclAllReduce(sum, double) of `n` doubles in place on stream `s` (test-hooks builds can make it fail on demand)
ncclResult_t rccl_allreduce(hpv_ctx* h, void* buf, size_t n, hipStream_t s);
const char* rccl_error_string(ncclResult_t r);
}  // namespace hpvd

#define HIPCHK(h, call)                                                                            \
    do {                                                                                           \
        hipError_t e_ = (call);                                                                    \
        if (e_ != hipSuccess) return hpvd::fail(h, -2, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

namespace hpvd {
// 16-point tiles of n boundary/data points riding inside the quadrature batch (hpv_ctx::merged): one loss partial per tile
inline int data_tiles(int n) { return (n + 15) / 16; }

template <typename T>
int dalloc(hpv_ctx* h, T** p, size_t n) {
    if (*p) { (void)hipFree(*p); *p = nullptr; }
    if (n == 0) return 0;
    HIPCHK(h, hipMalloc((void**)p, n * sizeof(T)));
    return 0;
}
}  // namespace hpvd
