// C-ABI of libhpvpinn.so (include/hpvpinn.h): host orchestration of one hp-VPINN training
// handle = one GPU's shard of elements + a replica of the network parameters.  (The multi-GPU exchanges live in hpv_exchange.hip,
// the timing / benchmark / debug hooks in hpv_bench.hip; hpv_ctx.h holds the handle and the helpers they share.)
#include "hpv_ctx.h"
#include "hpv_dual_norm.h"
#include "hpv_dual_dense.h"

using namespace hpvd;

namespace hpvd {
std::string g_create_error;

int fail(hpv_ctx* h, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (h) h->err = buf; else g_create_error = buf;
    return code;
}

int upload(hpv_ctx* h, double* dst, const double* src, size_t n) {
    if (n == 0) return 0;
    HIPCHK(h, hipMemcpyAsync(dst, src, n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}

// the integral constraints of hpv_set_moments and their buffers
void drop_moments(hpv_ctx* h) {
    h->n_mom = 0;
    for (double** p : {&h->d_mom, &h->d_mom_part, &h->d_mom_res, &h->d_mom_dcoef})
        if (*p) { (void)hipFree(*p); *p = nullptr; }
}

void drop_ansatz(hpv_ctx* h, int which) {
    if (h->ans_on[which]) h->batch_dirty = true;      // (whether the data points may ride in the quadrature batch is decided again)
    if (h->d_ans[which]) { (void)hipFree(h->d_ans[which]); h->d_ans[which] = nullptr; }
    h->ans_on[which] = false;
    h->ans_n[which] = 0;
}

void drop_graph(hpv_ctx* h) {
    if (h->g_stepK) { (void)hipGraphExecDestroy(h->g_stepK); h->g_stepK = nullptr; }
    for (hipGraphExec_t& g : h->g_rem) if (g) { (void)hipGraphExecDestroy(g); g = nullptr; }
}
}  // namespace hpvd

static int sync_check(hpv_ctx* h);

int hpv_test_hook_split_skip() {
#ifdef HPV_TEST_HOOKS   // libhpvpinn_testhooks.so only: the product library does not read the variable
    const char* dbg = getenv("HPV_DEBUG_SPLIT_SKIP");
    return dbg ? std::max(0, atoi(dbg)) : 0;
#else
    return 0;
#endif
}

namespace {

void free_batch(Batch& b) {
    if (b.m) hpv_mfma_destroy(b.m);
    if (b.X) (void)hipFree(b.X);
    if (b.ACT) (void)hipFree(b.ACT);
    if (b.OUT) (void)hipFree(b.OUT);
    if (b.GBAR) (void)hipFree(b.GBAR);
    if (b.GPART) (void)hipFree(b.GPART);
    b = Batch{};
}

// Build the network descriptor for a given tangent-channel selection.
NetDesc make_netdesc(const hpv_config& c, int nT1, const int* t1dim, int nT2, const int* t2idx) {
    NetDesc nd{};
    nd.d = c.layers[0];
    nd.nl = c.n_layers - 1;
    int off = 0;
    for (int l = 0; l < c.n_layers; ++l) nd.width[l] = c.layers[l];
    for (int l = 0; l < nd.nl; ++l) {
        nd.woff[l] = off; off += c.layers[l] * c.layers[l + 1];
        nd.boff[l] = off; off += c.layers[l + 1];
    }
    nd.P = off;
    nd.act = c.act;
    nd.nT1 = nT1; nd.nT2 = nT2;
    for (int i = 0; i < nT1; ++i) nd.t1dim[i] = t1dim[i];
    for (int i = 0; i < nT2; ++i) nd.t2idx[i] = t2idx[i];
    nd.t2w[0] = 1.0; nd.t2w[1] = 0.0;
    nd.C = 1 + nT1 + nT2;
    nd.nslot = 2 + nT1 + nT2;
    long a = 0;
    for (int l = 0; l < nd.nl - 1; ++l) { nd.actoff[l] = a; a += (long)nd.nslot * c.layers[l + 1]; }
    nd.actoff[nd.nl - 1] = a;  // total slots*width (per point)
    return nd;
}

int alloc_batch(hpv_ctx* h, Batch& b, const NetDesc& nd, long N, bool need_bwd) {
    free_batch(b);
    b.N = N; b.nd = nd;
    if (N == 0) return 0;
    int rc;
    if ((rc = dalloc(h, &b.X, (size_t)nd.d * N))) return rc;
    if ((rc = dalloc(h, &b.OUT, (size_t)nd.C * N))) return rc;
    if (need_bwd) {
        b.act_doubles = (size_t)nd.actoff[nd.nl - 1] * N;
        if ((rc = dalloc(h, &b.ACT, b.act_doubles))) return rc;
        if ((rc = dalloc(h, &b.GBAR, (size_t)nd.C * N))) return rc;
        HIPCHK(h, hipMemsetAsync(b.GBAR, 0, (size_t)nd.C * N * sizeof(double), h->stream));
        b.rows = mlp_bwd_generic_rows(N);
        if ((rc = dalloc(h, &b.GPART, (size_t)b.rows * nd.P))) return rc;
    }
    return 0;
}

// [n][d] row-major host values -> [d][N], zeros behind the n values of each row (N >= n)
std::vector<double> transposed(const double* X, long n, int d, long N) {
    std::vector<double> t((size_t)N * d, 0.0);
    for (long p = 0; p < n; ++p)
        for (int c = 0; c < d; ++c) t[(size_t)c * N + p] = X[(size_t)p * d + c];
    return t;
}
int upload_points(hpv_ctx* h, Batch& b, const double* X, long n, int d) {
    return upload(h, b.X, transposed(X, n, d, n).data(), (size_t)n * d);
}

// A forward-only batch of n points under channel set nd (prediction, evaluation and validation points), with the MFMA object where the
// shape has one; and the forward launch over it.
int points_batch(hpv_ctx* h, Batch& b, const NetDesc& nd, int n) {
    int rc = alloc_batch(h, b, nd, n, false);
    if (rc) return rc;
    if (n > 0 && h->cfg.backend != HPV_BACKEND_GENERIC) b.m = hpv_mfma_create(nd, n, nullptr, false);
    return 0;
}
int forward_only(hpv_ctx* h, Batch& b) {
    run_fwd(h, b, 0);
    HIPCHK(h, hipGetLastError());
    return 0;
}

}  // namespace

// The boundary/data points as a batch of their own: every structure but the merged batch of the MFMA path below.
int hpvd::assemble_data_batch(hpv_ctx* h) {
    int rc = alloc_batch(h, h->data, h->nd_val, h->n_data, true);
    if (!rc && h->n_data > 0) rc = upload_points(h, h->data, h->Xd_host.data(), h->n_data, h->dim);
    return rc;
}

namespace {

// Build the device point batches from the host copies.  MFMA path: ONE batch = quadrature points (padded
// to a 16-point tile) followed by the boundary/data points, so a single forward and a single reverse
// launch serve both loss terms (the data points just carry zero adjoints on the tangent channels).
// Generic path: separate batches.
int assemble_batches(hpv_ctx* h) {
    int rc;
    const long N = h->Nq;
    // a handle with an ansatz (hpv_set_ansatz) keeps its data points out of the quadrature batch: the merged forward launch takes their
    // loss on raw network values
    const bool merge = !has_ansatz(h);
    const int d = h->dim, nd = merge ? h->n_data : 0;
    bool var_done = false;
    free_batch(h->var);      // (with their objects: none outlives the batch it was sized for)
    free_batch(h->data);
    h->backend = HPV_BACKEND_GENERIC;
    h->merged = false;
    if (h->cfg.backend != HPV_BACKEND_GENERIC && N > 0) {
        const long Npad = (N + 15) / 16 * 16, Ntot = Npad + nd;
        std::string why;
        HpvMfma* m = hpv_mfma_create(h->nd_var, Ntot, &why);
        if (m) {
            h->backend = HPV_BACKEND_MFMA;
            h->merged = merge;
            var_done = true;
            h->data_off = Npad;
            hpv_mfma_set_err_flag(m, h->d_xerr);
            hpv_mfma_set_split_ok(m, h->shared_elem_ok);
            if ((rc = alloc_batch(h, h->var, h->nd_var, Ntot, true))) { hpv_mfma_destroy(m); return rc; }
            h->var.m = m;
            if (h->var.ACT) { (void)hipFree(h->var.ACT); h->var.ACT = nullptr; }   // the MFMA path has its own store
            const int rows = hpv_mfma_max_rows(m, h->n_elem, data_tiles(nd));
            if ((rc = dalloc(h, &h->var.GPART, (size_t)rows * h->P))) return rc;
            h->var.rows = hpv_mfma_grad_rows(m);
            std::vector<double> X((size_t)d * Ntot, 0.0);
            for (int c = 0; c < d; ++c) {
                for (long p = 0; p < N; ++p) X[(size_t)c * Ntot + p] = h->Xq_host[(size_t)c * N + p];
                for (int p = 0; p < nd; ++p) X[(size_t)c * Ntot + Npad + p] = h->Xd_host[(size_t)p * d + c];
            }
            if ((rc = upload(h, h->var.X, X.data(), X.size()))) return rc;
            HIPCHK(h, hipMemsetAsync(h->var.GBAR, 0, (size_t)h->nd_var.C * Ntot * sizeof(double), h->stream));
            HIPCHK(h, hipMemsetAsync(h->var.OUT, 0, (size_t)h->nd_var.C * Ntot * sizeof(double), h->stream));
            const size_t nparts = (size_t)std::max(64, data_tiles(nd));
            if ((rc = dalloc(h, &h->d_data_part, nparts))) return rc;
            HIPCHK(h, hipMemsetAsync(h->d_data_part, 0, nparts * sizeof(double), h->stream));
        } else if (h->cfg.backend == HPV_BACKEND_MFMA) {
            return fail(h, -4, "MFMA backend requested but not available for this shape: %s", why.c_str());
        } else {
            // no silent cliff: the generic kernels are one to two orders of magnitude slower than the MFMA path
            static std::atomic<int> warned{0};
            if (!warned.exchange(1))
                fprintf(stderr, "libhpvpinn: WARNING -- this network / channel set is not covered by the MFMA kernels (%s); running the "
                                "generic kernels, which are far slower (hpv_backend_in_use reports HPV_BACKEND_GENERIC)\n", why.c_str());
        }
    }
    if (!var_done) {
        if ((rc = alloc_batch(h, h->var, h->nd_var, N, true))) return rc;
        if (N > 0 && (rc = upload(h, h->var.X, h->Xq_host.data(), h->Xq_host.size()))) return rc;
    }
    if (!h->merged && (rc = assemble_data_batch(h))) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->batch_dirty = false;
    return 0;
}

}  // namespace

int hpvd::check_ready(hpv_ctx* h) {
    if (!h->have_quad) return fail(h, -3, "hpv_set_quadrature has not been called");
    if (!h->have_tables) return fail(h, -3, "hpv_set_tables has not been called");
    if (!h->have_elems) return fail(h, -3, "hpv_set_elements has not been called");
    if (h->linear && !h->have_lin) return fail(h, -3, "hpv_set_operator has not been called");
    if (h->nl_stale) return fail(h, -3, "hpv_set_nonlinear has not been called again");
    if (h->q_stale) return fail(h, -3, "hpv_set_quasilinear has not been called again");
    if (h->mom_stale) return fail(h, -3, "hpv_set_moments has not been called again: new elements dropped the measure planes of the integral constraints");
    if (h->dual_stale) return fail(h, -3, "hpv_set_residual_norm has not been called again: hpv_set_tables dropped the tables of the dual norm");
    if (h->gram_stale) return fail(h, -3, "hpv_set_residual_gram has not been called again: new tables, elements or counts dropped the Gram factors of the dual norm");
    if (h->n_coef && !h->have_dirs) return fail(h, -3, "hpv_set_trainable has not been called");
    if (!h->have_params) return fail(h, -3, "hpv_set_params has not been called");
    if (h->have_F && !h->d_F && h->n_elem > 0) return fail(h, -3, "internal: F not sliced");
    if (h->batch_dirty) return assemble_batches(h);
    return 0;
}

// The dense Gram factors (hpv_set_residual_gram) belong to the elements, their counts and the test-function tables: whoever changes
// one of those drops them, and a pass refuses until they are given again -- it must not silently train mean(R^2).
// the divergence form's matrices and 1 / det A (hpv_set_strong_form_div) belong to the rule and the elements: new ones orphan them
// (the caller has made sure no enqueued launch reads them: k_div_indicators runs only inside hpv_linear_indicators, which synchronises)
static void drop_strong_form_div(hpv_ctx* h) {
    if (!h->d_sfd) return;
    (void)hipFree(h->d_sfd); h->d_sfd = nullptr;
    if (h->d_inv_det) { (void)hipFree(h->d_inv_det); h->d_inv_det = nullptr; }
    h->sfd_stale = true;
}

static int drop_gram(hpv_ctx* h) {
    if (!h->d_gram) return 0;
    HIPCHK(h, hipStreamSynchronize(h->stream));      // (an enqueued pass may still read them)
    (void)hipFree(h->d_gram);
    h->d_gram = nullptr;
    h->gram_stale = true;
    return 0;
}

extern "C" {

const char* hpv_last_error(hpv_handle h) { return h ? h->err.c_str() : g_create_error.c_str(); }

// channel selection + integrand terms per (pde, var_form); returns what is wrong with the pair, or nullptr
static const char* form_terms(int pde, int vf, double V, ProjDesc& pd, int& nT1, int& nT2, bool& mixed) {
    pd = ProjDesc{};
    nT1 = nT2 = 0;
    mixed = false;
    auto term = [&](int dx, int dy, int eps_mult) -> TermDesc& {
        TermDesc& t = pd.t[pd.nterms++];
        t = TermDesc{}; t.dx = dx; t.dy = dy; t.eps_mult = eps_mult; return t;
    };
    if (pde == HPV_PDE_POISSON1D) {
        if (vf == 1) { nT1 = 1; nT2 = 1; term(0, 0, 0).a0[2] = 1.0; }            // P1:83-84  -J int u'' phi
        else if (vf == 2) { nT1 = 1; term(1, 0, 0).a0[1] = 1.0; }                // P1:86-87  int u' phi'
        else if (vf == 3) { term(2, 0, 0).a0[0] = 1.0; pd.edge = 1; }            // P1:89-91
        else return "Poisson-1D var_form must be 1, 2 or 3";
    } else if (pde == HPV_PDE_POISSON2D) {
        if (vf == 0) {                                                           // P2:91, 93-96: integrand u_xx + u_yy
            // ONE mixed second tangent (NetDesc::t2w = {1, 1}) instead of the two channels u_xx, u_yy: 4 channels through the
            // forward, the tangent recompute and the reverse pass instead of 5 (second-order channels propagate linearly)
            nT1 = 2; nT2 = 1; mixed = true; term(0, 0, 0).a0[3] = 1.0;
        }
        else if (vf == 1) { nT1 = 2; term(1, 0, 0).a0[1] = 1.0; term(0, 1, 0).a0[2] = 1.0; }            // P2:98-105
        else if (vf == 2) { term(2, 0, 0).a0[0] = 1.0; term(0, 2, 0).a0[0] = 1.0; }                     // P2:108-115
        else return "Poisson-2D var_form must be 0, 1 or 2";
    } else if (pde == HPV_PDE_ADVDIFF) {
        pd.has_eps = 1;
        if (vf == 0) {                                                           // P3:161-167
            nT1 = 2; nT2 = 1;  // channels u, u_x, u_t, u_xx
            TermDesc& t = term(0, 0, 0); t.a0[1] = V; t.a0[2] = 1.0; t.a1[3] = -1.0;
        } else if (vf == 1) {                                                    // P3:169-174
            nT1 = 2;
            TermDesc& t = term(0, 0, 0); t.a0[1] = V; t.a0[2] = 1.0;
            term(1, 0, 1).a0[1] = 1.0;
        } else return "AdvDiff var_form must be 0 or 1";
    } else if (pde == HPV_PDE_LINEAR1D || pde == HPV_PDE_LINEAR2D) {
        // channels u, u_x, (u_y); the three integrand terms carry per-point coefficients and live in k_project_lin (kernels_linop.hip),
        // not in this descriptor: nterms stays 0
        if (vf != 1) return "the linear problem takes var_form 1 (the once-integrated-by-parts form)";
        nT1 = pde == HPV_PDE_LINEAR1D ? 1 : 2;
    } else return "unknown pde";
    return nullptr;
}

int hpv_create(hpv_handle* out, const hpv_config* cfg) { return hpv_create_ex(out, cfg, 0); }

int hpv_create_ex(hpv_handle* out, const hpv_config* cfg, int n_coef) {
    if (!out || !cfg) return fail(nullptr, -1, "null argument");
    *out = nullptr;
    if (n_coef < 0 || n_coef > HPV_MAX_COEF) return fail(nullptr, -1, "n_coef = %d not in 0..%d", n_coef, HPV_MAX_COEF);
    if (n_coef && cfg->pde != HPV_PDE_LINEAR1D && cfg->pde != HPV_PDE_LINEAR2D)
        return fail(nullptr, -1, "trainable coefficients belong to the linear problems (HPV_PDE_LINEAR1D / _LINEAR2D)");
    if (cfg->n_layers < 2 || cfg->n_layers > HPV_MAX_LAYERS) return fail(nullptr, -1, "n_layers out of range");
    const int dim = (cfg->pde == HPV_PDE_POISSON1D || cfg->pde == HPV_PDE_LINEAR1D) ? 1 : 2;
    if (cfg->pde < 0 || cfg->pde > HPV_PDE_LINEAR2D) return fail(nullptr, -1, "unknown pde %d", cfg->pde);
    const bool linear = cfg->pde == HPV_PDE_LINEAR1D || cfg->pde == HPV_PDE_LINEAR2D;
    if (linear && cfg->scheme != HPV_SCHEME_VPINN)
        return fail(nullptr, -1, "the linear problem runs under the variational scheme only (the strong form needs derivatives of its coefficients)");
    if (cfg->layers[0] != dim) return fail(nullptr, -1, "layers[0]=%d but the problem is %d-D", cfg->layers[0], dim);
    if (cfg->layers[cfg->n_layers - 1] != 1) return fail(nullptr, -1, "the network must have one output");
    for (int l = 1; l < cfg->n_layers - 1; ++l)
        if (cfg->layers[l] < 1 || cfg->layers[l] > HPV_MAXH) return fail(nullptr, -1, "hidden width %d not in 1..%d", cfg->layers[l], HPV_MAXH);
    if (cfg->act != HPV_ACT_TANH && cfg->act != HPV_ACT_SIN) return fail(nullptr, -1, "unknown activation");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(nullptr, -2, "no HIP device available");
    if (cfg->device < 0 || cfg->device >= ndev) return fail(nullptr, -1, "device %d out of range (%d devices)", cfg->device, ndev);
    if (hipSetDevice(cfg->device) != hipSuccess) return fail(nullptr, -2, "hipSetDevice failed");

    hpv_ctx* h = new hpv_ctx();
    h->cfg = *cfg;
    h->dim = dim;
    h->linear = linear;
    if (hipStreamCreate(&h->stream) != hipSuccess) { delete h; return fail(nullptr, -2, "hipStreamCreate failed"); }
    h->own_stream = true;
    if (hipStreamCreateWithFlags(&h->stream2, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming) != hipSuccess) {
        delete h; return fail(nullptr, -2, "side stream / event creation failed");
    }
    { const char* ng = getenv("HPV_NO_GRAPH"); h->use_graph = !(ng && ng[0] == '1'); }
    { const char* nd = getenv("HPV_NO_DEFERRED_ADAM"); h->defer_ok = !(nd && nd[0] == '1'); }

    int t1[2] = {0, 1}, t2[2] = {0, 1};
    ProjDesc& pd = h->pd;
    int nT1 = 0, nT2 = 0;
    bool mixed = false;
    if (const char* bad = form_terms(cfg->pde, cfg->var_form, cfg->V, pd, nT1, nT2, mixed)) { delete h; return fail(nullptr, -1, "%s", bad); }
    h->has_eps = pd.has_eps;
    h->nd_var = make_netdesc(*cfg, nT1, t1, nT2, t2);
    h->nd_eval = h->nd_var;
    if (mixed) {
        h->nd_var.t2w[0] = 1.0; h->nd_var.t2w[1] = 1.0;
        h->nd_eval = make_netdesc(*cfg, 2, t1, 2, t2);      // what hpv_eval_channels reports: u, u_x, u_y, u_xx, u_yy
        h->eval_differs = true;
    }
    h->nd_val = make_netdesc(*cfg, 0, t1, 0, t2);
    h->nd_full = make_netdesc(*cfg, dim, t1, dim, t2);     // hpv_eval_points: u, u_x, (u_y | u_t), u_xx, (u_yy | u_tt)
    h->nd_grad = make_netdesc(*cfg, dim, t1, 0, t2);       // hpv_validate against exact gradients
    if (cfg->scheme == HPV_SCHEME_PINN) {
        // channels of the strong-form residual (k_pinn_residual): 1-D [u, u_x, u_xx] (P1:150-155); AdvDiff [u, u_x, u_t, u_xx]
        // (P3:247-253; t2w = {1, 0}); 2-D u_xx + u_yy as ONE mixed second tangent, NetDesc::t2w: four channels instead of five
        // through forward and reverse (P2:187-194)
        h->nd_pinn = make_netdesc(*cfg, dim, t1, 1, t2);
        if (cfg->pde == HPV_PDE_POISSON2D) { h->nd_pinn.t2w[0] = 1.0; h->nd_pinn.t2w[1] = 1.0; }
    } else if (cfg->scheme != HPV_SCHEME_VPINN) { delete h; return fail(nullptr, -1, "unknown scheme %d", cfg->scheme); }
    pd.C = h->nd_var.C;
    h->P = h->nd_var.P;
    h->n_coef = n_coef;
    h->Ptot = h->P + h->has_eps + n_coef;

    int rc = 0;
    rc |= dalloc(h, &h->d_theta, (size_t)h->Ptot);
    rc |= dalloc(h, &h->d_m, (size_t)h->Ptot);
    rc |= dalloc(h, &h->d_v, (size_t)h->Ptot);
    rc |= dalloc(h, &h->d_state, (size_t)adam_state_doubles(h->P));
    rc |= dalloc(h, &h->d_hist, (size_t)4 * HPV_HIST_CAP);
    rc |= dalloc(h, &h->d_hist_idx, (size_t)1);
    if (!rc) (void)hipMemset(h->d_hist_idx, 0, sizeof(int));
    rc |= dalloc(h, &h->d_xerr, (size_t)2);      // [0] the sticky flag; [1] "the deferred update was suppressed" (k_iter_fused prologue -> k_finalize)
    if (!rc) (void)hipMemset(h->d_xerr, 0, 2 * sizeof(int));
    rc |= dalloc(h, &h->d_nupd, (size_t)1);
    if (!rc) (void)hipMemset(h->d_nupd, 0, sizeof(unsigned long long));
    rc |= dalloc(h, &h->d_RB, (size_t)h->Ptot + 4);
    rc |= dalloc(h, &h->d_data_part, 64);
    if (rc) { g_create_error = h->err; hpv_destroy(h); return -2; }
    (void)hipMemset(h->d_RB, 0, ((size_t)h->Ptot + 4) * sizeof(double));
    (void)hipMemset(h->d_data_part, 0, 64 * sizeof(double));
    *out = h;
    return 0;
}

void hpv_destroy(hpv_handle h) {
    if (!h) return;
    (void)hipSetDevice(h->cfg.device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    drop_graph(h);
    if (h->stream2) { (void)hipStreamSynchronize(h->stream2); (void)hipStreamDestroy(h->stream2); }
    if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
    if (h->ev_join) (void)hipEventDestroy(h->ev_join);
    for (Batch* b : {&h->var, &h->data, &h->edge, &h->pred, &h->flux, &h->colloc, &h->evalp, &h->valb}) free_batch(*b);
    if (h->mfma_eval) hpv_mfma_destroy(h->mfma_eval);
    if (h->mfma_ind) hpv_mfma_destroy(h->mfma_ind);
    p2p_release(h);
    rccl_release(h);
    void* ptrs[] = {h->d_mom, h->d_mom_part, h->d_mom_res, h->d_mom_dcoef, h->d_dual, h->d_gram, h->d_dirs, h->d_dcoef_e, h->d_nl_zero, h->d_dir_mask, h->d_nl, h->d_qp, h->d_lin, h->d_jxy, h->d_flux_coef, h->d_flux_g, h->d_flux_part, h->d_eval_out, h->d_fcol, h->d_col_part, h->d_jac, h->d_wq, h->d_ind_out, h->d_sf, h->d_sfd, h->d_inv_det, h->d_ind_r,
                    h->d_ind_f, h->d_ind, h->d_res_f, h->d_res_r, h->d_val_u, h->d_val_du, h->d_val_buf, h->d_val_idx, h->d_upart,
                    h->d_wtx, h->d_wty, h->d_edge_dphi, h->d_coef, h->d_edge_coef, h->d_F, h->d_R, h->d_loss_e, h->d_deps_e, h->d_udata,
                    h->d_data_part, h->d_theta, h->d_m, h->d_v, h->d_state, h->d_RB, h->d_hist, h->d_hist_idx, h->d_xerr, h->d_nupd,
                    h->d_nact, h->d_nacty, h->d_lb, h->d_lb_ring};
    for (void* p : ptrs) if (p) (void)hipFree(p);
    for (double* p : h->d_ans) if (p) (void)hipFree(p);
    for (auto& t : h->timers) for (auto e : t.ev) (void)hipEventDestroy(e);
    if (h->own_stream && h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

int hpv_set_stream(hpv_handle h, void* s) {
    if (!h) return -1;
    if (h->own_stream && h->stream) { (void)hipStreamSynchronize(h->stream); (void)hipStreamDestroy(h->stream); }
    drop_graph(h);
    h->stream = (hipStream_t)s;
    h->own_stream = false;
    return 0;
}

int hpv_set_quadrature(hpv_handle h, const double* xi, const double* wx, int qx, const double* yi, const double* wy, int qy) {
    if (!h) return -1;
    if (!xi || !wx || qx < 1) return fail(h, -1, "bad x quadrature");
    if (h->dim == 1) { if (qy != 1) return fail(h, -1, "qy must be 1 for the 1-D problem"); }
    else if (!yi || !wy || qy < 1) return fail(h, -1, "bad y quadrature");
    h->xi.assign(xi, xi + qx); h->wx.assign(wx, wx + qx);
    if (h->dim == 2) { h->yi.assign(yi, yi + qy); h->wy.assign(wy, wy + qy); }
    else { h->yi.assign(1, 0.0); h->wy.assign(1, 1.0); }
    h->qx = qx; h->qy = qy;
    h->pd.qx = qx; h->pd.qy = qy;
    {   // the raw weights [qx | qy] for hpv_element_indicators (the tables on the device are w * phi)
        int rc;
        if ((rc = dalloc(h, &h->d_wq, (size_t)qx + qy))) return rc;
        if ((rc = upload(h, h->d_wq, h->wx.data(), (size_t)qx))) return rc;
        if ((rc = upload(h, h->d_wq + qx, h->wy.data(), (size_t)qy))) return rc;
    }
    if (h->d_sf) { (void)hipFree(h->d_sf); h->d_sf = nullptr; }      // (hpv_set_strong_form: the matrices belong to the old rule)
    drop_strong_form_div(h);                                         // (hpv_set_strong_form_div: as do these, and -3 says so)
    h->have_quad = true;
    drop_graph(h);
    h->have_tables = false;  // weighted tables depend on the weights
    h->have_elems = false;
    return 0;
}

int hpv_set_tables(hpv_handle h, const double* phix, const double* dphix, const double* d2phix, int ntx,
                   const double* phiy, const double* dphiy, const double* d2phiy, int nty, const double* edge_dphi) {
    if (!h) return -1;
    if (!h->have_quad) return fail(h, -3, "call hpv_set_quadrature first");
    if (!phix || !dphix || !d2phix || ntx < 1) return fail(h, -1, "bad x tables");
    if (h->dim == 1) { if (nty != 1) return fail(h, -1, "nty must be 1 for the 1-D problem"); }
    else if (!phiy || !dphiy || !d2phiy || nty < 1) return fail(h, -1, "bad y tables");
    for (size_t i = 0; i < h->nact_all.size(); ++i)     // counts given for an earlier, larger table set
        if (h->nact_all[i] > ntx)
            return fail(h, -1, "n_active[%zu] = %d exceeds the new ntest %d (hpv_set_active_tests(NULL) drops the counts)", i, h->nact_all[i], ntx);
    for (size_t i = 0; i < h->nacty_all.size(); ++i)    // ... and the second direction's (hpv_set_active_tests_2d)
        if (h->nacty_all[i] > nty)
            return fail(h, -1, "nay[%zu] = %d exceeds the new nty %d (hpv_set_active_tests_2d(NULL, NULL) drops the counts)", i, h->nacty_all[i], nty);
    const int qx = h->qx, qy = h->qy;
    {   // refused BEFORE anything of the old tables is replaced: a handle that had tables keeps them, with its ntx / nty
        ProjDesc pd = h->pd;
        pd.ntx = ntx; pd.nty = nty;
        const size_t lds = h->linear ? hpv_linop_lds_bytes(qx, qy, ntx, nty) : hpv_proj_lds_bytes(pd);
        if (lds > 64 * 1024) return fail(h, -1, "element too large for the projection kernel's LDS (%zu B)", lds);
    }
    std::vector<double> wtx((size_t)3 * ntx * qx), wty((size_t)3 * nty * qy);
    const double* tx[3] = {phix, dphix, d2phix};
    const double* ty[3] = {phiy, dphiy, d2phiy};
    for (int d = 0; d < 3; ++d)
        for (int r = 0; r < ntx; ++r)
            for (int i = 0; i < qx; ++i) wtx[((size_t)d * ntx + r) * qx + i] = h->wx[i] * tx[d][(size_t)r * qx + i];
    for (int d = 0; d < 3; ++d)
        for (int k = 0; k < nty; ++k)
            for (int j = 0; j < qy; ++j)
                wty[((size_t)d * nty + k) * qy + j] = (h->dim == 1) ? 1.0 : h->wy[j] * ty[d][(size_t)k * qy + j];
    int rc;
    if ((rc = dalloc(h, &h->d_wtx, wtx.size()))) return rc;
    if ((rc = dalloc(h, &h->d_wty, wty.size()))) return rc;
    if ((rc = upload(h, h->d_wtx, wtx.data(), wtx.size()))) return rc;
    if ((rc = upload(h, h->d_wty, wty.data(), wty.size()))) return rc;
    if (h->pd.edge) {
        if (!edge_dphi) return fail(h, -1, "var_form 3 needs edge_dphi");
        if ((rc = dalloc(h, &h->d_edge_dphi, (size_t)2 * ntx))) return rc;
        if ((rc = upload(h, h->d_edge_dphi, edge_dphi, (size_t)2 * ntx))) return rc;
    }
    h->ntx = ntx; h->nty = nty;
    h->pd.ntx = ntx; h->pd.nty = nty;
    h->have_tables = true;
    drop_graph(h);
    if (h->d_dual) {      // (hpv_set_residual_norm: its tables belong to the old test functions; a pass must not silently train mean(R^2))
        HIPCHK(h, hipStreamSynchronize(h->stream));
        (void)hipFree(h->d_dual);
        h->d_dual = nullptr;
        h->dual_stale = true;
    }
    return drop_gram(h);
}

// The elements of the whole mesh as boxes [ne_tot][2 * dim] = (x0, x1[, y0, y1]) and the owned slice [e_begin, e_end): the affine map of
// the reference nodes, |J_e| and the per-term coefficients of every pde / var_form.  Both hpv_set_elements (the boxes of a tensor grid,
// e = ex * ney + ey) and hpv_set_element_boxes (any list) end here; nothing below this function knows a grid.
// points != nullptr (hpv_set_element_points; `boxes` is then nullptr): unit elements, J = Jx = Jy = 1, whose quadrature points are
// the caller's [ne_tot][2][qy * qx] -- the same slicing, the same buffers, the same invalidation.
static int set_elements_from_boxes(hpv_ctx* h, const double* boxes, int ne_tot, int nex, int ney, int e_begin, int e_end,
                                   const double* points = nullptr) {
    if (e_begin < 0 || e_end > ne_tot || e_begin > e_end) return fail(h, -1, "bad element range [%d,%d) of %d", e_begin, e_end, ne_tot);
    // per-grid inputs given earlier must fit the new grid: checked BEFORE anything of the old grid is replaced
    if (!h->nact_all.empty() && (int)h->nact_all.size() != ne_tot)
        return fail(h, -1, "n_active has %zu entries but the new grid has %d elements (hpv_set_active_tests(NULL) drops them)", h->nact_all.size(), ne_tot);
    if (h->have_F && h->F_all.size() != (size_t)ne_tot * h->ntx * h->nty)
        return fail(h, -1, "F has %zu entries but the new grid needs %zu (hpv_set_rhs(NULL) drops it)", h->F_all.size(), (size_t)ne_tot * h->ntx * h->nty);
    const int bs = 2 * h->dim;
    h->ne_tot = ne_tot;
    h->nex = nex; h->ney = ney; h->e_begin = e_begin; h->e_end = e_end;
    const long ne = e_end - e_begin;
    h->n_elem = ne;
    const int qx = h->qx, qy = h->qy, NQ = qx * qy;
    const long N = ne * NQ;
    int rc;
    h->Nq = N;
    const int nterms = h->pd.nterms;
    std::vector<double> X((size_t)h->dim * N), coef((size_t)nterms * ne), ecoef((size_t)ne), EX((size_t)2 * ne), jac((size_t)ne);
    std::vector<double> jxy(h->linear ? (size_t)2 * ne : 0, 1.0);
    if (h->linear) {      // the coefficient planes belong to the old elements' points
        HIPCHK(h, hipStreamSynchronize(h->stream));
        if (int rcg = drop_gram(h)) return rcg;  // ... as do the Gram factors of hpv_set_residual_gram
        drop_ansatz(h, HPV_ANSATZ_QUAD);         // ... as do the ansatz planes
        drop_strong_form_div(h);                 // ... and 1 / det A of the divergence form
        h->have_lin = false;
        h->unit_elems = points != nullptr;
        if (h->d_lin) { (void)hipFree(h->d_lin); h->d_lin = nullptr; }
        if (h->nl_mask) h->nl_stale = true;      // a pass must not silently train the linear problem
        h->nl_mask = 0;
        if (h->d_nl) { (void)hipFree(h->d_nl); h->d_nl = nullptr; }
        if (h->q_mask) h->q_stale = true;        // ... nor the constant-diffusion one (hpv_set_quasilinear)
        h->q_mask = 0;
        if (h->d_qp) { (void)hipFree(h->d_qp); h->d_qp = nullptr; }
        if (h->n_mom) h->mom_stale = true;       // ... nor without its integral constraints (hpv_set_moments)
        drop_moments(h);
        h->have_dirs = false;                    // ... nor fixed coefficients
        h->dir_nl_mask = 0;
        for (double** p : {&h->d_dirs, &h->d_dcoef_e, &h->d_nl_zero})
            if (*p) { (void)hipFree(*p); *p = nullptr; }
    }
    for (long le = 0; le < ne && points; ++le) {      // (a 2-D linear handle: the caller has made sure)
        const double* px = points + (size_t)(e_begin + le) * 2 * NQ;
        std::copy_n(px, NQ, X.begin() + le * NQ);
        std::copy_n(px + NQ, NQ, X.begin() + N + le * NQ);
        jac[le] = 1.0;                                    // (jxy is all ones already)
    }
    for (long le = 0; le < ne && !points; ++le) {
        const double* box = boxes + (size_t)(e_begin + le) * bs;
        const double gx0 = box[0], gx1 = box[1];
        double gy0 = 0, gy1 = 0;
        if (h->dim == 2) { gy0 = box[2]; gy1 = box[3]; }
        // affine map of the reference nodes, same expression as P1:69 / P2:75-76 / P3:120-121
        for (int j = 0; j < qy; ++j)
            for (int i = 0; i < qx; ++i) {
                const long p = le * NQ + (long)j * qx + i;
                X[p] = gx0 + (gx1 - gx0) / 2 * (h->xi[i] + 1);
                if (h->dim == 2) X[(size_t)N + p] = gy0 + (gy1 - gy0) / 2 * (h->yi[j] + 1);
            }
        const double Jx = (gx1 - gx0) / 2;
        jac[le] = (h->dim == 1) ? Jx : ((gx1 - gx0) / 2) * ((gy1 - gy0) / 2);   // P1:276 / P2:393
        if (h->linear) {                                             // k_project_lin forms its coefficients from J, Jx, Jy itself
            jxy[le] = Jx;
            if (h->dim == 2) jxy[ne + le] = (gy1 - gy0) / 2;
        } else if (h->cfg.pde == HPV_PDE_POISSON1D) {
            const double J = Jx;                                     // P1:71
            if (h->cfg.var_form == 1) coef[le] = -J;
            else if (h->cfg.var_form == 2) coef[le] = 1.0;
            else { coef[le] = -1 / J; ecoef[le] = 1 / J; EX[2 * le] = gx0; EX[2 * le + 1] = gx1; }
        } else if (h->cfg.pde == HPV_PDE_POISSON2D) {
            const double Jy = (gy1 - gy0) / 2;
            const double J = Jx * Jy;                                // P2:77-79
            if (h->cfg.var_form == 0) coef[le] = J;
            else if (h->cfg.var_form == 1) { coef[le] = -(J / Jx); coef[ne + le] = -(J / Jy); }
            else { coef[le] = J; coef[ne + le] = J; }
        } else {
            const double J = (gy1 - gy0) / 2 * (gx1 - gx0) / 2;      // P3:115
            if (h->cfg.var_form == 0) coef[le] = J;
            else { coef[le] = J; coef[ne + le] = J / Jx; }
        }
    }
    if ((rc = dalloc(h, &h->d_coef, coef.size()))) return rc;
    if ((rc = dalloc(h, &h->d_jac, jac.size()))) return rc;
    if (ne > 0 && (rc = upload(h, h->d_jac, jac.data(), jac.size()))) return rc;
    if (h->linear) {
        if ((rc = dalloc(h, &h->d_jxy, jxy.size()))) return rc;
        if (ne > 0 && (rc = upload(h, h->d_jxy, jxy.data(), jxy.size()))) return rc;
    }
    if ((rc = dalloc(h, &h->d_R, (size_t)ne * h->ntx * h->nty))) return rc;
    // (per-element counts switch the row-split projection off -- set_proj_split below -- but its buffers are sized without them)
    h->proj_split = project_row_split(h->pd, ne, h->cfg.backend == HPV_BACKEND_GENERIC);
    // (the tall-element kernel shares an element among up to 64 workgroups, each with its own loss / d-epsilon / partial-sum slot)
    const bool tall = h->pd.qx == 80 && h->pd.qy == 80 && h->pd.ntx == 5 && h->pd.nty == 5 && h->cfg.backend != HPV_BACKEND_GENERIC && ne <= 128;
    const size_t nred = (size_t)ne * std::max(h->proj_split, tall ? 64 : 1);
    h->n_red_alloc = (long)nred;
    // (HPV_MAX_MOMENTS spare entries: the penalties of hpv_set_moments follow the element losses; deps_e's are zeroed with the rest)
    if ((rc = dalloc(h, &h->d_loss_e, nred + HPV_MAX_MOMENTS))) return rc;
    if ((rc = dalloc(h, &h->d_deps_e, nred + HPV_MAX_MOMENTS))) return rc;
    if ((rc = dalloc(h, &h->d_upart, h->proj_split > 1 ? (size_t)ne * h->proj_split * h->ntx * h->nty : 0))) return rc;
    h->Xq_host = X;
    h->batch_dirty = true;
    if (N > 0) {
        if ((rc = upload(h, h->d_coef, coef.data(), coef.size()))) return rc;
        const size_t nzero = nred + HPV_MAX_MOMENTS;      // (a name of its own: HIPCHK's message quotes the call)
        HIPCHK(h, hipMemsetAsync(h->d_deps_e, 0, nzero * sizeof(double), h->stream));
    }
    if (h->pd.edge) {
        if ((rc = alloc_batch(h, h->edge, h->nd_val, 2 * ne, true))) return rc;
        if ((rc = dalloc(h, &h->d_edge_coef, (size_t)ne))) return rc;
        if (ne > 0) {
            if ((rc = upload(h, h->edge.X, EX.data(), EX.size()))) return rc;
            if ((rc = upload(h, h->d_edge_coef, ecoef.data(), ecoef.size()))) return rc;
        }
    }
    h->have_elems = true;
    drop_graph(h);
    // (re)slice F if it was given before the elements
    if (h->have_F) {
        std::vector<double> F = h->F_all;
        if ((rc = hpv_set_rhs(h, F.data(), F.size()))) return rc;
    } else if (h->d_F) { (void)hipFree(h->d_F); h->d_F = nullptr; }
    if (!h->nact_all.empty()) {   // ... and the active test counts
        std::vector<int> na = h->nact_all, nay = h->nacty_all;
        if (!nay.empty()) { if ((rc = hpv_set_active_tests_2d(h, na.data(), nay.data(), (int)na.size()))) return rc; }
        else if ((rc = hpv_set_active_tests(h, na.data(), (int)na.size()))) return rc;
    }
    return 0;
}

int hpv_set_elements(hpv_handle h, const double* gridx, int nex, const double* gridy, int ney, int e_begin, int e_end) {
    if (!h) return -1;
    if (!h->have_quad || !h->have_tables) return fail(h, -3, "call hpv_set_quadrature and hpv_set_tables first");
    if (!gridx || nex < 1) return fail(h, -1, "bad x grid");
    if (h->dim == 1) { if (ney != 1) return fail(h, -1, "ney must be 1 for the 1-D problem"); }
    else if (!gridy || ney < 1) return fail(h, -1, "bad y grid");
    const int ne_tot = nex * ney, bs = 2 * h->dim;
    std::vector<double> boxes((size_t)ne_tot * bs);
    for (int e = 0; e < ne_tot; ++e) {
        const int ex = e / ney, ey = e % ney;
        boxes[(size_t)e * bs] = gridx[ex]; boxes[(size_t)e * bs + 1] = gridx[ex + 1];
        if (h->dim == 2) { boxes[(size_t)e * bs + 2] = gridy[ey]; boxes[(size_t)e * bs + 3] = gridy[ey + 1]; }
    }
    return set_elements_from_boxes(h, boxes.data(), ne_tot, nex, ney, e_begin, e_end);
}

int hpv_set_element_boxes(hpv_handle h, const double* boxes, int n_total, int e_begin, int e_end) {
    if (!h) return -1;
    if (!h->have_quad || !h->have_tables) return fail(h, -3, "call hpv_set_quadrature and hpv_set_tables first");
    if (!boxes || n_total < 1) return fail(h, -1, "bad element boxes");
    const int bs = 2 * h->dim;
    for (int e = 0; e < n_total; ++e)
        for (int c = 0; c < h->dim; ++c) {
            const double a = boxes[(size_t)e * bs + 2 * c], b = boxes[(size_t)e * bs + 2 * c + 1];
            if (!std::isfinite(a) || !std::isfinite(b) || !(a < b))
                return fail(h, -1, "element box %d: [%g, %g] in direction %d is not a finite interval with lower < upper", e, a, b, c);
        }
    return set_elements_from_boxes(h, boxes, n_total, n_total, 1, e_begin, e_end);
}

// Unit elements at the caller's quadrature points (include/hpvpinn.h): mapped elements whose geometry the host has folded into the planes.
int hpv_set_element_points(hpv_handle h, const double* X, int n_total, int e_begin, int e_end) {
    if (!h) return -1;
    if (!h->linear || h->dim != 2) return fail(h, -1, "hpv_set_element_points belongs to the 2-D problems of the linear class");
    if (!h->have_quad || !h->have_tables) return fail(h, -3, "call hpv_set_quadrature and hpv_set_tables first");
    if (!X || n_total < 1) return fail(h, -1, "bad element points");
    if (h->d_dual || h->dual_stale)
        return fail(h, -1, "the dual norm is set (hpv_set_residual_norm): the Gram matrix of the reference square is not the physical H^1 inner product of a mapped element");
    if (h->d_sf) return fail(h, -1, "the strong form is active (hpv_set_strong_form): it is not available on mapped elements");
    const size_t n = (size_t)n_total * 2 * h->qx * h->qy;
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(X[i])) return fail(h, -1, "element %zu holds a non-finite quadrature point (entry %zu)", i / ((size_t)2 * h->qx * h->qy), i);
    return set_elements_from_boxes(h, nullptr, n_total, n_total, 1, e_begin, e_end, X);
}

// the device copies of the per-element counts go; the row-split projection (which ignores counts) is on again where it applies
static void drop_device_counts(hpv_ctx* h) {
    h->nacty_all.clear();
    if (h->d_nact) { (void)hipFree(h->d_nact); h->d_nact = nullptr; }
    if (h->d_nacty) { (void)hipFree(h->d_nacty); h->d_nacty = nullptr; }
    h->pd.nact = nullptr;
    h->pd.nacty = nullptr;
    if (h->have_elems) h->proj_split = project_row_split(h->pd, h->n_elem, h->cfg.backend == HPV_BACKEND_GENERIC);
}

// p-refinement of the 1-D driver: element e uses only its first n_active[e] test functions (P1:66-67: Ntest_element =
// len(F_ext_total[e]); P1:268-281 builds F_ext_total from a per-element list N_testfcn_total).  n = elements of the whole grid.
int hpv_set_active_tests(hpv_handle h, const int* n_active, int n) {
    if (!h) return -1;
    drop_graph(h);
    if (int rcg = drop_gram(h)) return rcg;      // (hpv_set_residual_gram: the factors are those of the old counts)
    if (!n_active) {
        h->nact_all.clear();
        drop_device_counts(h);
        return 0;
    }
    if (h->dim != 1) return fail(h, -1, "per-element test-function counts of a 2-D problem go through hpv_set_active_tests_2d (one pair per element)");
    if (!h->have_tables) return fail(h, -3, "call hpv_set_tables first");
    for (int i = 0; i < n; ++i)
        if (n_active[i] < 1 || n_active[i] > h->ntx) return fail(h, -1, "n_active[%d] = %d is outside 1..%d", i, n_active[i], h->ntx);
    if (h->have_elems) {
        if (n != h->ne_tot) return fail(h, -1, "n_active has %d entries, expected %d", n, h->ne_tot);
        if (h->d_nact) { (void)hipFree(h->d_nact); h->d_nact = nullptr; }
        h->pd.nact = nullptr;
        if (h->n_elem > 0) {
            HIPCHK(h, hipMalloc((void**)&h->d_nact, (size_t)h->n_elem * sizeof(int)));
            HIPCHK(h, hipMemcpyAsync(h->d_nact, n_active + h->e_begin, (size_t)h->n_elem * sizeof(int), hipMemcpyHostToDevice, h->stream));
            HIPCHK(h, hipStreamSynchronize(h->stream));
            h->pd.nact = h->d_nact;
        }
    }
    if (n_active != h->nact_all.data()) h->nact_all.assign(n_active, n_active + n);
    return 0;
}

// p-refinement of the 2-D drivers: element e = ex * ney + ey projects onto its first nax[e] x nay[e] test functions (P2:72-73,
// P3:112-113: Ntest_elementx = N_testfcn[0][ex], Ntest_elementy = N_testfcn[1][ey]; one PAIR per element here, a superset of that
// product).  n = elements of the whole grid; the owned range is sliced here and again after hpv_set_elements.
int hpv_set_active_tests_2d(hpv_handle h, const int* nax, const int* nay, int n) {
    if (!h) return -1;
    drop_graph(h);
    if (int rcg = drop_gram(h)) return rcg;      // (hpv_set_residual_gram: the factors are those of the old counts)
    if (!nax && !nay) {
        h->nact_all.clear();
        drop_device_counts(h);
        return 0;
    }
    if (!nax || !nay) return fail(h, -1, "nax and nay are given together (or both NULL)");
    if (h->dim != 2) return fail(h, -1, "hpv_set_active_tests_2d is for the 2-D problems (1-D: hpv_set_active_tests)");
    if (h->cfg.scheme != HPV_SCHEME_VPINN) return fail(h, -1, "test-function counts belong to the variational scheme");
    if (!h->have_tables) return fail(h, -3, "call hpv_set_tables first");
    if (n < 1) return fail(h, -1, "bad number of counts %d", n);
    for (int i = 0; i < n; ++i) {
        if (nax[i] < 1 || nax[i] > h->ntx) return fail(h, -1, "nax[%d] = %d is outside 1..%d", i, nax[i], h->ntx);
        if (nay[i] < 1 || nay[i] > h->nty) return fail(h, -1, "nay[%d] = %d is outside 1..%d", i, nay[i], h->nty);
    }
    if (h->have_elems) {
        if (n != h->ne_tot) return fail(h, -1, "nax / nay have %d entries, expected %d", n, h->ne_tot);
        if (h->d_nact) { (void)hipFree(h->d_nact); h->d_nact = nullptr; }
        if (h->d_nacty) { (void)hipFree(h->d_nacty); h->d_nacty = nullptr; }
        h->pd.nact = nullptr;
        h->pd.nacty = nullptr;
        if (h->n_elem > 0) {
            const size_t bytes = (size_t)h->n_elem * sizeof(int);
            HIPCHK(h, hipMalloc((void**)&h->d_nact, bytes));
            HIPCHK(h, hipMalloc((void**)&h->d_nacty, bytes));
            HIPCHK(h, hipMemcpyAsync(h->d_nact, nax + h->e_begin, bytes, hipMemcpyHostToDevice, h->stream));
            HIPCHK(h, hipMemcpyAsync(h->d_nacty, nay + h->e_begin, bytes, hipMemcpyHostToDevice, h->stream));
            HIPCHK(h, hipStreamSynchronize(h->stream));
            h->pd.nact = h->d_nact;
            h->pd.nacty = h->d_nacty;
            h->proj_split = 1;      // (the row-split projection of tall elements knows no counts: one workgroup per element)
        }
    }
    if (nax != h->nact_all.data()) h->nact_all.assign(nax, nax + n);
    if (nay != h->nacty_all.data()) h->nacty_all.assign(nay, nay + n);
    return 0;
}

int hpv_set_rhs(hpv_handle h, const double* F, size_t n) {
    if (!h) return -1;
    drop_graph(h);
    if (!F) { h->have_F = false; h->F_all.clear(); if (h->d_F) { (void)hipFree(h->d_F); h->d_F = nullptr; } return 0; }
    if (h->have_elems) {
        const size_t NR = (size_t)h->ntx * h->nty;
        if (n != (size_t)h->ne_tot * NR) return fail(h, -1, "F has %zu entries, expected %zu", n, (size_t)h->ne_tot * NR);
        int rc;
        if ((rc = dalloc(h, &h->d_F, (size_t)h->n_elem * NR))) return rc;
        if (h->n_elem > 0 && (rc = upload(h, h->d_F, F + (size_t)h->e_begin * NR, (size_t)h->n_elem * NR))) return rc;
    }
    if (F != h->F_all.data()) h->F_all.assign(F, F + n);
    h->have_F = true;
    return 0;
}

int hpv_set_data(hpv_handle h, const double* X, const double* u, int n) {
    if (!h) return -1;
    if (n < 0 || (n > 0 && (!X || !u))) return fail(h, -1, "bad data arguments");
    int rc;
    if (h->ans_on[HPV_ANSATZ_DATA]) {           // the ansatz planes belong to the old points
        HIPCHK(h, hipStreamSynchronize(h->stream));
        drop_ansatz(h, HPV_ANSATZ_DATA);
    }
    h->n_data = n;
    drop_graph(h);
    h->Xd_host.assign(X, X + (size_t)n * h->dim);
    h->batch_dirty = true;
    if ((rc = dalloc(h, &h->d_udata, (size_t)n))) return rc;
    if (n > 0 && (rc = upload(h, h->d_udata, u, (size_t)n))) return rc;
    return 0;
}

// The coefficient planes of a linear problem at the owned quadrature points (include/hpvpinn.h); k_project_lin reads them in place.
// (both operator calls end here; a change of kind orphans the directions, whose plane count differs)
static int set_operator_planes(hpv_ctx* h, const double* coef, size_t n, bool tensor) {
    if (!h->have_elems) return fail(h, -3, "call hpv_set_elements first");
    const size_t K = tensor ? 7 : h->dim == 1 ? 3 : 5;
    if (!coef || n != K * (size_t)h->Nq) return fail(h, -1, "the operator has %zu entries, expected %zu planes of %ld", n, K, h->Nq);
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(coef[i])) return fail(h, -1, "coefficient plane %zu holds a non-finite value at point %zu", i / (size_t)std::max(h->Nq, 1L), i % (size_t)std::max(h->Nq, 1L));
    int rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));      // (an enqueued pass may still read the old planes)
    drop_graph(h);
    h->have_lin = false;
    if (tensor != h->lin_tensor) {
        h->have_dirs = false;
        h->dir_nl_mask = 0;
        for (double** p : {&h->d_dirs, &h->d_dcoef_e, &h->d_nl_zero})
            if (*p) { (void)hipFree(*p); *p = nullptr; }
    }
    h->lin_tensor = tensor;
    if ((rc = dalloc(h, &h->d_lin, n))) return rc;
    if ((rc = upload(h, h->d_lin, coef, n))) return rc;
    h->have_lin = true;
    return 0;
}

int hpv_set_operator(hpv_handle h, const double* coef, size_t n) {
    if (!h) return -1;
    if (!h->linear) return fail(h, -1, "hpv_set_operator belongs to the linear problems");
    return set_operator_planes(h, coef, n, false);
}

// The full diffusion tensor of a 2-D linear problem (include/hpvpinn.h); the TENSOR instantiations of the projection kernels read it in place.
int hpv_set_operator_tensor(hpv_handle h, const double* coef, size_t n) {
    if (!h) return -1;
    if (!h->linear || h->dim != 2) return fail(h, -1, "hpv_set_operator_tensor belongs to the 2-D problems of the linear class");
    return set_operator_planes(h, coef, n, true);
}

// The planes of the nonlinear term (include/hpvpinn.h); k_project_nl reads them in place.  The mask is decided here, once.
int hpv_set_nonlinear(hpv_handle h, const double* coef, size_t n) {
    if (!h) return -1;
    if (!h->linear) return fail(h, -1, "hpv_set_nonlinear belongs to the linear problems");
    if (!h->have_elems) return fail(h, -3, "call hpv_set_elements first");
    const size_t M = h->dim == 1 ? 4 : 5, Nq = (size_t)h->Nq;
    if ((!coef && n != 0) || (coef && n != M * Nq)) return fail(h, -1, "the nonlinear term has %zu entries, expected %zu planes of %ld", n, M, h->Nq);
    if (!coef) n = 0;
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(coef[i])) return fail(h, -1, "nonlinear plane %zu holds a non-finite value at point %zu", i / std::max(Nq, (size_t)1), i % std::max(Nq, (size_t)1));
    int mask = 0;
    for (size_t i = 0; i < n; ++i)
        if (coef[i] != 0.0) mask |= 1 << std::min(i / Nq, (size_t)3);      // (gx and gy are one term)
    if (mask && hpv_nonlin_lds_bytes(h->qx, h->qy, h->ntx, h->nty) > 64 * 1024)
        return fail(h, -1, "element too large for the nonlinear projection kernel's LDS (%zu B)", hpv_nonlin_lds_bytes(h->qx, h->qy, h->ntx, h->nty));
    int rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));      // (an enqueued pass may still read the old planes)
    drop_graph(h);
    h->nl_mask = 0;
    h->nl_stale = false;
    if (!mask) {                                     // no term: the handle runs k_project_lin again
        if (h->d_nl) { (void)hipFree(h->d_nl); h->d_nl = nullptr; }
        return 0;
    }
    if ((rc = dalloc(h, &h->d_nl, n))) return rc;
    if ((rc = upload(h, h->d_nl, coef, n))) return rc;
    h->nl_mask = mask;
    return 0;
}

// The multiplier mu = P(u) B(|grad u|^2) on the diffusive flux (include/hpvpinn.h); the _q instantiations of k_project_nl read the planes
// in place.  The two mask bits are decided here, once; with both clear nothing is kept and the handle launches what it did before.
int hpv_set_quasilinear(hpv_handle h, const double* planes, size_t n, double exponent) {
    if (!h) return -1;
    if (!h->linear) return fail(h, -3, "hpv_set_quasilinear belongs to the linear problems (HPV_PDE_LINEAR1D / _LINEAR2D)");
    if (h->n_coef) return fail(h, -3, "hpv_set_quasilinear on a handle with trainable coefficients: k_project_id does not carry the multiplier");
    if (!h->have_elems) return fail(h, -3, "call hpv_set_elements first");
    const size_t Nq = (size_t)h->Nq;
    if ((!planes && n != 0) || (planes && n != 4 * Nq))
        return fail(h, -1, "the quasilinear term has %zu entries, expected 4 planes (m0, m1, m2, delta) of %ld (NULL and 0 remove it)", n, h->Nq);
    if (!planes) n = 0;
    static const char* const names[] = {"m0", "m1", "m2", "delta"};
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(planes[i])) return fail(h, -1, "quasilinear plane %s holds a non-finite value at point %zu", names[i / std::max(Nq, (size_t)1)], i % std::max(Nq, (size_t)1));
    if (!std::isfinite(exponent)) return fail(h, -1, "the exponent of the quasilinear term is not finite");
    int mask = 0;
    if (n && exponent != 0.0) {
        mask |= HPV_NL_DIFF_GRAD;
        for (size_t i = 0; i < Nq; ++i)
            if (!(planes[3 * Nq + i] > 0.0))
                return fail(h, -1, "quasilinear plane delta = %g at point %zu; it must be > 0 where the exponent is not 0", planes[3 * Nq + i], i);
    }
    for (size_t i = 0; i < Nq && n; ++i)
        if (planes[i] != 1.0 || planes[Nq + i] != 0.0 || planes[2 * Nq + i] != 0.0) { mask |= HPV_NL_DIFF_U; break; }
    if (mask && hpv_nonlin_lds_bytes(h->qx, h->qy, h->ntx, h->nty) > 64 * 1024)
        return fail(h, -1, "element too large for the nonlinear projection kernel's LDS (%zu B)", hpv_nonlin_lds_bytes(h->qx, h->qy, h->ntx, h->nty));
    int rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));      // (an enqueued pass may still read the old planes)
    drop_graph(h);
    h->q_mask = 0;
    h->q_stale = false;
    h->q_exp = 0.0;
    if (!mask) {                                     // no multiplier: the handle launches what it launched before the first call
        if (h->d_qp) { (void)hipFree(h->d_qp); h->d_qp = nullptr; }
        return 0;
    }
    if ((rc = dalloc(h, &h->d_qp, n))) return rc;
    if ((rc = upload(h, h->d_qp, planes, n))) return rc;
    h->q_mask = mask;
    h->q_exp = exponent;
    return 0;
}

// Integral constraints (include/hpvpinn.h; kernels_moment.hip).  Everything is decided here; with n_terms == 0 nothing is kept and the
// handle launches what it launched before.
int hpv_set_moments(hpv_handle h, int n_terms, const int* power, const double* measure, size_t n, const double* target, const double* weight) {
    if (!h) return -1;
    if (!h->linear) return fail(h, -3, "hpv_set_moments belongs to the linear problems (HPV_PDE_LINEAR1D / _LINEAR2D)");
    // (removing terms is harmless on any handle: only SETTING them is refused under an exchange)
    if (n_terms > 0 && (h->rccl_on || h->p2p_on))
        return fail(h, -3, "hpv_set_moments on a handle with an exchange connected: the moments are integrals over the whole domain and there is no collective before the adjoint");
    if (!h->have_elems) return fail(h, -3, "call hpv_set_elements first");
    if (n_terms < 0 || n_terms > HPV_MAX_MOMENTS) return fail(h, -1, "n_terms = %d not in 0..%d", n_terms, HPV_MAX_MOMENTS);
    const size_t Nq = (size_t)h->Nq;
    if (n_terms > 0 && (!power || !measure || !target || !weight)) return fail(h, -1, "hpv_set_moments: a NULL array with n_terms = %d", n_terms);
    if (n != (size_t)n_terms * Nq) return fail(h, -1, "the measure has %zu entries, expected %d planes of %ld", n, n_terms, h->Nq);
    for (int k = 0; k < n_terms; ++k) {
        if (power[k] != 1 && power[k] != 2) return fail(h, -1, "term %d has power %d; 1 and 2 are supported", k, power[k]);
        if (!std::isfinite(target[k])) return fail(h, -1, "term %d has a non-finite target", k);
        if (!std::isfinite(weight[k])) return fail(h, -1, "term %d has a non-finite weight", k);
        if (weight[k] < 0.0) return fail(h, -1, "term %d has the negative weight %g", k, weight[k]);
    }
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(measure[i])) return fail(h, -1, "the measure of term %zu holds a non-finite value at point %zu", i / std::max(Nq, (size_t)1), i % std::max(Nq, (size_t)1));
    if (n_terms == 0 && !h->n_mom && !h->mom_stale) return 0;      // nothing was set: nothing to wait for, no graph to drop
    int rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));      // (an enqueued pass may still read the old planes)
    drop_graph(h);
    drop_moments(h);
    h->mom_stale = false;
    if (n_terms == 0 || h->n_elem == 0) return 0;
    if ((rc = dalloc(h, &h->d_mom, n))) return rc;
    if ((rc = upload(h, h->d_mom, measure, n))) return rc;
    if ((rc = dalloc(h, &h->d_mom_part, (size_t)n_terms * (size_t)h->n_elem))) return rc;
    const size_t nres = (size_t)3 * HPV_MAX_MOMENTS;      // (a name of its own: HIPCHK's message quotes the call)
    if ((rc = dalloc(h, &h->d_mom_res, nres))) return rc;
    HIPCHK(h, hipMemsetAsync(h->d_mom_res, 0, nres * sizeof(double), h->stream));
    if (h->n_coef && (rc = dalloc(h, &h->d_mom_dcoef, (size_t)h->n_coef * ((size_t)h->n_elem + n_terms)))) return rc;
    std::copy_n(power, n_terms, h->mom_power);
    std::copy_n(target, n_terms, h->mom_target);
    std::copy_n(weight, n_terms, h->mom_weight);
    h->n_mom = n_terms;
    return 0;
}

int hpv_read_moments(hpv_handle h, double* values, double* penalties, int n_terms) {
    if (!h || !values || !penalties) return -1;
    if (n_terms != h->n_mom) return fail(h, -1, "hpv_read_moments: n_terms = %d but the handle has %d terms", n_terms, h->n_mom);
    if (n_terms == 0) return 0;
    double res[3 * HPV_MAX_MOMENTS];
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(res, h->d_mom_res, sizeof res, hipMemcpyDeviceToHost));
    std::copy_n(res, n_terms, values);
    std::copy_n(res + HPV_MAX_MOMENTS, n_terms, penalties);
    return 0;
}

// The norm the residual is measured in (include/hpvpinn.h); the _dual instantiations of the projection kernels read the tables in place.
int hpv_set_residual_norm(hpv_handle h, int kind, double mass, const double* Sx, const double* lamx, const double* Sy, const double* lamy) {
    if (!h) return -1;
    if (!h->linear) return fail(h, -3, "hpv_set_residual_norm belongs to the linear problems (HPV_PDE_LINEAR1D / _LINEAR2D): the other classes and the whole-iteration kernels train mean(R^2)");
    if (h->cfg.scheme == HPV_SCHEME_PINN) return fail(h, -3, "hpv_set_residual_norm belongs to the variational scheme");
    if (kind != 0 && kind != 1) return fail(h, -1, "unknown residual norm %d (0 l2, 1 dual; 2, the dense factors, is hpv_set_residual_gram's)", kind);
    if (kind == 1 && h->unit_elems)
        return fail(h, -1, "the elements are mapped (hpv_set_element_points): the Gram matrix of the reference square is not their physical H^1 inner product");
    if (kind == 0) {
        if (!h->d_dual && !h->dual_stale && !h->d_gram && !h->gram_stale) return 0;
        HIPCHK(h, hipStreamSynchronize(h->stream));      // (an enqueued pass may still read the tables)
        drop_graph(h);
        if (h->d_dual) { (void)hipFree(h->d_dual); h->d_dual = nullptr; }
        if (h->d_gram) { (void)hipFree(h->d_gram); h->d_gram = nullptr; }      // (hpv_set_residual_gram)
        h->gram_stale = false;
        h->dual_stale = false;
        h->dual_mass = 0.0;
        return 0;
    }
    if (!h->have_tables) return fail(h, -3, "call hpv_set_tables first");
    const int ntx = h->ntx, nty = h->nty;
    if (!std::isfinite(mass) || mass < 0.0) return fail(h, -1, "the mass weight of the dual norm is %g; it must be finite and >= 0", mass);
    if (!Sx || !lamx) return fail(h, -1, "the dual norm needs the x tables");
    if (h->dim == 1 ? (Sy || lamy) : (!Sy || !lamy)) return fail(h, -1, "the y tables of the dual norm are NULL in 1-D and required in 2-D");
    const size_t nsx = (size_t)ntx * ntx * ntx, nlx = (size_t)ntx * ntx, nsy = (size_t)nty * nty * nty, nly = (size_t)nty * nty;
    std::vector<double> tab(hpv_dual_table_doubles(ntx, nty));
    std::copy_n(Sx, nsx, tab.begin());
    std::copy_n(lamx, nlx, tab.begin() + nsx);
    if (h->dim == 2) {
        std::copy_n(Sy, nsy, tab.begin() + nsx + nlx);
        std::copy_n(lamy, nly, tab.begin() + nsx + nlx + nsy);
    } else {      // nty == 1: S_y = 1, lam_y = 0 (d = lam_x / Jx + mass Jx with Jy = 1)
        tab[nsx + nlx] = 1.0;
        tab[nsx + nlx + nsy] = 0.0;
    }
    for (size_t i = 0; i < tab.size(); ++i)
        if (!std::isfinite(tab[i])) return fail(h, -1, "the tables of the dual norm hold a non-finite value at entry %zu", i);
    for (int n = 1; n <= ntx; ++n)      // (the entries behind the count are padding)
        for (int b = 0; b < n; ++b)
            if (!(lamx[(size_t)(n - 1) * ntx + b] > 0.0)) return fail(h, -1, "lam_x[%d][%d] = %g; the eigenvalues must be > 0", n - 1, b, lamx[(size_t)(n - 1) * ntx + b]);
    for (int n = 1; h->dim == 2 && n <= nty; ++n)
        for (int a = 0; a < n; ++a)
            if (!(lamy[(size_t)(n - 1) * nty + a] > 0.0)) return fail(h, -1, "lam_y[%d][%d] = %g; the eigenvalues must be > 0", n - 1, a, lamy[(size_t)(n - 1) * nty + a]);
    const size_t lds = hpv_dual_lds_bytes(h->qx, h->qy, ntx, nty);
    if (lds > 64 * 1024) return fail(h, -1, "element too large for the dual-norm projection kernels' LDS (%zu B)", lds);
    int rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));      // (an enqueued pass may still read the old tables)
    drop_graph(h);
    if (h->d_dual) { (void)hipFree(h->d_dual); h->d_dual = nullptr; }
    if ((rc = dalloc(h, &h->d_dual, tab.size()))) return rc;
    if ((rc = upload(h, h->d_dual, tab.data(), tab.size()))) { (void)hipFree(h->d_dual); h->d_dual = nullptr; return rc; }
    h->dual_mass = mass;
    h->dual_stale = false;
    if (h->d_gram) { (void)hipFree(h->d_gram); h->d_gram = nullptr; }      // (kind 1 replaces kind 2)
    h->gram_stale = false;
    return 0;
}

// The same norm through one dense inverse Gram factor per owned element (include/hpvpinn.h); the _dense instantiations of the
// projection kernels read the factors in place (csrc/hpv_dual_dense.h).
int hpv_set_residual_gram(hpv_handle h, const double* W, size_t n) {
    if (!h) return -1;
    if (!h->linear) return fail(h, -3, "hpv_set_residual_gram belongs to the linear problems (HPV_PDE_LINEAR1D / _LINEAR2D): the other classes and the whole-iteration kernels train mean(R^2)");
    if (h->cfg.scheme == HPV_SCHEME_PINN) return fail(h, -3, "hpv_set_residual_gram belongs to the variational scheme");
    if (!h->have_tables || !h->have_elems) return fail(h, -3, "call hpv_set_tables and hpv_set_elements first");
    const int ntx = h->ntx, nty = h->nty;
    const size_t NR = (size_t)ntx * nty, ne = (size_t)h->n_elem;
    const size_t lds = hpv_dual_dense_lds_bytes(h->qx, h->qy, ntx, nty);
    if (lds > 64 * 1024) return fail(h, -1, "element too large for the dense dual-norm projection kernels' LDS (%zu B)", lds);
    if (!W || n != ne * NR * NR) return fail(h, -1, "the Gram factors have %zu entries, expected %zu x %zu x %zu", W ? n : (size_t)0, ne, NR, NR);
    for (size_t e = 0; e < ne; ++e) {
        const int nax = h->nact_all.empty() ? ntx : h->nact_all[h->e_begin + e];
        const int nay = h->nacty_all.empty() ? nty : h->nacty_all[h->e_begin + e];
        const double* We = W + e * NR * NR;
        auto active = [&](size_t i) { return (int)(i % ntx) < nax && (int)(i / ntx) < nay; };
        for (size_t i = 0; i < NR; ++i)
            for (size_t j = 0; j < NR; ++j) {
                const double v = We[i * NR + j];
                if (!std::isfinite(v)) return fail(h, -1, "the Gram factor of element %zu holds a non-finite value at [%zu][%zu]", h->e_begin + e, i, j);
                if (j > i && v != 0.0) return fail(h, -1, "the Gram factor of element %zu is not lower triangular: [%zu][%zu] = %g", h->e_begin + e, i, j, v);
                if (v != 0.0 && (!active(i) || !active(j)))
                    return fail(h, -1, "the Gram factor of element %zu is %g at [%zu][%zu], in the row or column of an inactive test function (%d x %d active)", h->e_begin + e, v, i, j, nax, nay);
                if (i == j && active(i) && !(v > 0.0)) return fail(h, -1, "the Gram factor of element %zu has the diagonal entry [%zu] = %g; it must be > 0", h->e_begin + e, i, v);
            }
    }
    int rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));      // (an enqueued pass may still read the old factors or tables)
    drop_graph(h);
    double* d_new = nullptr;
    if ((rc = dalloc(h, &d_new, n))) return rc;
    if (n > 0 && (rc = upload(h, d_new, W, n))) { (void)hipFree(d_new); return rc; }
    if (h->d_gram) (void)hipFree(h->d_gram);
    h->d_gram = d_new;
    h->gram_stale = false;
    if (h->d_dual) { (void)hipFree(h->d_dual); h->d_dual = nullptr; }      // (kind 2 replaces kind 1)
    h->dual_stale = false;
    h->dual_mass = 0.0;
    return 0;
}

// The directions of the trainable coefficients (include/hpvpinn.h); k_project_id reads them in place.  The masks are decided here, once.
int hpv_set_trainable(hpv_handle h, const double* dirs, size_t n) {
    if (!h) return -1;
    if (h->q_mask || h->q_stale) return fail(h, -3, "hpv_set_trainable on a handle with the quasilinear term (hpv_set_quasilinear): k_project_id does not carry the multiplier");
    if (!h->n_coef) return fail(h, -1, "the handle was created without trainable coefficients (hpv_create_ex)");
    if (!h->have_elems) return fail(h, -3, "call hpv_set_elements first");
    const size_t K = h->lin_tensor ? 7 : h->dim == 1 ? 3 : 5, M = h->dim == 1 ? 4 : 5, Nq = (size_t)h->Nq, NP = K + M;
    if (!dirs || n != (size_t)h->n_coef * NP * Nq)
        return fail(h, -1, "the directions have %zu entries, expected %d x %zu planes of %ld", n, h->n_coef, NP, h->Nq);
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(dirs[i])) return fail(h, -1, "direction %zu holds a non-finite value in plane %zu at point %zu", i / std::max(NP * Nq, (size_t)1), i / std::max(Nq, (size_t)1) % NP, i % std::max(Nq, (size_t)1));
    int dm[HPV_MAX_COEF] = {}, nlm = 0;
    for (size_t i = 0; i < n; ++i)
        if (dirs[i] != 0.0) {
            const size_t p = i / Nq % NP;
            dm[i / (NP * Nq)] |= 1 << p;
            if (p >= K) nlm |= 1 << std::min(p - K, (size_t)3);      // (gx and gy are one term)
        }
    int rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));      // (an enqueued pass may still read the old directions)
    drop_graph(h);
    h->have_dirs = false;
    if ((rc = dalloc(h, &h->d_dirs, n))) return rc;
    if (n && (rc = upload(h, h->d_dirs, dirs, n))) return rc;
    if ((rc = dalloc(h, &h->d_dcoef_e, (size_t)h->n_coef * (size_t)h->n_elem))) return rc;
    if (!h->d_dir_mask && (rc = dalloc(h, &h->d_dir_mask, (size_t)HPV_MAX_COEF))) return rc;
    if ((rc = dalloc(h, &h->d_nl_zero, M * Nq))) return rc;      // (read where hpv_set_nonlinear holds no planes)
    if (Nq) HIPCHK(h, hipMemsetAsync(h->d_nl_zero, 0, M * Nq * sizeof(double), h->stream));
    HIPCHK(h, hipMemcpyAsync(h->d_dir_mask, dm, sizeof dm, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    std::copy_n(dm, HPV_MAX_COEF, h->dir_mask);
    h->dir_nl_mask = nlm;
    h->have_dirs = true;
    return 0;
}

// The ansatz planes of one point set (include/hpvpinn.h); k_ansatz_fwd / k_ansatz_adj read them in place.
int hpv_set_ansatz(hpv_handle h, int which, const double* planes, size_t n) {
    if (!h) return -1;
    if (!h->linear) return fail(h, -1, "hpv_set_ansatz belongs to the linear problems (HPV_PDE_LINEAR1D / _LINEAR2D)");
    if (which < HPV_ANSATZ_QUAD || which > HPV_ANSATZ_VALID) return fail(h, -1, "unknown point set %d (0 QUAD .. 3 VALID)", which);
    if (!planes && n != 0) return fail(h, -1, "NULL planes with n = %zu (NULL and 0 remove the planes)", n);
    int rc;
    if (!planes) {
        if (!h->ans_on[which]) return 0;
        HIPCHK(h, hipStreamSynchronize(h->stream));      // (an enqueued pass may still read the planes)
        drop_graph(h);
        drop_ansatz(h, which);
        return 0;
    }
    if (h->d_sf) return fail(h, -1, "the strong form is active (hpv_set_strong_form): its residual needs second derivatives of G and D, which are not available");
    if (which == HPV_ANSATZ_QUAD && !h->have_elems) return fail(h, -3, "call hpv_set_elements first");
    const long count[] = {h->Nq, (long)h->n_data, (long)h->n_flux, (long)h->n_val};
    const size_t np = (size_t)count[which], rows = 2 * (size_t)(1 + h->dim);
    if (n != np) return fail(h, -1, "the ansatz has n = %zu points, the set has %zu", n, np);
    for (size_t i = 0; i < rows * np; ++i)
        if (!std::isfinite(planes[i])) return fail(h, -1, "ansatz plane %zu holds a non-finite value at point %zu", i / np, i % np);
    HIPCHK(h, hipStreamSynchronize(h->stream));          // (an enqueued pass may still read the old planes)
    drop_graph(h);
    const bool had = has_ansatz(h);
    drop_ansatz(h, which);
    if ((rc = dalloc(h, &h->d_ans[which], rows * np))) return rc;
    if ((rc = upload(h, h->d_ans[which], planes, rows * np))) return rc;
    h->ans_on[which] = true;
    h->ans_n[which] = (long)np;
    if (!had) h->batch_dirty = true;                     // the first planes of the handle: the data points leave the quadrature batch
    return 0;
}

int hpv_set_flux_data(hpv_handle h, const double* X, const double* coef, const double* g, int n, double weight) {
    if (!h) return -1;
    if (n < 0 || (n > 0 && (!X || !coef || !g)) || !std::isfinite(weight)) return fail(h, -1, "bad flux data arguments");
    int rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));      // (an enqueued pass may still read the old set)
    drop_graph(h);
    drop_ansatz(h, HPV_ANSATZ_FLUX);             // the ansatz planes belong to the old points
    h->n_flux = 0;
    const int d = h->dim;
    const long N = ((long)n + 15) / 16 * 16;      // whole 16-point tiles; the padding sits at the origin and carries zero adjoints
    if ((rc = alloc_batch(h, h->flux, h->nd_grad, N, true))) return rc;
    if ((rc = dalloc(h, &h->d_flux_coef, (size_t)(1 + d) * n))) return rc;
    if ((rc = dalloc(h, &h->d_flux_g, (size_t)n))) return rc;
    if (n == 0) return 0;
    if (!h->d_flux_part) {
        if ((rc = dalloc(h, &h->d_flux_part, (size_t)65))) return rc;
        HIPCHK(h, hipMemsetAsync(h->d_flux_part, 0, 65 * sizeof(double), h->stream));
    }
    const std::vector<double> t = transposed(X, n, d, N), c = transposed(coef, n, 1 + d, n);      // -> [d][N], [1 + d][n]
    if ((rc = upload(h, h->flux.X, t.data(), t.size()))) return rc;
    if ((rc = upload(h, h->d_flux_coef, c.data(), c.size()))) return rc;
    if ((rc = upload(h, h->d_flux_g, g, (size_t)n))) return rc;
    h->w_flux = weight;
    h->n_flux = n;
    return 0;
}

int hpv_read_flux_loss(hpv_handle h, double* out2) {
    if (!h || !out2) return -1;
    double msf = 0.0;
    if (h->n_flux > 0) HIPCHK(h, hipMemcpyAsync(&msf, h->d_flux_part + 64, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    out2[0] = h->w_flux * msf;
    out2[1] = msf;
    return 0;
}

int hpv_set_collocation(hpv_handle h, const double* X, const double* f, int n) {
    return hpv_set_collocation_shard(h, X, f, n, (long)n);
}

int hpv_set_collocation_shard(hpv_handle h, const double* X, const double* f, int n, long n_total) {
    if (!h) return -1;
    if (h->cfg.scheme != HPV_SCHEME_PINN) return fail(h, -1, "collocation points belong to scheme PINNs");
    // f == NULL: zero right-hand side, AdvDiff only (P3:186 squares net_f itself; hpv_set_rhs does the same for the variational form)
    if (n < 1 || !X || (!f && h->cfg.pde != HPV_PDE_ADVDIFF) || n_total < n) return fail(h, -1, "bad collocation arguments");
    drop_graph(h);
    int rc;
    if ((rc = alloc_batch(h, h->colloc, h->nd_pinn, n, true))) return rc;
    if ((rc = upload_points(h, h->colloc, X, n, h->dim))) return rc;
    if ((rc = dalloc(h, &h->d_fcol, (size_t)n))) return rc;
    if (f) { if ((rc = upload(h, h->d_fcol, f, (size_t)n))) return rc; }
    else HIPCHK(h, hipMemsetAsync(h->d_fcol, 0, (size_t)n * sizeof(double), h->stream));
    if ((rc = dalloc(h, &h->d_col_part, 128))) return rc;      // [0..63] r^2 partials, [64..127] d epsilon partials
    h->n_col = n;
    h->n_col_total = n_total;
    return 0;
}

size_t hpv_num_params(hpv_handle h) { return h ? (size_t)h->Ptot : 0; }

int hpv_set_params(hpv_handle h, const double* theta, size_t n) {
    if (!h) return -1;
    if (!theta || n != (size_t)h->Ptot) return fail(h, -1, "theta has %zu entries, expected %d", n, h->Ptot);
    int rc;
    if ((rc = upload(h, h->d_theta, theta, n))) return rc;
    HIPCHK(h, hipMemsetAsync(h->d_m, 0, n * sizeof(double), h->stream));
    HIPCHK(h, hipMemsetAsync(h->d_v, 0, n * sizeof(double), h->stream));
    std::vector<double> st((size_t)adam_state_doubles(h->P));
    for (size_t i = 0; i < st.size(); i += 2) { st[i] = h->cfg.beta1; st[i + 1] = h->cfg.beta2; }   // beta^1, every copy
    if ((rc = upload(h, h->d_state, st.data(), st.size()))) return rc;
    h->have_params = true;
    return lbfgs_drop(h);      // (curvature pairs gathered along another trajectory say nothing about these parameters)
}

int hpv_get_params(hpv_handle h, double* theta, size_t n) {
    if (!h) return -1;
    if (!theta || n != (size_t)h->Ptot) return fail(h, -1, "theta buffer has %zu entries, expected %d", n, h->Ptot);
    HIPCHK(h, hipMemcpyAsync(theta, h->d_theta, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}

int hpv_forward_backward(hpv_handle h) { return h ? enqueue_pass(h, true) : -1; }
int hpv_eval_loss(hpv_handle h) { return h ? enqueue_pass(h, false) : -1; }

int hpv_reduce_buffer(hpv_handle h, void** dev_ptr, size_t* n_doubles) {
    if (!h || !dev_ptr || !n_doubles) return -1;
    *dev_ptr = h->d_RB;
    *n_doubles = (size_t)h->Ptot + 4;
    return 0;
}

int hpv_apply_adam(hpv_handle h) {
    if (!h) return -1;
    enqueue_adam(h);
    if (int rc = launch_check(h, "adam launch")) return rc;
    h->nupd_host += 1;
    return 0;
}

int hpv_sync(hpv_handle h) {
    if (!h) return -1;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return sync_check(h);     // (the caller-driven multi-GPU pieces -- forward_backward / apply_adam -- end their runs here)
}

static void loss_triple(hpv_ctx* h, const double* raw, double* loss3) {
    loss3[0] = raw[0] + raw[1];
    loss3[1] = (h->cfg.pde == HPV_PDE_ADVDIFF) ? raw[1] : raw[2];  // P3:184 folds the weight into lossb
    loss3[2] = raw[0];
}

int hpv_read_loss(hpv_handle h, double* loss3) {
    if (!h || !loss3) return -1;
    double t[4];
    HIPCHK(h, hipMemcpyAsync(t, h->d_RB + h->Ptot, 4 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    loss_triple(h, t, loss3);
    return 0;
}

int hpv_loss_and_grad(hpv_handle h, double* loss3, double* grad) {
    if (!h) return -1;
    int rc = enqueue_pass_x(h, grad != nullptr, false);
    if (rc) return rc;
    if (loss3 && (rc = hpv_read_loss(h, loss3))) return rc;
    if (grad) {
        HIPCHK(h, hipMemcpyAsync(grad, h->d_RB, (size_t)h->Ptot * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (grad && (rc = sync_check(h))) return rc;     // a gradient from a failed SPLIT-mode barrier is not a gradient
    return p2p_check(h);
}

// after a synchronisation point: did a SPLIT-mode element barrier time out (on this rank, or -- carried by the pad slot of the
// all-reduced buffer -- on any rank)?  The kernels have left theta, m, v, the beta powers and the loss history as they were
// before the failing iteration and have ignored every iteration since (sticky flag); here the failure is reported (-7), the
// flag cleared (the exchange is stateless: tagged granules), so that the caller may go on (e.g. with HPV_FUSE=s on a shared GPU).
static int sync_check(hpv_ctx* h) {
    if (!h->d_xerr || !h->var.m) return 0;
    if (!hpv_mfma_split_used(h->var.m) && !h->rccl_on && !h->p2p_on) return 0;   // nothing can have set it
    int err = 0;
    HIPCHK(h, hipMemcpyAsync(&err, h->d_xerr, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (!err) return 0;
    HIPCHK(h, hipMemsetAsync(h->d_xerr, 0, sizeof(int), h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return fail(h, -7, "whole-iteration kernel (SPLIT mode): the workgroups sharing an element did not meet at their barrier "
                       "(timeout) on some rank; the failing iteration and every later one of this call were NOT applied -- "
                       "parameters and optimizer state are those before it.  Is the GPU shared with another process?  HPV_FUSE=s "
                       "selects the barrier-free kernels");
}

// A run of `n` enqueued iterations ended with -7.  The device counter says how many of them were applied; unless the caller
// opted out (HPV_EXCHANGE_FALLBACK=0) the handle is switched to the launch structures without an in-kernel exchange and the
// caller finishes the run on those.  Handles connected to other ranks (in-library RCCL / mailbox exchange) take the same
// decision without talking to each other: the failure flag travels with the all-reduced buffer of the failing iteration, so
// every rank's k_adam / exchange kernel skips from the same iteration on, every rank's hpv_step sees -7 in the same call with
// the same count, and every rank enqueues the same number of remaining iterations (collectives stay matched).
// Returns the number of iterations that took place, or -1: report the -7.
static int after_exchange_timeout(hpv_ctx* h, int n) {
    long long dev = 0;
    if (hpv_updates_applied(h, &dev)) return -1;
    const long long done = dev - (h->nupd_host - n);
    h->nupd_host = dev;
    const char* e = getenv("HPV_EXCHANGE_FALLBACK");
    if ((e && e[0] == '0') || !h->shared_elem_ok || done < 0 || done > n) return -1;
    if (hpv_set_shared_element_kernels(h, 0)) return -1;
    if (h->n_fallbacks++ == 0)
        fprintf(stderr, "libhpvpinn: an in-kernel exchange between the workgroups of one element timed out after %lld of %d "
                        "iterations (is the GPU shared?); continuing on the launch structures without an exchange "
                        "(HPV_EXCHANGE_FALLBACK=0: return -7 instead)\n", done, n);
    h->err.clear();
    return (int)done;
}

int hpv_step(hpv_handle h, int n_iters, double* loss3_after) {
    if (!h) return -1;
    int rc;
    for (int left = n_iters, round = 0;; ++round) {
        if ((rc = enqueue_iterations(h, left))) return rc;
        if (loss3_after) {
            if ((rc = enqueue_pass_x(h, false, false))) return rc;
            if ((rc = hpv_read_loss(h, loss3_after))) return rc;
        } else {
            HIPCHK(h, hipStreamSynchronize(h->stream));
        }
        if ((rc = sync_check(h)) != -7 || round) break;
        const int done = after_exchange_timeout(h, left);      // the rest of the run on the barrier-free structures
        if (done < 0) break;
        left -= done;
    }
    if (rc) return rc;
    return p2p_check(h);
}

// ---- loss history (the reference records the loss after every update with a second forward pass, P2:243-244; the
//      forward pass of the NEXT iteration computes exactly that value, so the device keeps it) ----

int hpv_history_reset(hpv_handle h) {
    if (!h) return -1;
    HIPCHK(h, hipMemsetAsync(h->d_hist_idx, 0, sizeof(int), h->stream));
    return 0;
}

int hpv_history_read(hpv_handle h, int n, double* loss3_hist, double* eps_hist) {
    if (!h || !loss3_hist || n < 0) return -1;
    if (n > HPV_HIST_CAP) return fail(h, -1, "history holds %d entries, %d requested", HPV_HIST_CAP, n);
    int have = 0;
    std::vector<double> raw((size_t)4 * n);
    HIPCHK(h, hipMemcpyAsync(&have, h->d_hist_idx, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    if (n) HIPCHK(h, hipMemcpyAsync(raw.data(), h->d_hist, raw.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (have < n) return fail(h, -3, "only %d training iterations since hpv_history_reset, %d requested", have, n);
    for (int i = 0; i < n; ++i) {
        loss_triple(h, &raw[(size_t)4 * i], loss3_hist + 3 * i);
        if (eps_hist) eps_hist[i] = raw[(size_t)4 * i + 3];
    }
    return 0;
}

int hpv_time_iteration_kernel(hpv_handle h, int reps, double* avg_ms) {
    if (!h || reps < 1 || !avg_ms) return -1;
    int rc = check_ready(h);
    if (rc) return rc;
    if (h->cfg.scheme == HPV_SCHEME_PINN || !(h->var.m && h->backend == HPV_BACKEND_MFMA) || h->var.N <= 0)
        return fail(h, -4, "no whole-iteration kernel on this handle");
    if ((rc = enqueue_pass(h, true))) return rc;        // everything a first pass allocates / selects
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if ((rc = sync_check(h))) return rc;
    if (h->pass_structure != 2) return fail(h, -4, "the handle's iteration is not ONE whole-iteration launch without an in-kernel exchange");
    const MfmaDataTerm dt = pass_data_term(h, true);
    const ProjArgs pa = pass_proj_args(h, true);
    const MfmaPass p = pass_mfma(h, dt, pa);
    hipEvent_t e0 = nullptr, e1 = nullptr;
    HIPCHK(h, hipEventCreate(&e0));
    HIPCHK(h, hipEventCreate(&e1));
    bool ok = true;
    (void)hipEventRecord(e0, h->stream);
    for (int i = 0; i < reps && ok; ++i)
        ok = hpv_mfma_iter_fused(h->var.m, p);
    (void)hipEventRecord(e1, h->stream);
    hipError_t e = hipStreamSynchronize(h->stream);
    float ms = 0.0f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (!ok) return fail(h, -4, "the whole-iteration kernel declined the launch");
    if (e != hipSuccess) return fail(h, -2, "timing the iteration kernel failed: %s", hipGetErrorString(e));
    *avg_ms = (double)ms / reps;
    return 0;
}

int hpv_step_record(hpv_handle h, int n_iters, double* loss3_hist, double* eps_hist) {
    if (!h || !loss3_hist || n_iters < 0) return -1;
    int rc;
    std::vector<double> chunk((size_t)3 * HPV_HIST_CAP), ceps(HPV_HIST_CAP);
    for (int done = 0; done < n_iters;) {
        const int c = std::min(HPV_HIST_CAP, n_iters - done);
        if ((rc = hpv_history_reset(h))) return rc;
        if ((rc = enqueue_iterations(h, c))) return rc;
        HIPCHK(h, hipStreamSynchronize(h->stream));
        int got = c;       // (a skipped iteration records nothing: after a timeout the history holds the `got` that took place)
        if ((rc = sync_check(h)) == -7 && (got = after_exchange_timeout(h, c)) >= 0) rc = 0;
        if (rc || (rc = p2p_check(h))) return rc;
        if (got && (rc = hpv_history_read(h, got, chunk.data(), ceps.data()))) return rc;
        // entry j was computed by the forward pass that preceded update done+j+1, i.e. it belongs to the state after update done+j
        for (int j = 0; j < got; ++j)
            if (done + j >= 1) {
                std::copy_n(&chunk[(size_t)3 * j], 3, loss3_hist + (size_t)3 * (done + j - 1));
                if (eps_hist) eps_hist[done + j - 1] = ceps[j];
            }
        done += got;
    }
    if (n_iters > 0) {   // the state after the last update: one forward pass
        if ((rc = enqueue_pass_x(h, false, false))) return rc;
        if ((rc = hpv_read_loss(h, loss3_hist + (size_t)3 * (n_iters - 1)))) return rc;
        if (eps_hist) {
            eps_hist[n_iters - 1] = 0.0;
            if (h->Ptot > h->P) {      // epsilon of AdvDiff | the first trainable coefficient of a linear handle
                HIPCHK(h, hipMemcpyAsync(eps_hist + n_iters - 1, h->d_theta + h->P, sizeof(double), hipMemcpyDeviceToHost, h->stream));
                HIPCHK(h, hipStreamSynchronize(h->stream));
            }
        }
    }
    return 0;
}

int hpv_predict(hpv_handle h, const double* X, int n, double* u_out) {
    if (!h) return -1;
    if (!h->have_params) return fail(h, -3, "hpv_set_params has not been called");
    if (n < 0 || (n > 0 && (!X || !u_out))) return fail(h, -1, "bad predict arguments");
    if (n == 0) return 0;
    int rc;
    if (h->pred.N != n && (rc = points_batch(h, h->pred, h->nd_val, n))) return rc;
    if ((rc = upload_points(h, h->pred, X, n, h->dim))) return rc;
    if ((rc = forward_only(h, h->pred))) return rc;
    HIPCHK(h, hipMemcpyAsync(u_out, h->pred.OUT, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}

// ---- device-side validation: derivative channels and the strong residual at the caller's points, error norms against an exact
//      solution on a stored set, and a device-side history of those norms filled between training iterations (the reference takes
//      u_pred on its test grid through the host: P1:197-199, P2:255-257; its pointwise residual is net_f, P2:187-194, P3:247-253) ----
namespace {

// the full channel list at the caller's points: upload + ONE forward launch on the handle's own batch (re-created when n changes)
int eval_points_forward(hpv_ctx* h, const double* X, int n) {
    int rc;
    if (h->evalp.N != n) {
        if ((rc = points_batch(h, h->evalp, h->nd_full, n))) return rc;
        if ((rc = dalloc(h, &h->d_res_f, (size_t)n))) return rc;
        if ((rc = dalloc(h, &h->d_res_r, (size_t)n))) return rc;
    }
    if ((rc = upload_points(h, h->evalp, X, n, h->dim))) return rc;
    return forward_only(h, h->evalp);
}

int validation_ready(hpv_ctx* h) {
    if (!h->have_params) return fail(h, -3, "hpv_set_params has not been called");
    if (h->n_val <= 0) return fail(h, -3, "hpv_set_validation has not been called");
    return ansatz_ready(h, HPV_ANSATZ_VALID);
}

// forward over the stored set + the reduction, on the handle's stream; no synchronisation, no host read
int enqueue_validation(hpv_ctx* h, bool to_history) {
    int rc = forward_only(h, h->valb);
    if (rc) return rc;
    ansatz_fwd(h, HPV_ANSATZ_VALID, h->valb, h->n_val);
    const int cap = HPV_HIST_CAP;
    double* buf = h->d_val_buf;
    const ValArgs a{h->valb.OUT, h->valb.N, h->d_val_u, h->d_val_du, h->n_val, h->dim, buf + 6 + (size_t)6 * cap,
                    reinterpret_cast<unsigned int*>(h->d_val_idx + 1), buf, to_history ? buf + 6 : nullptr, h->d_val_idx, cap};
    launch_validate_reduce(a, validate_reduce_blocks(h->n_val), h->stream);
    HIPCHK(h, hipGetLastError());
    return 0;
}

}  // namespace

int hpv_eval_points(hpv_handle h, const double* X, int n, double* out, size_t n_out) {
    if (!h) return -1;
    if (!h->have_params) return fail(h, -3, "hpv_set_params has not been called");
    if (n < 0 || (n > 0 && (!X || !out))) return fail(h, -1, "bad evaluation arguments");
    const int C = h->nd_full.C;
    if (n_out != (size_t)C * n) return fail(h, -1, "channel buffer has %zu entries, expected %zu", n_out, (size_t)C * n);
    if (n == 0) return 0;
    int rc = eval_points_forward(h, X, n);
    if (rc) return rc;
    HIPCHK(h, hipMemcpyAsync(out, h->evalp.OUT, n_out * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}

int hpv_residual_points(hpv_handle h, const double* X, const double* f, int n, double* r_out) {
    if (!h) return -1;
    if (h->linear) return fail(h, -1, "the strong residual of a linear problem needs derivatives of its coefficients: not available");
    if (!h->have_params) return fail(h, -3, "hpv_set_params has not been called");
    if (n < 0 || (n > 0 && (!X || !r_out))) return fail(h, -1, "bad residual arguments");
    if (n == 0) return 0;
    int rc = eval_points_forward(h, X, n);
    if (rc) return rc;
    if (f && (rc = upload(h, h->d_res_f, f, (size_t)n))) return rc;
    launch_residual_points(h->cfg.pde, h->evalp.OUT, h->evalp.N, f ? h->d_res_f : nullptr, h->has_eps ? h->d_theta + h->P : nullptr,
                           h->cfg.V, n, h->d_res_r, h->stream);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(r_out, h->d_res_r, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}

int hpv_set_validation(hpv_handle h, const double* X, const double* u, const double* du, int n) {
    if (!h) return -1;
    if (n < 0 || (n > 0 && (!X || !u))) return fail(h, -1, "bad validation arguments");
    int rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));      // (an enqueued validation may still read the old set)
    if (h->ans_on[HPV_ANSATZ_VALID]) { drop_ansatz(h, HPV_ANSATZ_VALID); drop_graph(h); }      // the ansatz planes belong to the old points
    h->n_val = 0;
    if ((rc = points_batch(h, h->valb, du ? h->nd_grad : h->nd_val, n))) return rc;
    if ((rc = dalloc(h, &h->d_val_u, (size_t)n))) return rc;
    if ((rc = dalloc(h, &h->d_val_du, du ? (size_t)n * h->dim : 0))) return rc;
    if (n == 0) return 0;
    if (!h->d_val_buf) {
        const size_t doubles = 6 + (size_t)6 * HPV_HIST_CAP + (size_t)5 * HPV_VAL_MAX_BLOCKS;
        if ((rc = dalloc(h, &h->d_val_buf, doubles))) return rc;
        if ((rc = dalloc(h, &h->d_val_idx, (size_t)2))) return rc;
        HIPCHK(h, hipMemsetAsync(h->d_val_buf, 0, doubles * sizeof(double), h->stream));
        HIPCHK(h, hipMemsetAsync(h->d_val_idx, 0, 2 * sizeof(int), h->stream));
    }
    if ((rc = upload_points(h, h->valb, X, n, h->dim))) return rc;
    if ((rc = upload(h, h->d_val_u, u, (size_t)n))) return rc;
    if (du && (rc = upload(h, h->d_val_du, transposed(du, n, h->dim, n).data(), (size_t)n * h->dim))) return rc;      // -> [dim][n]
    h->n_val = n;
    return 0;
}

int hpv_validate(hpv_handle h, double* out6) {
    if (!h) return -1;
    if (!out6) return fail(h, -1, "bad validation arguments");
    int rc = validation_ready(h);
    if (rc || (rc = enqueue_validation(h, false))) return rc;
    HIPCHK(h, hipMemcpyAsync(out6, h->d_val_buf, 6 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}

int hpv_validation_reset(hpv_handle h) {
    if (!h) return -1;
    int rc = validation_ready(h);
    if (rc) return rc;
    HIPCHK(h, hipMemsetAsync(h->d_val_idx, 0, sizeof(int), h->stream));
    return 0;
}

int hpv_validate_enqueue(hpv_handle h) {
    if (!h) return -1;
    int rc = validation_ready(h);
    return rc ? rc : enqueue_validation(h, true);
}

int hpv_validation_read(hpv_handle h, int n, double* out) {
    if (!h) return -1;
    if (n < 0 || (n > 0 && !out)) return fail(h, -1, "bad validation arguments");
    const int cap = HPV_HIST_CAP;
    if (n > cap) return fail(h, -1, "validation history holds %d entries, %d requested", cap, n);
    int rc = validation_ready(h);
    if (rc) return rc;
    int have = 0;
    HIPCHK(h, hipMemcpyAsync(&have, h->d_val_idx, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    if (n) HIPCHK(h, hipMemcpyAsync(out, h->d_val_buf + 6, (size_t)6 * n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (have < n) return fail(h, -3, "only %d validations since hpv_validation_reset, %d requested", have, n);
    return 0;
}

// hpv_step with a validation enqueued behind every `every`-th update: chunks of `every` iterations (graph replays where hpv_step
// replays them -- the validation launches sit BETWEEN the replays, the captured iterations are untouched), one synchronisation and
// one read at the end.  An in-kernel exchange that timed out (-7) is handled as in hpv_step: the iterations that took place are
// kept with the samples they completed, the rest runs on the barrier-free structures.
int hpv_step_validate(hpv_handle h, int n_iters, int every, double* out, size_t n_out) {
    if (!h) return -1;
    if (n_iters < 0 || every < 1) return fail(h, -1, "bad arguments: %d iterations, a validation every %d", n_iters, every);
    const int ns = n_iters / every, cap = HPV_HIST_CAP;
    if (ns > cap) return fail(h, -1, "validation history holds %d entries, %d requested", cap, ns);
    if (n_out < (size_t)6 * ns || (ns > 0 && !out)) return fail(h, -1, "validation buffer has %zu entries, expected %zu", n_out, (size_t)6 * ns);
    int rc = validation_ready(h);
    if (rc) return rc;
    int it = 0;      // iterations that have taken place
    for (int round = 0;; ++round) {
        const int first = it / every;      // samples already complete
        HIPCHK(h, hipMemcpyAsync(h->d_val_idx, &first, sizeof(int), hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        for (int k = it; k < n_iters;) {
            const int c = std::min(every - k % every, n_iters - k);
            if ((rc = enqueue_iterations(h, c))) return rc;
            k += c;
            if (k % every == 0 && (rc = enqueue_validation(h, true))) return rc;
        }
        HIPCHK(h, hipStreamSynchronize(h->stream));
        if ((rc = sync_check(h)) != -7 || round) break;
        const int done = after_exchange_timeout(h, n_iters - it);
        if (done < 0) break;
        it += done;
    }
    if (rc || (rc = p2p_check(h))) return rc;
    return hpv_validation_read(h, ns, out);
}

// [theta | m | v | beta1^t | beta2^t]: everything a bit-exact resume needs.
int hpv_get_state(hpv_handle h, double* buf, size_t n) {
    if (!h || !buf) return -1;
    const size_t P = (size_t)h->Ptot;
    if (n != 3 * P + 2) return fail(h, -1, "state buffer has %zu entries, expected %zu", n, 3 * P + 2);
    HIPCHK(h, hipMemcpyAsync(buf, h->d_theta, P * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(buf + P, h->d_m, P * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(buf + 2 * P, h->d_v, P * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(buf + 3 * P, h->d_state, 2 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}

int hpv_set_state(hpv_handle h, const double* buf, size_t n) {
    if (!h || !buf) return -1;
    const size_t P = (size_t)h->Ptot;
    if (n != 3 * P + 2) return fail(h, -1, "state buffer has %zu entries, expected %zu", n, 3 * P + 2);
    int rc;
    if ((rc = upload(h, h->d_theta, buf, P))) return rc;
    if ((rc = upload(h, h->d_m, buf + P, P))) return rc;
    if ((rc = upload(h, h->d_v, buf + 2 * P, P))) return rc;
    std::vector<double> st((size_t)adam_state_doubles(h->P));
    for (size_t i = 0; i < st.size(); i += 2) { st[i] = buf[3 * P]; st[i + 1] = buf[3 * P + 1]; }
    if ((rc = upload(h, h->d_state, st.data(), st.size()))) return rc;
    h->have_params = true;
    return lbfgs_drop(h);      // (curvature pairs gathered along another trajectory say nothing about these parameters)
}

// F_ext[e][k][r] = J_e sum_q w_x phi_r w_y phi_k f(x_q)  (P1:289, P2:405-407) for the owned elements, from
// the values of f at this handle's quadrature points (element-major, q = j*qx+i): the driver-side RHS
// assembly done by the projection kernel instead of the reference's Python loops.
int hpv_assemble_rhs(hpv_handle h, const double* f_quad, size_t n, double* F_out, size_t n_out) {
    if (!h || !f_quad || !F_out) return -1;
    if (!h->have_quad || !h->have_tables || !h->have_elems) return fail(h, -3, "set quadrature, tables and elements first");
    const long NQ = (long)h->qx * h->qy, NR = (long)h->ntx * h->nty, ne = h->n_elem;
    if (n != (size_t)(ne * NQ) || n_out != (size_t)(ne * NR)) return fail(h, -1, "f has %zu / F has %zu entries, expected %ld / %ld", n, n_out, ne * NQ, ne * NR);
    if (ne == 0) return 0;
    double *d_f = nullptr, *d_F = nullptr, *d_le = nullptr;
    int rc = 0;
    rc |= dalloc(h, &d_f, n); rc |= dalloc(h, &d_F, n_out); rc |= dalloc(h, &d_le, (size_t)ne);
    if (!rc) rc = upload(h, d_f, f_quad, n);
    if (!rc) {
        ProjDesc pd{};
        pd.nterms = 1; pd.t[0].dx = 0; pd.t[0].dy = 0; pd.t[0].a0[0] = 1.0;
        pd.qx = h->qx; pd.qy = h->qy; pd.ntx = h->ntx; pd.nty = h->nty; pd.C = 1;
        ProjArgs pa{};      // residual only: no adjoint, no epsilon, no right-hand side to subtract
        pa.pd = pd; pa.OUT = d_f; pa.R = d_F; pa.coef = h->d_jac; pa.coef_stride = ne; pa.wtx = h->d_wtx; pa.wty = h->d_wty;
        pa.loss_e = d_le; pa.N = ne * NQ;
        if (h->cfg.backend == HPV_BACKEND_GENERIC || !launch_project_tp(pa, ne, h->stream)) launch_project(pa, ne, h->stream);
        hipError_t e = hipMemcpyAsync(F_out, d_F, n_out * sizeof(double), hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) rc = fail(h, -2, "hpv_assemble_rhs failed: %s", hipGetErrorString(e));
    }
    double* ptrs[] = {d_f, d_F, d_le};
    for (double* p : ptrs) if (p) (void)hipFree(p);
    return rc;
}

// Table generation on the device: the Gauss-Lobatto-Legendre rule of the drivers
// (GaussLobattoJacobiWeights(Q, 0, 0): P1:312, P2:355, P3:395) and the test-function tables (Test_fcn / dTest_fcn).
int hpv_gll_rule(hpv_handle h, int q, double* xi, double* w) {
    if (!h || !xi || !w || q < 2) return -1;
    double* d = nullptr;
    int rc = dalloc(h, &d, (size_t)2 * q);
    if (rc) return rc;
    launch_gll_rule(q, d, d + q, h->stream);
    hipError_t e = hipMemcpyAsync(xi, d, (size_t)q * sizeof(double), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(w, d + q, (size_t)q * sizeof(double), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    (void)hipFree(d);
    if (e != hipSuccess) return fail(h, -2, "hpv_gll_rule failed: %s", hipGetErrorString(e));
    return 0;
}

int hpv_test_tables(hpv_handle h, int ntest, const double* xi, int q, double* tab) {
    if (!h || !xi || !tab || ntest < 1 || q < 1) return -1;
    double* d = nullptr;
    const size_t nt = (size_t)3 * ntest * q;
    int rc = dalloc(h, &d, nt + q);
    if (rc) return rc;
    rc = upload(h, d + nt, xi, (size_t)q);
    if (!rc) {
        launch_test_tables(ntest, q, d + nt, d, h->stream);
        hipError_t e = hipMemcpyAsync(tab, d, nt * sizeof(double), hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) rc = fail(h, -2, "hpv_test_tables failed: %s", hipGetErrorString(e));
    }
    (void)hipFree(d);
    return rc;
}

int hpv_get_residuals(hpv_handle h, double* R, size_t n) {
    if (!h || !R) return -1;
    const size_t want = (size_t)h->n_elem * h->ntx * h->nty;
    if (n != want) return fail(h, -1, "R buffer has %zu entries, expected %zu", n, want);
    HIPCHK(h, hipMemcpyAsync(R, h->d_R, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}

int hpv_eval_channels(hpv_handle h, double* out, size_t n) {
    if (!h || !out) return -1;
    if (h->cfg.scheme != HPV_SCHEME_VPINN) return fail(h, -1, "hpv_eval_channels belongs to the variational scheme");
    int rc = check_ready(h);
    if (rc) return rc;
    const int C = h->nd_eval.C;
    if (n != (size_t)C * h->Nq) return fail(h, -1, "channel buffer has %zu entries, expected %zu", n, (size_t)C * h->Nq);
    if (h->Nq == 0) return 0;
    const double* src = h->var.OUT;
    if (h->eval_differs) {
        // the training pass runs on a reduced channel set: the reference's list through a forward-only launch of its own
        if (h->eval_N != h->var.N) {
            if (h->mfma_eval) { hpv_mfma_destroy(h->mfma_eval); h->mfma_eval = nullptr; }
            if ((rc = dalloc(h, &h->d_eval_out, (size_t)C * h->var.N))) return rc;
            if (h->backend == HPV_BACKEND_MFMA) h->mfma_eval = hpv_mfma_create(h->nd_eval, h->var.N, nullptr, false);
            h->eval_N = h->var.N;
        }
        if (h->mfma_eval) hpv_mfma_forward(h->mfma_eval, h->d_theta, h->var.X, h->d_eval_out, 0, h->stream);
        else launch_mlp_fwd_generic(h->nd_eval, h->d_theta, h->var.X, nullptr, h->d_eval_out, h->var.N, 0, h->stream);
        src = h->d_eval_out;
    } else {
        run_fwd(h, h->var, 0);
    }
    HIPCHK(h, hipGetLastError());
    for (int ch = 0; ch < C; ++ch)     // the device batch may carry padding / data points behind the quadrature points
        HIPCHK(h, hipMemcpyAsync(out + (size_t)ch * h->Nq, src + (size_t)ch * h->var.N, (size_t)h->Nq * sizeof(double),
                                 hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}

// Per-element refinement indicators at the current parameters (include/hpvpinn.h), all on the handle's stream, one synchronisation:
//   (1) the forward-only pass of hpv_eval_loss makes d_R current.  enqueue_pass(backward = false) never takes a whole-iteration
//       kernel (pass_whole_iteration is entered for reverse-mode passes only -- so neither SPLIT mode nor k_iter_tall can run here):
//       it is always forward -> projection, and every projection kernel (k_project, k_project_tp, k_project_wg, the row-split pair)
//       stores R of all owned elements before its forward-only return;
//   (2) one forward-only launch of the full channel set nd_full on the quadrature batch's own X;
//   (3) one k_elem_indicators launch, one workgroup per owned element;
//   (4) one copy of n_owned * HPV_IND_N doubles.
int hpv_element_indicators(hpv_handle h, const double* f_quad, size_t n, double* out, size_t n_out) {
    if (!h) return -1;
    if (h->cfg.scheme != HPV_SCHEME_VPINN) return fail(h, -1, "element indicators belong to the variational scheme");
    if (h->linear) return fail(h, -1, "the element indicators of a linear problem need its strong residual: not available");
    int rc = check_ready(h);
    if (rc) return rc;
    const long ne = h->n_elem, NQ = (long)h->qx * h->qy;
    if (f_quad && n != (size_t)(ne * NQ)) return fail(h, -1, "f has %zu entries, expected %ld", n, ne * NQ);
    if (n_out != (size_t)ne * HPV_IND_N || (ne > 0 && !out)) return fail(h, -1, "indicator buffer has %zu entries, expected %zu", n_out, (size_t)ne * HPV_IND_N);
    if (ne == 0) return 0;
    // the cached buffers are sized by three numbers, and all three are the key: d_ind_f by Nq = ne * NQ (NOT by var.N, which pads Nq
    // to 16 and adds the data points: two rules can share a var.N and differ in Nq), d_ind_out and the MFMA object by var.N, d_ind by ne
    if (h->ind_Nq != h->Nq || h->ind_N != h->var.N || h->ind_ne != ne) {
        if (h->mfma_ind) { hpv_mfma_destroy(h->mfma_ind); h->mfma_ind = nullptr; }
        h->ind_Nq = h->ind_N = h->ind_ne = -1;
        if ((rc = dalloc(h, &h->d_ind_out, (size_t)h->nd_full.C * h->var.N))) return rc;
        if ((rc = dalloc(h, &h->d_ind_f, (size_t)(ne * NQ)))) return rc;
        if ((rc = dalloc(h, &h->d_ind, (size_t)ne * HPV_IND_N))) return rc;
        if (h->backend == HPV_BACKEND_MFMA) h->mfma_ind = hpv_mfma_create(h->nd_full, h->var.N, nullptr, false);
        h->ind_Nq = h->Nq; h->ind_N = h->var.N; h->ind_ne = ne;
    }
    if (f_quad) HIPCHK(h, hipMemcpyAsync(h->d_ind_f, f_quad, n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if ((rc = enqueue_pass(h, false))) return rc;
    if (h->mfma_ind) hpv_mfma_forward(h->mfma_ind, h->d_theta, h->var.X, h->d_ind_out, 0, h->stream);
    else launch_mlp_fwd_generic(h->nd_full, h->d_theta, h->var.X, nullptr, h->d_ind_out, h->var.N, 0, h->stream);
    const IndArgs a{h->d_ind_out, h->var.N, f_quad ? h->d_ind_f : nullptr, h->has_eps ? h->d_theta + h->P : nullptr, h->cfg.V,
                    h->d_wq, h->d_wq + h->qx, h->qx, h->qy, h->d_jac, h->d_R, h->ntx, h->nty, h->pd.nact, h->pd.nacty, h->d_ind};
    launch_elem_indicators(h->cfg.pde, a, ne, h->stream);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(out, h->d_ind, n_out * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}

// The strong form of a linear handle, opted into (include/hpvpinn.h): the differentiation matrices of the current rule, kept on the
// device for k_lin_indicators alone.  No pass reads them, so the captured iteration graphs stay.
int hpv_set_strong_form(hpv_handle h, const double* Dx, size_t nx, const double* Dy, size_t ny) {
    if (!h) return -1;
    if (!h->linear) return fail(h, -1, "hpv_set_strong_form belongs to the linear problems (HPV_PDE_LINEAR1D / _LINEAR2D)");
    if (!Dx && !Dy && nx == 0 && ny == 0) {
        if (h->d_sf) { HIPCHK(h, hipStreamSynchronize(h->stream)); (void)hipFree(h->d_sf); h->d_sf = nullptr; }
        return 0;
    }
    if (has_ansatz(h)) return fail(h, -1, "the handle has an ansatz (hpv_set_ansatz): its strong residual needs second derivatives of G and D, which are not available");
    if (h->lin_tensor) return fail(h, -1, "the operator is a full tensor (hpv_set_operator_tensor): its strong form needs u_xy, which is not available");
    if (h->unit_elems) return fail(h, -1, "the elements are mapped (hpv_set_element_points): the strong form is not available on them");
    if (h->d_sfd || h->sfd_stale) return fail(h, -1, "the divergence form is active (hpv_set_strong_form_div): remove it first, the two kinds exclude each other");
    if (!h->have_quad) return fail(h, -3, "call hpv_set_quadrature first");
    const size_t wx = (size_t)h->qx * h->qx, wy = h->dim == 2 ? (size_t)h->qy * h->qy : 0;
    if (!Dx || nx != wx) return fail(h, -1, "Dx has %zu entries, expected %d x %d of the current rule", nx, h->qx, h->qx);
    if (h->dim == 1 ? (Dy || ny != 0) : (!Dy || ny != wy))
        return fail(h, -1, "Dy has %zu entries, expected %zu (1-D: NULL and 0; 2-D: %d x %d of the current rule)", ny, wy, h->qy, h->qy);
    for (size_t i = 0; i < wx; ++i)
        if (!std::isfinite(Dx[i])) return fail(h, -1, "Dx holds a non-finite value at entry %zu", i);
    for (size_t i = 0; i < wy; ++i)
        if (!std::isfinite(Dy[i])) return fail(h, -1, "Dy holds a non-finite value at entry %zu", i);
    const size_t lds = hpv_linadapt_lds_bytes(h->dim, h->qx, h->qy);
    if (lds > 64 * 1024) return fail(h, -1, "rule too large for the linear indicator kernel's LDS (%zu B)", lds);
    int rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if ((rc = dalloc(h, &h->d_sf, wx + wy))) return rc;
    h->ind_Nq = h->ind_N = h->ind_ne = -1;      // (the indicator buffers of the divergence kind hold no channel list)
    if ((rc = upload(h, h->d_sf, Dx, wx))) return rc;
    if (wy && (rc = upload(h, h->d_sf + wx, Dy, wy))) return rc;
    return 0;
}

// The strong form in divergence form (include/hpvpinn.h): the same matrices and, on unit elements, 1 / det A at the owned points,
// kept on the device for k_div_indicators alone.  No pass reads them, so the captured iteration graphs stay.
int hpv_set_strong_form_div(hpv_handle h, const double* Dx, size_t nx, const double* Dy, size_t ny, const double* inv_det, size_t n_det) {
    if (!h) return -1;
    if (!h->linear) return fail(h, -1, "hpv_set_strong_form_div belongs to the linear problems (HPV_PDE_LINEAR1D / _LINEAR2D)");
    if (!Dx && !Dy && !inv_det && nx == 0 && ny == 0 && n_det == 0) {
        if (h->d_sfd) { HIPCHK(h, hipStreamSynchronize(h->stream)); drop_strong_form_div(h); }
        h->sfd_stale = false;
        return 0;
    }
    if (h->d_sf) return fail(h, -1, "the elementwise strong form is active (hpv_set_strong_form): remove it first, the two kinds exclude each other");
    if (!h->have_quad) return fail(h, -3, "call hpv_set_quadrature first");
    if (!h->have_elems) return fail(h, -3, "call hpv_set_elements first (1 / det A belongs to the elements)");
    const size_t wx = (size_t)h->qx * h->qx, wy = h->dim == 2 ? (size_t)h->qy * h->qy : 0;
    if (!Dx || nx != wx) return fail(h, -1, "Dx has %zu entries, expected %d x %d of the current rule", nx, h->qx, h->qx);
    if (h->dim == 1 ? (Dy || ny != 0) : (!Dy || ny != wy))
        return fail(h, -1, "Dy has %zu entries, expected %zu (1-D: NULL and 0; 2-D: %d x %d of the current rule)", ny, wy, h->qy, h->qy);
    const size_t nd = h->unit_elems ? (size_t)h->Nq : 0;
    if (h->unit_elems ? (!inv_det || n_det != nd) : (inv_det || n_det != 0))
        return fail(h, -1, "inv_det has %zu entries, expected %zu (boxes: NULL and 0; unit elements: 1 / det A at the n_owned * qx * qy points)", n_det, nd);
    for (size_t i = 0; i < wx; ++i)
        if (!std::isfinite(Dx[i])) return fail(h, -1, "Dx holds a non-finite value at entry %zu", i);
    for (size_t i = 0; i < wy; ++i)
        if (!std::isfinite(Dy[i])) return fail(h, -1, "Dy holds a non-finite value at entry %zu", i);
    for (size_t i = 0; i < nd; ++i)
        if (!std::isfinite(inv_det[i]) || !(inv_det[i] > 0.0)) return fail(h, -1, "inv_det is not finite and > 0 at point %zu", i);
    const size_t lds = hpv_div_lds_bytes(h->dim, h->qx, h->qy);
    if (lds > 64 * 1024) return fail(h, -1, "rule too large for the divergence-form indicator kernel's LDS (%zu B)", lds);
    int rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if ((rc = dalloc(h, &h->d_sfd, wx + wy))) return rc;
    if ((rc = upload(h, h->d_sfd, Dx, wx))) return rc;
    if (wy && (rc = upload(h, h->d_sfd + wx, Dy, wy))) return rc;
    if ((rc = dalloc(h, &h->d_inv_det, nd))) return rc;
    if (nd && (rc = upload(h, h->d_inv_det, inv_det, nd))) return rc;
    h->sfd_stale = false;
    h->ind_Nq = h->ind_N = h->ind_ne = -1;      // (the indicator buffers of the other kind hold the full channel list)
    return 0;
}

// hpv_linear_indicators with the divergence form set; its sequence, on the handle's stream with one synchronisation:
//   (1) enqueue_pass(backward = false): forward -> (k_ansatz_fwd) -> k_project_lin | _nl | _id, which stores R and loss_e of all owned
//       elements and leaves u, u_x[, u_y] -- post-ansatz -- in the quadrature batch's OUT;
//   (2) one k_div_indicators launch on exactly those channels: no further forward launch, and no nd_full object;
//   (3) one copy of n_owned * HPV_IND_N doubles, and one of the strong residual where the caller asks.
static int div_indicators(hpv_ctx* h, const double* f_quad, size_t n, double* out, size_t n_out, double* r_out, size_t n_r) {
    if (!h->d_sfd) return fail(h, -3, "new elements or a new rule have orphaned the divergence form: hand the strong form over again (hpv_set_strong_form_div)");
    int rc = check_ready(h);
    if (rc) return rc;
    const long ne = h->n_elem, NQ = (long)h->qx * h->qy;
    if (f_quad && n != (size_t)(ne * NQ)) return fail(h, -1, "f has %zu entries, expected %ld", n, ne * NQ);
    if (n_out != (size_t)ne * HPV_IND_N || (ne > 0 && !out)) return fail(h, -1, "indicator buffer has %zu entries, expected %zu", n_out, (size_t)ne * HPV_IND_N);
    if (r_out && n_r != (size_t)(ne * NQ)) return fail(h, -1, "residual buffer has %zu entries, expected %ld", n_r, ne * NQ);
    if (ne == 0) return 0;
    // d_ind_f and d_ind under hpv_element_indicators' key; the full-channel buffer and its object are not needed and not made (both
    // hpv_set_strong_form* calls reset the key, so the elementwise kind never finds it without them)
    if (h->ind_Nq != h->Nq || h->ind_N != h->var.N || h->ind_ne != ne) {
        if (h->mfma_ind) { hpv_mfma_destroy(h->mfma_ind); h->mfma_ind = nullptr; }
        h->ind_Nq = h->ind_N = h->ind_ne = -1;
        if ((rc = dalloc(h, &h->d_ind_out, 0))) return rc;
        if ((rc = dalloc(h, &h->d_ind_f, (size_t)(ne * NQ)))) return rc;
        if ((rc = dalloc(h, &h->d_ind, (size_t)ne * HPV_IND_N))) return rc;
        h->ind_Nq = h->Nq; h->ind_N = h->var.N; h->ind_ne = ne;
    }
    if (r_out && h->ind_r_n != h->Nq) {
        h->ind_r_n = -1;
        if ((rc = dalloc(h, &h->d_ind_r, (size_t)(ne * NQ)))) return rc;
        h->ind_r_n = h->Nq;
    }
    if (f_quad) HIPCHK(h, hipMemcpyAsync(h->d_ind_f, f_quad, n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if ((rc = enqueue_pass(h, false))) return rc;
    const int terms_mask = h->nl_mask | (h->n_coef ? h->dir_nl_mask : 0);      // (what pass_linear hands its projection kernel)
    const size_t wx = (size_t)h->qx * h->qx;
    LinIndArgs a{};
    a.OUT = h->var.OUT; a.N = h->var.N; a.f = f_quad ? h->d_ind_f : nullptr;
    a.coef = h->d_lin; a.cs = h->Nq;
    a.nl = h->nl_mask ? h->d_nl : (h->n_coef ? h->d_nl_zero : nullptr); a.mask = terms_mask | h->q_mask;
    a.qp = h->q_mask ? h->d_qp : nullptr; a.qr = h->q_exp;      // (hpv_set_quasilinear: the QUASI instantiation)
    a.dirs = h->n_coef ? h->d_dirs : nullptr; a.c = h->d_theta + h->P + h->has_eps; a.n_coef = h->n_coef; a.dmask = h->d_dir_mask;
    a.Dx = h->d_sfd; a.Dy = h->dim == 2 ? h->d_sfd + wx : nullptr;
    a.wx = h->d_wq; a.wy = h->d_wq + h->qx;
    a.J = h->d_jac; a.Jx = h->d_jxy; a.Jy = h->d_jxy + h->n_elem;
    a.R = h->d_R; a.nact = h->pd.nact; a.nacty = h->pd.nacty;
    a.out = h->d_ind; a.r_out = r_out ? h->d_ind_r : nullptr;
    a.qx = h->qx; a.qy = h->qy; a.ntx = h->ntx; a.nty = h->nty; a.dim = h->dim;
    a.loss_e = (h->d_dual || h->d_gram) ? h->d_loss_e : nullptr;
    a.inv_det = h->d_inv_det; a.tensor = h->lin_tensor ? 1 : 0;
    launch_div_indicators(a, ne, h->stream);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(out, h->d_ind, n_out * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (r_out) HIPCHK(h, hipMemcpyAsync(r_out, h->d_ind_r, n_r * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}

// hpv_element_indicators for a linear handle with the strong form set; its sequence, its cached buffers under their three-number key:
//   (1) enqueue_pass(backward = false): forward -> k_project_lin | _nl | _id, which stores R of all owned elements;
//   (2) one forward-only launch of nd_full on the quadrature batch's own X;
//   (3) one k_lin_indicators launch, one workgroup per owned element;
//   (4) one copy of n_owned * HPV_IND_N doubles, and one of the strong residual where the caller asks; one synchronisation.
int hpv_linear_indicators(hpv_handle h, const double* f_quad, size_t n, double* out, size_t n_out, double* r_out, size_t n_r) {
    if (!h) return -1;
    if (!h->linear) return fail(h, -1, "hpv_linear_indicators belongs to the linear problems (others: hpv_element_indicators)");
    if (h->d_sfd || h->sfd_stale) return div_indicators(h, f_quad, n, out, n_out, r_out, n_r);
    if (h->q_mask || h->q_stale)
        return fail(h, -3, "the quasilinear term is set (hpv_set_quasilinear): the elementwise strong residual would need the derivative of mu along the element; the divergence form (hpv_set_strong_form_div) carries it");
    if (h->lin_tensor) return fail(h, -1, "the operator is a full tensor (hpv_set_operator_tensor): its strong residual needs u_xy, which is not available");
    if (h->unit_elems) return fail(h, -1, "the elements are mapped (hpv_set_element_points): the strong residual is not available on them");
    if (!h->d_sf) return fail(h, -1, "the strong residual of a linear problem needs the rule's differentiation matrices: call hpv_set_strong_form");
    int rc = check_ready(h);
    if (rc) return rc;
    const long ne = h->n_elem, NQ = (long)h->qx * h->qy;
    if (f_quad && n != (size_t)(ne * NQ)) return fail(h, -1, "f has %zu entries, expected %ld", n, ne * NQ);
    if (n_out != (size_t)ne * HPV_IND_N || (ne > 0 && !out)) return fail(h, -1, "indicator buffer has %zu entries, expected %zu", n_out, (size_t)ne * HPV_IND_N);
    if (r_out && n_r != (size_t)(ne * NQ)) return fail(h, -1, "residual buffer has %zu entries, expected %ld", n_r, ne * NQ);
    const size_t lds = hpv_linadapt_lds_bytes(h->dim, h->qx, h->qy);
    if (lds > 64 * 1024) return fail(h, -1, "rule too large for the linear indicator kernel's LDS (%zu B)", lds);
    if (ne == 0) return 0;
    if (h->ind_Nq != h->Nq || h->ind_N != h->var.N || h->ind_ne != ne) {      // (the key of hpv_element_indicators)
        if (h->mfma_ind) { hpv_mfma_destroy(h->mfma_ind); h->mfma_ind = nullptr; }
        h->ind_Nq = h->ind_N = h->ind_ne = -1;
        if ((rc = dalloc(h, &h->d_ind_out, (size_t)h->nd_full.C * h->var.N))) return rc;
        if ((rc = dalloc(h, &h->d_ind_f, (size_t)(ne * NQ)))) return rc;
        if ((rc = dalloc(h, &h->d_ind, (size_t)ne * HPV_IND_N))) return rc;
        if (h->backend == HPV_BACKEND_MFMA) h->mfma_ind = hpv_mfma_create(h->nd_full, h->var.N, nullptr, false);
        h->ind_Nq = h->Nq; h->ind_N = h->var.N; h->ind_ne = ne;
    }
    if (r_out && h->ind_r_n != h->Nq) {
        h->ind_r_n = -1;
        if ((rc = dalloc(h, &h->d_ind_r, (size_t)(ne * NQ)))) return rc;
        h->ind_r_n = h->Nq;
    }
    if (f_quad) HIPCHK(h, hipMemcpyAsync(h->d_ind_f, f_quad, n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if ((rc = enqueue_pass(h, false))) return rc;
    if (h->mfma_ind) hpv_mfma_forward(h->mfma_ind, h->d_theta, h->var.X, h->d_ind_out, 0, h->stream);
    else launch_mlp_fwd_generic(h->nd_full, h->d_theta, h->var.X, nullptr, h->d_ind_out, h->var.N, 0, h->stream);
    const int terms_mask = h->nl_mask | (h->n_coef ? h->dir_nl_mask : 0);      // (what pass_linear hands its projection kernel)
    const size_t wx = (size_t)h->qx * h->qx;
    LinIndArgs a{};
    a.OUT = h->d_ind_out; a.N = h->var.N; a.f = f_quad ? h->d_ind_f : nullptr;
    a.coef = h->d_lin; a.cs = h->Nq;
    a.nl = h->nl_mask ? h->d_nl : (h->n_coef ? h->d_nl_zero : nullptr); a.mask = terms_mask;
    a.dirs = h->n_coef ? h->d_dirs : nullptr; a.c = h->d_theta + h->P + h->has_eps; a.n_coef = h->n_coef; a.dmask = h->d_dir_mask;
    a.Dx = h->d_sf; a.Dy = h->dim == 2 ? h->d_sf + wx : nullptr;
    a.wx = h->d_wq; a.wy = h->d_wq + h->qx;
    a.J = h->d_jac; a.Jx = h->d_jxy; a.Jy = h->d_jxy + h->n_elem;
    a.R = h->d_R; a.nact = h->pd.nact; a.nacty = h->pd.nacty;
    a.out = h->d_ind; a.r_out = r_out ? h->d_ind_r : nullptr;
    a.qx = h->qx; a.qy = h->qy; a.ntx = h->ntx; a.nty = h->nty; a.dim = h->dim;
    a.loss_e = (h->d_dual || h->d_gram) ? h->d_loss_e : nullptr;      // (hpv_set_residual_norm | _gram: column 0 is the loss the pass above wrote)
    launch_lin_indicators(a, ne, h->stream);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(out, h->d_ind, n_out * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (r_out) HIPCHK(h, hipMemcpyAsync(r_out, h->d_ind_r, n_r * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}

#if defined(HPV_FZ_TIMING) || defined(HPV_PJ_TIMING)
// (debug hook of the timing builds only -- scripts/fz_timing.py, scripts/pj_timing.py: raw read of the adjoint channel buffer /
//  the activation store the instrumented kernels stamp)
int hpv_debug_read_out(hpv_handle h, double* out, size_t n) {
    if (!h || !out || !h->var.GBAR) return -1;
    const double* src = h->var.GBAR;
    size_t have = (size_t)h->nd_var.C * (size_t)h->var.N;
    if (getenv("HPV_DEBUG_READ_STORE") && h->var.m && hpv_mfma_activation_store(h->var.m)) {
        src = hpv_mfma_activation_store(h->var.m);
        have = hpv_mfma_activation_store_doubles(h->var.m);
    }
    if (getenv("HPV_DEBUG_READ_CHANNELS") && h->var.OUT) { src = h->var.OUT; have = (size_t)h->nd_var.C * (size_t)h->var.N; }
    if (n > have) return fail(h, -1, "debug read of %zu doubles from a buffer of %zu", n, have);
    return hipMemcpy(out, src, n * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess ? 0 : -2;
}
#endif
int hpv_pass_structure(hpv_handle h) { return h ? h->pass_structure : -1; }
int hpv_kernel_variant(hpv_handle h, char* buf, size_t n) {
    if (!h || !buf || n == 0) return -1;
    snprintf(buf, n, "%s", h->variant);
    return 0;
}
const char* hpv_build_info(void) {
    static std::string info;
    static std::once_flag once;
    std::call_once(once, [] {
        info = std::string("k_iter_fused=") + hpv_fused_build_state() + ";k_iter_fused_gen=" + hpv_fused_gen_build_state() +
               ";k_iter_tall=" + hpv_tall_build_state() + ";test_hooks=";
#ifdef HPV_TEST_HOOKS
        info += "1";
#else
        info += "0";
#endif
    });
    return info.c_str();
}
static int device_cus(int device) {      // 256 when no device can be queried
    hipDeviceProp_t prop;
    if (device >= 0 && hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) return prop.multiProcessorCount;
    (void)hipGetLastError();
    return 256;
}
int hpv_rule_advice(int device, int pde, int var_form, int n_hidden, int max_width, int q, int ntx, int nty, long n_elem_shard, int* q_dev, int* nt_dev) {
    ProjDesc pd;
    NetDesc nd{};
    bool mixed;
    if (!q_dev || !nt_dev || q < 1 || ntx < 1 || n_elem_shard < 0 || form_terms(pde, var_form, 1.0, pd, nd.nT1, nd.nT2, mixed)) return -1;
    *q_dev = q; *nt_dev = ntx;
    if (pde == HPV_PDE_LINEAR1D || pde == HPV_PDE_LINEAR2D) return 0;      // forward -> k_project_lin -> reverse takes any rule as it is
    const int n_cus = device_cus(device);
    const bool net20 = max_width <= 20 && n_hidden >= 2;       // the element-resident kernels are written for 20-wide layers
    if (pde == HPV_PDE_POISSON1D) {                   // kernels_tile.hip: 80 points / 60 test functions (P1:237-238), var_form 1 / 2, 2-4 hidden layers
        if (var_form == 3 || !net20 || n_hidden > 4 || q > 80 || ntx > 60) return 0;
        if (q == 80) { *nt_dev = 60; return 0; }      // fewer test functions: the first 60, per-element counts
        if (n_elem_shard <= hpv_rule1d_pad_max(q, n_cus) && n_elem_shard <= hpv_elem_resident_max(1, 80, n_cus)) { *q_dev = 80; *nt_dev = 60; }
        return 0;
    }
    if (pde == HPV_PDE_ADVDIFF && q <= 10) {          // kernels_tile.hip: 10x10 points, exactly 5x5 test functions (no run-time counts)
        if (net20 && n_hidden <= 3 && ntx == 5 && nty == 5 && n_elem_shard <= hpv_elem_resident_max(2, 10, n_cus)) *q_dev = 10;
        return 0;
    }
    // k_iter_small / k_iter_fused: pad only while ONE WORKGROUP PER ELEMENT of the next rule's kernel takes the shard -- where the element
    // loop (plan 2) or the separate launches (declined) take the grid, the padded points cost more than the structure saves
    nd.d = 2; nd.act = HPV_ACT_TANH;                  // the 2-D classes' networks (P2:165, P3:226)
    FusedShard in;
    in.nd = &nd; in.L = n_hidden; in.n_cus = n_cus; in.n_elem = n_elem_shard;
    in.H = max_width < 20 ? 20 : max_width;           // (narrower networks get the 20-wide answer, as they always have: DESIGN.md 8)
    in.loop_any_form = true;                          // (the general forms never run the loop, yet the advice has always planned with it: DESIGN.md 8)
    int q_rule;
    const FusedPlan p = hpv_fused_plan_rule(in, pd, q, ntx, nty, &q_rule);
    if (!p.declined && (p.gplan == 1 || p.gplan == 3)) *q_dev = q_rule;
    return 0;
}
int hpv_grid_plan(int device, int q, int n_hidden, long n_elem_shard) {
    ProjDesc pd;
    NetDesc nd{};
    bool mixed;
    (void)form_terms(HPV_PDE_POISSON2D, 1, 1.0, pd, nd.nT1, nd.nT2, mixed);
    nd.d = 2; nd.act = HPV_ACT_TANH;
    FusedShard in;
    in.nd = &nd; in.H = 20; in.L = n_hidden; in.n_cus = device_cus(device); in.n_elem = n_elem_shard;
    int q_rule;
    const FusedPlan p = hpv_fused_plan_rule(in, pd, q, 1, 1, &q_rule);
    if (q_rule != q || p.small || n_hidden < 2 || n_hidden > 3 || n_elem_shard < 1) return -1;
    return p.declined ? 0 : p.gplan;
}
int hpv_updates_applied(hpv_handle h, long long* n) {
    if (!h || !n) return -1;
    unsigned long long v = 0;
    HIPCHK(h, hipMemcpyAsync(&v, h->d_nupd, sizeof(v), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    *n = (long long)v;
    return 0;
}
int hpv_shared_element_kernels(hpv_handle h) { return !h ? -1 : (h->shared_elem_ok ? 1 : 0); }
int hpv_set_shared_element_kernels(hpv_handle h, int on) {
    if (!h) return -1;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->shared_elem_ok = on != 0;
    if (h->var.m) hpv_mfma_set_split_ok(h->var.m, h->shared_elem_ok);
    drop_graph(h);      // captured iterations hold the launch structure chosen before
    return 0;
}
int hpv_graphs_in_use(hpv_handle h) { return !h ? -1 : ((h->use_graph && h->own_stream && (h->g_stepK || h->g_rem[1] || h->g_rem[2] || h->g_rem[3] || h->g_rem[4] || h->g_rem[5] || h->g_rem[6] || h->g_rem[7])) ? 1 : 0); }
int hpv_backend_in_use(hpv_handle h) {
    if (!h) return -1;
    if (h->cfg.scheme == HPV_SCHEME_VPINN && h->have_quad && h->have_tables && h->have_elems && h->batch_dirty) {
        int rc = assemble_batches(h);   // decides the backend; surfaces "MFMA not available" early
        if (rc) return rc;
    }
    return h->backend;
}

}  // extern "C"
