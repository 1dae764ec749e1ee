// The pass engine of libhpvpinn.so: one pass over the loss terms of a handle (variational or strong-form scheme, the boundary/data and
// flux terms, k_finalize), the pass with its multi-GPU exchange, and sequences of training iterations as captured graphs.  The C-ABI
// (hpv_api.hip) calls in through the entry points declared in hpv_ctx.h; everything else here is local to this unit.
#include "hpv_ctx.h"

namespace hpvd {

static void tstart(hpv_ctx* h, int which) {
    if (!h->timing) return;
    TimerClass& t = h->timers[which];
    if (t.used + 2 > t.ev.size()) {
        size_t old = t.ev.size();
        t.ev.resize(old + 512);
        for (size_t i = old; i < t.ev.size(); ++i) (void)hipEventCreate(&t.ev[i]);
    }
    (void)hipEventRecord(t.ev[t.used], h->stream);
}
static void tstop(hpv_ctx* h, int which) {
    if (!h->timing) return;
    TimerClass& t = h->timers[which];
    (void)hipEventRecord(t.ev[t.used + 1], h->stream);
    t.used += 2;
    t.launches += 1;
    if (t.used >= 4096) {  // flush
        (void)hipStreamSynchronize(h->stream);
        for (size_t i = 0; i < t.used; i += 2) { float ms = 0; (void)hipEventElapsedTime(&ms, t.ev[i], t.ev[i + 1]); t.total_ms += ms; }
        t.used = 0;
    }
}

// forward / reverse launch over a batch: its own MFMA object where it has one, the generic kernels otherwise
void run_fwd(hpv_ctx* h, Batch& b, int save_act) {
    if (b.N == 0) return;
    if (b.m) hpv_mfma_forward(b.m, h->d_theta, b.X, b.OUT, save_act, h->stream);
    else launch_mlp_fwd_generic(b.nd, h->d_theta, b.X, b.ACT, b.OUT, b.N, save_act, h->stream);
}
static void run_bwd(hpv_ctx* h, Batch& b) {
    if (b.N == 0) return;
    if (b.m) hpv_mfma_backward(b.m, h->d_theta, b.X, b.GBAR, b.GPART, &b.rows, h->stream);
    else launch_mlp_bwd_generic(b.nd, h->d_theta, b.X, b.ACT, b.GBAR, b.GPART, b.rows, b.N, h->stream);
}

// ---- the ansatz u = G + D N of a point set (hpv_set_ansatz): k_ansatz_fwd behind the batch's forward launch, k_ansatz_adj in front of its
// reverse launch, on the first n points of the batch (padding behind them carries zero adjoints and is left alone) ----
void ansatz_fwd(hpv_ctx* h, int which, Batch& b, long n) {
    if (h->d_ans[which]) launch_ansatz_fwd(b.OUT, b.N, 0, std::min(n, h->ans_n[which]), h->dim, b.nd.C, h->d_ans[which], h->stream);
}
void ansatz_adj(hpv_ctx* h, int which, Batch& b, long n) {
    if (h->d_ans[which]) launch_ansatz_adj(b.GBAR, b.N, 0, std::min(n, h->ans_n[which]), h->dim, b.nd.C, h->d_ans[which], h->stream);
}
int ansatz_ready(hpv_ctx* h, int which) {
    // (the sets by their short names: tests/test_cabi.py counts the HPV_* words of the binary as environment switches)
    static const char* const names[] = {"set QUAD (the quadrature points)", "set DATA (the boundary / data points)",
                                        "set FLUX (the flux points)", "set VALID (the validation set)"};
    const long count[] = {h->Nq, (long)h->n_data, (long)h->n_flux, (long)h->n_val};
    if (!has_ansatz(h) || count[which] == 0 || (h->ans_on[which] && h->ans_n[which] == count[which])) return 0;
    return fail(h, -3, "the handle has an ansatz but no planes for %s: hpv_set_ansatz has not been called for this set", names[which]);
}

// A batch apart from the quadrature batch (boundary/data points, element edges, flux points, collocation points) moves to the MFMA
// kernels where they take its shape; its generic activation store is dropped.  required: staying on the generic kernels is an error.
static int ensure_small_mfma(hpv_ctx* h, Batch& b, bool required = false) {
    if (b.m || b.N == 0) return 0;
    std::string why;
    b.m = hpv_mfma_create(b.nd, b.N, &why);
    if (!b.m) return required ? fail(h, -4, "MFMA backend not available: %s", why.c_str()) : 0;
    if (b.ACT) { (void)hipFree(b.ACT); b.ACT = nullptr; }
    int rows = hpv_mfma_grad_rows(b.m);
    if (rows > b.rows) { int rc = dalloc(h, &b.GPART, (size_t)rows * h->P); if (rc) return rc; }
    b.rows = rows;
    return 0;
}

// Every such batch of the handle's scheme, outside any stream capture (creating an object allocates).  The collocation batch leads
// its scheme as the quadrature batch leads the variational one (assemble_batches): where it gets an object the handle is on the MFMA
// backend, and the other batches follow only then.
static int ensure_small_batches(hpv_ctx* h) {
    int rc;
    const bool pinn = h->cfg.scheme == HPV_SCHEME_PINN;
    if (pinn && h->cfg.backend != HPV_BACKEND_GENERIC) {
        if ((rc = ensure_small_mfma(h, h->colloc, h->cfg.backend == HPV_BACKEND_MFMA))) return rc;
        if (h->colloc.m) h->backend = HPV_BACKEND_MFMA;
    }
    if (h->backend != HPV_BACKEND_MFMA) return 0;
    if ((rc = ensure_small_mfma(h, h->data))) return rc;
    if (!pinn && h->pd.edge && (rc = ensure_small_mfma(h, h->edge))) return rc;
    return h->n_flux > 0 ? ensure_small_mfma(h, h->flux) : 0;
}

// ---- the flux term of a pass: forward over its batch, k_flux_loss, reverse (same sequence in both schemes) ----
static void pass_flux(hpv_ctx* h, bool backward) {
    if (h->n_flux <= 0) return;
    run_fwd(h, h->flux, backward ? 1 : 0);
    ansatz_fwd(h, HPV_ANSATZ_FLUX, h->flux, h->n_flux);
    launch_flux_loss(h->flux.OUT, h->flux.N, h->dim, h->d_flux_coef, h->d_flux_g, backward ? h->flux.GBAR : nullptr,
                     2.0 * h->w_flux / (double)h->n_flux, h->d_flux_part, h->n_flux, h->stream);
    if (backward) { ansatz_adj(h, HPV_ANSATZ_FLUX, h->flux, h->n_flux); run_bwd(h, h->flux); }
}
static FluxFin flux_fin(hpv_ctx* h, bool backward) {
    if (h->n_flux <= 0) return FluxFin{};
    return FluxFin{backward ? h->flux.GPART : nullptr, h->flux.rows, h->d_flux_part, flux_loss_parts(h->n_flux), h->w_flux, h->n_flux,
                   h->d_flux_part + 64};
}

static AdamArgs adam_args(hpv_ctx* h) {
    return AdamArgs{h->d_theta, h->d_m, h->d_v, h->d_state, h->cfg.lr, h->cfg.beta1, h->cfg.beta2, h->cfg.eps,
                    h->d_hist, h->d_hist_idx, HPV_HIST_CAP, h->d_xerr, h->d_nupd};
}
// k_adam on the reduced gradient in the packed buffer
void enqueue_adam(hpv_ctx* h) { launch_adam(adam_args(h), h->d_RB, h->P, h->Ptot, h->stream); }

// behind the launches of a step: "<what> failed: <HIP's error>" with -2 if one of them was refused
int launch_check(hpv_ctx* h, const char* what) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : fail(h, -2, "%s failed: %s", what, hipGetErrorString(e));
}

// ---- the boundary / data term on a batch of its own: forward, k_data_loss, reverse; returns the number of loss partials ----
static int pass_data(hpv_ctx* h, bool backward) {
    run_fwd(h, h->data, backward ? 1 : 0);
    ansatz_fwd(h, HPV_ANSATZ_DATA, h->data, h->n_data);
    launch_data_loss(h->data.OUT, h->d_udata, backward ? h->data.GBAR : nullptr, -2.0 * h->cfg.lossb_weight / (double)h->n_data,
                     h->d_data_part, h->n_data, h->stream);
    if (backward) { ansatz_adj(h, HPV_ANSATZ_DATA, h->data, h->n_data); run_bwd(h, h->data); }
    return data_loss_parts(h->n_data);
}

// what both schemes hand to k_finalize alike: the data term (n_data_part partials; rows of its own batch unless it rode in the merged
// one), the flux term, the packed buffer, the update when the pass ends a single-GPU training iteration
static FinalizeArgs pass_finalize_args(hpv_ctx* h, bool backward, int n_data_part, bool fuse_adam) {
    FinalizeArgs a{};
    a.g[1] = {backward && h->n_data > 0 && !h->merged ? h->data.GPART : nullptr, h->data.rows};
    a.data_part = h->d_data_part; a.n_data_part = n_data_part; a.lossb_weight = h->cfg.lossb_weight; a.n_data = h->n_data;
    a.P = h->P; a.has_eps = h->has_eps; a.n_coef = h->n_coef; a.dcoef_e = h->n_mom ? h->d_mom_dcoef : h->d_dcoef_e; a.RB = h->d_RB; a.write_grad = backward ? 1 : 0;
    if (backward && fuse_adam) a.adam = adam_args(h);
    a.fx = flux_fin(h, backward);
    return a;
}

static int enqueue_pinn_pass(hpv_ctx* h, bool backward, bool fuse_adam);

// the boundary / data term as the merged kernels see it, the projection arguments of the quadrature batch (edge: with the element-edge
// batch's pointers, for the stand-alone projection kernels that integrate that term) and the pass over that batch as the MFMA launch
// functions take it (one definition for enqueue_pass and the stand-alone timing of the iteration kernel)
MfmaDataTerm pass_data_term(hpv_ctx* h, bool backward) {
    return MfmaDataTerm{h->data_off, h->merged ? h->n_data : 0, h->d_udata, h->var.GBAR, h->d_data_part,
                        h->n_data > 0 ? -2.0 * h->cfg.lossb_weight / (double)h->n_data : 0.0, backward ? 1 : 0};
}
ProjArgs pass_proj_args(hpv_ctx* h, bool backward, bool edge) {
    const double* eps_ptr = h->has_eps ? h->d_theta + h->P : nullptr;
    ProjArgs pa{h->pd, h->var.OUT, h->var.GBAR, h->d_R, h->d_F, h->d_coef, h->n_elem, h->d_wtx, h->d_wty, eps_ptr,
                h->d_loss_e, h->d_deps_e, h->var.N, backward ? 1 : 0, nullptr, nullptr, nullptr, nullptr};
    if (edge) { pa.edge_u = h->edge.OUT; pa.edge_dphi = h->d_edge_dphi; pa.edge_coef = h->d_edge_coef; pa.edge_gbar = h->edge.GBAR; }
    return pa;
}
MfmaPass pass_mfma(hpv_ctx* h, const MfmaDataTerm& dt, const ProjArgs& pa) {
    return MfmaPass{h->d_theta, h->var.X, h->var.GBAR, h->var.GPART, &h->var.rows, h->stream, &dt, &pa, h->n_elem};
}

// ---- one pass over both loss terms ------------------------------------------------------------------------------------------
// What a pass did (hpv_pass_structure / hpv_kernel_variant report structure and names): filled while the pass walks its plan.
struct PassPlan {
    long n_loss;             // loss_e / deps_e entries the pass wrote
    bool fin_done = false;   // the whole-iteration tile kernel ran the finalize step itself
    bool xch_used = false;   // a shared-element kernel (SPLIT mode, k_iter_tall) ran: k_finalize advances the exchange's launch counter
    bool pend_taken = false; // the deferred TF1-Adam update rode in k_iter_fused's prologue: k_finalize stores it
};

// (1) The variational term as ONE launch -- the element-resident whole-iteration kernels, tried in the order of their speed on the
// shapes they take (each declines what it does not cover): k_iter_fused (two-term / general forms on 12x12, 16x16, 20x20 points;
// takes a deferred update `pend` into its prologue), k_iter_tile (one tile per wave: 1-D rules, 10x10 points; a one-workgroup grid
// finishes the iteration itself), k_iter_elem (any instantiated shape / channel set; first with HPV_FUSE=e), k_iter_tall (80x80
// points).  Timed as the reverse-pass class.  false: nothing was launched.
static bool pass_whole_iteration(hpv_ctx* h, const MfmaPass& p, bool fuse_adam, bool& pend, PassPlan& pl) {
    HpvMfma* m = h->var.m;
    int structure = -1;
    tstart(h, 2);
    if (pend) {      // the deferred update rides in k_iter_fused's prologue -- or is applied here, before anything else is launched
        const MfmaPendingAdam pre{adam_args(h), h->d_RB, h->Ptot};
        if (hpv_mfma_iter_fused(m, p, &pre)) { pl.pend_taken = true; structure = hpv_mfma_sync_failed_possible(m) ? 3 : 2; }
        else enqueue_adam(h);
        pend = false;
    }
    if (structure < 0 && hpv_mfma_prefers_elem(m) && hpv_mfma_iter_elem(m, p)) structure = 6;      // HPV_FUSE=e (A/B runs): the generic element-resident kernel first
    if (structure < 0 && hpv_mfma_iter_fused(m, p)) structure = hpv_mfma_sync_failed_possible(m) ? 3 : 2;
    if (structure < 0) {
        MfmaFinalize fin{adam_args(h), h->d_RB, h->cfg.lossb_weight, h->n_data, data_tiles(h->n_data), h->has_eps, adam_state_doubles(h->P) / 2};
        if (!fuse_adam) fin.ad.theta = nullptr;
        // (flux data: its launches follow this one, and their rows must reach the finalize step -- no in-kernel finalize)
        if (hpv_mfma_iter_tile(m, p, h->merged && h->n_flux == 0 ? &fin : nullptr, &pl.fin_done)) structure = 4;
    }
    if (structure < 0 && hpv_mfma_iter_elem(m, p)) structure = 6;
    if (structure < 0) {
        const int ts = hpv_mfma_tall_split(m, h->pd, h->n_elem);
        if (ts > 1 && h->n_elem * ts <= h->n_red_alloc && hpv_mfma_iter_tall(m, p)) { structure = 5; pl.n_loss = h->n_elem * ts; }
    }
    if (structure < 0) return false;     // (nothing was launched; the caller re-records the start event)
    tstop(h, 2);
    h->pass_structure = structure;
    snprintf(h->variant, sizeof h->variant, "%s", hpv_mfma_variant(m, 0));
    pl.xch_used = hpv_mfma_sync_failed_possible(m);
    return true;
}

// (2) / (3) The variational term as separate launches: forward (+ edge batch) -> projection -> reverse; on the MFMA path the
// projection rides inside the reverse kernel where that applies (element-block mode), otherwise it is the fastest projection
// kernel that takes the shape.
static void pass_separate(hpv_ctx* h, const MfmaPass& p, bool backward, bool use_mfma) {
    Batch& v = h->var;
    tstart(h, 0);
    if (use_mfma) hpv_mfma_forward(h->var.m, h->d_theta, v.X, v.OUT, backward ? 1 : 0, h->stream, p.dt);
    else run_fwd(h, v, backward ? 1 : 0);
    tstop(h, 0);
    if (h->pd.edge) run_fwd(h, h->edge, backward ? 1 : 0);
    bool bfused = false;
    if (backward && use_mfma) {
        tstart(h, 2);   // timed as the reverse-pass class (the projection is ~1 % of its flops)
        bfused = hpv_mfma_backward_fused(h->var.m, p);
        if (bfused) tstop(h, 2);
    }
    if (backward) h->pass_structure = bfused ? 1 : 0;
    if (bfused) { snprintf(h->variant, sizeof h->variant, "%s + %s", hpv_mfma_variant(h->var.m, 1), hpv_mfma_variant(h->var.m, 3)); }
    else {
        tstart(h, 1);
        // (the specialised kernels need GBAR's unused channels pre-zeroed: true for every batch, see alloc_batch)
        const bool special = h->cfg.backend != HPV_BACKEND_GENERIC;
        const ProjArgs pj = pass_proj_args(h, backward, true);
        // few elements (at most two per CU) of a 2-D shape: one workgroup per element before "a lane owns a line"
        bool small_grid = h->dim == 2 && h->n_elem <= 512 && h->proj_split == 1 && !h->pd.nact;
#ifdef HPV_TEST_HOOKS
        if (getenv("HPV_PJ_WG_SMALL")) small_grid = false;      // (A/B: "a lane owns a line" on small grids too)
#endif
        const char* pname = "k_project";
        if (special && small_grid && launch_project_wg(pj, h->n_elem, h->stream)) pname = "k_project_wg";
        else if (special && launch_project_tp(pj, h->n_elem, h->stream)) pname = "k_project_tp";
        else if (special && launch_project_wg(pj, h->n_elem, h->stream, h->d_upart)) pname = h->proj_split > 1 ? "k_project_rows" : "k_project_wg";
        else launch_project(pj, h->n_elem, h->stream);
        tstop(h, 1);
        if (backward) {
            snprintf(h->variant, sizeof h->variant, "%s + %s<%dx%d/%dx%d> + %s", use_mfma ? hpv_mfma_variant(h->var.m, 1) : "k_mlp_fwd_generic", pname,
                     h->pd.qx, h->pd.qy, h->pd.ntx, h->pd.nty, use_mfma ? hpv_mfma_variant(h->var.m, 2) : "k_mlp_bwd_generic");
            tstart(h, 2);
            if (use_mfma) hpv_mfma_backward(h->var.m, h->d_theta, v.X, v.GBAR, v.GPART, &v.rows, h->stream);
            else run_bwd(h, v);
            tstop(h, 2);
        }
    }
    if (backward && h->pd.edge) run_bwd(h, h->edge);
}

// The linear problems (hpv_set_operator): always forward -> k_project_lin -> reverse.  Their integrand carries per-point coefficients
// and a third term, which neither ProjDesc nor a whole-iteration kernel knows; the layer kernels are the ones every handle of the
// channel set u, u_x, (u_y) runs, the merged boundary points ride in the forward launch as ever.  With a nonlinear term
// (hpv_set_nonlinear) k_project_nl takes k_project_lin's place in the same launch slot, with trainable coefficients (hpv_set_trainable)
// k_project_id does; nothing else differs.
static void pass_linear(hpv_ctx* h, const MfmaPass& p, bool backward, bool use_mfma) {
    Batch& v = h->var;
    tstart(h, 0);
    if (use_mfma) hpv_mfma_forward(v.m, h->d_theta, v.X, v.OUT, backward ? 1 : 0, h->stream, p.dt);
    else run_fwd(h, v, backward ? 1 : 0);
    tstop(h, 0);
    ansatz_fwd(h, HPV_ANSATZ_QUAD, v, h->Nq);      // (outside the timed classes: the plain handle's three figures keep their meaning)
    tstart(h, 1);
    const LinProjArgs a{v.OUT, v.GBAR, h->d_lin, h->Nq, h->d_F, h->d_R, h->d_loss_e, h->d_wtx, h->d_wty, h->d_jac, h->d_jxy,
                        h->d_jxy + h->n_elem, h->pd.nact, h->pd.nacty, v.N, h->qx, h->qy, h->ntx, h->nty, h->dim, backward ? 1 : 0,
                        h->d_gram ? h->d_gram : h->d_dual, h->dual_mass,                                // (hpv_set_residual_norm | _gram)
                        h->lin_tensor ? 1 : 0,                                                          // (hpv_set_operator_tensor)
                        h->d_gram ? 1 : 0};                                                             // (hpv_set_residual_gram)
    const int terms_mask = h->nl_mask | (h->n_coef ? h->dir_nl_mask : 0);
    if (h->n_coef)                                                                                      // (hpv_set_trainable)
        launch_project_id(IdProjArgs{a, h->nl_mask ? h->d_nl : h->d_nl_zero, terms_mask, h->d_dirs, h->d_theta + h->P + h->has_eps, h->n_coef,
                                     h->d_dir_mask, h->d_dcoef_e}, h->n_elem, h->stream);
    else if (h->nl_mask | h->q_mask)                                                                    // (hpv_set_nonlinear | hpv_set_quasilinear)
        launch_project_nl(NlProjArgs{a, h->nl_mask ? h->d_nl : nullptr, h->nl_mask | h->q_mask, h->q_mask ? h->d_qp : nullptr, h->q_exp}, h->n_elem, h->stream);
    else launch_project_lin(a, h->n_elem, h->stream);
    tstop(h, 1);
    if (h->n_mom) {                                  // (hpv_set_moments; outside the timed classes, like the ansatz)
        MomentArgs ma{v.OUT, v.GBAR, h->d_mom, h->Nq, h->n_elem, h->qx * h->qy, h->n_mom, {}, {}, {}, h->d_mom_part, h->d_mom_res, h->d_loss_e,
                      h->n_coef, h->d_dcoef_e, backward && h->n_coef ? h->d_mom_dcoef : nullptr};
        std::copy_n(h->mom_power, HPV_MAX_MOMENTS, ma.power);
        std::copy_n(h->mom_target, HPV_MAX_MOMENTS, ma.target);
        std::copy_n(h->mom_weight, HPV_MAX_MOMENTS, ma.weight);
        launch_moments(ma, backward, h->stream);
    }
    if (!backward) return;
    h->pass_structure = 0;
    std::string terms;                               // the active terms of k_project_nl, e.g. ";u2,u3,exp,adv"
    static const char* const term_names[] = {"u2", "u3", "exp", "adv"};
    for (int t = 0; t < 4; ++t)
        if (terms_mask >> t & 1) terms += std::string(terms.empty() ? ";" : ",") + term_names[t];
    if (h->q_mask) terms += ";quasi";                                // (hpv_set_quasilinear: the _q instantiation of k_project_nl)
    if (h->lin_tensor) terms += ";tensor";                           // (hpv_set_operator_tensor: the TENSOR instantiation of the kernel)
    if (h->n_coef) terms += ";nc=" + std::to_string(h->n_coef);      // e.g. k_project_id<6x5/4x3;u3;nc=2>, k_project_id<6x5/4x3;u3;tensor;nc=2>
    if (has_ansatz(h)) terms += ";ansatz";                           // (hpv_set_ansatz: k_ansatz_fwd / k_ansatz_adj around the projection)
    if (h->d_dual) terms += ";dual";                                 // (hpv_set_residual_norm: the _dual instantiation of the kernel)
    if (h->d_gram) terms += ";dual=dense";                           // (hpv_set_residual_gram: the _dense instantiation)
    if (h->n_mom) terms += ";mom=" + std::to_string(h->n_mom);       // (hpv_set_moments: k_moment_part, _close, _adj behind the kernel)
    snprintf(h->variant, sizeof h->variant, "%s + k_project_%s<%dx%d/%dx%d%s> + %s", use_mfma ? hpv_mfma_variant(v.m, 1) : "k_mlp_fwd_generic",
             h->n_coef ? "id" : (h->nl_mask | h->q_mask) ? "nl" : "lin", h->qx, h->qy, h->ntx, h->nty, terms.c_str(), use_mfma ? hpv_mfma_variant(v.m, 2) : "k_mlp_bwd_generic");
    ansatz_adj(h, HPV_ANSATZ_QUAD, v, h->Nq);
    tstart(h, 2);
    if (use_mfma) hpv_mfma_backward(v.m, h->d_theta, v.X, v.GBAR, v.GPART, &v.rows, h->stream);
    else run_bwd(h, v);
    tstop(h, 2);
}

// backward: also the reverse pass and the gradient reduction; fuse_adam: the finalize kernel applies the TF1 Adam update itself
// (single-GPU training step); pend: RB holds the previous iteration's reduced gradient, its update not applied yet (multi-GPU
// sequence, see hpv_ctx::defer_adam): k_iter_fused takes it into its prologue and k_finalize stores it; any other structure gets a
// k_adam launch in front.
int enqueue_pass(hpv_ctx* h, bool backward, bool fuse_adam, bool pend) {
    // (an error exit BEFORE the pending update has been taken over by a launch applies it first, best effort: it was counted when
    //  its iteration was enqueued, and dropping it would leave the device one update behind the host's count -- advisor, round 5)
    auto apply_pend = [&] { if (pend) { enqueue_adam(h); pend = false; } };
    if (h->cfg.scheme == HPV_SCHEME_PINN || !backward) apply_pend();
    if (h->cfg.scheme == HPV_SCHEME_PINN) return enqueue_pinn_pass(h, backward, fuse_adam);
    int rc = check_ready(h);
    for (int w = HPV_ANSATZ_QUAD; !rc && w <= HPV_ANSATZ_FLUX; ++w) rc = ansatz_ready(h, w);      // (never a pass that mixes u and N)
    if (rc) { apply_pend(); return rc; }
    const bool use_mfma = h->var.m && h->backend == HPV_BACKEND_MFMA;
    // the deferred update can only ride in a whole-iteration kernel that is the ONLY reader of the parameters in this pass (boundary
    // points merged into it, no edge batch, no flux batch); otherwise it is applied here, before anything of this pass is launched or forked
    if (!(use_mfma && h->var.N > 0 && (h->merged || h->n_data == 0) && !h->pd.edge && h->n_flux == 0 && !hpv_mfma_prefers_elem(h->var.m)) || h->linear) apply_pend();
    if (!h->side_active && (rc = ensure_small_batches(h))) { apply_pend(); return rc; }   // (allocations are not allowed inside a stream capture)
    hipStream_t smain = h->stream;
    const bool fork = h->side_active && !h->merged && h->n_data > 0;
    if (fork) {
        (void)hipEventRecord(h->ev_fork, smain);
        (void)hipStreamWaitEvent(h->stream2, h->ev_fork, 0);
    }
    PassPlan pl{h->linear ? (long)h->n_elem : (long)h->n_elem * h->proj_split};      // (k_project_lin: one workgroup, one partial per element)
    // --- variational term on this shard's quadrature batch ---
    if (h->var.N > 0) {
        const MfmaDataTerm dt = pass_data_term(h, backward);
        const ProjArgs pa = pass_proj_args(h, backward);
        const MfmaPass p = pass_mfma(h, dt, pa);
        if (h->linear) { pass_linear(h, p, backward, use_mfma); pl.n_loss += h->n_mom; }      // (hpv_set_moments: pen_k behind the element losses)
        else if (!(backward && use_mfma && pass_whole_iteration(h, p, fuse_adam, pend, pl))) pass_separate(h, p, backward, use_mfma);
    }
    // --- boundary / data term: inside the quadrature batch (one partial per 16-point data tile), or its own small batch ---
    int ndp = 0;
    if (h->n_data > 0 && h->merged) {
        ndp = data_tiles(h->n_data);
    } else if (h->n_data > 0) {
        if (fork) h->stream = h->stream2;   // the launch helpers read h->stream
        ndp = pass_data(h, backward);
        h->stream = smain;
    }
    pass_flux(h, backward);      // on the main stream, behind the variational term
    if (fork) {
        (void)hipEventRecord(h->ev_join, h->stream2);
        (void)hipStreamWaitEvent(smain, h->ev_join, 0);
    }
    if (!pl.fin_done) {
        FinalizeArgs fa = pass_finalize_args(h, backward, ndp, fuse_adam || pl.pend_taken);
        fa.g[0] = {backward && h->var.N > 0 ? h->var.GPART : nullptr, h->var.rows};
        fa.g[2] = {backward && h->pd.edge && h->edge.N > 0 ? h->edge.GPART : nullptr, h->edge.rows};
        fa.loss_e = h->d_loss_e; fa.n_loss = pl.n_loss; fa.deps_e = h->d_deps_e;
        fa.xerr = h->d_xerr;
        fa.xiter_bump = pl.xch_used ? hpv_mfma_xiter(h->var.m) : nullptr;
        fa.pending_adam = pl.pend_taken ? 1 : 0;
        launch_finalize(fa, h->stream);
    }
    return launch_check(h, "kernel launch");
}

// scheme == 'PINNs' (P2:128-129; the same switch for the other two problems): loss = w*lossb + lossp, lossp = mean(r^2) at the
// collocation points with the problem's strong-form residual r (k_pinn_residual); AdvDiff: the partials of d lossp / d epsilon ride
// where the variational path puts its own (deps_e of k_finalize -> the packed buffer's slot [P])
static int enqueue_pinn_pass(hpv_ctx* h, bool backward, bool fuse_adam) {
    if (!h->have_params) return fail(h, -3, "hpv_set_params has not been called");
    if (h->n_col <= 0) return fail(h, -3, "hpv_set_collocation has not been called");
    int rc;
    if (h->batch_dirty) {   // only the data batch matters here
        if ((rc = assemble_data_batch(h))) return rc;
        h->merged = false;
        h->batch_dirty = false;
    }
    if (!h->side_active && (rc = ensure_small_batches(h))) return rc;
    run_fwd(h, h->colloc, backward ? 1 : 0);
    const int nparts = pinn_residual_parts(h->n_col);
    launch_pinn_residual(h->cfg.pde, PinnArgs{h->colloc.OUT, h->d_fcol, h->colloc.GBAR, h->d_col_part, h->d_col_part + 64,
                                              h->has_eps ? h->d_theta + h->P : nullptr, h->cfg.V, h->colloc.N, h->n_col,
                                              h->n_col_total, backward ? 1 : 0}, h->stream);
    if (backward) {
        run_bwd(h, h->colloc);
        // (hpv_kernel_variant: the layer kernels of the collocation batch -- recorded after their launches, as pass_separate does)
        HpvMfma* mc = h->colloc.m;
        snprintf(h->variant, sizeof h->variant, "%s + k_pinn_residual + %s", mc ? hpv_mfma_variant(mc, 1) : "k_mlp_fwd_generic",
                 mc ? hpv_mfma_variant(mc, 2) : "k_mlp_bwd_generic");
    }
    const int ndp = h->n_data > 0 ? pass_data(h, backward) : 0;
    pass_flux(h, backward);
    FinalizeArgs fa = pass_finalize_args(h, backward, ndp, fuse_adam);
    fa.g[0] = {backward ? h->colloc.GPART : nullptr, h->colloc.rows};
    fa.loss_e = h->d_col_part; fa.n_loss = nparts; fa.deps_e = h->has_eps ? h->d_col_part + 64 : nullptr;
    launch_finalize(fa, h->stream);
    return launch_check(h, "kernel launch");
}

// A pass whose packed buffer is made global: with the in-library exchange connected the reduced buffer (and, for a
// training iteration, the Adam update) follows the finalize kernel on the same stream; otherwise the plain pass.
int enqueue_pass_x(hpv_ctx* h, bool backward, bool fuse_adam) {
    if (h->rccl_on) {
        // ONE collective per iteration: ncclAllReduce(sum) of [grad | d eps | lossv | w*lossb | msq | pad] over
        // xGMI, on the handle's stream (captured into the iteration graphs like the kernels), then the identical TF1 Adam
        // update on every rank
        const bool pend = h->adam_pending;
        h->adam_pending = false;                  // (taken into this pass's kernels, or applied in front of them)
        int rc = enqueue_pass(h, backward, false, pend);
        if (rc) return rc;
        ncclResult_t r = rccl_allreduce(h, h->d_RB, (size_t)h->Ptot + 4, h->stream);
        if (r != ncclSuccess) return fail(h, -6, "ncclAllReduce failed: %s", rccl_error_string(r));
        if (backward && fuse_adam) {
            // inside a sequence of iterations the update is deferred into the NEXT iteration's kernels (two launches + one collective
            // per iteration); the sequence's last one -- and every stand-alone iteration -- is applied here
            if (h->defer_adam && h->defer_ok) h->adam_pending = true;
            else enqueue_adam(h);
        }
        return launch_check(h, "adam launch");
    }
    if (!h->p2p_on) return enqueue_pass(h, backward, fuse_adam);
    int rc = enqueue_pass(h, backward, false);
    if (rc) return rc;
    const AdamArgs ad = adam_args(h);
    launch_p2p_exchange(h->pp, h->d_RB, (backward && fuse_adam) ? &ad : nullptr, h->P, h->Ptot, h->stream);
    return launch_check(h, "exchange launch");
}

// end of a sequence of training iterations: the deferred update, if any, is applied (k_adam)
static void flush_adam(hpv_ctx* h) {
    if (h->adam_pending) enqueue_adam(h);
    h->adam_pending = false;
    h->defer_adam = false;
}

#define HPV_GRAPH_ITERS 8

// Capture `iters` whole training iterations (incl. the Adam updates) into an executable graph.
static int build_step_graph(hpv_ctx* h, int iters, hipGraphExec_t* out) {
    int rc;
    // one direct pass first: lazily created objects (small-batch MFMA stores) must exist before capture
    if ((rc = ensure_small_batches(h))) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    hipGraph_t graph = nullptr;
    HIPCHK(h, hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal));
    h->side_active = true;
    h->defer_adam = true;
    for (int k = 0; k < iters && !rc; ++k) rc = enqueue_pass_x(h, true, true);   // forward .. finalize (+ fused Adam / exchange)
    if (!rc) flush_adam(h); else { h->adam_pending = false; h->defer_adam = false; }
    h->side_active = false;
    hipError_t e = hipStreamEndCapture(h->stream, &graph);
    if (rc) { if (graph) (void)hipGraphDestroy(graph); return rc; }
    if (e != hipSuccess) return fail(h, -2, "hipStreamEndCapture failed: %s", hipGetErrorString(e));
    e = hipGraphInstantiate(out, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (e != hipSuccess) { *out = nullptr; return fail(h, -2, "hipGraphInstantiate failed: %s", hipGetErrorString(e)); }
    return 0;
}

// n_iters training iterations enqueued on the handle's stream (graph replays where possible), no synchronisation
int enqueue_iterations(hpv_ctx* h, int n_iters) {
    int rc;
    if (h->use_graph && h->own_stream && !h->timing && n_iters > 0 && h->cfg.scheme == HPV_SCHEME_VPINN) {
        if ((rc = check_ready(h))) return rc;
        for (int w = HPV_ANSATZ_QUAD; w <= HPV_ANSATZ_FLUX; ++w)      // (before a capture is begun for a pass that would refuse)
            if ((rc = ansatz_ready(h, w))) return rc;
        // n = a * HPV_GRAPH_ITERS + r: a replays of the K-iteration graph and ONE replay of an r-iteration graph (captured
        // the first time a call leaves that remainder -- callers that time a call run it once untimed before)
        static_assert(HPV_GRAPH_ITERS <= 8, "g_rem size");
        if (n_iters >= HPV_GRAPH_ITERS && !h->g_stepK && (rc = build_step_graph(h, HPV_GRAPH_ITERS, &h->g_stepK))) {
            if (!h->rccl_on) return rc;
            // a collective that refuses stream capture must not stop the run: eager launches from here on
            h->use_graph = false;
            h->err.clear();
            return enqueue_iterations(h, n_iters);
        }
        int it = 0;
        for (; it + HPV_GRAPH_ITERS <= n_iters; it += HPV_GRAPH_ITERS) HIPCHK(h, hipGraphLaunch(h->g_stepK, h->stream));
        const int rem = n_iters - it;
        if (rem > 0) {
            if (!h->g_rem[rem] && (rc = build_step_graph(h, rem, &h->g_rem[rem]))) {
                if (!h->rccl_on) { h->nupd_host += it; return rc; }
                h->use_graph = false;
                h->err.clear();
                h->nupd_host += it;           // (the iterations already launched through g_stepK: advisor, round 3)
                return enqueue_iterations(h, rem);
            }
            HIPCHK(h, hipGraphLaunch(h->g_rem[rem], h->stream));
        }
    } else {
        h->defer_adam = true;
        for (int it = 0; it < n_iters; ++it) {
            if ((rc = enqueue_pass_x(h, true, true))) { h->adam_pending = false; h->defer_adam = false; return rc; }
            h->nupd_host += 1;            // (counted per enqueued iteration: an error exit leaves the count right -- a pending update is
                                          //  either stored by the failing pass's k_finalize or applied by enqueue_pass's error exit; the
                                          //  handle is in a failed state afterwards: hpv_last_error says why)
        }
        flush_adam(h);
        return 0;
    }
    h->nupd_host += n_iters;
    return 0;
}

}  // namespace hpvd
