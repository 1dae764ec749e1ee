// The L-BFGS stage of the C-ABI (include/hpvpinn.h: hpv_lbfgs_step, hpv_lbfgs_reset): the driver loop of the optimiser on the host,
// its vectors on the device (kernels_lbfgs.hip), its line search over scalars (hpv_linesearch.h).  Built on the packed buffer a
// backward pass leaves behind -- RB = [grad | lossv | w*lossb | ..], the same on every problem class and both schemes -- and on
// nothing below it: no kernel of the pass, no launch structure, no graph and nothing of Adam's is touched.
//
// One function evaluation = k_lbfgs_trial (theta = theta0 + t d) -> the backward pass -> k_lbfgs_probe -> 32 bytes to the host.
// The iteration follows torch.optim.LBFGS(line_search_fn="strong_wolfe") decision for decision (curvature test y.s > 1e-10, H_diag
// of the newest pair, first step min(1, 1/|g|_1) lr, the exits on max|g|, g.d, max|t d| and |f - f_prev|), with two differences:
// the pair of an accepted step is stored at once (there: at the top of the next iteration -- the same pair), and a search that ends
// without a Wolfe point (max_ls, the evaluation budget, a non-finite loss) is a FAILURE here: the parameters go back to the last
// accepted iterate and the call says why.
#include "hpv_ctx.h"
#include "hpv_linesearch.h"

using namespace hpvd;

namespace {

constexpr int LB_SLOTS = 3;      // gradients the line search keeps: two bracket ends and the point being evaluated

LbfgsArgs lb_args(hpv_ctx* h) {
    const size_t P = (size_t)h->Ptot, m = (size_t)h->lb_m;
    LbfgsArgs a{};
    a.P = h->Ptot; a.m = h->lb_m;
    a.theta0 = h->d_lb; a.g = h->d_lb + P; a.d = h->d_lb + 2 * P;
    a.S = h->d_lb + (3 + LB_SLOTS) * P; a.Y = a.S + m * P;
    a.rho = a.Y + m * P; a.h_diag = a.rho + m; a.scal = a.h_diag + 1;
    a.ring = h->d_lb_ring; a.theta = h->d_theta;
    return a;
}
double* lb_slot(hpv_ctx* h, int s) { return h->d_lb + (size_t)(3 + s) * h->Ptot; }

int lb_clear(hpv_ctx* h) {      // no pairs, H_diag = 1
    const double one = 1.0;
    HIPCHK(h, hipMemsetAsync(h->d_lb_ring, 0, 4 * sizeof(int), h->stream));
    HIPCHK(h, hipMemcpyAsync(lb_args(h).h_diag, &one, sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->lb_iters = 0;
    return 0;
}

int lb_ensure(hpv_ctx* h, int m) {
    if (h->d_lb && h->lb_m == m) return 0;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    const size_t P = (size_t)h->Ptot;
    int rc;
    h->lb_m = 0;
    if ((rc = dalloc(h, &h->d_lb, (3 + LB_SLOTS + 2 * (size_t)m) * P + (size_t)m + 1 + 8))) return rc;
    if ((rc = dalloc(h, &h->d_lb_ring, (size_t)4))) return rc;
    h->lb_m = m;
    return lb_clear(h);      // (a ring of another capacity: the pairs are dropped with it)
}

bool lb_sharded(const hpv_ctx* h) {
    if (h->cfg.scheme == HPV_SCHEME_PINN) return h->n_col_total != (long)h->n_col;
    return h->have_elems && (h->e_begin != 0 || h->e_end != h->ne_tot);
}

// one function evaluation at the handle's live parameters: the backward pass, the probe, four doubles back
int lb_evaluate(hpv_ctx* h, const LbfgsArgs& a, double* g_keep, int with_d, double* out4) {
    int rc = enqueue_pass_x(h, true, false);
    if (rc) return rc;
    launch_lbfgs_probe(a, h->d_RB, g_keep, with_d, h->stream);
    if ((rc = launch_check(h, "lbfgs probe launch"))) return rc;
    HIPCHK(h, hipMemcpyAsync(out4, a.scal + 4, 4 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    return hpv_sync(h);
}

}  // namespace

namespace hpvd {
int lbfgs_drop(hpv_ctx* h) { return h->d_lb ? lb_clear(h) : 0; }
}  // namespace hpvd

extern "C" {

int hpv_lbfgs_reset(hpv_handle h) { return h ? lbfgs_drop(h) : -1; }

int hpv_lbfgs_step(hpv_handle h, const hpv_lbfgs_opts* o, double* loss3_hist, int* info) {
    if (!h || !o) return -1;
    if (hpv_exchange_in_use(h) != 0)
        return fail(h, -4, "hpv_lbfgs_step: this handle is connected to an exchange between GPUs; the L-BFGS stage runs on one GPU only");
    if (lb_sharded(h))
        return fail(h, -4, "hpv_lbfgs_step: this handle owns a shard of the model (part of the elements or collocation points); "
                           "the L-BFGS stage runs on one GPU only");
    if (o->history < 1) return fail(h, -4, "hpv_lbfgs_step: history is %d, at least one pair is needed", o->history);
    if (!h->have_params) return fail(h, -3, "hpv_lbfgs_step: no parameters set");
    const int m = std::min(o->history, HPV_LBFGS_MAX_HISTORY);
    const int max_iter = o->max_iter;
    const int max_eval = o->max_eval > 0 ? o->max_eval : (int)((long long)max_iter * 5 / 4);
    int it = 0, evals = 0, reason = HPV_LBFGS_MAX_ITER, rc;
    auto finish = [&](int skipped0) {
        int ring[4] = {0, 0, 0, 0};
        HIPCHK(h, hipMemcpyAsync(ring, h->d_lb_ring, sizeof ring, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        if (info) { info[0] = it; info[1] = evals; info[2] = ring[2] - skipped0; info[3] = reason; }
        return 0;
    };
    if (max_iter < 1) {
        if (info) { info[0] = 0; info[1] = 0; info[2] = 0; info[3] = reason; }
        return 0;
    }
    if ((rc = lb_ensure(h, m))) return rc;
    const LbfgsArgs a = lb_args(h);
    const size_t Pb = (size_t)h->Ptot * sizeof(double);
    int ring0[4] = {0, 0, 0, 0};
    HIPCHK(h, hipMemcpyAsync(ring0, h->d_lb_ring, sizeof ring0, hipMemcpyDeviceToHost, h->stream));
    // the accepted iterate is where the handle stands; its loss and gradient (into a.g)
    HIPCHK(h, hipMemcpyAsync(a.theta0, h->d_theta, Pb, hipMemcpyDeviceToDevice, h->stream));
    double e4[4], raw[4];
    if ((rc = lb_evaluate(h, a, a.g, 0, e4))) return rc;
    evals = 1;
    auto record = [&](int k) {      // {loss, lossb, lossv} of the accepted iterate from the packed buffer's slots
        if (!loss3_hist) return;
        loss3_hist[3 * k] = raw[0] + raw[1];
        loss3_hist[3 * k + 1] = h->cfg.pde == HPV_PDE_ADVDIFF ? raw[1] : raw[2];
        loss3_hist[3 * k + 2] = raw[0];
    };
    HIPCHK(h, hipMemcpyAsync(raw, h->d_RB + h->Ptot, sizeof raw, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    record(0);
    double loss = e4[0];
    if (!std::isfinite(loss)) { reason = HPV_LBFGS_NONFINITE; return finish(ring0[2]); }
    if (e4[2] <= o->tolerance_grad) { reason = HPV_LBFGS_TOL_GRAD; return finish(ring0[2]); }

    while (it < max_iter) {
        // direction from the ring, and the scalars that go with it
        launch_lbfgs_direction(a, h->stream);
        if ((rc = launch_check(h, "lbfgs direction launch"))) return rc;
        double s4[4];
        HIPCHK(h, hipMemcpyAsync(s4, a.scal, sizeof s4, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        const double gtd = s4[0], g_l1 = s4[2], d_norm = s4[3];
        double t = h->lb_iters == 0 ? std::min(1.0, 1.0 / g_l1) * o->lr : o->lr;
        if (gtd > -o->tolerance_change) { reason = HPV_LBFGS_TOL_DIRECTION; break; }      // (no descent left along d)
        if (max_eval - evals < 1) { reason = HPV_LBFGS_MAX_EVAL; break; }

        hpv_ls::Params lp;
        lp.tolerance_change = o->tolerance_change;
        lp.max_ls = std::min(25, max_eval - evals);
        int pass_rc = 0;
        double t_live = 0.0;      // the step the live parameters and the packed buffer stand at
        auto eval = [&](double tt, int slot, double* f, double* gd) {
            launch_lbfgs_trial(a, tt, h->stream);
            double r4[4];
            if ((pass_rc = lb_evaluate(h, a, lb_slot(h, slot), 1, r4))) return false;
            t_live = tt;
            *f = r4[0]; *gd = r4[1];
            return true;
        };
        const hpv_ls::Result r = hpv_ls::strong_wolfe(eval, t, d_norm, loss, gtd, lp);
        evals += r.evals;
        const bool ok = !r.failed && !r.exhausted && r.slot >= 0 && std::isfinite(r.f);
        if (!ok) {
            // back to the last accepted iterate (theta0 is a copy of it: bit for bit)
            HIPCHK(h, hipMemcpyAsync(h->d_theta, a.theta0, Pb, hipMemcpyDeviceToDevice, h->stream));
            HIPCHK(h, hipStreamSynchronize(h->stream));
            if (pass_rc) return pass_rc;
            reason = !std::isfinite(r.f) ? HPV_LBFGS_NONFINITE
                     : r.exhausted ? (max_eval - (evals - r.evals) < 25 ? HPV_LBFGS_MAX_EVAL : HPV_LBFGS_MAX_LS)
                                   : HPV_LBFGS_TOL_CHANGE;      // (the bracket closed on the starting point: no step to take)
            break;
        }
        t = r.t;
        if (t_live != t) {
            // the search returned an earlier trial point: the parameters go there, the loss slots are read again there (forward only:
            // its gradient was kept)
            launch_lbfgs_trial(a, t, h->stream);
            if ((rc = enqueue_pass_x(h, false, false))) return rc;
        }
        HIPCHK(h, hipMemcpyAsync(raw, h->d_RB + h->Ptot, sizeof raw, hipMemcpyDeviceToHost, h->stream));
        // the pair of this step, then g = g_new, theta0 = theta
        launch_lbfgs_push(a, t, lb_slot(h, r.slot), h->stream);
        if ((rc = launch_check(h, "lbfgs push launch"))) return rc;
        // max|g_new| for the optimality test: the probe's value if the point is the one evaluated last, else one more look at it
        double gmax;
        if (t_live == t) {
            HIPCHK(h, hipMemcpyAsync(&gmax, a.scal + 6, sizeof gmax, hipMemcpyDeviceToHost, h->stream));
            if ((rc = hpv_sync(h))) return rc;
        } else {
            launch_lbfgs_probe(a, a.g, lb_slot(h, r.slot), 0, h->stream);      // (a.g holds it now; the slot is free)
            HIPCHK(h, hipMemcpyAsync(&gmax, a.scal + 6, sizeof gmax, hipMemcpyDeviceToHost, h->stream));
            if ((rc = hpv_sync(h))) return rc;
        }
        const double prev_loss = loss;
        loss = r.f;
        ++it;
        h->lb_iters += 1;
        record(it);
        if (it == max_iter) { reason = HPV_LBFGS_MAX_ITER; break; }
        if (evals >= max_eval) { reason = HPV_LBFGS_MAX_EVAL; break; }
        if (gmax <= o->tolerance_grad) { reason = HPV_LBFGS_TOL_GRAD; break; }
        if (std::fabs(t) * d_norm <= o->tolerance_change) { reason = HPV_LBFGS_TOL_CHANGE; break; }
        if (std::fabs(loss - prev_loss) < o->tolerance_change) { reason = HPV_LBFGS_TOL_CHANGE; break; }
    }
    return finish(ring0[2]);
}

#ifdef HPV_TEST_HOOKS
// libhpvpinn_testhooks.so only: the kernels on the caller's vectors, without a handle (current device, default stream).
// direction: S, Y [m][P], rho [m], g [P] in; d [P], scal4 = {g . d, max|g|, sum|g|, max|d|} out.
int hpv_test_lbfgs_direction(int P, int m, int head, int n_hist, const double* S, const double* Y, const double* rho, double h_diag,
                             const double* g, double* d_out, double* scal4) {
    if (P < 1 || m < 1 || m > HPV_LBFGS_MAX_HISTORY || head < 0 || head >= m || n_hist < 0 || n_hist > m) return -1;
    const size_t Ps = (size_t)P, ms = (size_t)m, n = (2 + 2 * ms) * Ps + ms + 1 + 8;
    double* buf = nullptr;
    int* ring = nullptr;
    if (hipMalloc((void**)&buf, n * sizeof(double)) != hipSuccess) return -2;
    if (hipMalloc((void**)&ring, 4 * sizeof(int)) != hipSuccess) { (void)hipFree(buf); return -2; }
    LbfgsArgs a{};
    a.P = P; a.m = m; a.g = buf; a.d = buf + Ps; a.S = buf + 2 * Ps; a.Y = a.S + ms * Ps; a.rho = a.Y + ms * Ps; a.h_diag = a.rho + ms;
    a.scal = a.h_diag + 1; a.ring = ring;
    const int r4[4] = {head, n_hist, 0, 0};
    hipError_t e = hipMemcpy(a.g, g, Ps * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(a.S, S, ms * Ps * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(a.Y, Y, ms * Ps * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(a.rho, rho, ms * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(a.h_diag, &h_diag, sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(ring, r4, sizeof r4, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        launch_lbfgs_direction(a, nullptr);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(d_out, a.d, Ps * sizeof(double), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(scal4, a.scal, 4 * sizeof(double), hipMemcpyDeviceToHost);
    (void)hipFree(buf); (void)hipFree(ring);
    return e == hipSuccess ? 0 : -2;
}

// average duration (us) of k_lbfgs_direction over `reps` back-to-back launches with a ring of n_hist pairs (zeros: the work does not
// depend on the values), one event pair around all of them
int hpv_test_lbfgs_direction_time(int P, int m, int n_hist, int reps, double* avg_us) {
    if (P < 1 || m < 1 || m > HPV_LBFGS_MAX_HISTORY || n_hist < 0 || n_hist > m || reps < 1 || !avg_us) return -1;
    const size_t Ps = (size_t)P, ms = (size_t)m, n = (2 + 2 * ms) * Ps + ms + 1 + 8;
    double* buf = nullptr;
    int* ring = nullptr;
    if (hipMalloc((void**)&buf, n * sizeof(double)) != hipSuccess) return -2;
    if (hipMalloc((void**)&ring, 4 * sizeof(int)) != hipSuccess) { (void)hipFree(buf); return -2; }
    LbfgsArgs a{};
    a.P = P; a.m = m; a.g = buf; a.d = buf + Ps; a.S = buf + 2 * Ps; a.Y = a.S + ms * Ps; a.rho = a.Y + ms * Ps; a.h_diag = a.rho + ms;
    a.scal = a.h_diag + 1; a.ring = ring;
    const int r4[4] = {0, n_hist, 0, 0};
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t e = hipMemset(buf, 0, n * sizeof(double));
    if (e == hipSuccess) e = hipMemcpy(ring, r4, sizeof r4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    if (e == hipSuccess) { launch_lbfgs_direction(a, nullptr); e = hipDeviceSynchronize(); }      // (warm-up)
    if (e == hipSuccess) e = hipEventRecord(e0, nullptr);
    for (int i = 0; i < reps && e == hipSuccess; ++i) { launch_lbfgs_direction(a, nullptr); e = hipGetLastError(); }
    if (e == hipSuccess) e = hipEventRecord(e1, nullptr);
    if (e == hipSuccess) e = hipEventSynchronize(e1);
    float ms_total = 0.f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms_total, e0, e1);
    *avg_us = 1e3 * (double)ms_total / reps;
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    (void)hipFree(buf); (void)hipFree(ring);
    return e == hipSuccess ? 0 : -2;
}

// push: S, Y [m][P], rho [m], h_diag [1], ring [3] = {head, n_hist, skipped}, g [P] (the gradient at theta0), theta0 [P] in and out;
// d, g_new, theta [P] in.
int hpv_test_lbfgs_push(int P, int m, int* ring3, double* S, double* Y, double* rho, double* h_diag, double t, const double* d,
                        const double* g_new, double* g, const double* theta, double* theta0) {
    if (P < 1 || m < 1 || m > HPV_LBFGS_MAX_HISTORY || ring3[0] < 0 || ring3[0] >= m || ring3[1] < 0 || ring3[1] > m) return -1;
    const size_t Ps = (size_t)P, ms = (size_t)m, n = (5 + 2 * ms) * Ps + ms + 1 + 8;
    double* buf = nullptr;
    int* ring = nullptr;
    if (hipMalloc((void**)&buf, n * sizeof(double)) != hipSuccess) return -2;
    if (hipMalloc((void**)&ring, 4 * sizeof(int)) != hipSuccess) { (void)hipFree(buf); return -2; }
    LbfgsArgs a{};
    a.P = P; a.m = m; a.g = buf; a.d = buf + Ps; a.theta0 = buf + 2 * Ps; a.theta = buf + 3 * Ps;
    double* gn = buf + 4 * Ps;
    a.S = buf + 5 * Ps; a.Y = a.S + ms * Ps; a.rho = a.Y + ms * Ps; a.h_diag = a.rho + ms; a.scal = a.h_diag + 1; a.ring = ring;
    const int r4[4] = {ring3[0], ring3[1], ring3[2], 0};
    hipError_t e = hipMemcpy(a.g, g, Ps * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(a.d, d, Ps * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(a.theta0, theta0, Ps * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(a.theta, theta, Ps * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(gn, g_new, Ps * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(a.S, S, ms * Ps * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(a.Y, Y, ms * Ps * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(a.rho, rho, ms * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(a.h_diag, h_diag, sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(ring, r4, sizeof r4, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        launch_lbfgs_push(a, t, gn, nullptr);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    int r4o[4] = {0, 0, 0, 0};
    if (e == hipSuccess) e = hipMemcpy(g, a.g, Ps * sizeof(double), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(theta0, a.theta0, Ps * sizeof(double), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(S, a.S, ms * Ps * sizeof(double), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(Y, a.Y, ms * Ps * sizeof(double), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(rho, a.rho, ms * sizeof(double), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(h_diag, a.h_diag, sizeof(double), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(r4o, ring, sizeof r4o, hipMemcpyDeviceToHost);
    if (e == hipSuccess) { ring3[0] = r4o[0]; ring3[1] = r4o[1]; ring3[2] = r4o[2]; }
    (void)hipFree(buf); (void)hipFree(ring);
    return e == hipSuccess ? 0 : -2;
}
#endif

}  // extern "C"
