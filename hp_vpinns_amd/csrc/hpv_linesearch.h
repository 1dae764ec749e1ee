// Strong-Wolfe line search over scalars (t, f, gtd) for the L-BFGS stage (hpv_lbfgs_step): bracketing, then a zoom phase with
// safeguarded cubic interpolation.  Host-only, plain C++, no HIP: the caller hands in a function that evaluates phi(t) = f(x + t d)
// and phi'(t) = grad f(x + t d) . d; vectors never enter.
//
// The behaviour is that of torch.optim.LBFGS(line_search_fn="strong_wolfe") (the routine ported there from minFunc / lswolfe.lua):
// the same decisions in the same order and the same scalar arithmetic in IEEE double, so that both take the same trial steps --
// c1 = 1e-4 (sufficient decrease), c2 = 0.9 (curvature), extrapolation bounds [t + 0.01 (t - t_prev), 10 t] while bracketing, the
// 0.1-of-the-bracket safeguard while zooming, the exit when bracket width * max|d| < tolerance_change, at most max_ls steps.
// Non-finite values need no case of their own: every comparison with a NaN is false, and an interpolation that meets one falls
// back to the bisection of its bounds (py_min / py_max keep Python's operand order, which decides what a NaN does there).
//
// Gradients: the search keeps at most two bracket ends alive beside the point it evaluates.  The caller that wants the gradient of
// the accepted point without evaluating it again gives every evaluation a slot 0..2 to keep its gradient in; the search names a
// slot that no live bracket end uses, and reports the slot of the point it returns (-1: the starting point t = 0).
#pragma once
#include <cmath>

namespace hpv_ls {

inline double py_max(double a, double b) { return b > a ? b : a; }      // max(a, b) of Python: the first unless the second is greater
inline double py_min(double a, double b) { return b < a ? b : a; }

// minimiser of the cubic through (x1, f1, g1), (x2, f2, g2), clamped to [lo, hi]; the midpoint where the cubic has none
inline double cubic_interpolate(double x1, double f1, double g1, double x2, double f2, double g2, double lo, double hi) {
    const double d1 = g1 + g2 - 3.0 * (f1 - f2) / (x1 - x2);
    const double d2_square = d1 * d1 - g1 * g2;
    if (d2_square >= 0.0) {
        const double d2 = std::sqrt(d2_square);
        const double min_pos = x1 <= x2 ? x2 - (x2 - x1) * ((g2 + d2 - d1) / (g2 - g1 + 2.0 * d2))
                                        : x1 - (x1 - x2) * ((g1 + d2 - d1) / (g1 - g2 + 2.0 * d2));
        return py_min(py_max(min_pos, lo), hi);
    }
    return (lo + hi) / 2.0;
}
inline double cubic_interpolate(double x1, double f1, double g1, double x2, double f2, double g2) {
    return x1 <= x2 ? cubic_interpolate(x1, f1, g1, x2, f2, g2, x1, x2) : cubic_interpolate(x1, f1, g1, x2, f2, g2, x2, x1);
}

struct Params {
    double c1 = 1e-4, c2 = 0.9, tolerance_change = 1e-9;
    int max_ls = 25;
};

struct Result {
    double t = 0.0, f = 0.0, gtd = 0.0;   // the point returned: the lower end of the final bracket
    int slot = -1;                        // where its gradient was kept (-1: the starting point)
    int evals = 0;                        // evaluations made
    bool wolfe = false;                   // the point satisfies both conditions
    bool exhausted = false;               // max_ls steps went by without such a point (the lower bracket end is returned all the same)
    bool failed = false;                  // an evaluation reported a failure of its own; t, f, gtd are the starting point's
};

// eval(t, slot, &f, &gtd) -> bool (false: give up at once).  f, gtd: the value and directional derivative at t = 0 (gtd < 0);
// t: the first trial step; d_norm: max|d|.
template <class Eval>
Result strong_wolfe(Eval&& eval, double t, double d_norm, double f, double gtd, const Params& p = Params()) {
    Result r;
    r.f = f; r.gtd = gtd;
    const double c1 = p.c1, c2 = p.c2;
    const int max_ls = p.max_ls;
    double f_new, gtd_new;
    int slot_new = 0;
    if (!eval(t, slot_new, &f_new, &gtd_new)) { r.failed = true; return r; }
    int ls_func_evals = 1;

    double bracket[2] = {0.0, 0.0}, bracket_f[2] = {0.0, 0.0}, bracket_gtd[2] = {0.0, 0.0};
    int bracket_slot[2] = {-1, -1}, n_bracket = 0;
    auto free_slot = [&](int a, int b) { for (int s = 0; s < 3; ++s) if (s != a && s != b) return s; return 0; };

    // bracket an interval containing a point satisfying the Wolfe criteria
    double t_prev = 0.0, f_prev = f, gtd_prev = gtd;
    int slot_prev = -1;
    bool done = false;
    int ls_iter = 0;
    while (ls_iter < max_ls) {
        if (f_new > (f + c1 * t * gtd) || (ls_iter > 1 && f_new >= f_prev) ) {
            bracket[0] = t_prev; bracket[1] = t; bracket_f[0] = f_prev; bracket_f[1] = f_new;
            bracket_gtd[0] = gtd_prev; bracket_gtd[1] = gtd_new; bracket_slot[0] = slot_prev; bracket_slot[1] = slot_new;
            n_bracket = 2;
            break;
        }
        if (std::fabs(gtd_new) <= -c2 * gtd) {
            bracket[0] = t; bracket_f[0] = f_new; bracket_gtd[0] = gtd_new; bracket_slot[0] = slot_new;
            n_bracket = 1;
            done = true;
            break;
        }
        if (gtd_new >= 0.0) {
            bracket[0] = t_prev; bracket[1] = t; bracket_f[0] = f_prev; bracket_f[1] = f_new;
            bracket_gtd[0] = gtd_prev; bracket_gtd[1] = gtd_new; bracket_slot[0] = slot_prev; bracket_slot[1] = slot_new;
            n_bracket = 2;
            break;
        }
        // interpolate
        const double min_step = t + 0.01 * (t - t_prev), max_step = t * 10.0, tmp = t;
        t = cubic_interpolate(t_prev, f_prev, gtd_prev, t, f_new, gtd_new, min_step, max_step);
        // next step
        t_prev = tmp; f_prev = f_new; gtd_prev = gtd_new; slot_prev = slot_new;
        slot_new = free_slot(slot_prev, -1);
        if (!eval(t, slot_new, &f_new, &gtd_new)) { r.failed = true; r.evals = ls_func_evals; return r; }
        ls_func_evals += 1;
        ls_iter += 1;
    }
    // reached max number of iterations?
    if (ls_iter == max_ls) {
        bracket[0] = 0.0; bracket[1] = t; bracket_f[0] = f; bracket_f[1] = f_new;
        bracket_gtd[0] = gtd; bracket_gtd[1] = gtd_new; bracket_slot[0] = -1; bracket_slot[1] = slot_new;
        n_bracket = 2;
    }

    // zoom phase: a point satisfying the criteria, or a bracket around one, is at hand; the bracket is refined until the point is found
    bool insuf_progress = false;
    int low_pos = bracket_f[0] <= bracket_f[n_bracket - 1] ? 0 : 1, high_pos = 1 - low_pos;
    while (!done && ls_iter < max_ls) {
        // the bracket is so small
        if (std::fabs(bracket[1] - bracket[0]) * d_norm < p.tolerance_change) break;
        // new trial value
        t = cubic_interpolate(bracket[0], bracket_f[0], bracket_gtd[0], bracket[1], bracket_f[1], bracket_gtd[1]);
        // sufficient progress: a `t` this close to an end of the bracket is moved 0.1 of its length inside, if the step before
        // was as close or `t` sits on the end itself
        const double b_max = py_max(bracket[0], bracket[1]), b_min = py_min(bracket[0], bracket[1]);
        const double eps = 0.1 * (b_max - b_min);
        if (py_min(b_max - t, t - b_min) < eps) {
            if (insuf_progress || t >= b_max || t <= b_min) {
                t = std::fabs(t - b_max) < std::fabs(t - b_min) ? b_max - eps : b_min + eps;
                insuf_progress = false;
            } else {
                insuf_progress = true;
            }
        } else {
            insuf_progress = false;
        }
        // evaluate the new point
        slot_new = free_slot(bracket_slot[0], bracket_slot[1]);
        if (!eval(t, slot_new, &f_new, &gtd_new)) { r.failed = true; r.evals = ls_func_evals; return r; }
        ls_func_evals += 1;
        ls_iter += 1;

        if (f_new > (f + c1 * t * gtd) || f_new >= bracket_f[low_pos]) {
            // Armijo condition not satisfied, or not lower than the lowest point
            bracket[high_pos] = t; bracket_f[high_pos] = f_new; bracket_gtd[high_pos] = gtd_new; bracket_slot[high_pos] = slot_new;
            low_pos = bracket_f[0] <= bracket_f[1] ? 0 : 1;
            high_pos = 1 - low_pos;
        } else {
            if (std::fabs(gtd_new) <= -c2 * gtd) {
                done = true;      // Wolfe conditions satisfied
            } else if (gtd_new * (bracket[high_pos] - bracket[low_pos]) >= 0.0) {
                // old low becomes new high
                bracket[high_pos] = bracket[low_pos]; bracket_f[high_pos] = bracket_f[low_pos];
                bracket_gtd[high_pos] = bracket_gtd[low_pos]; bracket_slot[high_pos] = bracket_slot[low_pos];
            }
            // new point becomes new low
            bracket[low_pos] = t; bracket_f[low_pos] = f_new; bracket_gtd[low_pos] = gtd_new; bracket_slot[low_pos] = slot_new;
        }
    }
    if (n_bracket == 1) low_pos = 0;
    r.t = bracket[low_pos]; r.f = bracket_f[low_pos]; r.gtd = bracket_gtd[low_pos]; r.slot = bracket_slot[low_pos];
    r.evals = ls_func_evals;
    r.wolfe = done;
    r.exhausted = !done && ls_iter >= max_ls;
    return r;
}

}  // namespace hpv_ls
