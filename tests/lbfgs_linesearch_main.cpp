// Stand-alone program around hp_vpinns_amd/csrc/hpv_linesearch.h for tests/test_lbfgs_host.py: runs the strong-Wolfe search on a
// fixed set of 1-D functions phi(t) with analytic derivatives and prints every trial step and the point returned, 17 digits each.
// The same functions, with the same operation order, stand in the test, which runs the reference implementation on them.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

#include "hpv_linesearch.h"

namespace {

struct Case {
    const char* name;
    double (*phi)(double);
    double (*dphi)(double);
    double t0;
    int max_ls;
};

// convex quadratics a (t - c)^2: the minimum inside, (far) before and beyond the first step
double q_in(double t) { return 2.0 * (t - 0.5) * (t - 0.5); }
double dq_in(double t) { return 4.0 * (t - 0.5); }
double q_before(double t) { return 3.0 * (t - 0.05) * (t - 0.05); }
double dq_before(double t) { return 6.0 * (t - 0.05); }
double q_beyond(double t) { return 0.5 * (t - 7.3) * (t - 7.3); }
double dq_beyond(double t) { return t - 7.3; }
// quartic double well ((t - 1.7)^2 - 1)^2 - 0.1 t
double well(double t) { const double u = (t - 1.7) * (t - 1.7) - 1.0; return u * u - 0.1 * t; }
double dwell(double t) { const double u = (t - 1.7) * (t - 1.7) - 1.0; return 4.0 * (t - 1.7) * u - 0.1; }
// exp(-t) + t^2 / 10
double expq(double t) { return std::exp(-t) + t * t / 10.0; }
double dexpq(double t) { return -std::exp(-t) + t / 5.0; }
// a pole at t = 0.7, +inf at and beyond it: the first trial (t = 1) is not finite
double pole(double t) { return t < 0.7 ? 1.0 / (0.7 - t) - 6.0 * t : std::numeric_limits<double>::infinity(); }
double dpole(double t) { return t < 0.7 ? 1.0 / ((0.7 - t) * (0.7 - t)) - 6.0 : std::numeric_limits<double>::infinity(); }

const Case CASES[] = {
    {"quadratic_inside", q_in, dq_in, 1.0, 25},   {"quadratic_before", q_before, dq_before, 1.0, 25},
    {"quadratic_beyond", q_beyond, dq_beyond, 1.0, 25}, {"double_well", well, dwell, 1.0, 25},
    {"exp_quadratic", expq, dexpq, 0.1, 25},     {"nonfinite_first", pole, dpole, 1.0, 25},
    {"exhausts_max_ls", expq, dexpq, 1e-3, 3},
};

}  // namespace

int main(int argc, char** argv) {
    for (const Case& c : CASES) {
        if (argc > 1 && std::strcmp(argv[1], c.name) != 0) continue;
        std::printf("case %s\n", c.name);
        auto eval = [&](double t, int slot, double* f, double* gtd) {
            *f = c.phi(t); *gtd = c.dphi(t);
            std::printf("trial %.17g slot %d\n", t, slot);
            return true;
        };
        hpv_ls::Params p;
        p.max_ls = c.max_ls;
        const hpv_ls::Result r = hpv_ls::strong_wolfe(eval, c.t0, 1.0, c.phi(0.0), c.dphi(0.0), p);
        std::printf("result %.17g %.17g %.17g evals %d wolfe %d exhausted %d slot %d\n", r.t, r.f, r.gtd, r.evals, (int)r.wolfe,
                    (int)r.exhausted, r.slot);
    }
    return 0;
}
