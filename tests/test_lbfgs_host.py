"""The host side of the L-BFGS stage, on the CPU: the strong-Wolfe search of csrc/hpv_linesearch.h as a stand-alone program (built
with the address and undefined-behaviour sanitizers) against torch's own routine on the same 1-D functions, and the numpy / torch
references of tests/lbfgs_reference.py against independent facts."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import lbfgs_reference as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")

# name -> (phi, phi', first step, max_ls): the functions of tests/lbfgs_linesearch_main.cpp, operation for operation
FUNCS = {
    "quadratic_inside": (lambda t: 2.0 * (t - 0.5) * (t - 0.5), lambda t: 4.0 * (t - 0.5), 1.0, 25),
    "quadratic_before": (lambda t: 3.0 * (t - 0.05) * (t - 0.05), lambda t: 6.0 * (t - 0.05), 1.0, 25),
    "quadratic_beyond": (lambda t: 0.5 * (t - 7.3) * (t - 7.3), lambda t: t - 7.3, 1.0, 25),
    "double_well": (lambda t: ((t - 1.7) * (t - 1.7) - 1.0) * ((t - 1.7) * (t - 1.7) - 1.0) - 0.1 * t,
                    lambda t: 4.0 * (t - 1.7) * ((t - 1.7) * (t - 1.7) - 1.0) - 0.1, 1.0, 25),
    "exp_quadratic": (lambda t: math.exp(-t) + t * t / 10.0, lambda t: -math.exp(-t) + t / 5.0, 0.1, 25),
    "nonfinite_first": (lambda t: 1.0 / (0.7 - t) - 6.0 * t if t < 0.7 else INF,
                        lambda t: 1.0 / ((0.7 - t) * (0.7 - t)) - 6.0 if t < 0.7 else INF, 1.0, 25),
    "exhausts_max_ls": (lambda t: math.exp(-t) + t * t / 10.0, lambda t: -math.exp(-t) + t / 5.0, 1e-3, 3),
}


@pytest.fixture(scope="module")
def program_output(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the line-search program"
    exe = str(tmp_path_factory.mktemp("ls") / "lbfgs_linesearch")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-Wall", "-Werror", "-I", os.path.join(ROOT, "hp_vpinns_amd", "csrc"),
                    os.path.join(ROOT, "tests", "lbfgs_linesearch_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and not r.stderr, r.stderr
    out, cur = {}, None
    for line in r.stdout.splitlines():
        w = line.split()
        if w[0] == "case":
            cur = out.setdefault(w[1], dict(trials=[], slots=[]))
        elif w[0] == "trial":
            cur["trials"].append(float(w[1]))
            cur["slots"].append(int(w[3]))
        else:
            cur.update(t=float(w[1]), f=float(w[2]), gtd=float(w[3]), evals=int(w[5]), wolfe=int(w[7]), exhausted=int(w[9]), slot=int(w[11]))
    return out


def _torch_search(name):
    import torch
    from torch.optim.lbfgs import _strong_wolfe
    phi, dphi, t0, max_ls = FUNCS[name]
    trials = []

    def obj(x, t, d):
        t = float(t)
        trials.append(t)
        return phi(t), torch.tensor([dphi(t)], dtype=torch.float64)

    d = torch.tensor([1.0], dtype=torch.float64)
    g = torch.tensor([dphi(0.0)], dtype=torch.float64)
    f_new, g_new, t, n = _strong_wolfe(obj, [torch.zeros(1, dtype=torch.float64)], t0, d, phi(0.0), g, g.dot(d), max_ls=max_ls)
    return trials, float(t), float(f_new), float(g_new[0]), int(n)


@pytest.mark.parametrize("name", list(FUNCS))
def test_line_search_takes_torchs_steps(program_output, name):
    """The same number of evaluations and the same trial steps to 1e-14 relative (it is the same scalar arithmetic), the same point
    returned; torch's routine itself ends normally on every function (it returns, with finite values)."""
    trials, t, f, gtd, n = _torch_search(name)
    assert math.isfinite(t) and math.isfinite(f) and math.isfinite(gtd) and n == len(trials)
    mine = program_output[name]
    print(name, "torch", trials, "| program", mine["trials"])
    assert mine["evals"] == n == len(mine["trials"])
    for a, b in zip(mine["trials"], trials):
        assert abs(a - b) <= 1e-14 * abs(b), (a, b)
    assert abs(mine["t"] - t) <= 1e-14 * abs(t) and abs(mine["f"] - f) <= 1e-13 * max(abs(f), 1.0) and abs(mine["gtd"] - gtd) <= 1e-12 * max(abs(gtd), 1.0)
    phi, dphi, _, max_ls = FUNCS[name]
    f0, g0 = phi(0.0), dphi(0.0)
    if mine["wolfe"]:
        assert mine["f"] <= f0 + 1e-4 * mine["t"] * g0 and abs(mine["gtd"]) <= -0.9 * g0
    assert mine["exhausted"] == (1 if name == "exhausts_max_ls" else 0) and mine["wolfe"] == (0 if name == "exhausts_max_ls" else 1)
    # the gradient slots: a trial never takes the slot of a point that may still be returned, and the point returned names its own
    assert all(0 <= s <= 2 for s in mine["slots"])
    if mine["t"] != 0.0:
        k = max(i for i, a in enumerate(mine["trials"]) if a == mine["t"])
        assert mine["slot"] == mine["slots"][k] and mine["slot"] not in mine["slots"][k + 1:]


def test_first_trial_is_not_finite_where_it_should_be(program_output):
    assert FUNCS["nonfinite_first"][0](FUNCS["nonfinite_first"][2]) == INF and len(program_output["nonfinite_first"]["trials"]) > 1


@pytest.mark.parametrize("P,n", [(7, 0), (7, 1), (12, 5), (12, 12)])
def test_two_loop_is_the_dense_bfgs_product(P, n):
    rng = np.random.default_rng(100 * P + n)
    A = rng.standard_normal((P, P))
    A = A @ A.T + P * np.eye(P)                     # SPD: y = A s has y . s > 0
    S = rng.standard_normal((n, P))
    Y = S @ A
    g = rng.standard_normal(P)
    d, dd = lr.two_loop(S, Y, g), lr.dense_bfgs_direction(S, Y, g)
    assert np.linalg.norm(d - dd) <= 1e-11 * np.linalg.norm(dd)
    if n == 0:
        assert np.array_equal(d, -g)


def test_torch_lbfgs_reaches_the_rosenbrock_minimiser():
    def rosen(x):
        f = float(np.sum(100.0 * (x[1:] - x[:-1] ** 2) ** 2 + (1.0 - x[:-1]) ** 2))
        g = np.zeros_like(x)
        g[:-1] = -400.0 * x[:-1] * (x[1:] - x[:-1] ** 2) - 2.0 * (1.0 - x[:-1])
        g[1:] += 200.0 * (x[1:] - x[:-1] ** 2)
        return f, g
    out = lr.torch_lbfgs(rosen, np.full(16, -0.5), max_iter=400, history=20, max_eval=1000)
    assert np.abs(out["theta"] - 1.0).max() < 1e-5, out["theta"]
    # (within 1e-5 of the minimiser in every variable the function is below 0.5 * 1002 * 16 * 1e-10 < 1e-6: its Hessian there has
    #  no eigenvalue above 1002)
    assert out["func_evals"] == len(out["evals"]) and out["losses"][-1] < 1e-6
    assert all(b <= a for a, b in zip(out["losses"], out["losses"][1:]))
