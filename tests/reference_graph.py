"""The cases behind the `*_graph.npz` fixtures: what the reference's OWN VPINN classes computed (tests/golden/make_golden.py runs
their bodies verbatim on tests/golden/tf1_shim.py) -- loss triple, gradient, K Adam updates with the loss read after each, the
parameters after them and a strided prediction, all from one stored theta0.  A plain helper module like cases.py; no GPU needed.
tests/test_oracle.py holds the oracle against these numbers (1e-11), tests/test_gpu_reference_graph.py the HIP path (the figures of
DESIGN section 2).  Keys of a case inside its file: `<form>_<name>`, form = vf0 | vf1 | vf2 | vf3 | pinn."""
import numpy as np

import generic_point as gp
from cases import gold, p1_args, p2_args, p3_args

K = 6
MASK_REL, MASK_CAP = 1e-9, 0.05      # the mask of test_gpu_fuzz._against_oracle, and the share of entries it may take out

# (problem, tag, form, trajectory and prediction stored)
CASES = [
    ("poisson1d", "small", "vf1", True), ("poisson1d", "small", "vf2", True), ("poisson1d", "small", "vf3", True),
    ("poisson2d", "small", "vf0", True), ("poisson2d", "small", "vf1", True), ("poisson2d", "small", "vf2", True),
    ("poisson2d", "small", "pinn", True),
    ("advdiff", "small", "vf0", True), ("advdiff", "small", "vf1", True),
    ("poisson2d", "e2", "vf2", False),
]
FILES = sorted({"%s_%s_graph" % c[:2] for c in CASES})


def case_id(c):
    return "%s-%s-%s" % c[:3]


def load(c):
    """{name: array} of one case, and the set-up fixture of its tag"""
    f = gold("%s_%s_graph" % c[:2])
    pre = c[2] + "_"
    return {k[len(pre):]: f[k] for k in f.files if k.startswith(pre)}, gold("%s_%s" % c[:2])


def setup(c):
    """(positional arguments shared by the oracle and the product class, keyword arguments, layers, n_extra)"""
    d, g = load(c)
    problem, form = c[0], c[2]
    vf = 1 if form == "pinn" else int(form[2:])
    if problem == "poisson1d":
        a = p1_args(g)
        return a, dict(var_form=vf, lossb_weight=float(g["lossb_weight"]), LR=float(g["LR"])), a[8], 0
    if problem == "poisson2d":
        a = p2_args(g)
        return a, dict(var_form=vf, scheme="PINNs" if form == "pinn" else "VPINNs"), a[13], 0
    a = p3_args(g)
    return a, dict(var_form=vf, V=float(g["V"]), LR=float(g["LR"])), a[12], 1


def oracle(c):
    from oracle import vpinn_oracle as O
    a, kw, _, _ = setup(c)
    cls = {"poisson1d": O.OracleVPINN1D, "poisson2d": O.OracleVPINN2D, "advdiff": O.OracleVPINNAdvDiff}[c[0]]
    return cls(*a, init_params=load(c)[0]["theta0"], **kw)


def product(c, **more):
    from hp_vpinns_amd import vpinn
    a, kw, _, _ = setup(c)
    cls = {"poisson1d": vpinn.VPINN1D, "poisson2d": vpinn.VPINN2D, "advdiff": vpinn.VPINNAdvDiff}[c[0]]
    return cls(*a, init_params=load(c)[0]["theta0"], **kw, **more)


def step_mask(d):
    """the entries compared after Adam updates (|g| above MASK_REL of the largest); asserts the fixture's condition that the mask
    takes out at most MASK_CAP of them"""
    g = d["grad"]
    big = np.abs(g) > MASK_REL * np.abs(g).max()
    assert 1.0 - big.mean() <= MASK_CAP, ("the fixture masks %.3f of the gradient entries" % (1.0 - big.mean()))
    return big


def scalar_rel(a, b):
    """largest relative error of the entries of a against b"""
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    return float(np.max(np.abs(a - b) / np.abs(b)))


def gaps(d, layers, n_extra, l3, g, his=None, theta=None, pred=None):
    """dict of the measured gaps of (l3, g, his, theta, pred) against the fixture `d`"""
    out = {"loss3": scalar_rel(l3, d["loss3"])}
    out["block"], out["grad"] = gp.worst_block(g, d["grad"], layers, n_extra)
    if n_extra:
        out["d_eps"] = scalar_rel(g[-1], d["grad"][-1])
    if his is not None:
        big = step_mask(d)
        n = d["theta0"].size - n_extra
        out["his"] = scalar_rel(his, d["loss_his"])
        out["theta"] = float(np.linalg.norm((theta - d["theta_K"])[:n][big[:n]]) / np.linalg.norm(d["theta_K"][:n][big[:n]]))
        if n_extra:
            out["eps"] = scalar_rel(theta[-1], d["theta_K"][-1])
        out["pred"] = float(np.linalg.norm(np.ravel(pred) - np.ravel(d["u_pred"])) / np.linalg.norm(d["u_pred"]))
    return out
