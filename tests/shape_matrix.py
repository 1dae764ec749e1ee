"""The table of cases behind tests/test_shape_matrix_host.py (CPU) and tests/test_gpu_shape_matrix.py (GPU): one case per forward /
reverse pair of the per-layer MFMA kernels the dispatch tables instantiate -- k_fwd_mfma / k_bwd_mfma (csrc/kernels_mfma.hip, H = 20)
and k_fwd_wide / k_bwd_wide (csrc/kernels_wide.hip, H = 24 .. 64), templates over <D, NT1, NT2, act, L, H>.  A plain helper module
like cases.py and generic_point.py; no GPU needed.

Rows (the channel set D / NT1 / NT2 and the public configuration that reaches it):

  adv-pinn   221 tanh   VPINNAdvDiff(scheme="PINNs"), V = 0.6, epsilon = 0.9, lossb_weight = 3          full (H, L) grid
  p1-pinn    111 sin    VPINN1D(scheme="PINNs"), seeded random f_train                                   full grid
  p2-pinn    221 tanh   VPINN2D(scheme="PINNs"): the SAME instantiation as adv-pinn (the mixed second tangent u_xx + u_yy is a
                        run-time weight, NetDesc::t2w), so: every H at L = 3 and every L at H = 32
  p2-vf1     220 tanh   VPINN2D var_form 1 under HPV_FUSE=n (the layer kernels run at H = 20 as well)    full grid
  p2-vf2     200 tanh   VPINN2D var_form 2, HPV_FUSE=n                                                   full grid
  p1-vf2     110 sin    VPINN1D var_form 2, HPV_FUSE=n                                                   full grid
  p1-vf3     100 sin    VPINN1D var_form 3 (with its element-edge batch), HPV_FUSE=n                     full grid

  222 has no row: since Poisson-2D var_form 0 runs on four channels no public configuration launches k_bwd_*<D=2,NT1=2,NT2=2,..>; the
  forward half alone is reached by hpv_eval_channels on that form (profiles/shape_matrix.md).

Strong-form inputs: 17 seeded uniform collocation points in the domain (one full 16-point tile and a one-point tail), 7 data points
with seeded random u, seeded random right-hand sides.  Variational inputs: gp.warp_* grids -- 2 x 2 elements of 5 x 5 points with
(2, 3) test functions in 2-D, 3 elements of 10 points with 4 test functions in 1-D (seeded random F there: the driver's own is ~1e2
and hides the two boundary points) -- with HPV_NO_RULE_PADDING=1 beside HPV_FUSE=n, so that the device sees the rule as it is.
Parameters: gp.generic_theta with the scale of SCALE[H] (0.3 sqrt(20 / H): the perturbation's share of a pre-activation does not
grow with the width).

Seeds: per case the first of base, base + 1000, .. (at most five) at which the REFERENCE ALONE meets the conditions that
test_shape_matrix_host.py checks (every block >= gp.BLOCK_FLOOR of the gradient, both loss terms >= 1e-3 of the loss, two CPU
restatements within 1e-11 per block); base = 7000 + 100 * (row index) + (case index in the row).  scripts/shape_matrix_seeds.py does
that search and prints SEEDS; the literals below are its output."""
import functools

import numpy as np

import generic_point as gp

WIDTHS = (20, 24, 32, 40, 48, 64)                      # init.MFMA_WIDTH + init.WIDE_WIDTHS (= WIDE_WIDTHS of csrc/build.sh)
SCALE = {20: 0.3, 24: 0.27, 32: 0.24, 40: 0.21, 48: 0.19, 64: 0.17}
V, EPS0, LBW = 0.6, 0.9, 3
N_COLLOCATION, N_DATA = 17, 7
MAX_TRIES = 5
BLOCK_AGREE = 1e-11                                    # two CPU restatements, per block
TERM_FLOOR = 1e-3                                      # each loss term's share of the loss
VAR_ENV = {"HPV_FUSE": "n", "HPV_NO_RULE_PADDING": "1"}


def max_depth(H):
    """hidden layers the kernels are instantiated for at width H (init.pad_plan's rule; hpv_mfma_create's)"""
    return 6 if H <= 32 else 4


FULL = [(H, L) for H in WIDTHS for L in range(1, max_depth(H) + 1)]
CROSS = [(H, 3) for H in WIDTHS] + [(32, L) for L in range(1, 7) if L != 3]

# row -> (D, NT1, NT2, activation, problem, kind, var_form, the (H, L) it runs at)
ROWS = {
    "adv-pinn": (2, 2, 1, "tanh", "adv", "pinn", 0, FULL),
    "p1-pinn": (1, 1, 1, "sin", "p1", "pinn", 1, FULL),
    "p2-pinn": (2, 2, 1, "tanh", "p2", "pinn", 1, CROSS),
    "p2-vf1": (2, 2, 0, "tanh", "p2", "var", 1, FULL),
    "p2-vf2": (2, 0, 0, "tanh", "p2", "var", 2, FULL),
    "p1-vf2": (1, 1, 0, "sin", "p1", "var", 2, FULL),
    "p1-vf3": (1, 0, 0, "sin", "p1", "var", 3, FULL),
}
DEAD_SETS = ["222"]                                    # instantiated by pick_L / pick_wide_key, reached by no public configuration
INSTANTIATED_SETS = ["111", "110", "100", "222", "220", "200", "221"]      # the keys of pick_L (kernels_mfma.hip) / pick_wide_key

# the zero-padded networks of part 4: name -> (row-like tuple, user layers, device width)
PADDED = {
    "pad-adv-pinn-[2,21,7,1]": ((2, 2, 1, "tanh", "adv", "pinn", 0), [2, 21, 7, 1], 24),
    "pad-p1-pinn-[1,7,5,1]": ((1, 1, 1, "sin", "p1", "pinn", 1), [1, 7, 5, 1], 20),
    "pad-p2-vf1-[2,12,12,1]": ((2, 2, 0, "tanh", "p2", "var", 1), [2, 12, 12, 1], 20),
    "pad-p2-vf0-[2,33,50,12,1]": ((2, 2, 1, "tanh", "p2", "var", 0), [2, 33, 50, 12, 1], 64),
    "pad-p1-vf1-[1,30,30,30,30,30,1]": ((1, 1, 1, "sin", "p1", "var", 1), [1, 30, 30, 30, 30, 30, 1], 32),
}

# ---- the chosen seeds (scripts/shape_matrix_seeds.py prints this block) -------------------------------------------------------------
SEEDS = {
    "adv-pinn-H20-L1": 7000, "adv-pinn-H20-L2": 7001, "adv-pinn-H20-L3": 7002, "adv-pinn-H20-L4": 7003,
    "adv-pinn-H20-L5": 7004, "adv-pinn-H20-L6": 7005, "adv-pinn-H24-L1": 7006, "adv-pinn-H24-L2": 7007,
    "adv-pinn-H24-L3": 7008, "adv-pinn-H24-L4": 7009, "adv-pinn-H24-L5": 7010, "adv-pinn-H24-L6": 7011,
    "adv-pinn-H32-L1": 7012, "adv-pinn-H32-L2": 7013, "adv-pinn-H32-L3": 7014, "adv-pinn-H32-L4": 7015,
    "adv-pinn-H32-L5": 7016, "adv-pinn-H32-L6": 7017, "adv-pinn-H40-L1": 7018, "adv-pinn-H40-L2": 7019,
    "adv-pinn-H40-L3": 7020, "adv-pinn-H40-L4": 7021, "adv-pinn-H48-L1": 7022, "adv-pinn-H48-L2": 7023,
    "adv-pinn-H48-L3": 7024, "adv-pinn-H48-L4": 7025, "adv-pinn-H64-L1": 7026, "adv-pinn-H64-L2": 7027,
    "adv-pinn-H64-L3": 7028, "adv-pinn-H64-L4": 7029, "p1-pinn-H20-L1": 7100, "p1-pinn-H20-L2": 7101,
    "p1-pinn-H20-L3": 7102, "p1-pinn-H20-L4": 7103, "p1-pinn-H20-L5": 7104, "p1-pinn-H20-L6": 7105,
    "p1-pinn-H24-L1": 7106, "p1-pinn-H24-L2": 7107, "p1-pinn-H24-L3": 7108, "p1-pinn-H24-L4": 7109,
    "p1-pinn-H24-L5": 7110, "p1-pinn-H24-L6": 7111, "p1-pinn-H32-L1": 7112, "p1-pinn-H32-L2": 7113,
    "p1-pinn-H32-L3": 7114, "p1-pinn-H32-L4": 7115, "p1-pinn-H32-L5": 7116, "p1-pinn-H32-L6": 7117,
    "p1-pinn-H40-L1": 7118, "p1-pinn-H40-L2": 7119, "p1-pinn-H40-L3": 7120, "p1-pinn-H40-L4": 7121,
    "p1-pinn-H48-L1": 7122, "p1-pinn-H48-L2": 7123, "p1-pinn-H48-L3": 7124, "p1-pinn-H48-L4": 7125,
    "p1-pinn-H64-L1": 7126, "p1-pinn-H64-L2": 7127, "p1-pinn-H64-L3": 7128, "p1-pinn-H64-L4": 7129,
    "p2-pinn-H20-L3": 7200, "p2-pinn-H24-L3": 7201, "p2-pinn-H32-L3": 7202, "p2-pinn-H40-L3": 7203,
    "p2-pinn-H48-L3": 7204, "p2-pinn-H64-L3": 7205, "p2-pinn-H32-L1": 7206, "p2-pinn-H32-L2": 7207,
    "p2-pinn-H32-L4": 7208, "p2-pinn-H32-L5": 7209, "p2-pinn-H32-L6": 7210, "p2-vf1-H20-L1": 7300,
    "p2-vf1-H20-L2": 7301, "p2-vf1-H20-L3": 7302, "p2-vf1-H20-L4": 7303, "p2-vf1-H20-L5": 7304,
    "p2-vf1-H20-L6": 7305, "p2-vf1-H24-L1": 7306, "p2-vf1-H24-L2": 7307, "p2-vf1-H24-L3": 7308,
    "p2-vf1-H24-L4": 7309, "p2-vf1-H24-L5": 7310, "p2-vf1-H24-L6": 7311, "p2-vf1-H32-L1": 7312,
    "p2-vf1-H32-L2": 7313, "p2-vf1-H32-L3": 7314, "p2-vf1-H32-L4": 7315, "p2-vf1-H32-L5": 7316,
    "p2-vf1-H32-L6": 7317, "p2-vf1-H40-L1": 7318, "p2-vf1-H40-L2": 7319, "p2-vf1-H40-L3": 7320,
    "p2-vf1-H40-L4": 7321, "p2-vf1-H48-L1": 7322, "p2-vf1-H48-L2": 7323, "p2-vf1-H48-L3": 7324,
    "p2-vf1-H48-L4": 7325, "p2-vf1-H64-L1": 7326, "p2-vf1-H64-L2": 7327, "p2-vf1-H64-L3": 7328,
    "p2-vf1-H64-L4": 7329, "p2-vf2-H20-L1": 7400, "p2-vf2-H20-L2": 7401, "p2-vf2-H20-L3": 7402,
    "p2-vf2-H20-L4": 7403, "p2-vf2-H20-L5": 7404, "p2-vf2-H20-L6": 7405, "p2-vf2-H24-L1": 7406,
    "p2-vf2-H24-L2": 7407, "p2-vf2-H24-L3": 7408, "p2-vf2-H24-L4": 7409, "p2-vf2-H24-L5": 7410,
    "p2-vf2-H24-L6": 7411, "p2-vf2-H32-L1": 7412, "p2-vf2-H32-L2": 7413, "p2-vf2-H32-L3": 7414,
    "p2-vf2-H32-L4": 7415, "p2-vf2-H32-L5": 7416, "p2-vf2-H32-L6": 7417, "p2-vf2-H40-L1": 7418,
    "p2-vf2-H40-L2": 7419, "p2-vf2-H40-L3": 7420, "p2-vf2-H40-L4": 7421, "p2-vf2-H48-L1": 7422,
    "p2-vf2-H48-L2": 7423, "p2-vf2-H48-L3": 7424, "p2-vf2-H48-L4": 7425, "p2-vf2-H64-L1": 7426,
    "p2-vf2-H64-L2": 7427, "p2-vf2-H64-L3": 7428, "p2-vf2-H64-L4": 7429, "p1-vf2-H20-L1": 7500,
    "p1-vf2-H20-L2": 7501, "p1-vf2-H20-L3": 7502, "p1-vf2-H20-L4": 7503, "p1-vf2-H20-L5": 7504,
    "p1-vf2-H20-L6": 7505, "p1-vf2-H24-L1": 7506, "p1-vf2-H24-L2": 7507, "p1-vf2-H24-L3": 7508,
    "p1-vf2-H24-L4": 7509, "p1-vf2-H24-L5": 7510, "p1-vf2-H24-L6": 7511, "p1-vf2-H32-L1": 7512,
    "p1-vf2-H32-L2": 7513, "p1-vf2-H32-L3": 7514, "p1-vf2-H32-L4": 7515, "p1-vf2-H32-L5": 7516,
    "p1-vf2-H32-L6": 7517, "p1-vf2-H40-L1": 7518, "p1-vf2-H40-L2": 7519, "p1-vf2-H40-L3": 7520,
    "p1-vf2-H40-L4": 7521, "p1-vf2-H48-L1": 7522, "p1-vf2-H48-L2": 7523, "p1-vf2-H48-L3": 7524,
    "p1-vf2-H48-L4": 7525, "p1-vf2-H64-L1": 7526, "p1-vf2-H64-L2": 7527, "p1-vf2-H64-L3": 7528,
    "p1-vf2-H64-L4": 7529, "p1-vf3-H20-L1": 7600, "p1-vf3-H20-L2": 7601, "p1-vf3-H20-L3": 7602,
    "p1-vf3-H20-L4": 7603, "p1-vf3-H20-L5": 7604, "p1-vf3-H20-L6": 7605, "p1-vf3-H24-L1": 7606,
    "p1-vf3-H24-L2": 7607, "p1-vf3-H24-L3": 7608, "p1-vf3-H24-L4": 7609, "p1-vf3-H24-L5": 7610,
    "p1-vf3-H24-L6": 7611, "p1-vf3-H32-L1": 7612, "p1-vf3-H32-L2": 7613, "p1-vf3-H32-L3": 7614,
    "p1-vf3-H32-L4": 7615, "p1-vf3-H32-L5": 7616, "p1-vf3-H32-L6": 7617, "p1-vf3-H40-L1": 7618,
    "p1-vf3-H40-L2": 7619, "p1-vf3-H40-L3": 7620, "p1-vf3-H40-L4": 7621, "p1-vf3-H48-L1": 7622,
    "p1-vf3-H48-L2": 7623, "p1-vf3-H48-L3": 7624, "p1-vf3-H48-L4": 7625, "p1-vf3-H64-L1": 7626,
    "p1-vf3-H64-L2": 7627, "p1-vf3-H64-L3": 7628, "p1-vf3-H64-L4": 7629,
}
PADDED_SEEDS = {
    "pad-adv-pinn-[2,21,7,1]": 7900, "pad-p1-pinn-[1,7,5,1]": 7901, "pad-p2-vf1-[2,12,12,1]": 7902, "pad-p2-vf0-[2,33,50,12,1]": 7903,
    "pad-p1-vf1-[1,30,30,30,30,30,1]": 7904,
}
# ---- end of the generated block --------------------------------------------------------------------------------------------------


def base_seed(row, i):
    return 7000 + 100 * list(ROWS).index(row) + i


def variant_strings(D, NT1, NT2, act, L, H):
    """the exact names hpv_kernel_variant() reports for the pair"""
    fam = "mfma" if H == 20 else "wide"
    args = "<D=%d,NT1=%d,NT2=%d,%s,L=%d,H=%d>" % (D, NT1, NT2, act, L, H)
    return "k_fwd_" + fam + args, "k_bwd_" + fam + args


def _case(name, row, spec, layers, H, seed):
    D, NT1, NT2, act, prob, kind, vf = spec
    L = len(layers) - 2
    fwd, bwd = variant_strings(D, NT1, NT2, act, L, H)
    return dict(name=name, row=row, set="%d%d%d" % (D, NT1, NT2), H=H, L=L, layers=list(layers), prob=prob, kind=kind, vf=vf,
                seed=seed, scale=SCALE[H], fwd=fwd, bwd=bwd, env=dict(VAR_ENV) if kind == "var" else {},
                n_extra=1 if prob == "adv" else 0)


def matrix_cases(seeds=None):
    """one case dict per (row, H, L); `seeds` overrides SEEDS (the seed search)"""
    seeds = SEEDS if seeds is None else seeds
    out = []
    for row, spec in ROWS.items():
        for i, (H, L) in enumerate(spec[7]):
            name = "%s-H%d-L%d" % (row, H, L)
            out.append(_case(name, row, spec[:7], [spec[0]] + [H] * L + [1], H, seeds.get(name, base_seed(row, i))))
    return out


def padded_cases(seeds=None):
    seeds = PADDED_SEEDS if seeds is None else seeds
    return [_case(name, "padded", spec, layers, H, seeds.get(name, 7900 + i))
            for i, (name, (spec, layers, H)) in enumerate(PADDED.items())]


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _base_setup(prob, kind):
    """the drivers' setup dicts (tiny); the strong-form cases only borrow the arrays the constructors insist on"""
    from hp_vpinns_amd.drivers import advdiff, poisson1d, poisson2d
    if prob == "p1":
        return poisson1d.setup(N_Element=3, N_testfcn=4, N_Quad=10, N_F=N_COLLOCATION)
    if prob == "p2":
        return poisson2d.setup(N_el_x=2, N_el_y=2, N_test_x=2, N_test_y=3, N_quad=5, N_bound=7, with_test_grid=False)
    return advdiff.setup(N_el_x=2, N_el_t=2, N_test_x=2, N_test_t=3, N_quad=5, N_bound=7, with_test_grid=False)


def _uniform(rng, n, prob):
    if prob == "p1":
        return rng.uniform(-1, 1, (n, 1))
    lo, hi = (np.array([-1.0, 0.0]), np.array([1.0, 1.0])) if prob == "adv" else (np.array([-1.0, -1.0]), np.array([1.0, 1.0]))
    return lo + (hi - lo) * rng.uniform(size=(n, 2))


def inputs(c):
    """dict(a = positional arguments of the product class and of the oracle class, kw = keyword arguments of the product class, th =
    initial parameters, Xf / f / Xu / u = the strong-form point sets, n_res / n_elem = residual and element counts)"""
    prob, kind, seed = c["prob"], c["kind"], c["seed"]
    th = gp.generic_theta(c["layers"], seed, extra=[EPS0] if prob == "adv" else (), scale=c["scale"])
    s = dict(_base_setup(prob, kind))
    out = dict(th=th, n_res=0, n_elem=0)
    if kind == "pinn":
        rng = np.random.default_rng(seed + 500009)
        out["Xf"], out["Xu"] = _uniform(rng, N_COLLOCATION, prob), _uniform(rng, N_DATA, prob)
        out["u"], out["f"] = rng.standard_normal((N_DATA, 1)), rng.standard_normal((N_COLLOCATION, 1))
        if prob == "p1":
            s.update(X_u_train=out["Xu"], u_train=out["u"], X_f_train=out["Xf"], f_train=out["f"])
        elif prob == "p2":
            s.update(X_u_train=out["Xu"], u_train=out["u"], X_f_train=out["Xf"], f_train=out["f"])
        else:
            s.update(XT_u_train=out["Xu"], u_train=out["u"], XT_f_train=out["Xf"])
            out["f"] = None
        kw = dict(scheme="PINNs", lossb_weight=LBW)
    else:
        if prob == "p1":
            s = gp.warp_poisson1d(s, seed)
            # (the driver's own F is ~1e2: next to it the two boundary points are below TERM_FLOOR of the loss)
            s["F_ext_total"] = gp.random_F(np.shape(s["F_ext_total"]), seed + 1)
            out["n_elem"], out["n_res"] = 3, 3 * 4
        elif prob == "p2":
            s = gp.warp_poisson2d(s, seed)
            out["n_elem"], out["n_res"] = 4, 4 * 6
        else:
            s = gp.warp_advdiff(s, seed)
            out["n_elem"], out["n_res"] = 4, 4 * 6
        kw = dict(var_form=c["vf"], lossb_weight=LBW)
    if prob == "adv":
        kw["V"] = V
    out["a"] = {"p1": gp.p1_tuple, "p2": gp.p2_tuple, "adv": gp.p3_tuple}[prob](s, c["layers"])
    out["kw"] = kw
    return out


def product(c, inp, **more):
    from hp_vpinns_amd import vpinn
    cls = {"p1": vpinn.VPINN1D, "p2": vpinn.VPINN2D, "adv": vpinn.VPINNAdvDiff}[c["prob"]]
    return cls(*inp["a"], init_params=inp["th"], LR=0.001, **inp["kw"], **more)


# ---- the two CPU restatements -------------------------------------------------------------------------------------------------------
def reference(c, inp):
    """the reference the GPU file compares against: pinn_reference.py (1-D, AdvDiff strong form), OracleVPINN2D(scheme="PINNs"), the
    vectorised oracle (variational; leaves the residuals in .last["R"])"""
    from oracle import vpinn_oracle as O
    from pinn_reference import PinnRef1D, PinnRefAdvDiff
    prob, th, L = c["prob"], inp["th"], c["layers"]
    if c["kind"] == "pinn":
        if prob == "p1":
            return PinnRef1D(inp["Xu"], inp["u"], inp["Xf"], inp["f"], L, lossb_weight=LBW, init_params=th)
        if prob == "adv":
            return PinnRefAdvDiff(inp["Xu"], inp["u"], inp["Xf"], L, V=V, lossb_weight=LBW, init_params=th)
        return O.OracleVPINN2D(*inp["a"], scheme="PINNs", lossb_weight=LBW, init_params=th)
    o = _oracle_var(c, inp)
    o.vectorized = True
    return o


def _oracle_var(c, inp):
    from oracle import vpinn_oracle as O
    cls = {"p1": O.OracleVPINN1D, "p2": O.OracleVPINN2D, "adv": O.OracleVPINNAdvDiff}[c["prob"]]
    kw = dict(var_form=c["vf"], lossb_weight=LBW, init_params=inp["th"])
    if c["prob"] == "adv":
        kw["V"] = V
    return cls(*inp["a"], **kw)


def second(c, inp):
    """(loss triple, gradient) of the second, independent restatement: the oracle's element loop for the variational cases; for the
    strong form the numpy closed form below (forward-mode Taylor channels, hand-derived reverse pass: oracle/closed_form.py)"""
    if c["kind"] == "var":
        return _oracle_var(c, inp).loss_and_grad()
    return pinn_closed_form(c["prob"], inp["th"], c["layers"], inp["Xf"], inp["f"], inp["Xu"], inp["u"])


def pinn_closed_form(prob, theta, layers, Xf, f, Xu, u, lossb_weight=LBW, v=V):
    """Strong-form loss and gradient without autograd.  Residuals: 1-D -u_xx - f (P1:150-155), 2-D u_xx + u_yy - f (P2:187-194),
    AdvDiff u_t + V u_x - epsilon u_xx (P3:247-253); loss = lossb_weight * mean((u - u_NN)^2) + mean(r^2).  The triple reports lossb
    as the product does: the plain mean, the weighted one for AdvDiff."""
    from oracle.closed_form import taylor_backward, taylor_forward
    theta = np.asarray(theta, dtype=np.float64)
    n_eps = 1 if prob == "adv" else 0
    th = theta[:theta.size - n_eps]
    kind = "sin" if prob == "p1" else "tanh"
    t1, t2 = {"p1": ([], [0]), "p2": ([], [0, 1]), "adv": ([0, 1], [0])}[prob]
    ch, tape = taylor_forward(th, layers, np.asarray(Xf, dtype=np.float64), kind, t1, t2)
    n = Xf.shape[0]
    if prob == "p1":
        r = -ch[1] - f
        gbar = [np.zeros_like(r), -2.0 / n * r]
    elif prob == "p2":
        r = ch[1] + ch[2] - f
        gbar = [np.zeros_like(r), 2.0 / n * r, 2.0 / n * r]
    else:
        eps = theta[-1]
        r = ch[2] + v * ch[1] - eps * ch[3]
        gbar = [np.zeros_like(r), 2.0 / n * v * r, 2.0 / n * r, -2.0 / n * eps * r]
    lossp = float((r ** 2).sum() / n)
    g = taylor_backward(th, layers, tape, t1, t2, gbar)
    ud, tape_d = taylor_forward(th, layers, np.asarray(Xu, dtype=np.float64), kind, [], [])
    e = np.asarray(u, dtype=np.float64).reshape(-1, 1) - ud[0]
    msq = float((e ** 2).mean())
    g = g + taylor_backward(th, layers, tape_d, [], [], [-2.0 * lossb_weight / e.shape[0] * e])
    if n_eps:
        g = np.concatenate([g, [float((-2.0 / n * r * ch[3]).sum())]])
    return (lossb_weight * msq + lossp, lossb_weight * msq if n_eps else msq, lossp), g


# ---- the conditions a case must meet on the reference alone -------------------------------------------------------------------------
def conditions(c, inp=None):
    """dict(ok, why, floor = smallest block share of the gradient norm, terms = the two loss terms' shares, agree = worst block error
    between the two restatements, loss_agree)"""
    inp = inputs(c) if inp is None else inp
    l3, g = reference(c, inp).loss_and_grad()
    l3b, gb = second(c, inp)
    l3, l3b = np.asarray(l3, dtype=np.float64), np.asarray(l3b, dtype=np.float64)
    total = np.linalg.norm(g)
    floor = min(np.linalg.norm(g[lo:hi]) for _, lo, hi in gp.blocks(c["layers"], c["n_extra"])) / total
    terms = ((l3[0] - l3[2]) / l3[0], l3[2] / l3[0])
    out = dict(floor=float(floor), terms=terms, agree=np.inf, loss_agree=float(np.abs(l3b - l3).max() / abs(l3[0])))
    why = []
    if not np.all(np.isfinite(g)) or not np.all(np.isfinite(l3)):
        why.append("not finite")
    if floor < gp.BLOCK_FLOOR:
        why.append("a block has %.1e of the gradient norm" % floor)
    else:
        out["agree"] = gp.block_rel(gb, g, c["layers"], c["n_extra"])
        if out["agree"] > BLOCK_AGREE or out["loss_agree"] > BLOCK_AGREE:
            why.append("the restatements differ by %.1e (blocks) / %.1e (loss)" % (out["agree"], out["loss_agree"]))
    if min(terms) < TERM_FLOOR:
        why.append("a loss term has %.1e of the loss" % min(terms))
    out["ok"], out["why"] = not why, "; ".join(why)
    return out
