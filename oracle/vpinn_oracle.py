"""CPU ORACLE for the hp-VPINN hot path -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Only `tests/`, `__graft_entry__.smoke()` and the `cpu_baseline` leg of `bench.py` may import
this module; nothing under `hp_vpinns_amd/` does, and the product path raises if the HIP
library is missing instead of falling back to this.

What it is: a float64 torch-CPU restatement of the three TF1 loss graphs of the reference,
following them line by line (Python loop over elements, one multiply-reduce per test
function / test-function pair, derivatives by reverse-mode autodiff applied twice, TF1-rule
Adam, the reference's recording semantics).  It is deliberately *independent* of the product:
the product propagates closed-form Taylor channels forward and a hand-derived adjoint
backward in HIP; this file uses autograd (double backward) for every derivative and
scipy.special for the polynomial tables (as the reference does, Q:16-26,46-61).

Pinning status: the reference has no tests, golden vectors or known-answer fixtures and TensorFlow cannot
be installed here.  Pinned by *running* the reference's own code (tests/golden/make_golden.py): everything numpy in it (quadrature,
test-function tables, grids, F_ext_total, boundary sets -> tests/golden/*.npz), and the bodies of its three VPINN classes, executed
verbatim on a torch-fp64 stand-in for the `tf` symbols they use (tests/golden/tf1_shim.py -> tests/golden/*_graph.npz: loss triple,
gradient, six Adam updates with the loss read after each, parameters, prediction).  This file reproduces those numbers within 1e-11
(tests/test_oracle.py).  Still by documentation: what the TensorFlow ops themselves compute (the stand-in is not TensorFlow; its
semantics are checked on closed forms).  Further anchors: known answers (zero-network loss
= sum_e mean(F_e^2) + w*lossb, which reproduces the ~4e2 plateau of the reference's
`Results/loss.pdf`), the reference's own exact solutions (substituted for the network they make
the restated variational residual vanish against the reference-produced F_ext_total: round-off for
the strong form, quadrature error decreasing under refinement for the weak forms incl. the 1-D
element-edge terms -- tests/test_oracle.py), finite differences, full-length training runs landing
on the reference's published figures (profiles/r01_convergence.txt), and agreement of two
independent derivations.

Parameter packing (shared with the C-ABI, include/hpvpinn.h): theta = [W0, b0, W1, b1, ...,
(epsilon)] with W_l row-major `[in, out]` (row-vector convention H @ W, P1:128-138).
"""
import time

import numpy as np
import torch
from scipy.special import jacobi as _sp_jacobi
from scipy.special import roots_jacobi as _sp_roots_jacobi

torch.set_default_dtype(torch.float64)


# --------------------------------------------------------------------------------------
# L0/L1 restatement: quadrature + tables (reference: Q:24-61, P1:157-183)
# --------------------------------------------------------------------------------------
def Jacobi(n, a, b, x):
    """Q:24-26 -- scipy orthopoly1d call (stable eval_jacobi recurrence inside)."""
    x = np.array(x)
    return _sp_jacobi(n, a, b)(x)


def GaussLobattoJacobiWeights(Q, a, b):
    """Q:46-61, Legendre case (the only one the drivers use)."""
    assert a == 0 and b == 0
    X = _sp_roots_jacobi(Q - 2, a + 1, b + 1)[0]
    W = 2 / ((Q - 1) * Q * (Jacobi(Q - 1, 0, 0, X) ** 2))
    Wl = 2 / ((Q - 1) * Q * (Jacobi(Q - 1, 0, 0, -1) ** 2))
    Wr = 2 / ((Q - 1) * Q * (Jacobi(Q - 1, 0, 0, 1) ** 2))
    W = np.append(np.append(Wl, W), Wr)
    X = np.append(np.append(-1, X), 1)
    return [X, W]


def Test_fcn(N_test, x):
    """P1:157-162 / P2:196-208 / P3:257-262."""
    return np.asarray([Jacobi(n + 1, 0, 0, x) - Jacobi(n - 1, 0, 0, x) for n in range(1, N_test + 1)])


def dTest_fcn(N_test, x):
    """P1:164-183 / P2:210-229 / P3:265-284."""
    d1t, d2t = [], []
    for n in range(1, N_test + 1):
        if n == 1:
            d1 = ((n + 2) / 2) * Jacobi(n, 1, 1, x)
            d2 = ((n + 2) * (n + 3) / (2 * 2)) * Jacobi(n - 1, 2, 2, x)
        elif n == 2:
            d1 = ((n + 2) / 2) * Jacobi(n, 1, 1, x) - ((n) / 2) * Jacobi(n - 2, 1, 1, x)
            d2 = ((n + 2) * (n + 3) / (2 * 2)) * Jacobi(n - 1, 2, 2, x)
        else:
            d1 = ((n + 2) / 2) * Jacobi(n, 1, 1, x) - ((n) / 2) * Jacobi(n - 2, 1, 1, x)
            d2 = ((n + 2) * (n + 3) / (2 * 2)) * Jacobi(n - 1, 2, 2, x) \
                - ((n) * (n + 1) / (2 * 2)) * Jacobi(n - 3, 2, 2, x)
        d1t.append(d1)
        d2t.append(d2)
    return np.asarray(d1t), np.asarray(d2t)


# --------------------------------------------------------------------------------------
# parameter packing helpers
# --------------------------------------------------------------------------------------
def n_params(layers, extra=0):
    return sum(layers[l] * layers[l + 1] + layers[l + 1] for l in range(len(layers) - 1)) + extra


def unpack(theta, layers):
    ws, bs, o = [], [], 0
    for l in range(len(layers) - 1):
        i, j = layers[l], layers[l + 1]
        ws.append(theta[o:o + i * j].reshape(i, j)); o += i * j
        bs.append(theta[o:o + j].reshape(1, j)); o += j
    return ws, bs, theta[o:]


def xavier_theta(layers, seed=1234, extra=()):
    """Seeded truncated-normal (|z|<=2) Xavier init, zero biases (semantics of P1:110-126).

    TF's own seeded stream is not reproducible outside TF, so initial parameters are an
    *input* of every parity test; this is just a convenient generator for them.
    """
    rng = np.random.default_rng(seed)
    parts = []
    for l in range(len(layers) - 1):
        i, j = layers[l], layers[l + 1]
        std = np.sqrt(2.0 / (i + j))
        z = rng.standard_normal(i * j)
        bad = np.abs(z) > 2
        while bad.any():
            z[bad] = rng.standard_normal(bad.sum())
            bad = np.abs(z) > 2
        parts += [std * z, np.zeros(j)]
    parts.append(np.asarray(extra, dtype=np.float64))
    return np.concatenate(parts)


# --------------------------------------------------------------------------------------
# common machinery: MLP, autodiff derivatives, TF1 Adam, train loop
# --------------------------------------------------------------------------------------
class _OracleBase:
    act = staticmethod(torch.tanh)
    n_extra = 0

    # Shard support for the multi-GPU correctness tests: restrict the variational sum to the flattened
    # element range [e_range[0], e_range[1]) and/or drop the boundary term (ranks other than 0).
    e_range = None
    use_data = True

    def _owns(self, e):
        return self.e_range is None or (self.e_range[0] <= e < self.e_range[1])

    def _init_common(self, layers, init_params, LR):
        self.layers = list(layers)
        P = n_params(self.layers, self.n_extra)
        if init_params is None:
            init_params = xavier_theta(self.layers, 1234, extra=[1.0] * self.n_extra)
        th = np.asarray(init_params, dtype=np.float64).reshape(-1)
        assert th.size == P, (th.size, P)
        self.theta = torch.tensor(th, requires_grad=True)
        self.LR = LR
        # TF1 AdamOptimizer state (tf.train.AdamOptimizer defaults: P1:103, P2:131, P3:192)
        self.m = torch.zeros(P)
        self.v = torch.zeros(P)
        self.beta1, self.beta2, self.eps_adam = 0.9, 0.999, 1e-8
        self.beta1_power, self.beta2_power = self.beta1, self.beta2  # TF keeps running products

    def set_adam(self, beta1=0.9, beta2=0.999, eps=1e-8, LR=None):
        """Other tf.train.AdamOptimizer constants than the defaults (a fresh optimizer: moments zero, powers restarted)."""
        self.beta1, self.beta2, self.eps_adam = beta1, beta2, eps
        self.beta1_power, self.beta2_power = beta1, beta2
        self.m.zero_()
        self.v.zero_()
        if LR is not None:
            self.LR = LR

    # P1:128-138 / P2:158-169 / P3:219-230
    def neural_net(self, X, theta=None):
        ws, bs, _ = unpack(self.theta if theta is None else theta, self.layers)
        H = X
        for l in range(len(ws) - 1):
            H = self.act(torch.add(torch.matmul(H, ws[l]), bs[l]))
        return torch.add(torch.matmul(H, ws[-1]), bs[-1])

    @staticmethod
    def _grad(y, x):
        # tf.gradients(y, x)[0] == d(sum y)/dx (P1:146-147)
        return torch.autograd.grad(y.sum(), x, create_graph=True)[0]

    def loss_parts(self):
        raise NotImplementedError

    def loss_and_grad(self):
        loss, lossb, lossv = self.loss_parts()
        g, = torch.autograd.grad(loss, self.theta, allow_unused=False)
        return (float(loss.detach()), float(lossb.detach()), float(lossv.detach())), g.detach().numpy().copy()

    def adam_step(self):
        """One `sess.run(train_op_Adam)`: TF1 rule, epsilon OUTSIDE the bias correction."""
        loss, lossb, lossv = self.loss_parts()
        g, = torch.autograd.grad(loss, self.theta)
        with torch.no_grad():
            lr_t = self.LR * np.sqrt(1.0 - self.beta2_power) / (1.0 - self.beta1_power)
            self.m.mul_(self.beta1).add_(g, alpha=1.0 - self.beta1)
            self.v.mul_(self.beta2).addcmul_(g, g, value=1.0 - self.beta2)
            self.theta -= lr_t * self.m / (torch.sqrt(self.v) + self.eps_adam)
            self.beta1_power *= self.beta1
            self.beta2_power *= self.beta2
        return float(loss.detach()), float(lossb.detach()), float(lossv.detach())

    def get_params(self):
        return self.theta.detach().numpy().copy()

    def _predict(self, X):
        with torch.no_grad():
            return self.neural_net(torch.as_tensor(np.asarray(X, dtype=np.float64))).numpy()


# --------------------------------------------------------------------------------------
# Poisson 1-D  (reference P1:30-224)
# --------------------------------------------------------------------------------------
class OracleVPINN1D(_OracleBase):
    act = staticmethod(torch.sin)  # P1:134

    def __init__(self, X_u_train, u_train, X_quad, W_quad, F_exact_total, grid, X_test, u_test,
                 layers, X_f_train=None, f_train=None, *, var_form=1, lossb_weight=1, LR=0.001,
                 init_params=None):
        self.x, self.u = torch.as_tensor(X_u_train), torch.as_tensor(u_train)
        self.xquad, self.wquad = np.asarray(X_quad), torch.as_tensor(W_quad)
        # a list of per-element columns, possibly of different lengths (the driver's N_testfcn_total, P1:268-281; the
        # reference's np.asarray of such a list was an object array whose [e] the class indexes, P1:66-67)
        self.F_ext_total = [np.asarray(f, dtype=np.float64).reshape(-1, 1) for f in F_exact_total]
        self.Nelement = len(self.F_ext_total)                    # P1:43
        self.N_test = max(f.shape[0] for f in self.F_ext_total)  # tables for the longest element (P1:73 builds them per element)
        self.ragged = any(f.shape[0] != self.N_test for f in self.F_ext_total)
        self.grid = np.asarray(grid, dtype=np.float64)
        self.xtest, self.utest = X_test, u_test
        self.var_form, self.lossb_weight = var_form, lossb_weight
        self._init_common(layers, init_params, LR)
        # constants of the graph (P1:69-80): tables at the reference nodes, per element
        self._test = torch.as_tensor(Test_fcn(self.N_test, self.xquad))
        d1, d2 = dTest_fcn(self.N_test, self.xquad)
        self._d1test, self._d2test = torch.as_tensor(d1), torch.as_tensor(d2)
        self._d1test_bound = dTest_fcn(self.N_test, np.array([[-1.0], [1.0]]))[0]

    def net_u(self, x):
        return self.neural_net(torch.cat([x], 1))                # P1:140-142

    def net_du(self, x):                                         # P1:144-148
        u = self.net_u(x)
        d1u = self._grad(u, x)
        d2u = self._grad(d1u, x)
        return d1u, d2u

    def loss_parts_vectorized(self):
        """Same loss as `loss_parts` with all elements batched and the projection as one contraction (every var_form);
        proven equal to the element loop in tests/test_oracle.py, used where the loop would take minutes.
        Leaves the per-point channels and the residuals in `self.last` for the per-channel parity tests."""
        assert self.e_range is None and self.use_data and not self.ragged
        g, ne = self.grid, self.Nelement
        J = torch.as_tensor((g[1:] - g[:-1]) / 2).reshape(ne, 1)
        xq = torch.as_tensor(g[:-1]).reshape(ne, 1) + J * (torch.as_tensor(self.xquad).reshape(1, -1) + 1)
        x = xq.reshape(-1, 1).clone().requires_grad_(True)
        u = self.net_u(x)
        d1 = self._grad(u, x)
        d2 = self._grad(d1, x)
        w = self.wquad.reshape(1, -1)
        if self.var_form == 1:                                   # P1:82-84
            U = -J * torch.einsum("kq,eq->ek", self._test[:, :, 0] * w, d2.reshape(ne, -1))
        elif self.var_form == 2:                                 # P1:85-87
            U = torch.einsum("kq,eq->ek", self._d1test[:, :, 0] * w, d1.reshape(ne, -1))
        else:                                                    # P1:88-91
            xb = torch.as_tensor(np.stack([g[:-1], g[1:]], 1).reshape(-1, 1))
            ub = self.net_u(xb).reshape(ne, 2)
            d1b = torch.as_tensor(self._d1test_bound[:, :, 0])   # (N_test, 2): phi'(-1), phi'(1)
            U = -1 / J * torch.einsum("kq,eq->ek", self._d2test[:, :, 0] * w, u.reshape(ne, -1)) \
                + 1 / J * (ub[:, 1:2] * d1b[:, 1].reshape(1, -1) - ub[:, 0:1] * d1b[:, 0].reshape(1, -1))
        Res = U - torch.as_tensor(np.stack([f[:, 0] for f in self.F_ext_total]))
        lossv = torch.mean(torch.square(Res), dim=1).sum()
        lossb = torch.mean(torch.square(self.u - self.net_u(self.x)))
        self.last = {"channels": [t.detach().numpy().reshape(-1) for t in (u, d1, d2)], "R": Res.detach().numpy()}
        return self.lossb_weight * lossb + lossv, lossb, lossv

    def loss_parts(self):
        if getattr(self, "vectorized", False) and not self.ragged:
            return self.loss_parts_vectorized()
        varloss_total = 0
        grid = self.grid
        for e in range(self.Nelement):                           # P1:65
            if not self._owns(e):
                continue
            F_ext_element = torch.as_tensor(self.F_ext_total[e])
            Ntest_element = F_ext_element.shape[0]
            x_quad_element = torch.tensor(grid[e] + (grid[e + 1] - grid[e]) / 2 * (self.xquad + 1),
                                          requires_grad=True)    # P1:69
            x_b_element = torch.tensor(np.array([[grid[e]], [grid[e + 1]]]))
            jacobian = (grid[e + 1] - grid[e]) / 2               # P1:71
            u_NN = self.net_u(x_quad_element)                    # P1:75
            d1u_NN, d2u_NN = self.net_du(x_quad_element)         # P1:76
            u_NN_bound = self.net_u(x_b_element)                 # P1:78
            if self.var_form == 1:                               # P1:82-84
                U = torch.stack([-jacobian * torch.sum(self.wquad * d2u_NN * self._test[i])
                                 for i in range(Ntest_element)]).reshape(-1, 1)
            if self.var_form == 2:                               # P1:85-87
                U = torch.stack([torch.sum(self.wquad * d1u_NN * self._d1test[i])
                                 for i in range(Ntest_element)]).reshape(-1, 1)
            if self.var_form == 3:                               # P1:88-91
                d1b = self._d1test_bound
                U = torch.stack([-1 / jacobian * torch.sum(self.wquad * u_NN * self._d2test[i])
                                 + 1 / jacobian * torch.sum(
                                     u_NN_bound * torch.as_tensor(np.array([-d1b[i][0], d1b[i][-1]])))
                                 for i in range(Ntest_element)]).reshape(-1, 1)
            Res = U - F_ext_element                              # P1:94
            varloss_total = varloss_total + torch.mean(torch.square(Res))   # P1:95-96
        lossb = torch.mean(torch.square(self.u - self.net_u(self.x)))       # P1:98
        if not self.use_data:
            lossb = lossb * 0.0
        lossv = varloss_total
        loss = self.lossb_weight * lossb + lossv                 # P1:100
        return loss, lossb, lossv

    def predict(self, x):
        return self._predict(x)

    def train(self, nIter, tresh, total_record=None):
        """P1:201-224: loss is read back every 10 iterations, AFTER that iteration's update."""
        total_record = [] if total_record is None else total_record
        for it in range(nIter):
            self.adam_step()
            if it % 10 == 0:
                with torch.enable_grad():
                    loss_value = float(self.loss_parts()[0])
                total_record.append(np.array([it, loss_value]))
                if loss_value < tresh:
                    break
        return total_record


# --------------------------------------------------------------------------------------
# Poisson 2-D  (reference P2:27-257)
# --------------------------------------------------------------------------------------
class OracleVPINN2D(_OracleBase):
    act = staticmethod(torch.tanh)  # P2:165

    def __init__(self, X_u_train, u_train, X_f_train, f_train, X_quad, W_quad, U_exact_total,
                 F_exact_total, gridx, gridy, N_testfcn, X_test, u_test, layers, *, var_form=1,
                 scheme="VPINNs", LR=0.001, lossb_weight=10, init_params=None):
        X_u_train = np.asarray(X_u_train)
        self.x, self.y = torch.as_tensor(X_u_train[:, 0:1].copy()), torch.as_tensor(X_u_train[:, 1:2].copy())
        self.utrain = torch.as_tensor(u_train)
        X_quad = np.asarray(X_quad)
        self.xquad, self.yquad = X_quad[:, 0:1], X_quad[:, 1:2]
        self.wquad = torch.as_tensor(W_quad)
        self.Nelementx, self.Nelementy = np.size(N_testfcn[0]), np.size(N_testfcn[1])   # P2:43-44
        self.N_testfcn = N_testfcn
        self.F_ext_total = np.asarray(F_exact_total)
        self.gridx, self.gridy = np.asarray(gridx, dtype=np.float64), np.asarray(gridy, dtype=np.float64)
        self.xtest = X_test
        self.var_form, self.scheme = var_form, scheme
        self.lossb_weight = lossb_weight                         # P2:127 writes the 10 into the graph
        assert scheme in ("VPINNs", "PINNs")
        X_f_train = np.asarray(X_f_train)
        self.xf, self.yf = torch.as_tensor(X_f_train[:, 0:1].copy()), torch.as_tensor(X_f_train[:, 1:2].copy())
        self.ftrain = torch.as_tensor(np.asarray(f_train))
        self._init_common(layers, init_params, LR)
        self._tab = {}

    def _tables(self, n, q):
        key = (n, id(q))
        if key not in self._tab:
            t = torch.as_tensor(Test_fcn(n, q))
            d1, d2 = dTest_fcn(n, q)
            self._tab[key] = (t, torch.as_tensor(d1), torch.as_tensor(d2))
        return self._tab[key]

    def net_u(self, x, y):
        return self.neural_net(torch.cat([x, y], 1))             # P2:171-173

    def net_dxu(self, x, y):                                     # P2:175-179
        u = self.net_u(x, y)
        d1 = self._grad(u, x)
        return d1, self._grad(d1, x)

    def net_dyu(self, x, y):                                     # P2:181-185
        u = self.net_u(x, y)
        d1 = self._grad(u, y)
        return d1, self._grad(d1, y)

    def net_f(self, x, y):                                       # P2:187-194
        u = self.net_u(x, y)
        d1xu = self._grad(u, x)
        d2xu = self._grad(d1xu, x)
        d1yu = self._grad(u, y)
        d2yu = self._grad(d1yu, y)
        return d2xu + d2yu

    def loss_parts_vectorized(self):
        """Same loss as `loss_parts` (every var_form), all elements batched and the projection as one contraction --
        the "honest strong CPU baseline" (B) of BASELINE.md; proven equal to the element loop in tests/test_oracle.py.
        Leaves the per-point channels (element-major, q = j*Q+i) and the residuals in `self.last`."""
        assert self.scheme == "VPINNs" and self.e_range is None and self.use_data
        gx, gy = self.gridx, self.gridy
        nex, ney = self.Nelementx, self.Nelementy
        Ntx, Nty = self.N_testfcn[0][0], self.N_testfcn[1][0]
        jx = torch.as_tensor((gx[1:] - gx[:-1]) / 2).reshape(nex, 1, 1, 1)
        jy = torch.as_tensor((gy[1:] - gy[:-1]) / 2).reshape(1, ney, 1, 1)
        xq = torch.as_tensor(gx[:-1]).reshape(nex, 1, 1, 1) + jx * (torch.as_tensor(self.xquad).reshape(1, 1, -1, 1) + 1)
        yq = torch.as_tensor(gy[:-1]).reshape(1, ney, 1, 1) + jy * (torch.as_tensor(self.yquad).reshape(1, 1, -1, 1) + 1)
        x = xq.expand(nex, ney, -1, 1).reshape(-1, 1).clone().requires_grad_(True)
        y = yq.expand(nex, ney, -1, 1).reshape(-1, 1).clone().requires_grad_(True)
        u = self.net_u(x, y)
        chans = [u]
        tx, d1tx, d2tx = self._tables(Ntx, self.xquad)
        ty, d1ty, d2ty = self._tables(Nty, self.yquad)
        wx, wy = self.wquad[:, 0], self.wquad[:, 1]

        def A(a, b):                                             # [k][r][q] = w_x a_r w_y b_k
            return (a[:, :, 0] * wx)[None, :, :] * (b[:, :, 0] * wy)[:, None, :]
        J = (jx * jy).reshape(nex, ney, 1, 1)
        if self.var_form == 1:                                   # P2:98-105
            ux, uy = self._grad(u, x), self._grad(u, y)
            chans += [ux, uy]
            U = -(J / jx.reshape(nex, 1, 1, 1)) * torch.einsum("krq,xyq->xykr", A(d1tx, ty), ux.reshape(nex, ney, -1)) \
                - (J / jy.reshape(1, ney, 1, 1)) * torch.einsum("krq,xyq->xykr", A(tx, d1ty), uy.reshape(nex, ney, -1))
        elif self.var_form == 0:                                 # P2:93-96
            ux, uy = self._grad(u, x), self._grad(u, y)
            uxx, uyy = self._grad(ux, x), self._grad(uy, y)
            chans += [ux, uy, uxx, uyy]
            U = J * torch.einsum("krq,xyq->xykr", A(tx, ty), (uxx + uyy).reshape(nex, ney, -1))
        else:                                                    # P2:108-115
            U = J * torch.einsum("krq,xyq->xykr", A(d2tx, ty) + A(tx, d2ty), u.reshape(nex, ney, -1))
        Res = U - torch.as_tensor(self.F_ext_total)
        lossv = torch.mean(torch.square(Res), dim=(2, 3)).sum()
        lossb = torch.mean(torch.square(self.utrain - self.net_u(self.x, self.y)))
        self.last = {"channels": [t.detach().numpy().reshape(-1) for t in chans], "R": Res.detach().numpy()}
        return self.lossb_weight * lossb + lossv, lossb, lossv

    def loss_parts(self):
        if getattr(self, "vectorized", False):
            return self.loss_parts_vectorized()
        if self.scheme == "PINNs":                               # P2:124,128-129
            xf, yf = self.xf.clone().requires_grad_(True), self.yf.clone().requires_grad_(True)
            lossp = torch.mean(torch.square(self.net_f(xf, yf) - self.ftrain))
            lossb = torch.mean(torch.square(self.utrain - self.net_u(self.x, self.y)))
            return self.lossb_weight * lossb + lossp, lossb, lossp
        gridx, gridy, wq = self.gridx, self.gridy, self.wquad
        need2 = self.var_form == 0
        varloss_total = 0
        for ex in range(self.Nelementx):                         # P2:69
            for ey in range(self.Nelementy):                     # P2:70
                if not self._owns(ex * self.Nelementy + ey):
                    continue
                F_ext_element = torch.as_tensor(self.F_ext_total[ex, ey])
                Ntx, Nty = self.N_testfcn[0][ex], self.N_testfcn[1][ey]
                xq = torch.tensor(gridx[ex] + (gridx[ex + 1] - gridx[ex]) / 2 * (self.xquad + 1), requires_grad=True)
                yq = torch.tensor(gridy[ey] + (gridy[ey + 1] - gridy[ey]) / 2 * (self.yquad + 1), requires_grad=True)
                jacobian_x = (gridx[ex + 1] - gridx[ex]) / 2     # P2:77
                jacobian_y = (gridy[ey + 1] - gridy[ey]) / 2
                jacobian = jacobian_x * jacobian_y
                u_NN = self.net_u(xq, yq)                        # P2:81
                if need2:
                    d1xu, d2xu = self.net_dxu(xq, yq)            # P2:82
                    d1yu, d2yu = self.net_dyu(xq, yq)            # P2:83
                else:  # second derivatives are unused outside var_form 0 (TF prunes them)
                    d1xu = self._grad(self.net_u(xq, yq), xq)
                    d1yu = self._grad(self.net_u(xq, yq), yq)
                tx, d1tx, d2tx = self._tables(Ntx, self.xquad)   # P2:85-86
                ty, d1ty, d2ty = self._tables(Nty, self.yquad)   # P2:87-88
                wx, wy = wq[:, 0:1], wq[:, 1:2]
                if self.var_form == 0:                           # P2:93-96
                    integrand_1 = d2xu + d2yu
                    U = torch.stack([torch.stack([jacobian * torch.sum(wx * tx[r] * wy * ty[k] * integrand_1)
                                                  for r in range(Ntx)]) for k in range(Nty)])
                if self.var_form == 1:                           # P2:98-105
                    U1 = torch.stack([torch.stack([jacobian / jacobian_x * torch.sum(wx * d1tx[r] * wy * ty[k] * d1xu)
                                                   for r in range(Ntx)]) for k in range(Nty)])
                    U2 = torch.stack([torch.stack([jacobian / jacobian_y * torch.sum(wx * tx[r] * wy * d1ty[k] * d1yu)
                                                   for r in range(Ntx)]) for k in range(Nty)])
                    U = -U1 - U2
                if self.var_form == 2:                           # P2:108-115
                    U1 = torch.stack([torch.stack([jacobian * torch.sum(wx * d2tx[r] * wy * ty[k] * u_NN)
                                                   for r in range(Ntx)]) for k in range(Nty)])
                    U2 = torch.stack([torch.stack([jacobian * torch.sum(wx * tx[r] * wy * d2ty[k] * u_NN)
                                                   for r in range(Ntx)]) for k in range(Nty)])
                    U = U1 + U2
                Res = (U - F_ext_element).reshape(1, -1)         # P2:118
                varloss_total = varloss_total + torch.mean(torch.square(Res))   # P2:119-120
        lossb = torch.mean(torch.square(self.utrain - self.net_u(self.x, self.y)))  # P2:122
        if not self.use_data:
            lossb = lossb * 0.0
        lossv = varloss_total
        loss = self.lossb_weight * lossb + lossv                 # P2:127
        return loss, lossb, lossv

    def predict(self, X=None):
        X = self.xtest if X is None else X
        return self._predict(X)

    def train(self, nIter, loss_his=None):
        """P2:233-253: the loss is read back EVERY iteration, after the update."""
        loss_his = [] if loss_his is None else loss_his
        for it in range(nIter):
            self.adam_step()
            with torch.enable_grad():
                loss_his.append(float(self.loss_parts()[0]))
        return loss_his


# --------------------------------------------------------------------------------------
# Advection-diffusion coefficient identification  (reference P3:58-341)
# --------------------------------------------------------------------------------------
class OracleVPINNAdvDiff(_OracleBase):
    act = staticmethod(torch.tanh)  # P3:226
    n_extra = 1                     # trainable epsilon, shape [1], init 1.0 (P3:63)

    def __init__(self, XT_u_train, u_train, XT_f_train, XT_quad, W_quad, T_quad, WT_quad, grid_x,
                 grid_t, N_testfcn, XT_test, u_test, layers, lb=None, ub=None, *, var_form=0,
                 LR=0.001, V=1.0, lossb_weight=10, init_params=None):
        XT_u_train = np.asarray(XT_u_train)
        self.x, self.t = torch.as_tensor(XT_u_train[:, 0:1].copy()), torch.as_tensor(XT_u_train[:, 1:2].copy())
        self.u = torch.as_tensor(u_train)
        XT_quad = np.asarray(XT_quad)
        self.xquad, self.tquad = XT_quad[:, 0:1], XT_quad[:, 1:2]
        self.wquad = torch.as_tensor(W_quad)
        self.Nelementx, self.Nelementt = np.size(N_testfcn[0]), np.size(N_testfcn[1])
        self.N_testfcn = N_testfcn
        self.grid_x, self.grid_t = np.asarray(grid_x, dtype=np.float64), np.asarray(grid_t, dtype=np.float64)
        self.xtest = XT_test
        self.var_form, self.V = var_form, V
        self.lossb_weight = lossb_weight                         # P3:184 writes the 10 into the graph
        self._init_common(layers, init_params, LR)
        self._tab = {}

    _tables = OracleVPINN2D._tables

    @property
    def epsilon(self):
        return self.theta[-1:]

    def net_u(self, x, t):
        return self.neural_net(torch.cat([x, t], 1))             # P3:232-234

    def net_dxu(self, x, t):                                     # P3:236-240
        u = self.net_u(x, t)
        d1 = self._grad(u, x)
        return d1, self._grad(d1, x)

    def net_dtu(self, x, t):                                     # P3:242-245
        return self._grad(self.net_u(x, t), t)

    def loss_parts_vectorized(self):
        """Same loss as `loss_parts` (both var_forms) with all elements batched; proven equal to the element loop in
        tests/test_oracle.py.  Leaves the per-point channels [u, u_x, u_t, (u_xx)] and the residuals in `self.last`."""
        assert self.e_range is None and self.use_data
        gx, gt, V, eps = self.grid_x, self.grid_t, self.V, self.epsilon
        nex, net = self.Nelementx, self.Nelementt
        Ntx, Ntt = self.N_testfcn[0][0], self.N_testfcn[1][0]
        jx = torch.as_tensor((gx[1:] - gx[:-1]) / 2).reshape(nex, 1, 1, 1)
        jt = torch.as_tensor((gt[1:] - gt[:-1]) / 2).reshape(1, net, 1, 1)
        xq = torch.as_tensor(gx[:-1]).reshape(nex, 1, 1, 1) + jx * (torch.as_tensor(self.xquad).reshape(1, 1, -1, 1) + 1)
        tq = torch.as_tensor(gt[:-1]).reshape(1, net, 1, 1) + jt * (torch.as_tensor(self.tquad).reshape(1, 1, -1, 1) + 1)
        x = xq.expand(nex, net, -1, 1).reshape(-1, 1).clone().requires_grad_(True)
        t = tq.expand(nex, net, -1, 1).reshape(-1, 1).clone().requires_grad_(True)
        u = self.net_u(x, t)
        ux, ut = self._grad(u, x), self._grad(u, t)
        chans = [u, ux, ut]
        tx, d1tx, _ = self._tables(Ntx, self.xquad)
        tt, _, _ = self._tables(Ntt, self.tquad)
        wx, wt = self.wquad[:, 0], self.wquad[:, 1]

        def A(a, b):
            return (a[:, :, 0] * wx)[None, :, :] * (b[:, :, 0] * wt)[:, None, :]
        J = jt * jx                                              # P3:115
        if self.var_form == 0:                                   # P3:161-167
            uxx = self._grad(ux, x)
            chans.append(uxx)
            U = J * torch.einsum("krq,xyq->xykr", A(tx, tt), (ut + V * ux - eps * uxx).reshape(nex, net, -1))
        else:                                                    # P3:169-174
            U = J * torch.einsum("krq,xyq->xykr", A(tx, tt), (ut + V * ux).reshape(nex, net, -1)) \
                + eps * (J / jx) * torch.einsum("krq,xyq->xykr", A(d1tx, tt), ux.reshape(nex, net, -1))
        lossv = torch.mean(torch.square(U), dim=(2, 3)).sum()    # zero right-hand side (P3:180)
        lossb = self.lossb_weight * torch.mean(torch.square(self.u - self.net_u(self.x, self.t)))
        self.last = {"channels": [c.detach().numpy().reshape(-1) for c in chans], "R": U.detach().numpy()}
        return lossb + lossv, lossb, lossv

    def loss_parts(self):
        if getattr(self, "vectorized", False):
            return self.loss_parts_vectorized()
        gx, gt, wq, V = self.grid_x, self.grid_t, self.wquad, self.V
        eps = self.epsilon
        varloss_total = 0
        for ex in range(self.Nelementx):                         # P3:110
            for et in range(self.Nelementt):                     # P3:111
                if not self._owns(ex * self.Nelementt + et):
                    continue
                Ntx, Ntt = self.N_testfcn[0][ex], self.N_testfcn[1][et]
                jacobian = (gt[et + 1] - gt[et]) / 2 * (gx[ex + 1] - gx[ex]) / 2      # P3:115
                jacobian_x = (gx[ex + 1] - gx[ex]) / 2
                xq = torch.tensor(gx[ex] + (gx[ex + 1] - gx[ex]) / 2 * (self.xquad + 1), requires_grad=True)
                tq = torch.tensor(gt[et] + (gt[et + 1] - gt[et]) / 2 * (self.tquad + 1), requires_grad=True)
                d1xu, d2xu = self.net_dxu(xq, tq)                # P3:124
                d1tu = self.net_dtu(xq, tq)                      # P3:125
                tx, d1tx, _ = self._tables(Ntx, self.xquad)      # P3:127-128
                tt, _, _ = self._tables(Ntt, self.tquad)         # P3:129-130
                wx, wt = wq[:, 0:1], wq[:, 1:2]
                # P3:132-158 (edge quadratures) are dead code: nothing there reaches the loss.
                if self.var_form == 0:                           # P3:161-167
                    U = torch.stack([torch.stack([
                        jacobian * torch.sum(wx * tx[r] * wt * tt[k] * (d1tu + V * d1xu - eps * d2xu))
                        for r in range(Ntx)]) for k in range(Ntt)])
                if self.var_form == 1:                           # P3:169-174
                    U = torch.stack([torch.stack([
                        jacobian * torch.sum(wx * tx[r] * wt * tt[k] * (d1tu + V * d1xu))
                        + (eps * jacobian / jacobian_x * torch.sum(wx * d1tx[r] * wt * tt[k] * d1xu)).squeeze()
                        for r in range(Ntx)]) for k in range(Ntt)])
                Res = U.reshape(1, -1)                           # P3:180 (zero right-hand side)
                varloss_total = varloss_total + torch.mean(torch.square(Res))     # P3:181-182
        lossb = self.lossb_weight * torch.mean(torch.square(self.u - self.net_u(self.x, self.t)))   # P3:184
        if not self.use_data:
            lossb = lossb * 0.0
        lossv = varloss_total
        loss = lossb + lossv                                     # P3:187
        return loss, lossb, lossv

    def predict(self, X=None):
        X = self.xtest if X is None else X
        return self._predict(X)

    def train(self, nIter, tresh):
        """P3:291-341 -- returns the reference's 5-tuple."""
        total_time_train, min_loss = 0, 1e16
        total_records, u_records_iterhis, u_records = [], [], None
        loss_value = None
        for it in range(nIter):
            t0 = time.time()
            self.adam_step()
            total_time_train += time.time() - t0
            if it % 10 == 0:
                with torch.enable_grad():
                    loss_value = float(self.loss_parts()[0])
                epsilon_value = self.epsilon.detach().numpy().copy()
                total_records.append(np.array([it, loss_value, epsilon_value, 1], dtype=object))
                if loss_value < tresh:
                    break
                if it > 0.9 * nIter and loss_value < min_loss:
                    min_loss = loss_value
                    u_records = self.predict()
        error_records = [loss_value, 1]
        return error_records, total_records, u_records, u_records_iterhis, total_time_train
