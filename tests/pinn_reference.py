"""Expected values of the strong-form PINN scheme for Poisson-1D and AdvDiff (the oracle restates the reference classes and
has the scheme for Poisson-2D only): a torch-fp64 double-backward restatement of

    Poisson-1D   r = -u_xx - f_train        (net_f, P1:150-155; mean square against f_train as P2:124)
                 loss = lossb_weight * mean((u_b - u)^2) + mean(r^2)                  (P1:98-100 with lossv replaced, as P2:129)
    AdvDiff      r = u_t + V u_x - epsilon u_xx   (net_f, P3:247-253; columns of XT_f_train are (x, t))
                 loss = 10 * mean((u_b - u)^2) + mean(r^2)                            (P3:184, 186)

Network, parameter packing (`unpack`: weights and biases layer by layer, epsilon last) and the TF1-rule Adam step are the
oracle's own (`oracle.vpinn_oracle._OracleBase`).  `loss_parts` returns (loss, lossb, lossp) with lossb as the product reports
it: the plain mean in 1-D, the weighted one for AdvDiff (P3:184 folds the 10 into lossb).
"""
import numpy as np
import torch

from oracle.vpinn_oracle import _OracleBase, unpack


def _d(y, x):
    return torch.autograd.grad(y.sum(), x, create_graph=True)[0]


def residual_1d(u_fn, x, f):
    """-u_xx - f at the points x (n, 1) of a callable u_fn (P1:150-155)."""
    x = x.clone().requires_grad_(True)
    u_xx = _d(_d(u_fn(x), x), x)
    return -u_xx - f


def residual_advdiff(u_fn, x, t, V, eps):
    """u_t + V u_x - eps u_xx at (x, t), each (n, 1), of a callable u_fn(x, t) (P3:247-253)."""
    x, t = x.clone().requires_grad_(True), t.clone().requires_grad_(True)
    u = u_fn(x, t)
    u_x = _d(u, x)
    return _d(u, t) + V * u_x - eps * _d(u_x, x)


class _PinnRef(_OracleBase):
    def _data(self, X_u, u, X_f, n_total, use_data):
        self.X_u = torch.tensor(np.asarray(X_u, dtype=np.float64))
        self.u = torch.tensor(np.asarray(u, dtype=np.float64).reshape(-1, 1))
        self.X_f = torch.tensor(np.asarray(X_f, dtype=np.float64))
        self.n_total = self.X_f.shape[0] if n_total is None else n_total      # a shard: the mean runs over all shards' points
        self.use_data = use_data

    def _msq_data(self):
        if not self.use_data:
            return torch.zeros((), dtype=torch.float64)
        return torch.mean(torch.square(self.u - self.neural_net(self.X_u)))


class PinnRef1D(_PinnRef):
    act = staticmethod(torch.sin)      # P1:134

    def __init__(self, X_u_train, u_train, X_f_train, f_train, layers, lossb_weight=1, LR=0.001, init_params=None,
                 n_total=None, use_data=True):
        self._init_common(layers, init_params, LR)
        self._data(X_u_train, u_train, X_f_train, n_total, use_data)
        self.f = torch.tensor(np.asarray(f_train, dtype=np.float64).reshape(-1, 1))
        self.lossb_weight = lossb_weight

    def loss_parts(self):
        r = residual_1d(self.neural_net, self.X_f, self.f)
        lossp = torch.sum(torch.square(r)) / self.n_total
        lossb = self._msq_data()
        return self.lossb_weight * lossb + lossp, lossb, lossp


class PinnRefAdvDiff(_PinnRef):
    act = staticmethod(torch.tanh)     # P3:226
    n_extra = 1                        # epsilon, the last parameter (P3:63)

    def __init__(self, XT_u_train, u_train, XT_f_train, layers, V=1.0, lossb_weight=10, LR=0.001, init_params=None,
                 n_total=None, use_data=True):
        self._init_common(layers, init_params, LR)
        self._data(XT_u_train, u_train, XT_f_train, n_total, use_data)
        self.V, self.lossb_weight = V, lossb_weight

    def loss_parts(self):
        eps = unpack(self.theta, self.layers)[2][0]
        r = residual_advdiff(lambda x, t: self.neural_net(torch.cat([x, t], 1)), self.X_f[:, 0:1], self.X_f[:, 1:2], self.V, eps)
        lossp = torch.sum(torch.square(r)) / self.n_total
        lossb = self.lossb_weight * self._msq_data()
        return lossb + lossp, lossb, lossp
