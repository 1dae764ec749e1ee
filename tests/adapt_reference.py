"""Reference of the box-list quantities from the oracle classes (oracle/vpinn_oracle.py): per box the oracle class is built on the
1 x 1 grid [x0, x1] x [y0, y1] with that box's counts and that box's block of F.

  box_loss_and_grad   loss3 and gradient of a box list: the sum over the boxes of the oracle's variational term, plus the oracle's
                      boundary term once
  indicators          the five numbers of hpv_element_indicators per box: R from the oracle's per-element residuals
                      (loss_parts_vectorized leaves them in `last`), r from the oracle's net_f / derivative methods at the mapped points

The right-hand side blocks F are formed here in numpy with the drivers' expression J * (w_y phi_k) f (w_x phi_r) (P2:405-407)."""
import numpy as np
import torch

from oracle.vpinn_oracle import OracleVPINN1D, OracleVPINN2D, OracleVPINNAdvDiff, Test_fcn


def f_blocks(mesh, f, xi, wx, yi=None, wy=None):
    """[(nay_e, nax_e) block of F per box] (1-D: (nax_e,) columns); f None: zeros"""
    out = []
    for e in range(len(mesh)):
        b, nx, ny = mesh.boxes[e], int(mesh.nax[e]), int(mesh.nay[e])
        xq = b[0] + (b[1] - b[0]) / 2 * (xi + 1)
        ax = Test_fcn(nx, xi.reshape(-1, 1))[:, :, 0] * wx
        if mesh.dim == 1:
            J = (b[1] - b[0]) / 2
            out.append(np.zeros(nx) if f is None else J * (ax @ f(xq)))
            continue
        yq = b[2] + (b[3] - b[2]) / 2 * (yi + 1)
        by = Test_fcn(ny, yi.reshape(-1, 1))[:, :, 0] * wy
        J = ((b[1] - b[0]) / 2) * ((b[3] - b[2]) / 2)
        out.append(np.zeros((ny, nx)) if f is None else J * (by @ f(xq[None, :] + 0 * yq[:, None], yq[:, None] + 0 * xq[None, :]) @ ax.T))
    return out


def _rule2d(xi, wx, yi, wy):
    xx, yy = np.meshgrid(xi, yi)
    wxx, wyy = np.meshgrid(wx, wy)
    return (np.hstack((xx.flatten()[:, None], yy.flatten()[:, None])), np.hstack((wxx.flatten()[:, None], wyy.flatten()[:, None])))


def box_oracle(prob, vf, mesh, e, Fe, rule, data, layers, th, V=1.0, lossb_weight=None):
    """the oracle class on the 1 x 1 grid of box e; prob: 'p1' | 'p2' | 'adv'; rule = (xi, wx[, yi, wy]); data = (X_u, u)"""
    b, nx, ny = mesh.boxes[e], int(mesh.nax[e]), int(mesh.nay[e])
    kw = {} if lossb_weight is None else dict(lossb_weight=lossb_weight)
    if prob == "p1":
        xi, wx = rule
        o = OracleVPINN1D(data[0], data[1], xi.reshape(-1, 1), wx.reshape(-1, 1), [Fe.reshape(-1)], b[:2], None, None, layers,
                          var_form=vf, init_params=th, **kw)
    elif prob == "p2":
        XY, W = _rule2d(*rule)
        dummy = np.zeros((1, 2))
        o = OracleVPINN2D(data[0], data[1], dummy, np.zeros((1, 1)), XY, W, None, Fe.reshape(1, 1, ny, nx), b[:2], b[2:], [[nx], [ny]],
                          None, None, layers, var_form=vf, init_params=th, **kw)
    else:
        XY, W = _rule2d(*rule)
        o = OracleVPINNAdvDiff(data[0], data[1], None, XY, W, None, None, b[:2], b[2:], [[nx], [ny]], None, None, layers, None, None,
                               var_form=vf, V=V, init_params=th, **kw)
    o.vectorized = True
    return o


def box_loss_and_grad(prob, vf, mesh, F, rule, data, layers, th, V=1.0, e_range=None, use_data=True, lossb_weight=None):
    """(loss, lossb, lossv), gradient of the box list (or of its slice e_range, the boundary term only with use_data)"""
    lo, hi = (0, len(mesh)) if e_range is None else e_range
    lossv, grad, lossb, wlossb = 0.0, 0.0, 0.0, 0.0
    for e in range(lo, hi):
        o = box_oracle(prob, vf, mesh, e, F[e], rule, data, layers, th, V, lossb_weight)
        loss, lb, lv = o.loss_parts()
        g, = torch.autograd.grad(lv, o.theta, retain_graph=True, allow_unused=True)
        grad = grad + (g.numpy() if g is not None else 0.0)
        lossv += float(lv.detach())
        if use_data and e == lo:
            gb, = torch.autograd.grad(loss - lv, o.theta)
            grad = grad + gb.numpy()
            lossb, wlossb = float(lb.detach()), float((loss - lv).detach())
    if use_data and hi == lo:      # (an empty slice still owns the boundary term when asked to)
        raise ValueError("empty slice")
    return (lossv + wlossb, lossb, lossv), np.asarray(grad, dtype=np.float64)


def strong_residual(o, prob, X, V=1.0):
    """r without the right-hand side at the points X (n, dim), from the oracle's own derivative methods"""
    cols = [torch.tensor(X[:, c:c + 1].copy(), requires_grad=True) for c in range(X.shape[1])]
    if prob == "p1":
        return -o.net_du(cols[0])[1].detach().numpy().reshape(-1)                        # -u_xx (P1:150-155)
    if prob == "p2":
        return o.net_f(cols[0], cols[1]).detach().numpy().reshape(-1)                    # u_xx + u_yy (P2:187-194)
    d1x, d2x = o.net_dxu(cols[0], cols[1])
    d1t = o.net_dtu(cols[0], cols[1])
    return (d1t + V * d1x - o.epsilon * d2x).detach().numpy().reshape(-1)                # P3:247-253


def indicators(prob, vf, mesh, f, rule, data, layers, th, V=1.0):
    """(n, 5): loss_e, eta2_e, sumR2_e, topx_e, topy_e of every box"""
    F = f_blocks(mesh, f, *rule)
    out = np.zeros((len(mesh), 5))
    J = mesh.jacobians()
    for e in range(len(mesh)):
        # the oracle's AdvDiff class has a zero right-hand side: F is subtracted here
        o = box_oracle(prob, vf, mesh, e, F[e] if prob != "adv" else None, rule, data, layers, th, V)
        o.loss_parts()
        R = np.asarray(o.last["R"], dtype=np.float64)
        nx, ny = int(mesh.nax[e]), int(mesh.nay[e])
        R = R.reshape(ny, nx)
        if prob == "adv":
            R = R - F[e]
        P = ElementPoints(mesh, e, rule)
        r = strong_residual(o, prob, P, V)
        if f is not None:
            r = r - np.asarray(f(*[P[:, c] for c in range(P.shape[1])])).reshape(-1)
        w = rule[1] if mesh.dim == 1 else (rule[1][None, :] * rule[3][:, None]).reshape(-1)
        s = float((R ** 2).sum())
        out[e] = [s / (nx * ny), J[e] * float((w * r * r).sum()), s, float((R[:, nx - 1] ** 2).sum()),
                  float((R[ny - 1, :] ** 2).sum()) if mesh.dim == 2 else 0.0]
    return out


def ElementPoints(mesh, e, rule):
    return mesh.quad_points(rule[0], rule[2] if mesh.dim == 2 else None, e, e + 1)


def zero_network_indicators(mesh, f, rule):
    """Known answers for a network that is identically zero (all parameters 0; AdvDiff: any epsilon): r = -f, R = -F."""
    F = f_blocks(mesh, f, *rule)
    J = mesh.jacobians()
    out = np.zeros((len(mesh), 5))
    for e in range(len(mesh)):
        P = ElementPoints(mesh, e, rule)
        fq = np.asarray(f(*[P[:, c] for c in range(P.shape[1])])).reshape(-1)
        w = rule[1] if mesh.dim == 1 else (rule[1][None, :] * rule[3][:, None]).reshape(-1)
        nx, ny = int(mesh.nax[e]), int(mesh.nay[e])
        R = F[e].reshape(ny, nx)
        s = float((R ** 2).sum())
        out[e] = [s / (nx * ny), J[e] * float((w * fq * fq).sum()), s, float((R[:, nx - 1] ** 2).sum()),
                  float((R[ny - 1, :] ** 2).sum()) if mesh.dim == 2 else 0.0]
    return out
