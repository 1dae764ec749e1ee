"""The reference's `VPINN(...)` class surface on top of libhpvpinn.so.

Three classes, one per reference driver, with the reference's positional constructor
signatures, array layouts and `train` / `predict` semantics:

  VPINN1D      <- main/Poisson-1D/hp-VPINN-Poisson-1D.py:30-224            (P1)
  VPINN2D      <- main/Poisson-2D/hp-VPINN-Poisson-2D.py:27-257            (P2)
  VPINNAdvDiff <- main/AdvDiff-Identification/...-Identification.py:58-341 (P3)

Host work here is set-up only (tables, packing, sharding); every iteration -- MLP forward with
its input derivatives, test-function projection, residual, gradients, Adam -- runs in the HIP
library.

Module-level globals.  The reference classes read names of the module they are defined in: the
hyper-parameters `var_form`, `LR`, `lossb_weight`, `scheme`, `V` while the graph is built in
`__init__` (P1:82-102, P2:93-128, P3:161-191) and the history lists `total_record` / `loss_his`
while `train` runs (P1:214, P2:244) -- the drivers create those lists AFTER the constructor
(P1:333 then :335, P2:430 then :433).  The classes here keep that timing: every such name is a
keyword argument; one that is not given is looked up in the dict passed as `module_globals=`
(the documented, explicit binding: `VPINN(..., module_globals=globals())`) or, without one, in
the CALLER's module globals (frame lookup; HPV_NO_CALLER_GLOBALS=1 switches it off) -- the
hyper-parameters when the constructor runs, the lists when `train` runs -- and only then falls
back to the reference's default / a private list.  So `from hp_vpinns_amd.vpinn import VPINN2D
as VPINN` is the whole binding.
"""
import os
import sys
import time

import numpy as np

from . import _lib
from .adapt import _FD_STEP, _FD_TOL, ElementMesh, MappedMesh, mark, refine
from .dist import Reducer, dist_info, shard_range
from .init import n_params, pad_plan, xavier_init
from .quadrature import diff_matrix
from .testfcn import dTest_fcn, tables_1d


def _group_ready():
    try:
        import torch.distributed as dist
        return dist.is_available() and dist.is_initialized()
    except Exception:
        return False


def _tensor_rule(X_quad, W_quad):
    """Recover the 1-D rules from the flattened tensor-product arrays of P2:355-360 (x fastest); the x and y rules may
    have different lengths (the C ABI takes qx and qy separately)."""
    X_quad, W_quad = np.asarray(X_quad, dtype=np.float64), np.asarray(W_quad, dtype=np.float64)
    if X_quad.ndim != 2 or X_quad.shape[1] != 2 or W_quad.shape != X_quad.shape:
        raise ValueError("X_quad and W_quad must both have shape (Qx*Qy, 2)")
    nq = X_quad.shape[0]
    qx = 1                                    # x runs fastest: the first row ends where y changes for the first time
    while qx < nq and X_quad[qx, 1] == X_quad[0, 1]:
        qx += 1
    if nq % qx:
        raise ValueError("X_quad is not a Qx x Qy tensor-product rule")
    xi, yi = X_quad[:qx, 0].copy(), X_quad[::qx, 1].copy()
    wx, wy = W_quad[:qx, 0].copy(), W_quad[::qx, 1].copy()
    xx, yy = np.meshgrid(xi, yi)
    wxx, wyy = np.meshgrid(wx, wy)
    ok = (np.array_equal(xx.flatten(), X_quad[:, 0]) and np.array_equal(yy.flatten(), X_quad[:, 1])
          and np.array_equal(wxx.flatten(), W_quad[:, 0]) and np.array_equal(wyy.flatten(), W_quad[:, 1]))
    if not ok:
        raise ValueError("quadrature arrays are not the x-fastest tensor product the reference builds (P2:355-360)")
    return xi, wx, yi, wy


# Quadrature rules the element-resident whole-iteration kernels are instantiated for, the forms and networks they take and the shard
# sizes up to which each of them runs one workgroup per element live in the LIBRARY (csrc/hpv_mfma.h, the plan of the dispatch itself);
# `_lib.rule_advice` (hpv_rule_advice) answers for this problem and this rank's shard on this rank's device.


def _pad_rule(xi, w, q_dev):
    """N_quad is a free hyper-parameter (P1:237, P2:282, P3:47).  A rule with fewer points than an instantiated one is handed to the
    device padded with ZERO-WEIGHT points (at the last node): the tables the kernels contract with are w * phi, so a padded point
    adds exact zeros to every residual and receives a zero adjoint -- the integrals and their gradients are those of the rule itself,
    and the problem runs on the element-resident kernel of the next instantiated rule instead of the general launches."""
    n = q_dev - xi.size
    if n <= 0:
        return xi, w
    return np.concatenate([xi, np.full(n, xi[-1])]), np.concatenate([w, np.zeros(n)])


def _device_rule_2d(xi, wx, yi, wy, ntx, nty, n_elem_shard, pde, var_form, hidden, device=0, backend="auto"):
    """The (possibly padded) 2-D rule for the device, as the library advises for problem `pde` in form `var_form` under a network of
    `hidden` layer widths and a shard of `n_elem_shard` elements on `device`."""
    if xi.size != yi.size or backend == "generic" or os.environ.get("HPV_NO_RULE_PADDING"):
        return xi, wx, yi, wy
    q_dev, _ = _lib.rule_advice(device, pde, var_form, len(hidden), max(hidden), xi.size, ntx, nty, n_elem_shard)
    return _pad_rule(xi, wx, q_dev) + _pad_rule(yi, wy, q_dev)


def _device_rule_1d(xi, wq, ntx, n_elem_shard, pde, var_form, hidden, device=0, backend="auto"):
    """(xi, wq, nt_dev) for the device, 1-D problem: the element-resident 1-D kernel (csrc/kernels_tile.hip) is instantiated for the
    reference's own rule, 80 points and 60 test functions (P1:237-238), for var_forms 1 / 2 on 20-wide networks of 2-4 hidden layers.
    Where THAT kernel can run:
      * fewer test functions (N_testfcn is a free hyper-parameter) ride as a p-refinement with equal counts -- the device gets the
        first 60 test functions (phi_k does not depend on how many follow), F padded with zeros, the count per element;
      * a smaller rule is padded with zero-weight points to 80 -- only while the library says the shard is small enough for one
        workgroup per element to beat the separate launches on the rule as it is (hpv_rule_advice; advisor, round 4: an h-refined
        grid of 10 k elements x 10 points must NOT run 8x the points and 12x the test functions).
    Everywhere else (generic backend, var_form 3, wider / deeper networks) the device sees the problem as it is: nt_dev == ntx.
    One definition for the constructor and for set_mesh."""
    if backend == "generic":
        return xi, wq, ntx
    force = bool(os.environ.get("HPV_FORCE_RULE_PADDING"))     # (measurement knob, scripts/rule1d_sweep.py: the advice for ONE element)
    q_dev, nt_dev = _lib.rule_advice(device, pde, var_form, len(hidden), max(hidden), xi.size, ntx, 1, 1 if force else n_elem_shard)
    pad_rule = q_dev > xi.size and (force or not os.environ.get("HPV_NO_RULE_PADDING"))
    nt = nt_dev if (pad_rule or xi.size == 80) else ntx
    if pad_rule:
        xi, wq = _pad_rule(xi, wq, 80)
    return xi, wq, nt


def _caller_globals(depth=2):
    """Module globals of whoever called the public method `depth - 1` frames above this function -- the IMPLICIT half of the binding
    (what makes the one-line import swap enough).  The explicit, documented half is `module_globals=globals()` in the constructor
    call; HPV_NO_CALLER_GLOBALS=1 switches the frame lookup off altogether (keyword arguments, `module_globals=` and the reference
    defaults remain): a wrapper module or a notebook cell then cannot change a training through a name it happens to hold."""
    if os.environ.get("HPV_NO_CALLER_GLOBALS"):
        return {}
    try:
        return sys._getframe(depth).f_globals
    except ValueError:      # pragma: no cover - no such frame
        return {}


_logged_globals = set()


def _note_global(name, v, ns):
    """Say ONCE per (module, name) which value came from the caller's module globals: a wrapper module or a notebook that happens to
    hold a numeric `LR` / `var_form` / ... would otherwise change the training silently (advisor, round 4).  HPV_QUIET_GLOBALS=1
    silences it; passing the name as a keyword argument (or `module_globals=`) avoids the lookup."""
    mod = ns.get("__name__", "?") if ns is not None else "?"
    if (mod, name) in _logged_globals or os.environ.get("HPV_QUIET_GLOBALS"):
        return
    _logged_globals.add((mod, name))
    shown = v if not isinstance(v, list) else "<list of %d entries>" % len(v)
    print("hp_vpinns_amd: %s = %s taken from the module globals of %r (what the reference class reads; pass %s= to override)"
          % (name, shown, mod, name), file=sys.stderr)


def _resolve(value, name, ns, default, kinds):
    """keyword argument > the caller's module global of that name (what the reference class reads) > reference default."""
    if value is not None:
        return value
    v = ns.get(name) if ns is not None else None
    if isinstance(v, kinds) and not isinstance(v, bool):
        _note_global(name, v, ns)
        return v
    return default


_NUM = (int, float, np.integer, np.floating)


def _counts_2d(N_testfcn):
    """The reference's N_testfcn = [[per element column], [per element row]] (read per element at P2:72-73 / P3:112-113) ->
    (counts per column, counts per row, the pair of every element flattened e = ex * ney + ey, whether any count differs)."""
    nax = np.array([int(v) for v in np.ravel(N_testfcn[0])], dtype=np.int32)
    nay = np.array([int(v) for v in np.ravel(N_testfcn[1])], dtype=np.int32)
    if nax.size < 1 or nay.size < 1 or nax.min() < 1 or nay.min() < 1:
        raise ValueError("N_testfcn needs at least one test function per direction in every element")
    ragged = bool(np.any(nax != nax.max()) or np.any(nay != nay.max()))
    return nax, nay, np.repeat(nax, nay.size), np.tile(nay, nax.size), ragged


def _dense_rhs_2d(F, nax, nay):
    """F_exact_total of the 2-D class as the dense (nex, ney, max nty, max ntx) array hpv_set_rhs takes.  Given as that array
    (entries beyond an element's counts are ignored by the library), or as what the reference class indexes with [ex, ey]: an
    (nex, ney) object array / nested list of (nty_ey, ntx_ex) blocks, padded with zeros here."""
    nex, ney, ntx, nty = nax.size, nay.size, int(nax.max()), int(nay.max())
    try:
        Fd = np.asarray(F, dtype=np.float64)
    except (ValueError, TypeError):      # ragged blocks / an object array of blocks
        Fd = None
    if Fd is not None and Fd.ndim != 2:
        if Fd.shape != (nex, ney, nty, ntx):
            raise ValueError(f"F_exact_total has shape {Fd.shape}, expected {(nex, ney, nty, ntx)} (P2:414)")
        return Fd
    if len(F) != nex or any(len(F[ex]) != ney for ex in range(nex)):
        raise ValueError(f"F_exact_total must hold one block per element: {nex} x {ney}")
    out = np.zeros((nex, ney, nty, ntx))
    for ex in range(nex):
        for ey in range(ney):
            b = np.asarray(F[ex][ey], dtype=np.float64)
            if b.shape != (nay[ey], nax[ex]):
                raise ValueError(f"F_exact_total[{ex}][{ey}] has shape {b.shape}, but N_testfcn gives that element "
                                 f"{(int(nay[ey]), int(nax[ex]))} test functions (y, x)")
            out[ex, ey, :nay[ey], :nax[ex]] = b
    return out


def _check_scheme(scheme, X_f, f=None, need_f=False):
    """The `scheme` switch of P2:125-129 as the 1-D and AdvDiff classes take it: an explicit keyword (P1 and P3 have no such module
    global, so it is never looked up in the caller's).  Raises before any library call."""
    if scheme not in ("VPINNs", "PINNs"):
        raise ValueError("scheme is either 'PINNs' or 'VPINNs' (P2:269)")
    if scheme == "PINNs":
        if X_f is None or np.size(X_f) == 0:
            raise ValueError("scheme 'PINNs' needs collocation points")
        if need_f and f is None:
            raise ValueError("scheme 'PINNs' needs f_train, the right-hand side at the collocation points")
        if need_f and np.size(f) != np.shape(X_f)[0]:
            raise ValueError("f_train needs one value per collocation point")
    return scheme


def _next_chunk(it, nIter, every=10):
    """Iterations `it .. it+n-1` run back to back on the device; `rec` says whether the last of
    them is a recording iteration (it % every == 0, P1:210 / P3:314)."""
    r = it if it % every == 0 else (it // every + 1) * every
    if r < nIter:
        return r - it + 1, True
    return nIter - it, False


class _VPINNBase:
    """Common machinery: handle creation, sharding, the iteration loop pieces."""

    _pde = None
    _act = None
    _n_extra = 0
    _trainable = ()            # VPINNLinear / VPINNNonlinear: the trainable coefficients (dicts: name, init, the direction's fields)

    def _create(self, layers, var_form, LR, lossb_weight, V, init_params, seed, backend, device,
                scheme=_lib.SCHEME_VPINN):
        self.layers = [int(v) for v in layers]
        self.rank, self.world, local_rank = dist_info()
        # the collective code path is taken whenever a process group with >1 ranks exists; HPV_FORCE_DIST=1
        # takes it with a 1-rank group too (lets a single-GPU box exercise exactly what N GPUs run)
        self._dist = self.world > 1 or (os.environ.get("HPV_FORCE_DIST") == "1" and _group_ready())
        if device is None:
            device = local_rank if self._dist else 0
        self.device = device
        bk = {"auto": _lib.BACKEND_AUTO, "generic": _lib.BACKEND_GENERIC, "mfma": _lib.BACKEND_MFMA,
              "hip": _lib.BACKEND_AUTO}[backend]
        # Narrow networks (the reference defaults are 5 wide: P2:280, P3:46) are zero-padded onto the 20-wide MFMA kernels
        # -- exact (init.pad_plan) -- unless the generic kernels are asked for; the library then sees a 20-wide network
        # and this class maps parameters / gradients between the two layouts.
        plan = None if backend == "generic" else pad_plan(self.layers, self._n_extra)
        self._dev_layers, self._pad_idx = (plan if plan is not None else (self.layers, None))
        self._handle_args = ((self._pde, var_form, self._act, self._dev_layers),
                             dict(lr=LR, lossb_weight=lossb_weight, V=V, device=device, backend=bk, scheme=scheme))
        self._populate = None      # set by the subclass: hands the problem (rule, tables, elements, F, data) to self.h
        if self._trainable:
            self._handle_args[1]["n_coef"] = len(self._trainable)
        self.h = _lib.Handle(*self._handle_args[0], **self._handle_args[1])
        if init_params is None:
            init_params = xavier_init(self.layers, seed, extra=[t["init"] for t in self._trainable] if self._trainable else [1.0] * self._n_extra)
        self._init_params = np.asarray(init_params, dtype=np.float64).reshape(-1).copy()
        if self._init_params.size != n_params(self.layers, self._n_extra):
            raise ValueError("init_params has the wrong length")
        self._reducer = None
        self._dist_warm = False
        self._dist_graphs = {}
        self._rccl = False     # in-library ncclAllReduce connected (the multi-GPU default)
        self._p2p = False      # in-library mailbox exchange connected (opt-in: HPV_EXCHANGE=p2p)
        self._coll = False     # multi-GPU through torch.distributed collectives (the fallback)
        if self._dist:
            import torch
            torch.cuda.set_device(device)

    def _history(self, name, handed_in, caller_ns):
        """The list `train` appends to: the one handed to the constructor, else the module-level list of that name the
        caller holds NOW (the reference appends to its module global at train time: P1:214, P2:244 -- the drivers create
        it after the constructor), else the private one this object has kept since construction."""
        if handed_in is not None:
            return handed_in
        for ns in (self._module_globals, caller_ns):
            lst = ns.get(name) if ns is not None else None
            if isinstance(lst, list):
                _note_global(name, lst, ns)
                return lst
        return getattr(self, name)

    def _to_dev(self, theta):
        """user parameter layout -> the layout the library holds (zero-padded for narrow networks)."""
        theta = np.asarray(theta, dtype=np.float64).reshape(-1)
        if self._pad_idx is None:
            return theta
        out = np.zeros(n_params(self._dev_layers, self._n_extra))
        out[self._pad_idx] = theta
        return out

    def _from_dev(self, v):
        return v if self._pad_idx is None else np.ascontiguousarray(np.asarray(v)[self._pad_idx])

    def _replace_handle(self):
        """A bounded library call on a helper thread did not return in time (`_connect_rccl`): that thread may still be inside
        the library with this handle, and after a hung collective the handle's stream may never drain.  The handle is told
        (hpv_rccl_abandon: the late call then touches nothing), is never destroyed (`leak`), and a FRESH handle takes its
        place -- two threads never share a handle (advisor, round 3)."""
        old = self.h
        old.rccl_abandon()
        old.leak()
        self.h = self._new_handle()

    def _new_handle(self):
        """A fresh library handle holding this model's problem and initial parameters (what the constructor built)."""
        prev = self.h
        try:
            self.h = _lib.Handle(*self._handle_args[0], **self._handle_args[1])
            self._populate()
            self._hand_flux()
            self.h.set_params(self._to_dev(self._init_params))
            self.h.backend_in_use()
            return self.h
        finally:
            self.h = prev

    def _finish(self):
        self.h.set_params(self._to_dev(self._init_params))
        self.h.backend_in_use()   # assembles the device batches; raises if a requested backend is unavailable
        if (self.backend() == "generic" and self._handle_args[1]["backend"] == _lib.BACKEND_AUTO and self.rank == 0
                and self._handle_args[1]["scheme"] == _lib.SCHEME_VPINN):     # (the PINN branch picks its kernels at the first pass)
            import warnings
            warnings.warn(f"hp_vpinns_amd: layers {self.layers} are not covered by the MFMA kernels; this model runs on the "
                          "generic kernels, which are one to two orders of magnitude slower (see README.md, 'network shapes')")
        if self._dist:
            # Exchange of the packed buffer, in order of preference (every rank takes the same decision):
            #   "rccl"  (default) ncclAllReduce issued by the library on its own stream, inside its iteration graphs;
            #   "p2p"   (HPV_EXCHANGE=p2p) peer-mapped mailboxes, no collective-library call in the iteration;
            #   "torch" torch.distributed all_reduce on torch's stream -- the fallback when the others cannot be set up.
            want = os.environ.get("HPV_EXCHANGE", "rccl")
            if os.environ.get("HPV_P2P") == "0" and want == "p2p":
                want = "rccl"
            if want == "p2p" and 1 < self.world <= 8:
                self._p2p = self._connect_p2p()
            if not self._p2p and want in ("rccl", "p2p"):
                self._rccl = self._connect_rccl()
            if not (self._p2p or self._rccl):
                import torch
                self._coll = True
                self.h.set_stream(torch.cuda.current_stream().cuda_stream)
                ptr, n = self.h.reduce_buffer()
                self._reducer = Reducer(ptr, n, self.device, force=True)

    def exchange(self):
        """'none' | 'rccl' (in-library ncclAllReduce) | 'p2p' (peer-mapped mailboxes) | 'torch' (torch.distributed)."""
        return "torch" if self._coll else ("p2p" if self._p2p else ("rccl" if self._rccl else "none"))

    def _connect_rccl(self):
        """In-library RCCL communicator (include/hpvpinn.h, hpv_rccl_*).  Every step that can fail locally is AGREED on by all
        ranks before any rank enters the collective that follows it (a rank that has already failed would otherwise leave its
        peers blocked inside ncclCommInitRank): (1) every rank can load librccl; (2) rank 0's ncclUniqueId reaches every
        rank; (3) every rank joins -- bounded by wall clock (HPV_RCCL_TIMEOUT_S, default 120 s): the blocking call runs on a
        helper thread, and a rank whose call has not returned in time votes "failed" and abandons it; (4) two known-answer
        all-reduces give the right sums, same bound.  Any failure or timeout on any rank sends EVERY rank to the
        torch.distributed fallback; ranks that had joined leave the communicator.  A rank that abandoned a call never
        uses that handle again (`_replace_handle`): the helper thread may return late -- a late ncclCommInitRank success
        would otherwise connect the handle in the middle of the fallback's training."""
        import threading

        import torch.distributed as dist

        budget = float(os.environ.get("HPV_RCCL_TIMEOUT_S", "120"))

        def agree(flag):
            flags = [None] * self.world
            dist.all_gather_object(flags, bool(flag))
            return all(flags)

        def bounded(fn):
            """fn() on a helper thread (ctypes releases the GIL inside the library): (finished in time, result or exception)."""
            box = {}

            def run():
                try:
                    box["v"] = fn()
                except BaseException as e:  # noqa: BLE001 -- reported to the caller below
                    box["e"] = e
            t = threading.Thread(target=run, daemon=True)
            t.start()
            t.join(budget)
            if t.is_alive():
                return False, None
            if "e" in box:
                if isinstance(box["e"], _lib.HpvError):
                    return True, box["e"]
                raise box["e"]
            return True, box.get("v")

        try:
            ready = bool(self.h.rccl_available())
        except _lib.HpvError:
            ready = False
        if not agree(ready):
            return False
        uid = None
        if self.rank == 0:
            try:
                uid = self.h.rccl_unique_id()
            except _lib.HpvError:
                uid = None
        box = [uid]
        dist.broadcast_object_list(box, src=0)
        if box[0] is None:
            return False
        hh = self.h
        done, res = bounded(lambda: hh.rccl_connect(self.world, self.rank, box[0]))
        ok = done and not isinstance(res, _lib.HpvError)
        if not done:
            self._replace_handle()       # the helper thread is still inside ncclCommInitRank with the old handle
        if not agree(ok):
            if ok:
                self.h.rccl_disconnect()
            return False
        n = self.h.reduce_buffer()[1]
        expect = self.world * (self.world + 1) / 2 + self.world * 1e-3 * np.arange(n)

        def selftest():
            return all(np.abs(hh.rccl_selftest(n) - expect).max() < 1e-12 for _ in range(2))
        done, res = bounded(selftest)
        good = done and res is True
        if not done:
            # the call that never returned still owns the communicator AND the handle's stream (a collective that never
            # completes blocks everything enqueued behind it): the fallback trains on a fresh handle
            self._replace_handle()
        if not agree(good):
            if done:
                self.h.rccl_disconnect()
            return False
        return True

    def _connect_p2p(self):
        """Set up the in-library exchange (include/hpvpinn.h, hpv_p2p_*): all-gather the ranks' IPC mailbox handles,
        map them, and verify three known-answer exchanges on every rank.  Any failure on any rank -- no peer access,
        IPC refused, a peer not arriving -- makes every rank fall back to the torch.distributed all-reduce."""
        import torch.distributed as dist

        def agree(flag):
            flags = [None] * self.world
            dist.all_gather_object(flags, bool(flag))
            return all(flags)

        try:
            mine = self.h.p2p_export(self.world, self.rank)
        except _lib.HpvError:
            mine = None
        handles = [None] * self.world
        dist.all_gather_object(handles, mine)
        ok = all(hd is not None for hd in handles)
        if ok:
            try:
                self.h.p2p_connect(b"".join(handles))
            except _lib.HpvError:
                ok = False
        if not agree(ok):
            if mine is not None:
                self.h.p2p_disconnect()
            return False
        n = self.h.reduce_buffer()[1]
        expect = self.world * (self.world + 1) / 2 + self.world * 1e-3 * np.arange(n)
        good = True
        for _ in range(3):                      # both mailbox parities and a re-use
            out, timed_out = self.h.p2p_selftest(n)
            good = good and not timed_out and np.abs(out - expect).max() < 1e-12
        if not agree(good):
            self.h.p2p_disconnect()
            return False
        return True

    # -- iteration pieces -----------------------------------------------------------------
    def _step(self, n, read_loss):
        """n Adam iterations; returns loss3 evaluated after the last update if read_loss."""
        if not self._coll:
            return self.h.step(n, read_loss)
        left = n
        if n >= 4 and os.environ.get("HPV_DIST_GRAPH", "1") != "0":
            if not self._dist_warm:      # communicator set-up and lazily created device objects must precede a capture
                self._dist_iter()
                self._dist_warm = True
                left -= 1
            k = left if left <= 16 else self._DIST_GRAPH_ITERS
            g = self._dist_graph(k) if k >= 2 else None
            if g is not None:
                for _ in range(left // k):
                    g.replay()
                left %= k
        for _ in range(left):
            self._dist_iter()
        if not read_loss:
            return None
        self.h.eval_loss()
        self._reducer.allreduce()
        return self.h.read_loss()

    _DIST_GRAPH_ITERS = 8

    def prepare(self, *step_counts):
        """Do every one-off set-up a later `_step(n)` would otherwise do lazily (multi-GPU: communicator warm-up through a
        loss evaluation -- no parameter update -- and capture of the iteration graphs for the given step counts), so that
        a timed region contains iterations only.  Single-GPU handles capture their graphs at the first step."""
        if not self._coll or os.environ.get("HPV_DIST_GRAPH", "1") == "0":
            return
        if not self._dist_warm:
            self.h.eval_loss()
            self._reducer.allreduce()
            self.h.forward_backward()      # lazily created device objects of the backward path (gradient not applied)
            self.h.sync()
            self._dist_warm = True
        for n in step_counts:
            if n >= 4:
                k = n if n <= 16 else self._DIST_GRAPH_ITERS
                self._dist_graph(k)

    def _dist_iter(self):
        """One multi-GPU iteration: partial sums of this shard -> one all-reduce of the packed buffer -> Adam."""
        self.h.forward_backward()
        self._reducer.allreduce()
        self.h.apply_adam()

    def _dist_graph(self, k):
        """`k` multi-GPU iterations -- kernels AND the RCCL all-reduce -- captured once into a hipGraph
        (through torch's capture so that ProcessGroupNCCL records the collective on the capture stream):
        the host then issues one graph launch per k iterations instead of 3k enqueues.  Any failure to
        capture falls back to the eager loop for the rest of the run."""
        if k in self._dist_graphs:
            return self._dist_graphs[k]
        import torch
        g = None
        main = torch.cuda.current_stream()
        try:
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, capture_error_mode="thread_local"):
                self.h.set_stream(torch.cuda.current_stream().cuda_stream)
                for _ in range(k):
                    self._dist_iter()
        except Exception as e:  # noqa: BLE001 -- eager loop is always available
            import warnings
            warnings.warn(f"hp_vpinns_amd: multi-GPU graph capture unavailable ({e}); running the eager loop")
            g = None
            for kk in (2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16):
                self._dist_graphs[kk] = None
        finally:
            self.h.set_stream(main.cuda_stream)
        self._dist_graphs[k] = g
        return g

    def _step_record(self, n):
        """n Adam iterations; ((n, 3) array {loss, lossb, lossv}, (n,) epsilon) AFTER each update.  The loss after update
        k is what the forward pass of iteration k+1 computes anyway, and the device keeps a history of it
        (hpv_step_record / hpv_history_*): per-iteration recording costs one extra forward pass per call instead of one
        per iteration."""
        if not self._coll:
            return self.h.step_record(n)
        out, eps = np.empty((n, 3)), np.zeros(n)
        done = 0
        while done < n:
            c = min(_lib.HIST_CAP, n - done)
            self.h.history_reset()
            self._step(c, False)
            hist, he = self.h.history_read(c)  # entry j: forward pass before update done+j+1 = state after update done+j
            lo = 1 if done == 0 else 0
            out[done + lo - 1:done + c - 1] = hist[lo:]
            eps[done + lo - 1:done + c - 1] = he[lo:]
            done += c
        if n > 0:
            out[n - 1] = self.loss()
            if self._n_extra:
                eps[n - 1] = self.h.get_params()[-self._n_extra]      # (the first of them: what the history's column holds)
        return out, eps

    _RECORD_CHUNK = 1000

    def _recorded_run(self, it, n, tresh, every=10):
        """Iterations it .. it+n-1 in one device run; returns ([(iteration, loss3, epsilon)] for the recording iterations
        (index % every == 0), stop) where stop is the first recorded iteration whose loss is below `tresh` (the
        reference leaves its loop there, P1:215 / P3:320) or None.  On such a stop the state saved before the run is
        restored and the run repeated up to exactly that iteration, so the parameters are those the reference ends with."""
        state = self.h.get_state() if tresh > 0 else None
        hist, eps = self._step_record(n)
        recs, stop = [], None
        for k in range((-it) % every, n, every):
            recs.append((it + k, hist[k], eps[k]))
            if hist[k][0] < tresh:
                stop = it + k
                break
        if stop is not None and stop < it + n - 1:
            self.h.set_state(state)
            self._step(stop - it + 1, False)
        return recs, stop

    def loss_and_grad(self):
        """({loss, lossb, lossv}, d loss / d theta) at the current parameters (global over ranks)."""
        if not self._coll:
            loss3, g = self.h.loss_and_grad(True)
            return loss3, self._from_dev(g)
        self.h.forward_backward()
        t = self._reducer.allreduce()
        loss3 = self.h.read_loss()
        return loss3, self._from_dev(t[: self.h.num_params()].cpu().numpy())

    def loss(self):
        if not self._coll:
            return self.h.loss_and_grad(False)[0]
        self.h.eval_loss()
        self._reducer.allreduce()
        return self.h.read_loss()

    # -- L-BFGS stage after Adam (hpv_lbfgs_step) ------------------------------------------------------
    def _record_lbfgs(self, losses):
        """Append the losses after the accepted iterations to the class's history the way its `train` does (overridden per class;
        VPINNAdvDiff keeps none -- its `train` returns its records -- and the caller has them in the returned dict)."""

    def train_lbfgs(self, max_iter, history=20, lr=1.0, tolerance_grad=1e-7, tolerance_change=1e-9, max_eval=None):
        """Up to `max_iter` L-BFGS iterations with a strong-Wolfe line search on ALL parameters (the network, epsilon, trainable
        coefficients), device-resident; the options are those of torch.optim.LBFGS (`history` = history_size, at most 64;
        max_eval None = max_iter * 5 // 4).  The loss after every accepted iteration goes to the class's loss history like the
        losses of `train`.  Returns {"iters", "func_evals", "pairs_skipped", "reason", "loss"}: `loss` the (iters + 1, 3) array
        {loss, lossb, lossv} from the starting point on, `reason` why it stopped (_lib.LBFGS_REASONS).  Adam's moments are left
        alone -- a later `train` continues Adam from its own state at the new parameters -- and the curvature history survives
        between calls until `lbfgs_reset`, `set_params` or `load_checkpoint`.  One GPU only."""
        if self.world > 1 or self._coll or self._rccl or self._p2p:
            raise RuntimeError("train_lbfgs runs on one GPU only (this model is one rank of several)")
        hist, info = self.h.lbfgs_step(max_iter, history, lr, tolerance_grad, tolerance_change, max_eval)
        self._record_lbfgs(hist[1:])
        info["loss"] = hist
        return info

    def lbfgs_reset(self):
        """Drop the curvature history of `train_lbfgs`: its next iteration steps along the negative gradient."""
        self.h.lbfgs_reset()

    # -- flux term: Neumann / Robin conditions and derivative observations (hpv_set_flux_data) ------
    _flux = None      # (X, coef, g, weight) as handed to the library, kept for a handle that is rebuilt

    def set_flux_data(self, X, g=None, a=0.0, b=None, weight=1.0):
        """Add  lossf = weight * mean((a u + b . grad u - g)^2)  at the points X (n, dim) to the loss; grad u = (u_x) in 1-D,
        (u_x, u_y) in 2-D, (u_x, u_t) for AdvDiff.  `a` a scalar or (n,); `b` an (n, dim) array or one vector for all points
        (None: zero); `g` (n,) targets.  Neumann: a = 0, b = the outward normal, g = the flux; Robin: both; a derivative sensor:
        b = e_c.  X None clears the term.  Multi-GPU: every rank calls it, rank 0 holds the points (as the boundary points)."""
        if X is None:
            self._flux = None
            self.h.set_flux_data(None, None, None)
            return
        d = self.layers[0]
        X = np.asarray(X, dtype=np.float64).reshape(-1, d)
        n = X.shape[0]
        if g is None:
            raise ValueError("set_flux_data needs one target value g per point")
        coef = np.zeros((n, 1 + d))
        coef[:, 0] = np.broadcast_to(np.asarray(a, dtype=np.float64).reshape(-1), (n,))
        if b is not None:
            b = np.asarray(b, dtype=np.float64)
            coef[:, 1:] = np.broadcast_to(b.reshape(1, d) if b.size == d else b.reshape(n, d), (n, d))
        g = np.asarray(g, dtype=np.float64).reshape(-1)
        if g.size != n:
            raise ValueError("set_flux_data needs one target value g per point")
        self._flux = (X.copy(), coef, g.copy(), float(weight))
        self._hand_flux()

    def _hand_flux(self):
        if self._flux is not None and self.rank == 0:
            self.h.set_flux_data(*self._flux)

    def flux_loss(self):
        """(weight * msf, msf) of the flux term in the most recent pass on this rank's handle; zeros without the term."""
        return self.h.read_flux_loss()

    def get_params(self):
        return self._from_dev(self.h.get_params())

    def set_params(self, theta):
        """New parameters; the Adam moments and beta powers are RESET (a fresh optimizer, as after `initialize_NN`).
        Use `load_checkpoint` / `h.set_state` to continue a run."""
        self.h.set_params(self._to_dev(theta))

    def backend(self):
        return {_lib.BACKEND_GENERIC: "generic", _lib.BACKEND_MFMA: "mfma"}[self.h.backend_in_use()]

    # -- evaluation & persistence around the path -----------------------------
    def rel_l2_error(self, X, u_exact):
        """||u_exact - u_NN||_2 / ||u_exact||_2 on the given points: the L2-error half of the metric."""
        u_exact = np.asarray(u_exact, dtype=np.float64).reshape(-1, 1)
        return float(np.linalg.norm(u_exact - self._predict(X), 2) / np.linalg.norm(u_exact, 2))

    # -- device-side validation: derivatives, residual and the error history (hpv_eval_points .. hpv_step_validate) -------------
    _channel_names = ("u", "u_x", "u_y", "u_xx", "u_yy")      # 2-D; the 1-D and AdvDiff classes name their own
    _val_default = ("X_test", "utest")                        # attributes holding the stored test grid

    def evaluate(self, X):
        """The network and its input derivatives at the points X (n, dim): a dict of (n, 1) arrays keyed `u, u_x, u_xx` in 1-D,
        `u, u_x, u_y, u_xx, u_yy` in 2-D (`u_t`, `u_tt` for the second coordinate of AdvDiff) -- one forward launch."""
        ch = self.h.eval_points(np.asarray(X, dtype=np.float64))
        return {k: ch[i][:, None].copy() for i, k in enumerate(self._channel_names)}

    def residual(self, X, f=None):
        """The strong PDE residual at the points X (n, dim) as an (n, 1) array, in either scheme: -u_xx - f (Poisson-1D),
        u_xx + u_yy - f (Poisson-2D), u_t + V u_x - epsilon u_xx - f (AdvDiff, epsilon as currently trained); f None = 0."""
        return self.h.residual_points(np.asarray(X, dtype=np.float64), f)[:, None]

    def set_validation(self, X=None, u=None, du=None):
        """Upload the validation set once: points (n, dim), exact values, optionally exact gradients (n, dim).  Without arguments
        the test grid handed to the constructor.  Multi-GPU: every rank holds and evaluates the whole set (no collective)."""
        if X is None and u is None:
            X, u = (getattr(self, a) for a in self._val_default)
        if X is None or u is None:
            raise ValueError("set_validation needs points and exact values (or no arguments: the stored test grid)")
        self._val_has_du = du is not None
        self.h.set_validation(X, u, du)

    def clear_validation(self):
        self._val_has_du = False
        self.h.set_validation(None, None)

    def _val_dict(self, raw):
        raw = np.asarray(raw, dtype=np.float64)
        h1 = float(np.sqrt(raw[3] / raw[4])) if getattr(self, "_val_has_du", False) else None
        return dict(rel_l2=float(np.sqrt(raw[0] / raw[1])), max_abs=float(raw[2]), rel_h1=h1, raw=raw)

    def validate(self):
        """Error norms on the validation set, reduced on the device: dict(rel_l2, max_abs, rel_h1 (the relative error of the
        gradient in L2; None without exact gradients), raw = the six sums of hpv_validate)."""
        return self._val_dict(self.h.validate())

    def train_validated(self, nIter, every):
        """nIter Adam iterations with the validation error sampled after every `every`-th update, nothing read back in between:
        (iterations, rel_l2, max_abs) arrays of nIter // every entries, iterations = number of updates applied at the sample.
        A remainder nIter % every is trained, not validated."""
        nIter, every = int(nIter), int(every)
        if every < 1 or nIter < 0:
            raise ValueError("train_validated needs nIter >= 0 and every >= 1")
        ns = nIter // every
        rows = np.empty((ns, 6))
        done = 0
        while done < ns or done == 0:
            c = min(_lib.HIST_CAP, ns - done)
            last = done + c == ns
            n = c * every + (nIter - ns * every if last else 0)       # (the remainder rides in the last call)
            if not self._coll:
                rows[done:done + c] = self.h.step_validate(n, every)
            else:
                self.h.validation_reset()
                for _ in range(c):
                    self._step(every, False)
                    self.h.validate_enqueue()
                if n > c * every:
                    self._step(n - c * every, False)
                rows[done:done + c] = self.h.validation_read(c)
            done += c
            if last:
                break
        return every * np.arange(1, ns + 1), np.sqrt(rows[:, 0] / rows[:, 1]), rows[:, 2].copy()

    # -- local hp-refinement: element boxes, device-side indicators, refine-and-continue (adapt.py; hpv_set_element_boxes,
    #    hpv_element_indicators) ---------------------------------------------------------------------------------------------
    _mesh = None               # the box list handed to set_mesh (None: the constructor's grid)
    _dev_rule = None           # (xi, yi) of the rule the device holds (yi None in 1-D); set by the populate step

    def _need_vpinns(self, what):
        if getattr(self, "scheme", "VPINNs") != "VPINNs":
            raise ValueError(f"{what} belongs to the variational scheme")

    @property
    def mesh(self):
        """The elements as an `adapt.ElementMesh` (a copy): what `set_mesh` was given last, else the constructor's grid."""
        return (self._mesh if self._mesh is not None else self._grid_mesh()).copy()

    def _f_at_quad(self, mesh, f, eb, ee):
        """f at the DEVICE rule's points of the elements [eb, ee), element-major (q = j * qx + i)."""
        xi, yi = self._dev_rule
        P = mesh.quad_points(xi, yi, eb, ee)
        fq = np.asarray(f(*[P[:, c] for c in range(P.shape[1])]), dtype=np.float64)
        return np.broadcast_to(fq.reshape(-1) if fq.size > 1 else fq, (P.shape[0],)).copy()

    def _populate_mesh(self, mesh, f):
        """The populate step on a box list: rule advice for the new shard, tables for the maximal counts, the boxes, F assembled on
        the device from f at the device rule's points, the active counts.  Data / boundary points are left as they are."""
        h, n = self.h, len(mesh)
        eb, ee = shard_range(n, self.rank, self.world)
        ntx, nty = int(mesh.nax.max()), int(mesh.nay.max())
        xi, wx, yi, wy, ntx_dev = self._mesh_rule(ee - eb, ntx, nty)
        if mesh.dim == 1:
            h.set_active_tests(None)
        else:
            h.set_active_tests_2d(None, None)
        h.set_rhs(None)                                    # (counts and F of the old mesh would be checked against the new one)
        h.set_quadrature(xi, wx, yi, wy)
        edge = None
        if mesh.dim == 1 and self.var_form == 3:
            edge = np.ascontiguousarray(dTest_fcn(ntx_dev, np.array([-1.0, 1.0]))[0])
        h.set_tables(tables_1d(ntx_dev, xi), None if mesh.dim == 1 else tables_1d(nty, yi), edge)
        self._dev_rule = (xi, yi)
        self._hand_elements(mesh, eb, ee)
        if f is not None:
            NR = ntx_dev * nty
            F = np.zeros((n, NR))                          # (only the owned rows are read: hpv_set_rhs slices [eb, ee))
            if ee > eb:
                F[eb:ee] = h.assemble_rhs(self._f_at_quad(mesh, f, eb, ee), (ee - eb) * NR).reshape(ee - eb, NR)
            h.set_rhs(F.reshape(-1))
        if mesh.dim == 1:
            if np.any(mesh.nax != ntx_dev):
                h.set_active_tests(mesh.nax)
        elif np.any(mesh.nax != ntx) or np.any(mesh.nay != nty):
            h.set_active_tests_2d(mesh.nax, mesh.nay)

    def _hand_elements(self, mesh, eb, ee):
        if isinstance(mesh, MappedMesh):
            raise ValueError("mapped elements (adapt.MappedMesh) belong to VPINNLinear / VPINNNonlinear")
        self.h.set_element_boxes(mesh.boxes, eb, ee)

    def set_mesh(self, mesh, f=None):
        """Continue on another set of elements: `mesh` an `adapt.ElementMesh` (any list of boxes with per-element counts), `f` a
        callable f(x) / f(x, y) on flat arrays giving the right-hand side, or None where it is zero (AdvDiff).  Parameters, Adam
        moments and step counters are untouched -- `h.get_state()` is the same before and after, bit for bit -- and the histories
        are kept; only the variational term's elements change.  Multi-GPU: every rank calls it with the same mesh and takes
        its `shard_range(len(mesh), rank, world)`."""
        self._need_vpinns("set_mesh")
        if not isinstance(mesh, ElementMesh) or mesh.dim != self.layers[0]:
            raise ValueError("set_mesh needs an adapt.ElementMesh of the problem's dimension")
        mesh = mesh.copy()
        self._populate_mesh(mesh, f)
        self._mesh = mesh

        def populate():                                    # what a fresh handle would be given: the mesh AND the data points
            self._populate_mesh(mesh, f)
            self._hand_data()
        self._populate = populate
        self.h.backend_in_use()                            # assembles the device batches; raises if a requested backend is unavailable

    def element_indicators(self, f=None):
        """(n_owned, 5) refinement indicators of this rank's elements at the current parameters, computed on the device:
        columns loss_e, eta2_e, sumR2_e, topx_e, topy_e (include/hpvpinn.h, hpv_element_indicators).  `f` as in `set_mesh`."""
        self._need_vpinns("element_indicators")
        mesh = self._mesh if self._mesh is not None else self._grid_mesh()
        eb, ee = shard_range(len(mesh), self.rank, self.world)
        fq = None if f is None or ee == eb else self._f_at_quad(mesh, f, eb, ee)
        return self.h.element_indicators(fq)

    def adapt(self, f=None, **mark_kw):
        """One round of indicators -> `adapt.mark` -> `adapt.refine` -> `set_mesh`; returns the new mesh.  Keyword arguments go to
        `mark` (theta, smooth, p_max, max_elements).  Single GPU only: gathering the indicators across ranks is not implemented."""
        if self.world > 1:
            raise NotImplementedError("adapt() on several GPUs needs the indicators of all ranks; not implemented")
        mesh = self.mesh
        new = refine(mesh, mark(self.element_indicators(f), mesh, **mark_kw), p_max=mark_kw.get("p_max"))
        self.set_mesh(new, f)
        return new

    def train_adaptive(self, nIter, adapt_every, f=None, max_elements=None, **mark_kw):
        """nIter iterations of `train`, with one `adapt` round after every `adapt_every` of them (none after the last chunk).
        Returns [(iterations done, elements after the round, loss on the new mesh)], one entry per adaptation."""
        if self.world > 1:
            raise NotImplementedError("train_adaptive() on several GPUs needs the indicators of all ranks; not implemented")
        nIter, adapt_every = int(nIter), int(adapt_every)
        if adapt_every < 1:
            raise ValueError("adapt_every >= 1")
        out, it = [], 0
        while it < nIter:
            n = min(adapt_every, nIter - it)
            self._train_n(n)
            it += n
            if it < nIter:
                new = self.adapt(f, max_elements=max_elements, **mark_kw)
                out.append((it, len(new), float(self.loss()[0])))
        return out

    @staticmethod
    def _ckpt_path(path):
        path = os.fspath(path)
        return path if path.endswith(".npz") else path + ".npz"     # what np.savez would write

    def save_checkpoint(self, path):
        """Parameters + Adam moments + beta powers (.npz appended when missing, for saving and loading alike); the
        reference never saves weights."""
        np.savez(self._ckpt_path(path), state=self.h.get_state(), layers=np.asarray(self.layers),
                 dev_layers=np.asarray(self._dev_layers), cls=type(self).__name__)

    def load_checkpoint(self, path):
        """Restores parameters AND optimizer state (unlike `set_params`, which resets the Adam moments and beta powers)."""
        d = np.load(self._ckpt_path(path), allow_pickle=False)
        if list(d["layers"]) != list(self.layers) or str(d["cls"]) != type(self).__name__:
            raise ValueError("checkpoint was written by a different model")
        if "dev_layers" in d and list(d["dev_layers"]) != list(self._dev_layers):
            raise ValueError("checkpoint was written with a different device layout (backend='generic' vs padded MFMA)")
        self.h.set_state(d["state"])

    def _predict(self, X):
        X = np.asarray(X, dtype=np.float64)
        return self.h.predict(X)[:, None]

    def _set_collocation_shard(self, X_f, f):
        """Strong-form branch, multi-GPU: the collocation points shard over the ranks in contiguous blocks (lossp is a mean of
        independent point-wise terms), the boundary term stays on rank 0, one all-reduce of the packed buffer per iteration.
        f None: zero right-hand side (AdvDiff)."""
        Xf = np.asarray(X_f, dtype=np.float64)
        ff = None if f is None else np.asarray(f, dtype=np.float64).reshape(-1)
        if Xf.shape[0] < self.world:
            raise ValueError("fewer collocation points than ranks")
        cb, ce = shard_range(Xf.shape[0], self.rank, self.world)
        self.h.set_collocation(Xf[cb:ce], None if ff is None else ff[cb:ce], n_total=Xf.shape[0])


class VPINN1D(_VPINNBase):
    """Poisson 1-D hp-VPINN (reference P1:30-224; constructor P1:31-32, call site P1:333-334)."""

    _pde, _act = _lib.PDE_POISSON1D, _lib.ACT_SIN   # tf.sin, P1:134
    _channel_names = ("u", "u_x", "u_xx")
    _val_default = ("xtest", "utest")

    def __init__(self, X_u_train, u_train, X_quad, W_quad, F_exact_total, grid, X_test, u_test, layers,
                 X_f_train=None, f_train=None, *, var_form=None, lossb_weight=None, LR=None, init_params=None,
                 seed=1234, backend="auto", device=None, total_record=None, module_globals=None, scheme="VPINNs"):
        # scheme 'PINNs' (an extension: P1 has no such switch; it follows P2:124-129): the variational term is replaced by
        # lossp = mean((-u_xx - f_train)^2) at X_f_train (net_f, P1:150-155), loss = lossb_weight * lossb + lossp
        self.scheme = _check_scheme(scheme, X_f_train, f_train, need_f=True)
        ns = module_globals if module_globals is not None else _caller_globals()
        self._module_globals = module_globals
        var_form = _resolve(var_form, "var_form", ns, 1, (int, np.integer))              # P1:234 (read at P1:82-91)
        lossb_weight = _resolve(lossb_weight, "lossb_weight", ns, 1, _NUM)               # P1:240 (read at P1:100)
        LR = _resolve(LR, "LR", ns, 0.001, _NUM)                                         # P1:231 (read at P1:102)
        self.x, self.u = np.asarray(X_u_train, dtype=np.float64), np.asarray(u_train, dtype=np.float64)
        self.xf, self.f = X_f_train, f_train
        self.xquad, self.wquad = np.asarray(X_quad, dtype=np.float64), np.asarray(W_quad, dtype=np.float64)
        self.xtest, self.utest = X_test, u_test
        # F_ext_total[e] may be shorter in some elements (p-refinement: the driver's N_testfcn_total list, P1:268-281; the
        # class reads Ntest_element = len(F_ext_total[e]), P1:66-67): padded here to the longest, with the counts passed on
        Fe = [np.asarray(f, dtype=np.float64).reshape(-1) for f in F_exact_total]
        self.Nelement = len(Fe)                            # P1:43
        self._n_active = np.array([f.size for f in Fe], dtype=np.int32)
        self.N_test = int(self._n_active.max())            # P1:44 (the reference reads element 0; equal when uniform)
        self.F_ext_total = np.zeros((self.Nelement, self.N_test, 1))
        for e, f in enumerate(Fe):
            self.F_ext_total[e, :f.size, 0] = f
        self._N_test_dev = self.N_test                     # (may grow to the 80 / 60 kernel's 60 below, once the backend is known)
        self.grid = np.asarray(grid, dtype=np.float64)
        self.var_form, self.LR, self.lossb_weight = var_form, LR, lossb_weight
        self._total_record_arg = total_record
        self.total_record = [] if total_record is None else total_record
        if self.grid.size != self.Nelement + 1:
            raise ValueError("grid must have Nelement+1 entries")
        self._create(layers, var_form, LR, lossb_weight, 1.0, init_params, seed, backend, device,
                     scheme=_lib.SCHEME_PINN if scheme == "PINNs" else _lib.SCHEME_VPINN)

        # the rule and the table size the device gets: one decision, shared with set_mesh (_device_rule_1d)
        dev_rule = None
        if scheme == "VPINNs":
            eb, ee = shard_range(self.Nelement, self.rank, self.world)
            dev_rule = _device_rule_1d(self.xquad.reshape(-1), self.wquad.reshape(-1), self.N_test, ee - eb, self._pde, var_form,
                                       self.layers[1:-1], self.device, backend)
            self._N_test_dev = dev_rule[2]

        def populate():
            if scheme == "PINNs":
                self._set_collocation_shard(X_f_train, f_train)
                if self.rank == 0:
                    self.h.set_data(self.x, self.u.reshape(-1))
                return
            xi, wq = dev_rule[0], dev_rule[1]
            self.h.set_quadrature(xi, wq)
            self._dev_rule = (xi, None)
            edge = None
            nt = self._N_test_dev
            if var_form == 3:
                d1b = dTest_fcn(nt, np.array([-1.0, 1.0]))[0]     # (N_test, 2): phi'(-1), phi'(1)  (P1:79)
                edge = np.ascontiguousarray(d1b)
            self.h.set_tables(tables_1d(nt, xi), None, edge)
            eb, ee = shard_range(self.Nelement, self.rank, self.world)
            self.h.set_elements(self.grid, None, eb, ee)
            Fd = self.F_ext_total
            if nt != self.N_test:
                Fd = np.zeros((self.Nelement, nt, 1))
                Fd[:, :self.N_test] = self.F_ext_total
            self.h.set_rhs(Fd.reshape(-1))
            if np.any(self._n_active != nt):
                self.h.set_active_tests(self._n_active)
            if self.rank == 0:
                self.h.set_data(self.x, self.u.reshape(-1))
        self._populate = populate
        self._backend_arg = backend
        populate()
        self._finish()

    def _grid_mesh(self):
        return ElementMesh.from_grid(self.grid, None, self._n_active)

    def _mesh_rule(self, n_shard, ntx, nty):
        xi, wq, nt = _device_rule_1d(self.xquad.reshape(-1), self.wquad.reshape(-1), ntx, n_shard, self._pde, self.var_form,
                                     self.layers[1:-1], self.device, self._backend_arg)
        return xi, wq, None, None, nt

    def _hand_data(self):
        if self.rank == 0:
            self.h.set_data(self.x, self.u.reshape(-1))

    def _train_n(self, n):
        self.train(n, 0.0)

    def _record_lbfgs(self, losses):
        self.total_record = self._history("total_record", self._total_record_arg, None)
        it = int(self.total_record[-1][0]) + 1 if len(self.total_record) else 0
        for k, l3 in enumerate(losses):
            self.total_record.append(np.array([it + k, float(l3[0])]))

    def predict(self, x):                                   # P1:197-199
        return self._predict(x)

    def train(self, nIter, tresh):
        """P1:201-224.  The loss is read back every 10 iterations, AFTER that iteration's update,
        appended to `total_record` as [it, loss]; early exit when loss < tresh.  `total_record` is the list handed to the
        constructor, else the caller's module-level `total_record` as it exists now (P1:335 creates it after P1:333).
        (scheme 'PINNs': the Lossv column of the progress line is lossp.)"""
        self.total_record = self._history("total_record", self._total_record_arg, _caller_globals())
        start_time = time.time()
        it = 0
        while it < nIter:
            n = min(self._RECORD_CHUNK, nIter - it)
            recs, stop = self._recorded_run(it, n, tresh)
            it += n
            for last, loss3, _ in recs:
                loss_value, loss_valueb, loss_valuev = float(loss3[0]), float(loss3[1]), float(loss3[2])
                self.total_record.append(np.array([last, loss_value]))
                if last == stop:
                    print('It: %d, Loss: %.3e' % (last, loss_value))
                    break
                if last % 100 == 0 and self.rank == 0:
                    elapsed = time.time() - start_time
                    print('It: %d, Lossb: %.3e, Lossv: %.3e, Time: %.2f' % (last, loss_valueb, loss_valuev, elapsed))
                    start_time = time.time()
            if stop is not None:
                break
        self.h.sync()


class VPINN2D(_VPINNBase):
    """Poisson 2-D hp-VPINN (reference P2:27-257; constructor P2:28-29, call site P2:430-431)."""

    _pde, _act = _lib.PDE_POISSON2D, _lib.ACT_TANH   # tf.tanh, P2:165

    def __init__(self, X_u_train, u_train, X_f_train, f_train, X_quad, W_quad, U_exact_total, F_exact_total,
                 gridx, gridy, N_testfcn, X_test, u_test, layers, *, var_form=None, scheme=None, LR=0.001,
                 lossb_weight=10, init_params=None, seed=1234, backend="auto", device=None, loss_his=None,
                 module_globals=None):
        ns = module_globals if module_globals is not None else _caller_globals()
        self._module_globals = module_globals
        var_form = _resolve(var_form, "var_form", ns, 1, (int, np.integer))              # P2:281 (read at P2:93-115)
        scheme = _resolve(scheme, "scheme", ns, "VPINNs", str)                           # P2:279 (read at P2:125-128)
        if scheme not in ("VPINNs", "PINNs"):
            raise ValueError("scheme is either 'PINNs' or 'VPINNs' (P2:269)")
        self.scheme = scheme
        self.X_u_train = np.asarray(X_u_train, dtype=np.float64)
        self.utrain = np.asarray(u_train, dtype=np.float64)
        self.xf_train, self.ftrain = X_f_train, f_train
        self.U_ext_total = U_exact_total                   # stored, never used (P2:47)
        self.Nelementx, self.Nelementy = np.size(N_testfcn[0]), np.size(N_testfcn[1])   # P2:43-44
        # the counts may differ from element column to column and row to row (p-refinement; the class reads them per element,
        # P2:72-73): tables, rule padding and F are built for the maxima, the pairs are handed to the library
        nax, nay, self._nax_e, self._nay_e, ragged = _counts_2d(N_testfcn)
        self.Ntestx, self.Ntesty = int(nax.max()), int(nay.max())     # P2:45-46 (the reference reads element 0; equal when uniform)
        self.F_ext_total = _dense_rhs_2d(F_exact_total, nax, nay)
        self.gridx, self.gridy = np.asarray(gridx, dtype=np.float64), np.asarray(gridy, dtype=np.float64)
        self.X_test, self.utest = X_test, u_test
        self.var_form = var_form
        self._loss_his_arg = loss_his
        self.loss_his = [] if loss_his is None else loss_his
        self._create(layers, var_form, LR, lossb_weight, 1.0, init_params, seed, backend, device,
                     scheme=_lib.SCHEME_PINN if scheme == "PINNs" else _lib.SCHEME_VPINN)

        def populate():
            if scheme == "PINNs":
                # strong-form branch (P2:128-129): loss = 10 lossb + mean((u_xx+u_yy-f)^2) at X_f_train
                self._set_collocation_shard(X_f_train, f_train)
            else:
                xi, wx, yi, wy = _tensor_rule(X_quad, W_quad)
                # (var_form 1 runs on the one-hot instantiations of the whole-iteration kernel, var_form 0 on the FOUR-channel ones: 12x12, 16x16 and
                #  20x20 points -- 18 / 19-point rules padded onto 20x20 95.2 / 96.1 -> 84.8 / 85.2 us, 17 points level: scripts/pad_probe.py)
                eb, ee = shard_range(self.Nelementx * self.Nelementy, self.rank, self.world)
                xi, wx, yi, wy = _device_rule_2d(xi, wx, yi, wy, self.Ntestx, self.Ntesty, ee - eb, self._pde, var_form, self.layers[1:-1],
                                                 self.device, backend)
                self.h.set_quadrature(xi, wx, yi, wy)
                self._dev_rule = (xi, yi)
                self.h.set_tables(tables_1d(self.Ntestx, xi), tables_1d(self.Ntesty, yi))
                eb, ee = shard_range(self.Nelementx * self.Nelementy, self.rank, self.world)
                self.h.set_elements(self.gridx, self.gridy, eb, ee)
                self.h.set_rhs(self.F_ext_total.reshape(-1))
                if ragged:
                    self.h.set_active_tests_2d(self._nax_e, self._nay_e)
            if self.rank == 0:
                self.h.set_data(self.X_u_train, self.utrain.reshape(-1))
        self._populate = populate
        self._backend_arg, self._rule_args = backend, (X_quad, W_quad)
        populate()
        self._finish()

    def _grid_mesh(self):
        return ElementMesh(ElementMesh.from_grid(self.gridx, self.gridy).boxes, self._nax_e, self._nay_e)

    def _mesh_rule(self, n_shard, ntx, nty):
        xi, wx, yi, wy = _tensor_rule(*self._rule_args)
        return _device_rule_2d(xi, wx, yi, wy, ntx, nty, n_shard, self._pde, self.var_form, self.layers[1:-1], self.device,
                               self._backend_arg) + (ntx,)

    def _hand_data(self):
        if self.rank == 0:
            self.h.set_data(self.X_u_train, self.utrain.reshape(-1))

    def _train_n(self, n):
        self.train(n)

    def _record_lbfgs(self, losses):
        self.loss_his = self._history("loss_his", self._loss_his_arg, None)
        self.loss_his.extend(float(l3[0]) for l3 in losses)

    def predict(self, X=None):                              # P2:255-257 (stored test grid)
        return self._predict(self.X_test if X is None else X)

    def train(self, nIter, record_every=1):
        """P2:233-253: the loss is read back EVERY iteration (after the update) into `loss_his`.
        `record_every=k` reads it every k-th iteration instead (the device then runs k iterations
        back to back); the default 1 is the reference behaviour.  `loss_his` is the list handed to the constructor, else the
        caller's module-level `loss_his` as it exists now (P2:433 creates it after P2:430)."""
        self.loss_his = self._history("loss_his", self._loss_his_arg, _caller_globals())
        start_time = time.time()
        it = 0
        while it < nIter:
            if record_every == 1:      # every update recorded: device-side loss history, one read-back per chunk
                n = min(self._RECORD_CHUNK, nIter - it)
                losses = self._step_record(n)[0][:, 0]
            else:
                n = min(record_every, nIter - it)
                losses = [float(self._step(n, True)[0])]
            for k, loss_value in enumerate(losses):
                i = it + (k if record_every == 1 else n - 1)        # index of the iteration this value belongs to
                self.loss_his.append(float(loss_value))
                if i % 100 == 0 and self.rank == 0:
                    elapsed = time.time() - start_time
                    print('It: %d, Loss: %.3e, Time: %.2f' % (i, loss_value, elapsed))
                    start_time = time.time()
            it += n
        self.h.sync()


class VPINNAdvDiff(_VPINNBase):
    """Advection-diffusion with trainable diffusion coefficient (reference P3:58-341;
    constructor P3:60-61, call site P3:488-489)."""

    _pde, _act = _lib.PDE_ADVDIFF, _lib.ACT_TANH   # tf.tanh, P3:226
    _n_extra = 1                                   # epsilon, init 1.0 (P3:63)
    _channel_names = ("u", "u_x", "u_t", "u_xx", "u_tt")
    _val_default = ("XT_test", "utest")

    def __init__(self, XT_u_train, u_train, XT_f_train, XT_quad, W_quad, T_quad, WT_quad, grid_x, grid_t,
                 N_testfcn, XT_test, u_test, layers, lb=None, ub=None, *, var_form=None, LR=None, V=None,
                 lossb_weight=10, init_params=None, seed=1234, backend="auto", device=None, module_globals=None,
                 scheme="VPINNs"):
        # scheme 'PINNs' (an extension: P3 builds lossp at P3:186 but never trains on it; the switch follows P2:124-129): the
        # variational term is replaced by lossp = mean((u_t + V u_x - epsilon u_xx)^2) at XT_f_train (net_f, P3:247-253),
        # loss = lossb + lossp with lossb = 10 * mean(...) (P3:184); epsilon stays trainable
        self.scheme = _check_scheme(scheme, XT_f_train)
        ns = module_globals if module_globals is not None else _caller_globals()
        self._module_globals = module_globals
        var_form = _resolve(var_form, "var_form", ns, 0, (int, np.integer))              # P3:38 (read at P3:161-174)
        LR = _resolve(LR, "LR", ns, 0.001, _NUM)                                         # P3:35 (read at P3:191)
        V = _resolve(V, "V", ns, 1.0, _NUM)                                              # P3:43 (read at P3:163,171)
        self.lb, self.ub = lb, ub
        self.XT_u_train = np.asarray(XT_u_train, dtype=np.float64)
        self.u = np.asarray(u_train, dtype=np.float64)
        self.XT_f_train = XT_f_train
        self.Nelementx, self.Nelementt = np.size(N_testfcn[0]), np.size(N_testfcn[1])
        # (the counts may differ per element column / row: P3:112-113; see VPINN2D)
        nax, nat, self._nax_e, self._nat_e, ragged = _counts_2d(N_testfcn)
        self.Ntestx, self.Ntestt = int(nax.max()), int(nat.max())
        self.grid_x, self.grid_t = np.asarray(grid_x, dtype=np.float64), np.asarray(grid_t, dtype=np.float64)
        self.XT_test, self.utest = XT_test, u_test
        self.var_form, self.V = var_form, V
        self._create(layers, var_form, LR, lossb_weight, V, init_params, seed, backend, device,
                     scheme=_lib.SCHEME_PINN if scheme == "PINNs" else _lib.SCHEME_VPINN)

        def populate():
            if scheme == "PINNs":
                self._set_collocation_shard(XT_f_train, None)      # zero right-hand side (P3:186)
                if self.rank == 0:
                    self.h.set_data(self.XT_u_train, self.u.reshape(-1))
                return
            xi, wx, ti, wt = _tensor_rule(XT_quad, W_quad)
            # rules below 10 points onto the 10x10 / 5x5 tile kernel, rules between the instantiated ones onto the whole-iteration kernel's
            # general forms (round 6): var_form 1 has three channels (every shape), var_form 0 four (12x12, 16x16, 20x20)
            eb, ee = shard_range(self.Nelementx * self.Nelementt, self.rank, self.world)
            xi, wx, ti, wt = _device_rule_2d(xi, wx, ti, wt, self.Ntestx, self.Ntestt, ee - eb, self._pde, var_form, self.layers[1:-1],
                                             self.device, backend)
            self.h.set_quadrature(xi, wx, ti, wt)
            self._dev_rule = (xi, ti)
            self.h.set_tables(tables_1d(self.Ntestx, xi), tables_1d(self.Ntestt, ti))
            eb, ee = shard_range(self.Nelementx * self.Nelementt, self.rank, self.world)
            self.h.set_elements(self.grid_x, self.grid_t, eb, ee)
            self.h.set_rhs(None)                               # zero right-hand side (P3:180)
            if ragged:
                self.h.set_active_tests_2d(self._nax_e, self._nat_e)
            if self.rank == 0:
                self.h.set_data(self.XT_u_train, self.u.reshape(-1))
        self._populate = populate
        self._backend_arg, self._rule_args = backend, (XT_quad, W_quad)
        populate()
        self._finish()

    def _grid_mesh(self):
        return ElementMesh(ElementMesh.from_grid(self.grid_x, self.grid_t).boxes, self._nax_e, self._nat_e)

    _mesh_rule = VPINN2D._mesh_rule

    def _hand_data(self):
        if self.rank == 0:
            self.h.set_data(self.XT_u_train, self.u.reshape(-1))

    def _train_n(self, n):
        self.train(n, 0.0)

    @property
    def epsilon(self):
        return self.get_params()[-1:]

    def predict(self, X=None):
        return self._predict(self.XT_test if X is None else X)

    def train(self, nIter, tresh):
        """P3:291-341 -- returns (error_records, total_records, u_records, u_records_iterhis,
        total_time_train) like the reference.  (scheme 'PINNs': the Lossv column of the progress line is lossp.)"""
        total_time_train, min_loss = 0.0, 1e16
        total_records, u_records_iterhis, u_records = [], [], None
        loss_value, start_time = None, time.time()
        it = 0
        while it < nIter:
            if it + self._RECORD_CHUNK - 1 <= 0.9 * nIter:
                # outside the last tenth of the run (where new minima snapshot the prediction, P3:324-326) the records come
                # from the device-side loss / epsilon history: one read-back per chunk instead of one per 10 iterations
                n = min(self._RECORD_CHUNK, nIter - it)
                t0 = time.time()
                recs, stop = self._recorded_run(it, n, tresh)
                total_time_train += time.time() - t0
                it += n
                for last, loss3, eps in recs:
                    loss_value, epsilon_value = float(loss3[0]), np.array([eps])
                    total_records.append(np.array([last, loss_value, epsilon_value, 1], dtype=object))
                    if last == stop:
                        print('It: %d, Loss: %.3e' % (last, loss_value))
                        break
                    if last % 100 == 0 and self.rank == 0:
                        elapsed = time.time() - start_time
                        print('It: %d, Lossv: %.3e, Lossp: %.3e, Lossb: %.3e, Time: %.2f, epsilon: %.4f'
                              % (last, loss3[2], 1, loss3[1], elapsed, float(eps)))
                        start_time = time.time()
                if stop is not None:
                    break
                continue
            n, rec = _next_chunk(it, nIter)
            last = it + n - 1
            t0 = time.time()
            loss3 = self._step(n, rec)
            total_time_train += time.time() - t0
            it += n
            if rec:
                loss_value = float(loss3[0])
                epsilon_value = self.epsilon
                total_records.append(np.array([last, loss_value, epsilon_value, 1], dtype=object))
                if loss_value < tresh:
                    print('It: %d, Loss: %.3e' % (last, loss_value))
                    break
                if last > 0.9 * nIter and loss_value < min_loss:
                    min_loss = loss_value
                    u_records = self.predict()
                if last % 100 == 0 and self.rank == 0:
                    elapsed = time.time() - start_time
                    print('It: %d, Lossv: %.3e, Lossp: %.3e, Lossb: %.3e, Time: %.2f, epsilon: %.4f'
                          % (last, loss3[2], 1, loss3[1], elapsed, float(epsilon_value[0])))
                    start_time = time.time()
        self.h.sync()
        error_records = [loss_value, 1]
        return error_records, total_records, u_records, u_records_iterhis, total_time_train


def _coef_field(c, P, dim, what, vector):
    """A coefficient at the points P (n, dim): `c` a constant (a scalar; for a vector-valued coefficient also one (dim,) vector) or a
    callable of P returning (n, dim) -- or (n,) for a scalar field, which an isotropic kappa may also be.  Returns (n, dim) for
    vector-valued coefficients, (n,) otherwise."""
    n = P.shape[0]
    if callable(c):
        v = np.asarray(c(P), dtype=np.float64)
        if v.shape == (n, 1) and (not vector or dim == 1):
            v = v.reshape(n)
        if v.shape == (n,):
            return np.repeat(v[:, None], dim, axis=1) if vector else v.copy()
        if vector and v.shape == (n, dim):
            return v.copy()
        raise ValueError(f"{what}(points) returned shape {v.shape}; expected {(n, dim) if vector else (n,)}")
    v = np.asarray(c, dtype=np.float64)
    if v.size == 1:
        return np.full((n, dim) if vector else (n,), float(v.reshape(-1)[0]))
    if vector and v.shape == (dim,):
        return np.broadcast_to(v, (n, dim)).copy()
    raise ValueError(f"a constant {what} is a scalar" + (f" or a vector of {dim} entries" if vector else ""))


def _kappa_field(c, P, dim):
    """kappa at the points P (n, dim): what `_coef_field` returns, (n, dim), for a diagonal or isotropic one; (n, 2, 2) for a full
    tensor -- in 2-D a constant (2, 2) array or a callable returning (n, 2, 2), rows [[kxx, kxy], [kyx, kyy]], symmetric or not."""
    n = P.shape[0]
    if dim == 2 and callable(c):
        v = np.asarray(c(P), dtype=np.float64)
        return v.copy() if v.shape == (n, 2, 2) else _coef_field(lambda _P: v, P, dim, "kappa", True)
    if dim == 2 and np.shape(c) == (2, 2):
        return np.broadcast_to(np.asarray(c, dtype=np.float64), (n, 2, 2)).copy()
    return _coef_field(c, P, dim, "kappa", True)


# _FD_STEP = eps^(1/3) ~ 6.1e-6 and _FD_TOL = 1e4 _FD_STEP^2 ~ 3.7e-7 per unit of scale (adapt.py): see _check_ansatz_field


def _ansatz_field(c, P, dim, what):
    """One field of the ansatz u = G + D N at the points P (n, dim) as (n, 1 + dim): the value and its gradient.  `c` a callable of P
    returning exactly that, or a constant (zero gradient)."""
    n = P.shape[0]
    if callable(c):
        v = np.asarray(c(P), dtype=np.float64)
        if v.shape != (n, 1 + dim):
            raise ValueError(f"hard_bc {what}(points) returned shape {v.shape}; expected {(n, 1 + dim)}: the value and the gradient")
        return v.copy()
    v = np.asarray(c, dtype=np.float64)
    if v.size != 1:
        raise ValueError(f"a constant hard_bc {what} is a scalar")
    out = np.zeros((n, 1 + dim))
    out[:, 0] = float(v.reshape(-1)[0])
    return out


def _check_ansatz_field(c, P, dim, what):
    """The supplied gradient of a callable field against central differences of its supplied values at the points P.  Step
    h = eps^(1/3) ~ 6.1e-6: a central difference is off by h^2 |f'''| / 6 (truncation) + eps |f| / h (rounding), both ~ h^2 = 3.7e-11 per
    unit of |f|, |f'''|.  Tolerance 1e4 h^2 max(1, |f|, |grad f|) ~ 3.7e-7: room for third derivatives four orders above the
    field itself (a layer-resolving lift), while a wrong sign, a missing factor or swapped columns are off by the gradient itself."""
    if not callable(c) or P.shape[0] == 0:
        return
    v = _ansatz_field(c, P, dim, what)
    for k in range(dim):
        e = np.zeros(dim)
        e[k] = _FD_STEP
        fd = (_ansatz_field(c, P + e, dim, what)[:, 0] - _ansatz_field(c, P - e, dim, what)[:, 0]) / (2.0 * _FD_STEP)
        scale = np.maximum(1.0, np.maximum(np.abs(v[:, 0]), np.abs(v[:, 1 + k])))
        bad = np.abs(fd - v[:, 1 + k]) > _FD_TOL * scale
        if np.any(bad):
            i = int(np.argmax(bad))
            raise ValueError(f"hard_bc field {what!r}: the supplied derivative along coordinate {k} is {v[i, 1 + k]:.6g} at {P[i]}, "
                             f"central differences of the supplied values give {fd[i]:.6g}")


class VPINNLinear(_VPINNBase):
    """Variable-coefficient linear convection-diffusion-reaction problems in 1-D and 2-D (no reference counterpart; the library's
    linear problems, include/hpvpinn.h: hpv_set_operator):

        div(kappa grad u) + beta . grad u + sigma u = f        kappa = diag(kx, ky), one scalar field for both directions, or a full 2 x 2 tensor

    with the sign convention that makes Poisson kappa = 1.  Everything is a keyword argument and nothing is looked up in the
    caller's module.  `layers[0]` (1 or 2) is the dimension.  The elements are a grid per direction (`grid_x`[, `grid_y`]) or an
    `adapt.ElementMesh` (`mesh`: any list of boxes, with its per-element test-function counts).  `n_quad` is the number of
    Gauss-Lobatto points per direction (one number or a pair) unless `rule` = ((xi, wx)[, (yi, wy)]) hands the 1-D rules over;
    `n_test` the test-function counts of a grid: one number, a pair (x, y), or per-element arrays (one, or a pair in 2-D).
    `kappa`, `beta`, `sigma`, `f`: a constant, or a callable of the points (n, dim); `kappa` and `beta` return (n, dim) -- kappa
    also (n,) when isotropic -- and a constant `beta` may be one vector.  They are evaluated at the handle's own quadrature points;
    F is assembled on the device (hpv_assemble_rhs).  `X_u_train`, `u_train`: Dirichlet data, weighted by `lossb_weight`.

    Coefficient identification (hpv_set_trainable): `trainable` is a list of dicts, one per unknown scalar c_m that is trained with
    the network -- `name`, `init` (its initial value) and any of kappa=, beta=, sigma= (VPINNNonlinear also quadratic=, cubic=,
    exponential=, advection=), each a constant or a callable with the meaning it has above: together they are the DIRECTION the
    scalar multiplies, and the coefficients the problem is solved with are the constructor's plus sum_m c_m * direction_m.  An
    unknown isotropic conductivity is dict(name="kappa", init=1.0, kappa=1.0); two subdomain conductivities are two dicts whose
    kappa= are the indicator functions; an unknown Burgers viscosity is kappa=(-1.0, 0.0).  The scalars follow the network in
    `get_params()` and in checkpoints; `coefficients()` returns {name: value}.  At most 8; the fields not named are zero.

    Local hp-refinement: `strong_form=None` (the default) refuses everything that needs the strong residual -- `element_indicators`,
    `adapt`, `train_adaptive`, `residual` -- because it takes derivatives of kappa.  `strong_form="elementwise"` differentiates the
    interpolant of kappa's nodal values on each element's tensor rule (hpv_set_strong_form; one differentiation matrix per
    direction) and gives `element_indicators(f=None)`, `strong_residual_at_quad()`, `adapt(f=None, **mark_kw)` and `train_adaptive(nIter,
    adapt_every, f=None, max_elements=None, **mark_kw)` -- the base class's, f None meaning the model's own f; `residual(X)` at arbitrary points stays refused.  ASSUMPTION: kappa is smooth
    inside each element.  A jump of kappa must lie on element edges; refinement bisects elements, so edges on dyadic positions of
    the first mesh stay edges.  The rule's nodes must be distinct (no zero-weight padding).
    `strong_form="divergence"` (hpv_set_strong_form_div) gives the same five entry points from the residual in divergence form:
    the fluxes kappa grad u at the element's own points -- which the projection forms anyway -- are interpolated on the tensor rule
    and the interpolant's divergence is taken with the same differentiation matrices.  That needs no second derivative of the
    network, of an element map or of the ansatz functions, so it also works on a `MappedMesh` (the Piola-transformed fluxes of
    `_fold`, the result divided by det A: `_inv_det`), with a full tensor kappa, trainable or not, and under `hard_bc`.  ASSUMPTION:
    the flux is smooth inside each element.

    Exact Dirichlet conditions (hpv_set_ansatz): `hard_bc=dict(g=.., d=..)` trains u = G + D N with N the network: `d` a callable
    of the points (n, dim) returning (n, 1 + dim) = the value and the gradient of a function that vanishes exactly where the
    condition holds, `g` the same for a function that matches the boundary (and initial) data there, or a constant.  The condition
    then holds for every parameter vector and `X_u_train` is not needed (it may still be given).  The supplied gradients are compared
    with central differences of the supplied values at a handful of quadrature points (`_check_ansatz_field`: step eps^(1/3), tolerance
    1e4 eps^(2/3) ~ 3.7e-7 relative); a mismatch raises a ValueError naming the field.  Planes go to the library with every point
    set -- the mesh (`set_mesh`, sharding), the data, `set_flux_data`, `set_validation` -- and `set_hard_bc` changes or removes the
    ansatz of a live model.  `predict`, `rel_l2_error` and `evaluate` apply the map on the host to the raw network channels the
    library returns; under an ansatz `evaluate` returns `u, u_x[, u_y]` only (second derivatives would need those of G and D).
    Not together with `strong_form="elementwise"`, for the same reason; `strong_form="divergence"` goes with it.

    The norm of the residual (hpv_set_residual_norm): `residual_norm="l2"` (the default) is the reference's mean over the test functions
    of R^2; `"dual"`, or `dict(kind="dual", mass=gamma)`, measures each element's residual functional in the dual norm of its discrete
    test space, loss_e = R_e^T G_e^{-1} R_e with G_e the Gram matrix of the element's active test functions in (grad v, grad w) +
    gamma (v, w) -- robust VPINNs.  For kappa = 1, beta = sigma = 0 this is the squared energy norm of the Galerkin projection of
    the error, so sqrt(loss) estimates the H^1 error, `element_indicators` column 0 is the natural refinement indicator, and loss
    values compare across `n_test`, element shapes and the meshes of a `train_adaptive` run.  `set_residual_norm` changes it on a
    live model; checkpoints store the setting.  The data and flux terms keep their mean(square).

    A full diffusion tensor (hpv_set_operator_tensor): in 2-D `kappa` may also be a constant (2, 2) array or a callable returning
    (n, 2, 2) = [[kxx, kxy], [kyx, kyy]] per point, symmetric or not; the same holds for `kappa=` in a `trainable` dict.  Mapped
    elements (hpv_set_element_points): `mesh=adapt.MappedMesh(..)` -- parameter boxes under one global map such as polar
    coordinates, or one bilinear map per quadrilateral (`MappedMesh.from_quads`).  "The points" of every callable are then the
    PHYSICAL quadrature points, and the geometry is folded into the planes in one place (`_fold`: K_eff = adj(A) K, everything
    else times det A, with A the Jacobian of the element's map); the library runs unit elements with a full tensor.  `set_operator`,
    `set_nonlinear`, `set_mesh` (box to mapped and back, state untouched), checkpoints, sharding, `hard_bc`, `set_flux_data`,
    validation and `predict` work as on boxes.  The dual norm there and in the energy metric (hpv_set_residual_gram):
    `residual_norm=dict(kind="dual", metric="reference" | "physical" | "energy", mass=gamma, gram_points=None)` -- "reference" (the
    default, what plain "dual" means) is the H^1 product of the box through the eigen tables; "physical" the H^1 product of the physical
    element, the tables on boxes and dense Gram factors (`quadrature.gram_factors`) on a MappedMesh; "energy" the product
    (sym(kappa) grad v, grad w) of the model's own kappa, always dense, re-handed by `set_operator(kappa=)`.  Refused with a reason:
    "energy" with a trainable kappa or a kappa that is not positive definite at a Gram point, a metric on "l2".  Out of scope, each a
    ValueError that says why: plain `residual_norm="dual"` with a MappedMesh (metric="physical" is the one that works there),
    `strong_form="elementwise"` with a MappedMesh or a tensor kappa, and `adapt` / `train_adaptive` in those cases unless
    `strong_form="divergence"`; `residual(X)` at arbitrary points and `adapt` on several GPUs under either kind; also 1-D graded
    maps, solution-dependent tensors and triangles.

    Integral constraints (hpv_set_moments): `constraints=[dict(name=, kind="mean" | "l2" | "moment", density=None | callable | array,
    power=, target=, weight=)]` adds, per entry, weight * (I - target)^2 with I = int density u^power over the domain (power 1 or 2; at
    most 8 entries) -- "mean" is power 1, "l2" power 2, both with density 1, "moment" takes everything explicitly; a callable density is
    evaluated at the (physical) quadrature points, an array holds its values there.  This is the normalisation int u^2 = 1 and the
    deflation int u v_k = 0 of an eigenvalue problem (lambda a trainable scalar on sigma), the constant of a pure-Neumann problem, a
    prescribed mass.  `set_constraints(list | None)` changes them on a live model, `constraints()` returns {name: (value, penalty)};
    the penalties are part of the variational loss the model reports.  `set_mesh` / `adapt` re-evaluate callables and refuse an array
    density (hand it over again on the new mesh); checkpoints store kinds, powers, targets, weights and the density values, and
    `load_checkpoint` restores "mean" and "l2" entries as they were and every "moment" entry -- a callable density too -- with the ARRAY
    of its values on the checkpoint's mesh, so such an entry must be handed over again before the mesh changes.  One GPU only:
    the moments are integrals over the whole domain and there is no collective before the adjoint.  Out of scope: powers above 2,
    moments of grad u, inequality constraints, multiplier updates."""

    _n_extra = 0
    _val_default = ("X_test", "utest")
    X_test = utest = None
    var_form = 1
    scheme = "VPINNs"

    def __init__(self, layers, *, grid_x=None, grid_y=None, mesh=None, n_quad=10, rule=None, n_test=5, kappa=1.0, beta=0.0,
                 sigma=0.0, f=0.0, X_u_train=None, u_train=None, lossb_weight=1.0, activation="tanh", LR=0.001,
                 init_params=None, seed=1234, backend="auto", device=None, trainable=None, strong_form=None, hard_bc=None,
                 residual_norm="l2", constraints=None):
        dim = int(layers[0])
        self._constraints = self._check_constraints(constraints)
        self._con_rho, self._con_handed = None, False
        self._residual_norm = self._check_residual_norm(residual_norm)
        self._norm_metric = self._check_norm_metric(residual_norm)
        if strong_form not in (None, "elementwise", "divergence"):
            raise ValueError('strong_form is None, "elementwise" or "divergence"')
        if strong_form == "elementwise" and hard_bc is not None:
            raise ValueError('hard_bc and strong_form="elementwise" do not go together: the strong residual of u = G + D N needs '
                             "second derivatives of G and D")
        self._strong_form = strong_form
        self._trainable = self._check_trainable(trainable)
        self._n_extra = len(self._trainable)
        if dim not in (1, 2):
            raise ValueError("layers[0] is the dimension of the problem: 1 or 2")
        self._pde = _lib.PDE_LINEAR1D if dim == 1 else _lib.PDE_LINEAR2D
        self._act = {"tanh": _lib.ACT_TANH, "sin": _lib.ACT_SIN}[activation]
        self._channel_names = ("u", "u_x", "u_xx") if dim == 1 else ("u", "u_x", "u_y", "u_xx", "u_yy")
        self._module_globals = None
        if mesh is None:
            if grid_x is None or (dim == 2 and grid_y is None):
                raise ValueError("give the elements as grid_x[, grid_y] or as mesh=ElementMesh(...)")
            nt = n_test if isinstance(n_test, (tuple, list)) and dim == 2 else (n_test, n_test)
            g = ElementMesh.from_grid(grid_x, grid_y if dim == 2 else None)
            mesh = ElementMesh(g.boxes, nt[0], nt[1] if dim == 2 else None)
        if not isinstance(mesh, ElementMesh) or mesh.dim != dim:
            raise ValueError("mesh must be an adapt.ElementMesh of the problem's dimension")
        if rule is None:
            from .quadrature import GaussLobattoJacobiWeights
            nq = tuple(n_quad) if isinstance(n_quad, (tuple, list)) else (n_quad,) * dim
            rule = tuple(GaussLobattoJacobiWeights(int(q), 0, 0) for q in nq)
        elif dim == 1 and len(rule) == 2 and np.ndim(rule[0]) == 1:
            rule = (rule,)
        if len(rule) != dim:
            raise ValueError("rule holds one (nodes, weights) pair per direction")
        self._rule = tuple((np.asarray(x, dtype=np.float64).reshape(-1), np.asarray(w, dtype=np.float64).reshape(-1)) for x, w in rule)
        self._op = dict(kappa=kappa, beta=beta, sigma=sigma)
        self._f = f
        self._check_scope(mesh)
        self._hard_bc = self._check_hard_bc(hard_bc, mesh)
        self._val_X = None
        self.X_u_train = None if X_u_train is None else np.asarray(X_u_train, dtype=np.float64).reshape(-1, dim)
        self.utrain = None if u_train is None else np.asarray(u_train, dtype=np.float64).reshape(-1)
        self.LR, self.lossb_weight = LR, lossb_weight
        self.loss_his = []
        self._backend_arg = backend
        self._create(layers, 1, LR, lossb_weight, 1.0, init_params, seed, backend, device)
        self._no_constraints_on_several_gpus(self._constraints)
        mesh = mesh.copy()
        self._mesh = mesh

        def populate():
            self._populate_mesh(self._mesh, self._f)
            self._hand_data()
        self._populate = populate
        populate()
        self._finish()

    # -- the populate step: _VPINNBase._populate_mesh with this class's rule and point convention, then the operator ----------
    def _grid_mesh(self):
        return self._mesh

    def _mesh_rule(self, n_shard, ntx, nty):
        (xi, wx), (yi, wy) = self._rule[0], (self._rule[1] if len(self._rule) == 2 else (None, None))
        return xi, wx, yi, wy, ntx

    def _quad_points(self, mesh, eb, ee):
        xi, yi = self._dev_rule
        return mesh.quad_points(xi, yi, eb, ee)

    # -- mapped elements and the full diffusion tensor (hpv_set_element_points, hpv_set_operator_tensor) -----------------------------
    def _hand_elements(self, mesh, eb, ee):
        if not isinstance(mesh, MappedMesh):
            self.h.set_element_boxes(mesh.boxes, eb, ee)
            return
        xi, yi = self._dev_rule
        if self._residual_norm[0] == "dual":                # (set_mesh from boxes: the table norm of the boxes is refused on mapped
            self.h.set_residual_norm(_lib.NORM_L2)          #  elements; _hand_residual_norm hands the dense factors over afterwards)
        X = mesh.quad_points(xi, yi, 0, len(mesh))          # (the library slices [eb, ee) itself, as it slices boxes)
        self.h.set_element_points(X.reshape(len(mesh), -1, 2).transpose(0, 2, 1), eb, ee)

    def _geometry(self, mesh, eb, ee):
        """(P, A): the (physical) quadrature points of the elements [eb, ee) and, for a MappedMesh, the Jacobian of each element's
        map with respect to its reference coordinates at them (None for boxes, whose geometry the library holds)"""
        xi, yi = self._dev_rule
        if isinstance(mesh, MappedMesh):
            return mesh.geometry(xi, yi, eb, ee)
        return mesh.quad_points(xi, yi, eb, ee), None

    def _inv_det(self, mesh, eb, ee):
        """1 / det A at the quadrature points of the elements [eb, ee), element-major: what hpv_set_strong_form_div takes on mapped
        elements to turn the residual of the folded planes into the physical one (None for boxes)"""
        A = self._geometry(mesh, eb, ee)[1]
        return None if A is None else 1.0 / (A[:, 0, 0] * A[:, 1, 1] - A[:, 0, 1] * A[:, 1, 0])

    def _tensor_mode(self, mesh):
        """whether the handle takes a full diffusion tensor: a mapped mesh (the fold fills it), or a kappa -- the operator's or a
        direction's -- that is one"""
        if isinstance(mesh, MappedMesh):
            return True
        if mesh.dim != 2:
            return False
        P = mesh.quad_points(self._rule[0][0], self._rule[1][0], 0, 1)[:1]
        return any(_kappa_field(k, P, 2).ndim == 3 for k in [self._op["kappa"]] + [t["kappa"] for t in self._trainable if "kappa" in t])

    @staticmethod
    def _fold(A, tensor, kappa, scaled):
        """THE fold of a mapped element onto a unit element (include/hpvpinn.h, hpv_set_element_points), the one place it happens:
        with A (n, 2, 2) the Jacobian at the points, d = det A and M = adj A = d A^-1,  K_eff = M K  and every other plane times d.
        kappa: (n, dim), (n, 2, 2) or None; scaled: arrays (n,) or (n, c).  Returns the rows (planes, n): kappa's -- four,
        (kxx, kxy, kyx, kyy), where `tensor`, else its dim diagonal ones -- then one per column of each of `scaled`.
        A None (boxes): nothing is folded, the values are only laid out as rows."""
        rows = []
        if kappa is not None and tensor:
            K = kappa
            if K.ndim == 2:                                 # (a diagonal kappa on a tensor handle)
                K = np.zeros(K.shape + (2,))
                K[:, 0, 0], K[:, 1, 1] = kappa[:, 0], kappa[:, 1]
            if A is not None:
                M = np.stack([np.stack([A[:, 1, 1], -A[:, 0, 1]], 1), np.stack([-A[:, 1, 0], A[:, 0, 0]], 1)], 1)
                K = np.einsum("nab,nbc->nac", M, K)
            rows.append(K.reshape(-1, 4).T)
        elif kappa is not None:
            rows.append(kappa.T)
        d = None if A is None else A[:, 0, 0] * A[:, 1, 1] - A[:, 0, 1] * A[:, 1, 0]
        for v in scaled:
            v = v.reshape(v.shape[0], -1)
            rows.append(v.T if d is None else (v * d[:, None]).T)
        return np.concatenate(rows, axis=0)

    def _check_scope(self, mesh, residual_norm=None):
        """what is out of scope on mapped elements and with a full tensor, each refused with its reason"""
        mapped = isinstance(mesh, MappedMesh)
        rn = residual_norm or self._rn4
        if mapped and rn[0] == "dual" and rn[2] == "reference":
            raise ValueError('residual_norm="dual" on a MappedMesh: the Gram matrix of the reference square is not the physical H^1 '
                             'inner product of a mapped element; dict(kind="dual", metric="physical") is (dense Gram factors)')
        if rn[2] == "energy" and any("kappa" in t for t in self._trainable):
            raise ValueError('metric="energy" with a trainable kappa: the Gram matrix of the energy inner product would move with '
                             "the unknown coefficient")
        if mapped and self._strong_form == "elementwise":
            raise ValueError('strong_form="elementwise" on a MappedMesh: the strong residual on mapped elements is not implemented')
        if self._strong_form == "elementwise" and self._tensor_mode(mesh):
            raise ValueError('strong_form="elementwise" with a full tensor kappa: the strong form of div(K grad u) needs u_xy, '
                             "which is not available")

    def _no_adapt(self, what):
        mesh = self._mesh
        if self._strong_form == "divergence":              # (the divergence form needs neither the maps' second derivatives nor u_xy)
            return
        if isinstance(mesh, MappedMesh) or self._tensor_mode(mesh):
            raise ValueError(f"{what} needs the strong residual, which is not available on a MappedMesh or with a full tensor kappa "
                             "(it would need the maps' second derivatives / u_xy)")

    def _f_at_quad(self, mesh, f, eb, ee):
        P, A = self._geometry(mesh, eb, ee)
        return self._fold(A, False, None, (_coef_field(f, P, mesh.dim, "f", False),))[0]

    def _hand_operator(self, mesh):
        """kappa, beta, sigma at this rank's quadrature points as the planes hpv_set_operator (hpv_set_operator_tensor) takes"""
        eb, ee = shard_range(len(mesh), self.rank, self.world)
        (P, A), d, tensor = self._geometry(mesh, eb, ee), mesh.dim, self._tensor_mode(mesh)
        k, b = _kappa_field(self._op["kappa"], P, d), _coef_field(self._op["beta"], P, d, "beta", True)
        s = _coef_field(self._op["sigma"], P, d, "sigma", False)
        planes = self._fold(A, tensor, k, (b, s))
        if tensor:
            self.h.set_operator_tensor(planes)
        else:
            self.h.set_operator(planes)

    # -- the norm of the residual (hpv_set_residual_norm, hpv_set_residual_gram) --------------------------------------------------
    _METRICS = ("reference", "physical", "energy")

    @staticmethod
    def _check_residual_norm(rn):
        """("l2" | "dual", mass) of "l2" | "dual" | dict(kind=, mass=, metric=, gram_points=); the last two: `_check_norm_metric`"""
        d = dict(kind=rn) if isinstance(rn, str) else dict(rn) if isinstance(rn, dict) else None
        if d is None or set(d) - {"kind", "mass", "metric", "gram_points"} or d.get("kind") not in ("l2", "dual"):
            raise ValueError('residual_norm is "l2", "dual" or dict(kind="dual", metric="reference" | "physical" | "energy", mass=gamma, '
                             "gram_points=None)")
        mass = float(d.get("mass", 0.0))
        if not np.isfinite(mass) or mass < 0.0 or (d["kind"] == "l2" and mass != 0.0):
            raise ValueError("residual_norm: mass is a finite number >= 0 and belongs to kind=\"dual\"")
        VPINNLinear._check_norm_metric(d)
        return d["kind"], mass

    @staticmethod
    def _check_norm_metric(rn):
        """(metric, gram_points) of a residual_norm= that `_check_residual_norm` has seen: ("reference", None) unless a dict says otherwise"""
        d = rn if isinstance(rn, dict) else {}
        if d.get("kind") == "l2" and (d.get("metric") is not None or d.get("gram_points") is not None):
            raise ValueError('residual_norm: metric and gram_points belong to kind="dual" (the l2 norm has no inner product to choose)')
        metric = d.get("metric") or "reference"
        if metric not in VPINNLinear._METRICS:
            raise ValueError(f"residual_norm: metric is one of {VPINNLinear._METRICS}")
        gp = d.get("gram_points")
        if gp is not None and (int(gp) != gp or int(gp) < 1):
            raise ValueError("residual_norm: gram_points is a positive number of Gauss-Legendre points per direction, or None")
        return metric, None if gp is None else int(gp)

    @staticmethod
    def _norm4(rn):
        """(kind, mass, metric, gram_points) of a residual_norm= argument"""
        return VPINNLinear._check_residual_norm(rn) + VPINNLinear._check_norm_metric(rn)

    def _dense_norm(self, mesh, rn=None):
        """whether the dual norm needs dense Gram factors: on mapped elements and in the energy metric -- "physical" on boxes is the
        inner product of "reference" and takes the tables"""
        rn = rn or self._rn4
        return rn[0] == "dual" and (rn[2] == "energy" or isinstance(mesh, MappedMesh))

    def _gram_factors(self, mesh, eb, ee, rn=None):
        """quadrature.gram_factors of the elements [eb, ee): the geometry and, in the energy metric, sym(kappa) at the Gram rule's points"""
        from .quadrature import gram_factors, gram_rule
        _, mass, metric, gp = rn or self._rn4
        dim = mesh.dim
        ntx, nty = int(mesh.nax.max()), int(mesh.nay.max()) if dim == 2 else 1
        x = gram_rule(ntx, nty, gp)[0]
        ne, ng = ee - eb, x.size
        if isinstance(mesh, MappedMesh):
            P, A = mesh.geometry(x, x, eb, ee)
            A = A.reshape(ne, ng * ng, 2, 2)
        else:
            P = mesh.quad_points(x, x if dim == 2 else None, eb, ee)
            b = mesh.boxes[eb:ee]
            if dim == 1:
                A = np.repeat(((b[:, 1] - b[:, 0]) / 2)[:, None], ng, axis=1)
            else:
                A = np.zeros((ne, ng * ng, 2, 2))
                A[:, :, 0, 0], A[:, :, 1, 1] = ((b[:, 1] - b[:, 0]) / 2)[:, None], ((b[:, 3] - b[:, 2]) / 2)[:, None]
        S = None
        if metric == "energy":
            k = _kappa_field(self._op["kappa"], P, dim)
            S = k[:, 0].reshape(ne, ng) if dim == 1 else k.reshape((ne, ng * ng) + k.shape[1:])
        return gram_factors(dim, ntx, nty, mesh.nax[eb:ee], mesh.nay[eb:ee] if dim == 2 else 1, A, S, mass, gp, first=eb)

    def _hand_residual_norm(self, mesh):
        """the eigen tables of the Gram matrices for the counts 1 .. max of the mesh (they go with the test-function tables), or --
        mapped elements, the energy metric -- this rank's dense factors (they go with the elements, the counts and kappa too)"""
        kind, mass = self._residual_norm[:2]
        if kind == "l2":
            self.h.set_residual_norm(_lib.NORM_L2)
            return
        if self._dense_norm(mesh):
            eb, ee = shard_range(len(mesh), self.rank, self.world)
            self.h.set_residual_gram(self._gram_factors(mesh, eb, ee))
            return
        from .quadrature import gram_stacks
        sx = gram_stacks(int(mesh.nax.max()))
        sy = gram_stacks(int(mesh.nay.max())) if mesh.dim == 2 else (None, None)
        self.h.set_residual_norm(_lib.NORM_DUAL, mass, sx[0], sx[1], sy[0], sy[1])

    def set_residual_norm(self, residual_norm):
        """Change the norm of the residual on the live model: "l2", "dual" or dict(kind="dual", metric=, mass=gamma, gram_points=).
        Parameters and optimizer state stay; the loss history goes on in the new norm."""
        rn = self._norm4(residual_norm)
        self._check_scope(self._mesh, rn)
        if self._dense_norm(self._mesh, rn):               # (a kappa that is not positive definite is refused before anything changes)
            eb, ee = shard_range(len(self._mesh), self.rank, self.world)
            self._gram_factors(self._mesh, eb, ee, rn)
        self._residual_norm, self._norm_metric = rn[:2], rn[2:]
        self._hand_residual_norm(self._mesh)

    @property
    def residual_norm(self):
        """"l2", dict(kind="dual", mass=gamma) in the reference metric with the default rule, else dict(kind="dual", mass=gamma,
        metric=, gram_points=)"""
        kind, mass, metric, gp = self._rn4
        if kind == "l2":
            return "l2"
        return dict(kind="dual", mass=mass) if (metric, gp) == ("reference", None) else dict(kind="dual", mass=mass, metric=metric, gram_points=gp)

    @property
    def _rn4(self):
        return tuple(self._residual_norm) + tuple(self._norm_metric)

    def save_checkpoint(self, path):
        """As `_VPINNBase.save_checkpoint`, with the norm of the residual."""
        kind, mass, metric, gp = self._rn4
        np.savez(self._ckpt_path(path), state=self.h.get_state(), layers=np.asarray(self.layers), dev_layers=np.asarray(self._dev_layers),
                 cls=type(self).__name__, residual_norm=kind, residual_norm_mass=mass, residual_norm_metric=metric,
                 residual_norm_gram_points=0 if gp is None else gp, **self._constraints_ckpt())

    def _constraints_ckpt(self):
        """the constraints as arrays: names, powers, targets, weights and the unfolded density values at the quadrature points"""
        c = self._constraints
        if not c:
            return {}
        return dict(con_name=np.asarray([k["name"] for k in c]), con_kind=np.asarray([k.get("kind", "moment") for k in c]), con_power=np.asarray([k["power"] for k in c]),
                    con_target=np.asarray([k["target"] for k in c]), con_weight=np.asarray([k["weight"] for k in c]), con_density=self._con_rho)

    def load_checkpoint(self, path):
        """As `_VPINNBase.load_checkpoint`; a checkpoint that stores the norm of the residual sets it on the model (one written before
        the metrics existed is "reference")."""
        super().load_checkpoint(path)
        d = np.load(self._ckpt_path(path), allow_pickle=False)
        if "residual_norm" in d:
            kind = str(d["residual_norm"])
            metric = str(d["residual_norm_metric"]) if "residual_norm_metric" in d else "reference"
            gp = int(d["residual_norm_gram_points"]) if "residual_norm_gram_points" in d else 0
            rn = (kind, float(d["residual_norm_mass"]), metric, gp or None)
            if rn != self._rn4:
                self.set_residual_norm("l2" if kind == "l2" else dict(kind=kind, mass=rn[1], metric=metric, gram_points=rn[3]))
        if "con_power" in d:                               # (the densities as the arrays they were on the checkpoint's mesh)
            kinds = d["con_kind"] if "con_kind" in d else ["moment"] * len(d["con_power"])
            self.set_constraints([dict(name=str(n), kind=str(k), target=float(t), weight=float(w)) if str(k) != "moment" else
                                  dict(name=str(n), kind="moment", density=np.asarray(r), power=int(p), target=float(t), weight=float(w))
                                  for n, k, r, p, t, w in zip(d["con_name"], kinds, d["con_density"], d["con_power"], d["con_target"], d["con_weight"])])

    # -- exact Dirichlet conditions by ansatz u = G + D N (hpv_set_ansatz) ------------------------------------------------------
    def _check_hard_bc(self, hard_bc, mesh):
        """hard_bc as dict(g=, d=) with the gradients checked at (up to) five quadrature points spread over the mesh; None stays None"""
        if hard_bc is None:
            return None
        hb = dict(hard_bc)
        if set(hb) != {"g", "d"} or not callable(hb["d"]):
            raise ValueError("hard_bc is dict(g=, d=): g a callable or a constant, d a callable, of the points (n, dim) returning (n, 1 + dim)")
        dim = mesh.dim
        P = mesh.quad_points(self._rule[0][0], self._rule[1][0] if dim == 2 else None, 0, len(mesh))
        P = P[np.unique(np.linspace(0, P.shape[0] - 1, 5).astype(int))]
        for k in ("g", "d"):
            _check_ansatz_field(hb[k], P, dim, k)
        return hb

    def _ansatz_planes(self, P):
        """(2 * (1 + dim), n): the rows (G, G_x[, G_y], D, D_x[, D_y]) of hpv_set_ansatz at the points P"""
        dim = self.layers[0]
        P = np.asarray(P, dtype=np.float64).reshape(-1, dim)
        return np.concatenate([_ansatz_field(self._hard_bc[k], P, dim, k).T for k in ("g", "d")], axis=0)

    def _hand_ansatz(self, which, P):
        if self._hard_bc is not None and P is not None:
            self.h.set_ansatz(which, self._ansatz_planes(P))

    def _hand_ansatz_quad(self, mesh):
        eb, ee = shard_range(len(mesh), self.rank, self.world)
        self._hand_ansatz(_lib.ANSATZ_QUAD, self._quad_points(mesh, eb, ee))

    def _hand_flux(self):
        super()._hand_flux()
        if self._flux is not None and self.rank == 0:
            self._hand_ansatz(_lib.ANSATZ_FLUX, self._flux[0])

    def set_validation(self, X=None, u=None, du=None):
        """As `_VPINNBase.set_validation` (points and exact values are required); under an ansatz the errors are those of u = G + D N."""
        super().set_validation(X, u, du)
        self._val_X = np.asarray(X, dtype=np.float64).reshape(-1, self.layers[0]).copy()
        self._hand_ansatz(_lib.ANSATZ_VALID, self._val_X)

    def clear_validation(self):
        super().clear_validation()
        self._val_X = None

    def set_hard_bc(self, g=None, d=None):
        """Change the ansatz u = G + D N of the live model: the fields given replace the stored ones (a model without an ansatz needs
        both), they are checked as in the constructor and handed to the library for every point set it holds.  `set_hard_bc()` removes
        the ansatz: the model trains the raw network again.  Parameters and optimizer state stay."""
        if self._strong_form == "elementwise":
            raise ValueError('hard_bc and strong_form="elementwise" do not go together')
        if g is None and d is None:
            self._hard_bc = None
            for which in (_lib.ANSATZ_QUAD, _lib.ANSATZ_DATA, _lib.ANSATZ_FLUX, _lib.ANSATZ_VALID):
                self.h.set_ansatz(which, None)
            return
        old = self._hard_bc or {}
        hb = dict(g=old.get("g") if g is None else g, d=old.get("d") if d is None else d)
        if hb["g"] is None or hb["d"] is None:
            raise ValueError("a model without an ansatz needs both g and d")
        self._hard_bc = self._check_hard_bc(hb, self._mesh)
        self._hand_ansatz_quad(self._mesh)
        if self.rank == 0:
            self._hand_ansatz(_lib.ANSATZ_DATA, self.X_u_train)
            if self._flux is not None:
                self._hand_ansatz(_lib.ANSATZ_FLUX, self._flux[0])
        self._hand_ansatz(_lib.ANSATZ_VALID, self._val_X)

    def _predict(self, X):
        X = np.asarray(X, dtype=np.float64).reshape(-1, self.layers[0])
        raw = super()._predict(X)
        if self._hard_bc is None:
            return raw
        pl = self._ansatz_planes(X)
        return pl[0][:, None] + pl[1 + self.layers[0]][:, None] * raw

    def evaluate(self, X):
        """As `_VPINNBase.evaluate`.  Under an ansatz: u = G + D N and its first derivatives, keyed `u, u_x[, u_y]` -- the second
        derivatives would need those of G and D and are not returned."""
        if self._hard_bc is None:
            return super().evaluate(X)
        dim = self.layers[0]
        X = np.asarray(X, dtype=np.float64).reshape(-1, dim)
        ch, pl = self.h.eval_points(X), self._ansatz_planes(X)
        G, D = pl[:1 + dim], pl[1 + dim:]
        out = {"u": (G[0] + D[0] * ch[0])[:, None]}
        for c in range(dim):
            out[self._channel_names[1 + c]] = (G[1 + c] + D[1 + c] * ch[0] + D[0] * ch[1 + c])[:, None]
        return out

    _DIR_FIELDS = ("kappa", "beta", "sigma")      # the fields a direction may name, in this class

    def _check_trainable(self, trainable):
        out = []
        for t in (trainable or ()):
            t = dict(t)
            unknown = set(t) - {"name", "init"} - set(self._DIR_FIELDS)
            if unknown or "name" not in t or "init" not in t:
                raise ValueError(f"a trainable coefficient is dict(name=, init=, and any of {self._DIR_FIELDS}); got {sorted(t)}")
            t["init"] = float(t["init"])
            out.append(t)
        if len(out) > _lib.MAX_COEF or len({t["name"] for t in out}) != len(out):
            raise ValueError(f"at most {_lib.MAX_COEF} trainable coefficients, with distinct names")
        return tuple(out)

    def _direction(self, t, P, d, A=None, tensor=False):
        """the planes (K + M, n) of one trainable coefficient's direction at the points P: set_operator's rows (set_operator_tensor's
        where `tensor`), then set_nonlinear's -- folded like them"""
        k, b = _kappa_field(t.get("kappa", 0.0), P, d), _coef_field(t.get("beta", 0.0), P, d, "beta", True)
        s = _coef_field(t.get("sigma", 0.0), P, d, "sigma", False)
        a = [_coef_field(t.get(f, 0.0), P, d, f, False) for f in ("quadratic", "cubic", "exponential")]
        g = _coef_field(t.get("advection", 0.0), P, d, "advection", True)
        return self._fold(A, tensor, k, (b, s, *a, g))

    def _hand_trainable(self, mesh):
        """the directions at this rank's quadrature points (after the planes they add to: new elements orphan all of them)"""
        if not self._trainable:
            return
        eb, ee = shard_range(len(mesh), self.rank, self.world)
        (P, A), tensor = self._geometry(mesh, eb, ee), self._tensor_mode(mesh)
        self.h.set_trainable(np.stack([self._direction(t, P, mesh.dim, A, tensor) for t in self._trainable], 0))

    def coefficients(self):
        """{name: current value} of the trainable coefficients"""
        n = len(self._trainable)
        return dict(zip((t["name"] for t in self._trainable), (float(v) for v in self.get_params()[-n:]))) if n else {}

    def _populate_mesh(self, mesh, f):
        super()._populate_mesh(mesh, f)
        if self._strong_form:                              # (set_quadrature dropped the matrices: they belong to the rule)
            xi, yi = self._dev_rule
            Dx, Dy = diff_matrix(xi), None if yi is None else diff_matrix(yi)
            if self._strong_form == "divergence":          # (... and the new elements 1 / det A)
                eb, ee = shard_range(len(mesh), self.rank, self.world)
                self.h.set_strong_form_div(Dx, Dy, self._inv_det(mesh, eb, ee))
            else:
                self.h.set_strong_form(Dx, Dy)
        self._hand_operator(mesh)
        self._hand_trainable(mesh)
        self._hand_ansatz_quad(mesh)
        self._hand_residual_norm(mesh)                     # (set_tables dropped the tables: they belong to the test functions)
        self._hand_constraints(mesh)                       # (the new elements orphaned the measure planes)

    # -- integral constraints (hpv_set_moments) -----------------------------------------------------------------------------------
    _CON_KINDS = {"mean": 1, "l2": 2}

    @staticmethod
    def _check_constraints(constraints):
        """the list of dict(name=, kind="mean" | "l2" | "moment", density=, power=, target=, weight=) with kind resolved: "mean" is
        power 1, "l2" power 2, both with density 1; "moment" takes everything explicitly.  None and [] are no constraints."""
        out = []
        for c in constraints or ():
            c = dict(c)
            kind = c.get("kind", "moment")
            if kind not in ("mean", "l2", "moment") or set(c) - {"name", "kind", "density", "power", "target", "weight"} or "name" not in c:
                raise ValueError('a constraint is dict(name=, kind="mean" | "l2" | "moment", density=, power=, target=, weight=)')
            if kind != "moment":
                if c.get("density") is not None or c.get("power", VPINNLinear._CON_KINDS[kind]) != VPINNLinear._CON_KINDS[kind]:
                    raise ValueError(f'kind="{kind}" fixes density 1 and power {VPINNLinear._CON_KINDS[kind]}; kind="moment" takes them explicitly')
                c["power"], c["density"] = VPINNLinear._CON_KINDS[kind], None
            elif "power" not in c:
                raise ValueError('kind="moment" needs power=1 or power=2')
            if c["power"] not in (1, 2):
                raise ValueError("constraints: power is 1 or 2 (higher powers and moments of grad u are out of scope)")
            c["target"], c["weight"] = float(c.get("target", 0.0)), float(c.get("weight", 1.0))
            if not (np.isfinite(c["target"]) and np.isfinite(c["weight"]) and c["weight"] >= 0.0):
                raise ValueError("constraints: target is finite, weight is finite and not negative (the penalty is weight * (I - target)^2)")
            d = c.get("density")
            c["density"] = d if d is None or callable(d) else np.asarray(d, dtype=np.float64)
            out.append(c)
        if len(out) > _lib.MAX_MOMENTS:
            raise ValueError(f"at most {_lib.MAX_MOMENTS} constraints")
        if len({c["name"] for c in out}) != len(out):
            raise ValueError("constraints: the names must differ")
        return out

    def _no_constraints_on_several_gpus(self, constraints):
        if constraints and self.world > 1:
            raise ValueError("constraints on several GPUs: the moments are integrals over the whole domain and there is no collective "
                             "before the adjoint")

    def _measure(self, mesh, eb, ee, constraints):
        """THE measure planes of the constraints, the one place they are built: (rho (K, n), m (K, n)) at the quadrature points of the
        elements [eb, ee) -- rho the density's values there (the physical points on a MappedMesh), m = rho x tensor quadrature
        weight x the element's Jacobian (the half widths' product of a box) x det A on a MappedMesh.  A zero-weight padding point
        gets m = 0 exactly."""
        P, A = self._geometry(mesh, eb, ee)
        n, dim = P.shape[0], mesh.dim
        w = self._rule[0][1] if dim == 1 else np.outer(self._rule[1][1], self._rule[0][1]).reshape(-1)
        if A is not None:
            jac = A[:, 0, 0] * A[:, 1, 1] - A[:, 0, 1] * A[:, 1, 0]
        else:
            b = np.asarray(mesh.boxes, dtype=np.float64)[eb:ee]
            jac = np.repeat(np.prod([(b[:, 2 * a + 1] - b[:, 2 * a]) / 2 for a in range(dim)], axis=0), w.size)
        rho = np.ones((len(constraints), n))
        for k, c in enumerate(constraints):
            d = c["density"]
            if callable(d):
                rho[k] = _coef_field(d, P, dim, "density of constraint %r" % c["name"], False)
            elif d is not None:
                if d.size != n:
                    raise ValueError(f"constraint {c['name']!r}: the density array has {d.size} values but the mesh has {n} quadrature "
                                     "points; an array belongs to the mesh it was sampled on -- hand it over again (set_constraints)")
                rho[k] = d.reshape(-1)
        return rho, self._fold_measure(rho, w, jac)

    @staticmethod
    def _fold_measure(rho, w, jac):
        """rho (K, n) density values, w (NQ,) the tensor rule's weights, jac (n,) the Jacobian at the points: m = rho w jac, and
        exactly 0 where the weight is 0 (whatever the density is there)"""
        wj = np.tile(w, jac.size // w.size) * jac
        m = rho * wj[None, :]
        m[:, wj == 0.0] = 0.0
        return m

    def _hand_constraints(self, mesh):
        if not self._constraints:                          # (a model that never had constraints never calls the library for them)
            self._con_rho = None
            if self._con_handed:
                self.h.set_moments(None, None, None, None)
            self._con_handed = False
            return
        eb, ee = shard_range(len(mesh), self.rank, self.world)
        c = self._constraints
        self._con_rho, m = self._measure(mesh, eb, ee, c)
        self._con_handed = True                            # (before the call: a refusal may have removed the old terms already)
        self.h.set_moments([k["power"] for k in c], m, [k["target"] for k in c], [k["weight"] for k in c])

    def set_constraints(self, constraints):
        """Replace the integral constraints on the live model (None or [] removes them); densities are evaluated at the current mesh's
        quadrature points.  Parameters and optimizer state stay."""
        new = self._check_constraints(constraints)
        self._no_constraints_on_several_gpus(new)
        old, self._constraints = self._constraints, new
        try:
            self._hand_constraints(self._mesh)
        except Exception:                                  # (a ValueError of a density, a refusal of the library: the old terms again)
            self._constraints = old
            try:
                self._hand_constraints(self._mesh)
            except Exception:                              # (the handle refuses them too: the model then has none, as the handle has)
                self._constraints, self._con_rho = [], None
            raise

    def constraints(self):
        """{name: (value, penalty)}: I_k = int density u^power and weight (I_k - target)^2 of the most recent pass.  The penalties are
        part of the loss the model reports as its variational part (the last entry of the loss triple, `loss_his`)."""
        if not self._constraints:
            return {}
        I, pen = self.h.read_moments(len(self._constraints))
        return {c["name"]: (float(I[k]), float(pen[k])) for k, c in enumerate(self._constraints)}

    def _hand_data(self):
        if self.rank == 0 and self.X_u_train is not None:
            self.h.set_data(self.X_u_train, self.utrain)
            self._hand_ansatz(_lib.ANSATZ_DATA, self.X_u_train)

    def set_operator(self, kappa=None, beta=None, sigma=None):
        """Re-evaluate the operator on the live model: the coefficients given replace the stored ones (the others stay), all three
        are evaluated at the current mesh's quadrature points and handed to the library.  Parameters and optimizer state stay."""
        old = dict(self._op)
        for k, v in (("kappa", kappa), ("beta", beta), ("sigma", sigma)):
            if v is not None:
                self._op[k] = v
        energy = self._norm_metric[0] == "energy"
        try:
            self._check_scope(self._mesh)
            if energy:                                     # (a kappa that is not positive definite is refused before anything changes)
                eb, ee = shard_range(len(self._mesh), self.rank, self.world)
                W = self._gram_factors(self._mesh, eb, ee)
        except ValueError:
            self._op = old
            raise
        self._hand_operator(self._mesh)
        self._hand_trainable(self._mesh)
        if energy:                                         # (the Gram matrix of the energy inner product is kappa's)
            self.h.set_residual_gram(W)

    def set_mesh(self, mesh, f=None):
        """As `_VPINNBase.set_mesh`; the coefficients are re-evaluated on the new elements.  f None keeps the model's own f."""
        if f is None:
            f = self._f
        if isinstance(mesh, ElementMesh) and mesh.dim == self.layers[0]:
            self._check_scope(mesh)
        for c in self._constraints:
            if isinstance(c["density"], np.ndarray):
                raise ValueError(f"constraint {c['name']!r} has an array density, which belongs to the mesh it was sampled on: remove it "
                                 "(set_constraints) before the mesh changes and hand it over again afterwards")
        self._f = f
        super().set_mesh(mesh, f)

    def _no_strong_form(self, what):
        raise NotImplementedError(f"{what} needs the strong residual of the problem, which takes derivatives of kappa: "
                                  "not available for VPINNLinear.  strong_form=\"elementwise\" gives it at the elements' own "
                                  "quadrature points (indicators and adaptivity; residual(X) stays refused).")

    def _owned_f_quad(self, f):
        mesh = self._mesh
        eb, ee = shard_range(len(mesh), self.rank, self.world)
        return None if ee == eb else self._f_at_quad(mesh, self._f if f is None else f, eb, ee)

    def element_indicators(self, f=None):
        """With strong_form="elementwise" | "divergence": (n_owned, 5) refinement indicators as `_VPINNBase.element_indicators`, column 1 from the
        strong residual at the elements' own quadrature points (hpv_linear_indicators).  f None: the model's own f."""
        if not self._strong_form:
            self._no_strong_form("element_indicators")
        return self.h.linear_indicators(self._owned_f_quad(f))

    def strong_residual_at_quad(self):
        """With strong_form="elementwise" | "divergence": (n_owned, qy, qx), the strong residual at this rank's quadrature points
        (on a MappedMesh the physical one)."""
        if not self._strong_form:
            self._no_strong_form("strong_residual_at_quad")
        xi, yi = self._dev_rule
        r = self.h.linear_indicators(self._owned_f_quad(None), want_r=True)[1]
        return r.reshape(-1, 1 if yi is None else len(yi), len(xi))

    def residual(self, X, f=None):
        self._no_strong_form("residual")

    def adapt(self, f=None, **mark_kw):
        """With strong_form="elementwise" | "divergence": `_VPINNBase.adapt`; f None (the usual call) is the model's own f.  Single GPU only."""
        self._no_adapt("adapt")
        if not self._strong_form:
            self._no_strong_form("adapt")
        return super().adapt(f, **mark_kw)                 # (element_indicators and set_mesh of this class take f None as self._f)

    def train_adaptive(self, nIter, adapt_every, f=None, max_elements=None, **mark_kw):
        """With strong_form="elementwise" | "divergence": `_VPINNBase.train_adaptive`; f None is the model's own f.  Single GPU only."""
        self._no_adapt("train_adaptive")
        if not self._strong_form:
            self._no_strong_form("train_adaptive")
        return super().train_adaptive(nIter, adapt_every, f, max_elements, **mark_kw)

    def _train_n(self, n):
        self.train(n)

    def _record_lbfgs(self, losses):
        self.loss_his.extend(float(l3[0]) for l3 in losses)

    def predict(self, X):
        return self._predict(np.asarray(X, dtype=np.float64).reshape(-1, self.layers[0]))

    def train(self, nIter, verbose=False):
        """nIter Adam iterations; the loss after every update is appended to `loss_his` (device-side history)."""
        it = 0
        while it < nIter:
            n = min(self._RECORD_CHUNK, nIter - it)
            self.loss_his.extend(float(v) for v in self._step_record(n)[0][:, 0])
            it += n
            if verbose and self.rank == 0:
                print('It: %d, Loss: %.3e' % (it, self.loss_his[-1]))
        self.h.sync()


class VPINNNonlinear(VPINNLinear):
    """`VPINNLinear` with a pointwise nonlinear term (include/hpvpinn.h: hpv_set_nonlinear; the projection runs in k_project_nl):

        div(kappa grad u) + beta . grad u + sigma u + N(x; u, grad u) = f
        N = quadratic u^2 + cubic u^3 + exponential exp(u) + u (advection . grad u)

    `quadratic`, `cubic`, `exponential`: a constant or a callable of the points (n, dim) returning (n,); `advection` is vector-valued
    like `beta` (a constant, one (dim,) vector, or a callable returning (n, dim)).  They are evaluated at the rank's own quadrature
    points with the operator and again in `set_mesh`.  A term that is zero everywhere is not evaluated on the device; with all four
    zero the model runs exactly what `VPINNLinear` runs.  Steady Bratu is kappa = 1, exponential = lambda; Allen-Cahn kappa = eps^2,
    sigma = 1, cubic = -1; space-time viscous Burgers (y = t) kappa = (-nu, 0), beta = (0, 1), advection = (1, 0).
    Everything else is `VPINNLinear`'s: the strong form is refused by default, and `strong_form="elementwise"` | `"divergence"` opts into the
    indicators and adaptivity with N in the strong residual (only the terms that are switched on are evaluated).

    Quasilinear diffusion (hpv_set_quasilinear; the _q instantiations of k_project_nl): `diffusivity=dict(poly=(m0, m1, m2), shift=delta,
    power=r)` turns the operator into

        div(mu kappa grad u) + ..        mu = (m0 + m1 u + m2 u^2) (delta + |grad u|^2)^r

    with m0, m1, m2, delta each a constant or a callable of the points returning (n,); the defaults are (1, 0, 0), 1.0 and 0.0, and a
    factor that is identically 1 is not evaluated on the device.  k(u) = 1 + u^2 is poly=(1, 0, 1); the regularised p-Laplacian
    shift=eps^2, power=(p - 2) / 2; the minimal-surface equation shift=1, power=-1/2.  |grad u|^2 is the physical one on a
    MappedMesh too.  `set_nonlinear(diffusivity=...)` changes it on a live model.  `hard_bc` applies before mu (mu sees u = G + D N);
    data and flux terms, validation, `predict`, checkpoints, graphs, sharding and `strong_form="divergence"` (indicators, `adapt`,
    `train_adaptive`) work as without it.  `residual_norm` with metric="energy" keeps using kappa alone for its Gram matrices, never
    mu kappa.  No check is made that the polynomial stays positive at the solution: a mu that changes sign makes the problem
    ill-posed without any error.  Refused with a reason: `trainable=` together with `diffusivity`, `strong_form="elementwise"`
    together with it, and power != 0 with a shift that is not positive at some quadrature point.  Out of scope: exp-type k(u) and
    solution-dependent anisotropy (mu is a scalar on kappa)."""

    _DIR_FIELDS = VPINNLinear._DIR_FIELDS + ("quadratic", "cubic", "exponential", "advection")

    def __init__(self, layers, *, quadratic=0.0, cubic=0.0, exponential=0.0, advection=0.0, diffusivity=None, **kw):
        self._nl = dict(quadratic=quadratic, cubic=cubic, exponential=exponential, advection=advection)
        self._diffusivity = self._check_diffusivity(diffusivity, kw.get("trainable"), kw.get("strong_form"))
        super().__init__(layers, **kw)

    # -- quasilinear diffusion (hpv_set_quasilinear) ----------------------------------------------------------------------------------
    @staticmethod
    def _check_diffusivity(diffusivity, trainable, strong_form):
        """dict(poly=(m0, m1, m2), shift=, power=) with the defaults filled in, or None; what does not go with it is refused here"""
        if diffusivity is None:
            return None
        d = dict(diffusivity)
        if set(d) - {"poly", "shift", "power"}:
            raise ValueError("diffusivity is dict(poly=(m0, m1, m2), shift=delta, power=r): mu = (m0 + m1 u + m2 u^2) (delta + |grad u|^2)^r")
        poly = tuple(d.get("poly", (1.0, 0.0, 0.0)))
        power = float(d.get("power", 0.0))
        if len(poly) != 3 or not np.isfinite(power):
            raise ValueError("diffusivity: poly holds the three coefficients (m0, m1, m2), power is a finite number")
        if trainable:
            raise ValueError("diffusivity and trainable= do not go together: the identification kernel (k_project_id) does not carry "
                             "the multiplier mu(u, |grad u|^2)")
        if strong_form == "elementwise":
            raise ValueError('diffusivity and strong_form="elementwise" do not go together: the elementwise strong residual would need '
                             'the derivative of mu along the element; strong_form="divergence" carries it')
        return dict(poly=poly, shift=d.get("shift", 1.0), power=power)

    def _quasi_planes(self, mesh, eb, ee):
        """(4, n): the rows (m0, m1, m2, delta) of hpv_set_quasilinear at the (physical) quadrature points of the elements [eb, ee) --
        plain rows also on a MappedMesh: mu multiplies K_eff, which already carries the geometry, so nothing is times det A here"""
        d, dim = self._diffusivity, mesh.dim
        P = self._geometry(mesh, eb, ee)[0]
        rows = [_coef_field(c, P, dim, "diffusivity poly[%d]" % i, False) for i, c in enumerate(d["poly"])]
        rows.append(_coef_field(d["shift"], P, dim, "diffusivity shift", False))
        if d["power"] != 0.0 and np.any(rows[3] <= 0.0):
            i = int(np.argmin(rows[3]))
            raise ValueError(f"diffusivity: power = {d['power']} needs shift > 0 at every point, but shift = {rows[3][i]} at {P[i]}")
        return self._fold(None, False, None, rows)

    def _hand_quasilinear(self, mesh):
        """the multiplier at this rank's quadrature points, next to `_hand_nonlinear` (new elements orphan the planes of both)"""
        if self._diffusivity is None:
            return
        eb, ee = shard_range(len(mesh), self.rank, self.world)
        self.h.set_quasilinear(self._quasi_planes(mesh, eb, ee), self._diffusivity["power"])

    def _hand_nonlinear(self, mesh):
        """the four terms at this rank's quadrature points as the planes hpv_set_nonlinear takes"""
        eb, ee = shard_range(len(mesh), self.rank, self.world)
        (P, A), d = self._geometry(mesh, eb, ee), mesh.dim
        a = [_coef_field(self._nl[k], P, d, k, False) for k in ("quadratic", "cubic", "exponential")]
        g = _coef_field(self._nl["advection"], P, d, "advection", True)
        self.h.set_nonlinear(self._fold(A, False, None, (*a, g)))

    def _populate_mesh(self, mesh, f):
        super()._populate_mesh(mesh, f)
        self._hand_nonlinear(mesh)
        self._hand_quasilinear(mesh)

    def set_nonlinear(self, quadratic=None, cubic=None, exponential=None, advection=None, diffusivity=None):
        """Re-evaluate the nonlinear term on the live model: the coefficients given replace the stored ones (the others stay), all
        are evaluated at the current mesh's quadrature points and handed to the library.  `diffusivity=dict(poly=, shift=, power=)`
        replaces the multiplier as a whole (keys left out take their defaults, so `diffusivity={}` removes it).  Parameters and
        optimizer state stay."""
        if diffusivity is not None:
            new = self._check_diffusivity(diffusivity, self._trainable, self._strong_form)
            old, self._diffusivity = self._diffusivity, new
            try:
                eb, ee = shard_range(len(self._mesh), self.rank, self.world)
                self._quasi_planes(self._mesh, eb, ee)
            except ValueError:
                self._diffusivity = old
                raise
        for k, v in (("quadratic", quadratic), ("cubic", cubic), ("exponential", exponential), ("advection", advection)):
            if v is not None:
                self._nl[k] = v
        self._hand_nonlinear(self._mesh)
        self._hand_quasilinear(self._mesh)
        self._hand_trainable(self._mesh)
