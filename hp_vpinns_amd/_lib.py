"""ctypes binding of libhpvpinn.so (include/hpvpinn.h).

The library is the product: if it is missing, cannot be loaded, or reports no HIP device,
every call raises -- there is no CPU fallback (the oracle under `oracle/` is test
infrastructure and is never imported from here).
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("HPV_LIBRARY") or os.path.join(_HERE, "libhpvpinn.so")   # (override: another build of the same library)

HPV_MAX_LAYERS = 16
HIST_CAP = 4096          # HPV_HIST_CAP of csrc/hpv_internal.h: loss-history entries the device keeps
PDE_POISSON1D, PDE_POISSON2D, PDE_ADVDIFF = 0, 1, 2
PDE_LINEAR1D, PDE_LINEAR2D = 3, 4      # variable-coefficient linear problems (hpv_set_operator)
ACT_TANH, ACT_SIN = 0, 1
BACKEND_AUTO, BACKEND_GENERIC, BACKEND_MFMA = 0, 1, 2
SCHEME_VPINN, SCHEME_PINN = 0, 1

# every symbol include/hpvpinn.h declares (tests check the .so exports all of them)
EXPORTS = [
    "hpv_create", "hpv_destroy", "hpv_last_error", "hpv_set_stream", "hpv_set_quadrature",
    "hpv_set_tables", "hpv_set_elements", "hpv_set_rhs", "hpv_set_data", "hpv_num_params",
    "hpv_set_params", "hpv_get_params", "hpv_loss_and_grad", "hpv_step", "hpv_forward_backward",
    "hpv_reduce_buffer", "hpv_apply_adam", "hpv_eval_loss", "hpv_read_loss", "hpv_sync",
    "hpv_predict", "hpv_get_residuals", "hpv_backend_in_use", "hpv_pass_structure", "hpv_set_active_tests", "hpv_enable_timing",
    "hpv_kernel_time_ms", "hpv_time_iteration_kernel", "hpv_bench_projection", "hpv_debug_activation", "hpv_get_state", "hpv_set_state",
    "hpv_assemble_rhs", "hpv_set_collocation", "hpv_gll_rule", "hpv_test_tables",
    "hpv_step_record", "hpv_history_reset", "hpv_history_read",
    "hpv_p2p_export", "hpv_p2p_connect", "hpv_p2p_selftest", "hpv_p2p_disconnect",
    "hpv_eval_channels", "hpv_bench_residual",
    "hpv_set_collocation_shard", "hpv_rccl_unique_id", "hpv_rccl_connect", "hpv_rccl_selftest", "hpv_rccl_disconnect", "hpv_exchange_in_use",
    "hpv_rccl_available", "hpv_graphs_in_use", "hpv_updates_applied", "hpv_set_shared_element_kernels", "hpv_shared_element_kernels",
    "hpv_kernel_variant", "hpv_build_info", "hpv_rccl_abandon", "hpv_bench_residual_checksums", "hpv_rule_advice",
    "hpv_rccl_info", "hpv_rccl_time_allreduce", "hpv_grid_plan", "hpv_set_active_tests_2d",
    "hpv_eval_points", "hpv_residual_points", "hpv_set_validation", "hpv_validate", "hpv_validation_reset", "hpv_validate_enqueue",
    "hpv_validation_read", "hpv_step_validate",
    "hpv_set_element_boxes", "hpv_element_indicators",
    "hpv_set_flux_data", "hpv_read_flux_loss",
    "hpv_set_operator", "hpv_set_nonlinear",
    "hpv_create_ex", "hpv_set_trainable",
    "hpv_set_strong_form", "hpv_linear_indicators", "hpv_set_strong_form_div",
    "hpv_set_ansatz",
    "hpv_set_residual_norm", "hpv_set_residual_gram",
    "hpv_set_operator_tensor", "hpv_set_element_points",
    "hpv_set_quasilinear",
    "hpv_set_moments", "hpv_read_moments",
    "hpv_lbfgs_step", "hpv_lbfgs_reset",
]
NORM_L2, NORM_DUAL, NORM_DUAL_DENSE = 0, 1, 2      # kind of hpv_set_residual_norm; HPV_NORM_DUAL_DENSE is what hpv_set_residual_gram sets
ANSATZ_QUAD, ANSATZ_DATA, ANSATZ_FLUX, ANSATZ_VALID = 0, 1, 2, 3      # HPV_ANSATZ_* of include/hpvpinn.h: the point sets of hpv_set_ansatz
MAX_MOMENTS = 8          # HPV_MAX_MOMENTS of include/hpvpinn.h: integral constraints of a linear handle
MAX_COEF = 8             # HPV_MAX_COEF of include/hpvpinn.h: trainable coefficients of a linear handle
LBFGS_MAX_HISTORY = 64   # HPV_LBFGS_MAX_HISTORY of csrc/hpv_internal.h: pairs the ring of hpv_lbfgs_step holds at most
# HPV_LBFGS_* of include/hpvpinn.h: why hpv_lbfgs_step stopped
LBFGS_REASONS = ("max_iter", "max_eval", "tolerance_grad", "tolerance_change", "tolerance_direction", "max_ls", "non_finite")
IND_N = 5                # HPV_IND_N of include/hpvpinn.h: loss_e, eta2_e, sumR2_e, topx_e, topy_e


def rule_advice(device, pde, var_form, n_hidden, max_width, q, ntx, nty, n_elem_shard):
    """hpv_rule_advice: (q_dev, nt_dev) -- the instantiated rule a shard's rule should be zero-weight padded to (q_dev == q: leave it
    alone) and, in 1-D, the test-function count the device tables should have, for problem `pde` in form `var_form` under a network of
    `n_hidden` hidden layers at most `max_width` wide.  The answer is the dispatch's own plan."""
    qd, nd = C.c_int(0), C.c_int(0)
    rc = load().hpv_rule_advice(int(device), int(pde), int(var_form), int(n_hidden), int(max_width), int(q), int(ntx), int(nty),
                                int(n_elem_shard), C.byref(qd), C.byref(nd))
    if rc:
        raise HpvError(f"hpv_rule_advice({pde}, {var_form}, {n_hidden}, {max_width}, {q}, {ntx}, {nty}, {n_elem_shard}) returned {rc}")
    return qd.value, nd.value


def grid_plan(device, q, n_hidden, n_elem_shard):
    """hpv_grid_plan: 0 separate launches | 1 one workgroup per element | 2 element loop | 3 full rounds + split tail."""
    rc = load().hpv_grid_plan(int(device), int(q), int(n_hidden), int(n_elem_shard))
    if rc < 0:
        raise HpvError(f"hpv_grid_plan({q}, {n_hidden}, {n_elem_shard}) returned {rc}")
    return rc


class HpvConfig(C.Structure):
    _fields_ = [
        ("pde", C.c_int), ("var_form", C.c_int), ("act", C.c_int), ("n_layers", C.c_int),
        ("layers", C.c_int * HPV_MAX_LAYERS),
        ("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double),
        ("lossb_weight", C.c_double), ("V", C.c_double),
        ("device", C.c_int), ("backend", C.c_int), ("scheme", C.c_int),
    ]


class HpvLbfgsOpts(C.Structure):
    _fields_ = [("history", C.c_int), ("max_iter", C.c_int), ("max_eval", C.c_int),
                ("lr", C.c_double), ("tolerance_grad", C.c_double), ("tolerance_change", C.c_double)]


class HpvError(RuntimeError):
    """A libhpvpinn entry point returned non-zero; `code` is that value (include/hpvpinn.h lists them)."""
    code = None

EXCHANGE_TIMEOUT = -7      # an in-kernel exchange between the workgroups of one element timed out (hpv_step and friends)


TEST_HOOKS_LIB_PATH = os.path.join(_HERE, "libhpvpinn_testhooks.so")   # the -DHPV_TEST_HOOKS build (fault-injection knobs; tests only)

_lib = None
_libs = {}                # path -> loaded library (the product library and, in the test suite, the test-hooks build beside it)
_current = [None]         # path new Handles bind to (None: LIB_PATH); see `library`
_dp = C.POINTER(C.c_double)


class library:
    """Context manager: Handles created inside bind to another build of the library (e.g. TEST_HOOKS_LIB_PATH).  Both builds
    are linked -Bsymbolic, so two of them may live in one process; a Handle keeps the library it was created with."""

    def __init__(self, path):
        self.path = path

    def __enter__(self):
        self.prev = _current[0]
        _current[0] = self.path
        return load()

    def __exit__(self, *exc):
        _current[0] = self.prev
        return False


def load():
    """Load libhpvpinn.so (after torch, so that both share one HIP runtime)."""
    global _lib
    path = _current[0] or LIB_PATH
    if path in _libs:
        return _libs[path]
    if not os.path.exists(path):
        raise HpvError(f"{path} is missing: build it with hp_vpinns_amd/csrc/build.sh "
                       "(or __graft_entry__.build()); there is no CPU fallback")
    try:  # torch first: its bundled libamdhip64 (same soname) then serves both
        import torch  # noqa: F401
    except Exception:  # pragma: no cover - torch is optional for the single-GPU path
        pass
    lib = C.CDLL(path, mode=C.RTLD_GLOBAL if path == LIB_PATH else C.RTLD_LOCAL)
    h = C.c_void_p
    lib.hpv_create.argtypes = [C.POINTER(h), C.POINTER(HpvConfig)]
    lib.hpv_create_ex.argtypes = [C.POINTER(h), C.POINTER(HpvConfig), C.c_int]
    lib.hpv_set_trainable.argtypes = [h, _dp, C.c_size_t]
    lib.hpv_destroy.argtypes = [h]
    lib.hpv_destroy.restype = None
    lib.hpv_last_error.argtypes = [h]
    lib.hpv_last_error.restype = C.c_char_p
    lib.hpv_set_stream.argtypes = [h, C.c_void_p]
    lib.hpv_set_quadrature.argtypes = [h, _dp, _dp, C.c_int, _dp, _dp, C.c_int]
    lib.hpv_set_tables.argtypes = [h, _dp, _dp, _dp, C.c_int, _dp, _dp, _dp, C.c_int, _dp]
    lib.hpv_set_elements.argtypes = [h, _dp, C.c_int, _dp, C.c_int, C.c_int, C.c_int]
    lib.hpv_set_rhs.argtypes = [h, _dp, C.c_size_t]
    lib.hpv_set_data.argtypes = [h, _dp, _dp, C.c_int]
    lib.hpv_set_flux_data.argtypes = [h, _dp, _dp, _dp, C.c_int, C.c_double]
    lib.hpv_read_flux_loss.argtypes = [h, _dp]
    lib.hpv_set_operator.argtypes = [h, _dp, C.c_size_t]
    lib.hpv_set_operator_tensor.argtypes = [h, _dp, C.c_size_t]
    lib.hpv_set_nonlinear.argtypes = [h, _dp, C.c_size_t]
    lib.hpv_set_quasilinear.argtypes = [h, _dp, C.c_size_t, C.c_double]
    lib.hpv_set_moments.argtypes = [h, C.c_int, C.POINTER(C.c_int), _dp, C.c_size_t, _dp, _dp]
    lib.hpv_read_moments.argtypes = [h, _dp, _dp, C.c_int]
    lib.hpv_set_collocation.argtypes = [h, _dp, _dp, C.c_int]
    lib.hpv_num_params.argtypes = [h]
    lib.hpv_num_params.restype = C.c_size_t
    lib.hpv_set_params.argtypes = [h, _dp, C.c_size_t]
    lib.hpv_get_params.argtypes = [h, _dp, C.c_size_t]
    lib.hpv_loss_and_grad.argtypes = [h, _dp, _dp]
    lib.hpv_step.argtypes = [h, C.c_int, _dp]
    lib.hpv_forward_backward.argtypes = [h]
    lib.hpv_reduce_buffer.argtypes = [h, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    lib.hpv_apply_adam.argtypes = [h]
    lib.hpv_eval_loss.argtypes = [h]
    lib.hpv_read_loss.argtypes = [h, _dp]
    lib.hpv_sync.argtypes = [h]
    lib.hpv_predict.argtypes = [h, _dp, C.c_int, _dp]
    lib.hpv_get_residuals.argtypes = [h, _dp, C.c_size_t]
    lib.hpv_backend_in_use.argtypes = [h]
    lib.hpv_pass_structure.argtypes = [h]
    lib.hpv_set_active_tests.argtypes = [h, C.POINTER(C.c_int), C.c_int]
    lib.hpv_set_active_tests_2d.argtypes = [h, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int]
    lib.hpv_enable_timing.argtypes = [h, C.c_int]
    lib.hpv_kernel_time_ms.argtypes = [h, C.c_int, _dp, C.POINTER(C.c_long)]
    lib.hpv_time_iteration_kernel.argtypes = [h, C.c_int, _dp]
    lib.hpv_bench_projection.argtypes = [h, C.c_long, C.c_int, _dp, _dp]
    lib.hpv_debug_activation.argtypes = [h, _dp, C.c_int, _dp, _dp, _dp]
    lib.hpv_get_state.argtypes = [h, _dp, C.c_size_t]
    lib.hpv_set_state.argtypes = [h, _dp, C.c_size_t]
    lib.hpv_assemble_rhs.argtypes = [h, _dp, C.c_size_t, _dp, C.c_size_t]
    lib.hpv_gll_rule.argtypes = [h, C.c_int, _dp, _dp]
    lib.hpv_step_record.argtypes = [h, C.c_int, _dp, _dp]
    lib.hpv_history_reset.argtypes = [h]
    lib.hpv_p2p_export.argtypes = [h, C.c_int, C.c_int, C.c_char_p]
    lib.hpv_p2p_connect.argtypes = [h, C.c_char_p]
    lib.hpv_p2p_selftest.argtypes = [h, _dp, C.c_size_t, C.POINTER(C.c_int)]
    lib.hpv_p2p_disconnect.argtypes = [h]
    lib.hpv_history_read.argtypes = [h, C.c_int, _dp, _dp]
    lib.hpv_test_tables.argtypes = [h, C.c_int, _dp, C.c_int, _dp]
    lib.hpv_eval_channels.argtypes = [h, _dp, C.c_size_t]
    lib.hpv_bench_residual.argtypes = [h, C.c_long, C.c_int, C.c_int, _dp, _dp]
    lib.hpv_set_collocation_shard.argtypes = [h, _dp, _dp, C.c_int, C.c_long]
    lib.hpv_rccl_available.argtypes = []
    lib.hpv_graphs_in_use.argtypes = [h]
    lib.hpv_updates_applied.argtypes = [h, C.POINTER(C.c_longlong)]
    lib.hpv_set_shared_element_kernels.argtypes = [h, C.c_int]
    lib.hpv_shared_element_kernels.argtypes = [h]
    lib.hpv_rccl_unique_id.argtypes = [h, C.c_char_p]
    lib.hpv_rccl_connect.argtypes = [h, C.c_int, C.c_int, C.c_char_p]
    lib.hpv_rccl_selftest.argtypes = [h, _dp, C.c_size_t]
    lib.hpv_rccl_disconnect.argtypes = [h]
    lib.hpv_exchange_in_use.argtypes = [h]
    lib.hpv_rccl_abandon.argtypes = [h]
    lib.hpv_rccl_info.argtypes = [h, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.hpv_rccl_time_allreduce.argtypes = [h, C.c_int, _dp]
    lib.hpv_bench_residual_checksums.argtypes = [h, C.c_long, C.c_int, _dp]
    lib.hpv_kernel_variant.argtypes = [h, C.c_char_p, C.c_size_t]
    lib.hpv_build_info.argtypes = []
    lib.hpv_grid_plan.argtypes = [C.c_int, C.c_int, C.c_int, C.c_long]
    lib.hpv_rule_advice.argtypes = [C.c_int] * 8 + [C.c_long, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.hpv_eval_points.argtypes = [h, _dp, C.c_int, _dp, C.c_size_t]
    lib.hpv_residual_points.argtypes = [h, _dp, _dp, C.c_int, _dp]
    lib.hpv_set_validation.argtypes = [h, _dp, _dp, _dp, C.c_int]
    lib.hpv_validate.argtypes = [h, _dp]
    lib.hpv_validation_reset.argtypes = [h]
    lib.hpv_validate_enqueue.argtypes = [h]
    lib.hpv_validation_read.argtypes = [h, C.c_int, _dp]
    lib.hpv_step_validate.argtypes = [h, C.c_int, C.c_int, _dp, C.c_size_t]
    lib.hpv_set_element_boxes.argtypes = [h, _dp, C.c_int, C.c_int, C.c_int]
    lib.hpv_set_element_points.argtypes = [h, _dp, C.c_int, C.c_int, C.c_int]
    lib.hpv_element_indicators.argtypes = [h, _dp, C.c_size_t, _dp, C.c_size_t]
    lib.hpv_set_strong_form.argtypes = [h, _dp, C.c_size_t, _dp, C.c_size_t]
    lib.hpv_linear_indicators.argtypes = [h, _dp, C.c_size_t, _dp, C.c_size_t, _dp, C.c_size_t]
    lib.hpv_set_strong_form_div.argtypes = [h, _dp, C.c_size_t, _dp, C.c_size_t, _dp, C.c_size_t]
    lib.hpv_set_ansatz.argtypes = [h, C.c_int, _dp, C.c_size_t]
    lib.hpv_set_residual_norm.argtypes = [h, C.c_int, C.c_double, _dp, _dp, _dp, _dp]
    lib.hpv_set_residual_gram.argtypes = [h, _dp, C.c_size_t]
    lib.hpv_lbfgs_step.argtypes = [h, C.POINTER(HpvLbfgsOpts), _dp, C.POINTER(C.c_int)]
    lib.hpv_lbfgs_reset.argtypes = [h]
    lib.hpv_build_info.restype = C.c_char_p
    if path == TEST_HOOKS_LIB_PATH:      # the kernel-level hooks of the L-BFGS stage (csrc/hpv_lbfgs.hip)
        _ip = C.POINTER(C.c_int)
        lib.hpv_test_lbfgs_direction.argtypes = [C.c_int] * 4 + [_dp, _dp, _dp, C.c_double, _dp, _dp, _dp]
        lib.hpv_test_lbfgs_push.argtypes = [C.c_int, C.c_int, _ip, _dp, _dp, _dp, _dp, C.c_double, _dp, _dp, _dp, _dp, _dp]
    _libs[path] = lib
    if path == LIB_PATH:
        _lib = lib
    return lib


def build_info(lib=None):
    """{'k_iter_fused': 'ok' | 'no-quarter-tile' | 'absent', 'k_iter_tall': ..., 'test_hooks': '0' | '1'} of a loaded build."""
    raw = (lib or load()).hpv_build_info().decode()
    return dict(kv.split("=", 1) for kv in raw.split(";"))


def _p(a):
    return None if a is None else a.ctypes.data_as(_dp)


def _c(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float64)


def _points(X, dim, what):
    """(n, dim) float64 C-contiguous point array -- the C side reads n*dim doubles, so the row length is checked here."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    if X.ndim != 2 or X.shape[1] != dim:
        raise ValueError(f"{what} must have shape (n, {dim}), got {X.shape}")
    return X


_LEAKED = []       # handles abandoned with a call still inside the library (Handle.leak)


class Handle:
    """Thin RAII wrapper over an `hpv_handle`; every method maps 1:1 onto a C entry point."""

    def __init__(self, pde, var_form, act, layers, lr=1e-3, lossb_weight=1.0, V=1.0, device=0,
                 backend=BACKEND_AUTO, beta1=0.9, beta2=0.999, eps=1e-8, scheme=SCHEME_VPINN, n_coef=0):
        """n_coef: trainable coefficients behind the network parameters (hpv_create_ex; linear problems only)."""
        self.lib = load()
        cfg = HpvConfig()
        cfg.pde, cfg.var_form, cfg.act = int(pde), int(var_form), int(act)
        layers = [int(v) for v in layers]
        if len(layers) > HPV_MAX_LAYERS:
            raise HpvError("too many layers")
        cfg.n_layers = len(layers)
        for i, v in enumerate(layers):
            cfg.layers[i] = v
        cfg.lr, cfg.beta1, cfg.beta2, cfg.eps = lr, beta1, beta2, eps
        cfg.lossb_weight, cfg.V = float(lossb_weight), float(V)
        cfg.device, cfg.backend, cfg.scheme = int(device), int(backend), int(scheme)
        self._h = C.c_void_p()
        rc = self.lib.hpv_create_ex(C.byref(self._h), C.byref(cfg), int(n_coef))
        if rc != 0:
            msg = self.lib.hpv_last_error(None)
            self._h = None
            err = HpvError(f"hpv_create failed ({rc}): {msg.decode() if msg else ''}")
            err.code = int(rc)
            raise err
        self.cfg = cfg
        self.n_coef = int(n_coef)
        self.layers = layers
        self.n_owned = None        # elements this handle owns (set_elements / set_element_boxes)
        self.n_quad = None         # quadrature points per element (set_quadrature)
        self._keep = []

    def _chk(self, rc):
        if rc != 0:
            msg = self.lib.hpv_last_error(self._h)
            err = HpvError(f"libhpvpinn error {rc}: {msg.decode() if msg else ''}")
            err.code = int(rc)
            raise err

    def close(self):
        if getattr(self, "_h", None):
            self.lib.hpv_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- set-up -------------------------------------------------------------------------
    def set_stream(self, stream_ptr):
        self._chk(self.lib.hpv_set_stream(self._h, C.c_void_p(stream_ptr)))

    def set_quadrature(self, xi, wx, yi=None, wy=None):
        xi, wx, yi, wy = _c(xi), _c(wx), _c(yi), _c(wy)
        self._chk(self.lib.hpv_set_quadrature(self._h, _p(xi), _p(wx), xi.size, _p(yi), _p(wy),
                                              1 if yi is None else yi.size))
        self.n_quad = xi.size * (1 if yi is None else yi.size)      # (points per element: what linear_indicators sizes r by)

    def set_tables(self, tx, ty=None, edge_dphi=None):
        """tx / ty: (3, ntest, q) arrays of phi, phi', phi''."""
        tx = _c(tx)
        ty = _c(ty)
        ed = _c(edge_dphi)
        a = [_p(tx[0]), _p(tx[1]), _p(tx[2]), tx.shape[1]]
        b = [None, None, None, 1] if ty is None else [_p(ty[0]), _p(ty[1]), _p(ty[2]), ty.shape[1]]
        self._chk(self.lib.hpv_set_tables(self._h, *a, *b, _p(ed)))

    def set_elements(self, gridx, gridy=None, e_begin=0, e_end=None):
        gx, gy = _c(gridx), _c(gridy)
        nex = gx.size - 1
        ney = 1 if gy is None else gy.size - 1
        if e_end is None:
            e_end = nex * ney
        self._chk(self.lib.hpv_set_elements(self._h, _p(gx), nex, _p(gy), ney, int(e_begin), int(e_end)))
        self.n_owned = int(e_end) - int(e_begin)           # (what element_indicators returns rows for)

    def set_element_boxes(self, boxes, e_begin=0, e_end=None):
        """boxes: (n, 2*dim) rows (x0, x1[, y0, y1]) -- any list of axis-parallel elements (hpv_set_element_boxes); the handle owns
        the rows [e_begin, e_end)."""
        b = np.ascontiguousarray(boxes, dtype=np.float64)
        if b.ndim != 2 or b.shape[1] != 2 * self.layers[0]:
            raise ValueError(f"boxes must have shape (n, {2 * self.layers[0]}), got {b.shape}")
        e_end = b.shape[0] if e_end is None else int(e_end)
        self._chk(self.lib.hpv_set_element_boxes(self._h, _p(b), b.shape[0], int(e_begin), e_end))
        self.n_owned = e_end - int(e_begin)

    def set_element_points(self, X, e_begin=0, e_end=None):
        """X: (n, 2, qy * qx) -- per element the physical x and y of its quadrature points, q = j * qx + i: unit elements at the
        caller's points (hpv_set_element_points; mapped elements whose geometry the caller folds into the planes).  The handle owns
        the rows [e_begin, e_end)."""
        X = np.ascontiguousarray(X, dtype=np.float64)
        if X.ndim != 3 or X.shape[1] != 2 or X.shape[2] != (self.n_quad or X.shape[2]):
            raise ValueError(f"element points must have shape (n, 2, {self.n_quad}), got {X.shape}")
        e_end = X.shape[0] if e_end is None else int(e_end)
        self._chk(self.lib.hpv_set_element_points(self._h, _p(X), X.shape[0], int(e_begin), e_end))
        self.n_owned = e_end - int(e_begin)

    def element_indicators(self, f_quad=None):
        """(n_owned, 5): loss_e, eta2_e, sumR2_e, topx_e, topy_e of the owned elements at the current parameters
        (hpv_element_indicators); f_quad: f at the handle's own quadrature points, element-major, or None (zero).  n_owned is what
        the last set_elements / set_element_boxes gave this handle."""
        f = None if f_quad is None else _c(f_quad).reshape(-1)
        out = np.empty((self.n_owned or 0, IND_N))         # (no elements yet: the library refuses the call)
        self._chk(self.lib.hpv_element_indicators(self._h, _p(f), 0 if f is None else f.size, _p(out), out.size))
        return out

    def set_strong_form(self, Dx=None, Dy=None):
        """Opt a linear handle into its strong form (hpv_set_strong_form): the (qx, qx) differentiation matrix of the device rule's
        x nodes on the reference interval and, in 2-D, the (qy, qy) one of its y nodes.  Both None removes them."""
        Dx, Dy = _c(Dx), _c(Dy)
        self._chk(self.lib.hpv_set_strong_form(self._h, _p(Dx), 0 if Dx is None else Dx.size, _p(Dy), 0 if Dy is None else Dy.size))

    def set_strong_form_div(self, Dx=None, Dy=None, inv_det=None):
        """Opt a linear handle into its strong form in divergence form (hpv_set_strong_form_div): the matrices of `set_strong_form`
        and, on unit (mapped) elements, 1 / det A at the owned quadrature points, element-major.  All None removes it."""
        Dx, Dy, d = _c(Dx), _c(Dy), None if inv_det is None else _c(inv_det).reshape(-1)
        self._chk(self.lib.hpv_set_strong_form_div(self._h, _p(Dx), 0 if Dx is None else Dx.size, _p(Dy), 0 if Dy is None else Dy.size,
                                                   _p(d), 0 if d is None else d.size))

    def linear_indicators(self, f_quad=None, want_r=False):
        """(n_owned, 5) as `element_indicators`, for a linear handle after `set_strong_form` (hpv_linear_indicators).  want_r: also
        the strong residual at every owned quadrature point, (n_owned, qx * qy) element-major -- returns (indicators, r)."""
        f = None if f_quad is None else _c(f_quad).reshape(-1)
        out = np.empty((self.n_owned or 0, IND_N))
        r = None
        if want_r:
            r = np.empty((self.n_owned or 0, self.n_quad or 0))
        self._chk(self.lib.hpv_linear_indicators(self._h, _p(f), 0 if f is None else f.size, _p(out), out.size,
                                                 _p(r), 0 if r is None else r.size))
        return (out, r) if want_r else out

    def set_rhs(self, F):
        F = _c(F)
        self._chk(self.lib.hpv_set_rhs(self._h, _p(F), 0 if F is None else F.size))

    def set_collocation(self, X, f, n_total=None):
        """X, f: this handle's collocation points; n_total: their number over all shards (default: these are all).  f None: zero
        right-hand side (AdvDiff only; the library refuses it for the Poisson problems)."""
        X, f = _points(X, self.layers[0], "collocation points"), (None if f is None else _c(f).reshape(-1))
        if f is not None and f.size != X.shape[0]:
            raise ValueError("one right-hand-side value per collocation point")
        self._chk(self.lib.hpv_set_collocation_shard(self._h, _p(X), _p(f), X.shape[0],
                                                     X.shape[0] if n_total is None else int(n_total)))

    def set_data(self, X, u):
        if X is None:
            self._chk(self.lib.hpv_set_data(self._h, None, None, 0))
            return
        X, u = _points(X, self.layers[0], "data points"), _c(u).reshape(-1)
        if u.size != X.shape[0]:
            raise ValueError("one target value per data point")
        self._chk(self.lib.hpv_set_data(self._h, _p(X), _p(u), X.shape[0]))

    def set_flux_data(self, X, coef, g, weight=1.0):
        """The flux term (hpv_set_flux_data): points (n, dim), coefficients (n, 1 + dim) = (a, b_0 .. b_{dim-1}), targets (n,) and
        the weight w_f.  X None removes the term."""
        if X is None:
            self._chk(self.lib.hpv_set_flux_data(self._h, None, None, None, 0, 0.0))
            return
        d = self.layers[0]
        X, coef, g = _points(X, d, "flux points"), np.ascontiguousarray(coef, dtype=np.float64), _c(g).reshape(-1)
        if coef.shape != (X.shape[0], 1 + d) or g.size != X.shape[0]:
            raise ValueError(f"flux data needs coefficients of shape (n, {1 + d}) and one target per point")
        self._chk(self.lib.hpv_set_flux_data(self._h, _p(X), _p(coef), _p(g), X.shape[0], float(weight)))

    def set_operator(self, coef):
        """The coefficient planes of a linear problem (hpv_set_operator): (K, n_owned * qx * qy), K = 3 rows (k, b, s) in 1-D, 5 rows
        (kx, ky, bx, by, s) in 2-D, each element-major over the owned elements, q = j * qx + i."""
        coef = None if coef is None else _c(coef).reshape(-1)
        self._chk(self.lib.hpv_set_operator(self._h, _p(coef), 0 if coef is None else coef.size))

    def set_operator_tensor(self, coef):
        """The planes of a 2-D linear problem with a full diffusion tensor (hpv_set_operator_tensor): (7, n_owned * qx * qy), rows
        (kxx, kxy, kyx, kyy, bx, by, s) laid out like set_operator's.  The operator call made last decides which kernels run."""
        coef = None if coef is None else _c(coef).reshape(-1)
        self._chk(self.lib.hpv_set_operator_tensor(self._h, _p(coef), 0 if coef is None else coef.size))

    def set_nonlinear(self, coef):
        """The planes of the nonlinear term of a linear problem (hpv_set_nonlinear): (M, n_owned * qx * qy), M = 4 rows (a2, a3, ae, g)
        in 1-D, 5 rows (a2, a3, ae, gx, gy) in 2-D, laid out like set_operator's.  None, or all zeros, removes the term."""
        coef = None if coef is None else _c(coef).reshape(-1)
        self._chk(self.lib.hpv_set_nonlinear(self._h, _p(coef), 0 if coef is None else coef.size))

    def set_quasilinear(self, planes, exponent=0.0):
        """The multiplier mu = (m0 + m1 u + m2 u^2) (delta + |grad u|^2)^exponent on the diffusive flux of a linear problem
        (hpv_set_quasilinear): (4, n_owned * qx * qy), rows (m0, m1, m2, delta) laid out like set_operator's.  None removes the term."""
        planes = None if planes is None else _c(planes).reshape(-1)
        self._chk(self.lib.hpv_set_quasilinear(self._h, _p(planes), 0 if planes is None else planes.size, float(exponent)))

    def set_moments(self, power, measure, target, weight):
        """The integral constraints of a linear problem (hpv_set_moments): per term the power (1 or 2), the measure plane
        (n_owned * qx * qy,) laid out like set_operator's, the target and the weight of w (I - c)^2.  power None removes the terms."""
        if power is None:
            self._chk(self.lib.hpv_set_moments(self._h, 0, None, None, 0, None, None))
            return
        power = np.ascontiguousarray(power, dtype=np.int32).reshape(-1)
        K = power.size
        measure, target, weight = _c(measure).reshape(-1), _c(target).reshape(-1), _c(weight).reshape(-1)
        if target.size != K or weight.size != K:
            raise ValueError("one target and one weight per term")
        self._chk(self.lib.hpv_set_moments(self._h, K, power.ctypes.data_as(C.POINTER(C.c_int)), _p(measure), measure.size, _p(target), _p(weight)))

    def read_moments(self, n_terms):
        """(I_k, pen_k) of the most recent pass (hpv_read_moments), two arrays of n_terms."""
        I, pen = np.zeros(max(int(n_terms), 1)), np.zeros(max(int(n_terms), 1))
        self._chk(self.lib.hpv_read_moments(self._h, _p(I), _p(pen), int(n_terms)))
        return I[:int(n_terms)], pen[:int(n_terms)]

    def set_trainable(self, dirs):
        """The directions of the trainable coefficients (hpv_set_trainable): (n_coef, K + M, n_owned * qx * qy) -- per coefficient the
        planes of set_operator (of set_operator_tensor on a tensor handle) followed by those of set_nonlinear, laid out like them."""
        dirs = None if dirs is None else _c(dirs).reshape(-1)
        self._chk(self.lib.hpv_set_trainable(self._h, _p(dirs), 0 if dirs is None else dirs.size))

    def set_ansatz(self, which, planes, n=None):
        """The ansatz u = G + D N of one point set (hpv_set_ansatz): `which` one of ANSATZ_QUAD / _DATA / _FLUX / _VALID, planes
        (2 * (1 + dim), n) rows (G, G_x[, G_y], D, D_x[, D_y]) at the set's points in the order they were handed over.  None removes the
        planes of that set.  n: the point count handed to the library (default: the planes' own)."""
        if planes is None:
            self._chk(self.lib.hpv_set_ansatz(self._h, int(which), None, 0 if n is None else int(n)))
            return
        planes = np.ascontiguousarray(planes, dtype=np.float64)
        rows = 2 * (1 + self.layers[0])
        if planes.ndim != 2 or planes.shape[0] != rows:
            raise ValueError(f"ansatz planes must have shape ({rows}, n), got {planes.shape}")
        self._chk(self.lib.hpv_set_ansatz(self._h, int(which), _p(planes), planes.shape[1] if n is None else int(n)))

    def set_residual_norm(self, kind, mass=0.0, Sx=None, lamx=None, Sy=None, lamy=None):
        """The norm of the variational residual of a linear problem (hpv_set_residual_norm): NORM_L2, or NORM_DUAL with the weight of
        the L2 part and the stacks of `quadrature.gram_stacks` for ntx (and nty in 2-D): S (nt, nt, nt), lam (nt, nt)."""
        Sx, lamx, Sy, lamy = _c(Sx), _c(lamx), _c(Sy), _c(lamy)
        self._chk(self.lib.hpv_set_residual_norm(self._h, int(kind), float(mass), _p(Sx), _p(lamx), _p(Sy), _p(lamy)))

    def set_residual_gram(self, W):
        """The dual norm through dense factors (hpv_set_residual_gram): W (n_owned, NR, NR) of `quadrature.gram_factors`, NR = ntx * nty,
        the inverse Cholesky factor of each owned element's Gram matrix.  set_residual_norm(NORM_L2) removes it."""
        W = _c(W)
        self._chk(self.lib.hpv_set_residual_gram(self._h, _p(W), 0 if W is None else W.size))

    def read_flux_loss(self):
        """(w_f * msf, msf) of the most recent pass (hpv_read_flux_loss); zeros without the term."""
        out = np.empty(2)
        self._chk(self.lib.hpv_read_flux_loss(self._h, _p(out)))
        return float(out[0]), float(out[1])

    # ---- parameters ---------------------------------------------------------------------
    def num_params(self):
        return int(self.lib.hpv_num_params(self._h))

    def set_params(self, theta):
        theta = _c(theta).reshape(-1)
        self._chk(self.lib.hpv_set_params(self._h, _p(theta), theta.size))

    def get_params(self):
        out = np.empty(self.num_params())
        self._chk(self.lib.hpv_get_params(self._h, _p(out), out.size))
        return out

    # ---- compute ------------------------------------------------------------------------
    def loss_and_grad(self, want_grad=True):
        loss3 = np.empty(3)
        g = np.empty(self.num_params()) if want_grad else None
        self._chk(self.lib.hpv_loss_and_grad(self._h, _p(loss3), _p(g)))
        return loss3, g

    def step(self, n_iters, read_loss=True):
        loss3 = np.empty(3) if read_loss else None
        self._chk(self.lib.hpv_step(self._h, int(n_iters), _p(loss3)))
        return loss3

    def forward_backward(self):
        self._chk(self.lib.hpv_forward_backward(self._h))

    def reduce_buffer(self):
        ptr, n = C.c_void_p(), C.c_size_t()
        self._chk(self.lib.hpv_reduce_buffer(self._h, C.byref(ptr), C.byref(n)))
        return ptr.value, n.value

    def apply_adam(self):
        self._chk(self.lib.hpv_apply_adam(self._h))

    def eval_loss(self):
        self._chk(self.lib.hpv_eval_loss(self._h))

    def read_loss(self):
        loss3 = np.empty(3)
        self._chk(self.lib.hpv_read_loss(self._h, _p(loss3)))
        return loss3

    def sync(self):
        self._chk(self.lib.hpv_sync(self._h))

    def predict(self, X):
        X = _points(X, self.layers[0], "prediction points")
        out = np.empty(X.shape[0])
        self._chk(self.lib.hpv_predict(self._h, _p(X), X.shape[0], _p(out)))
        return out

    def eval_points(self, X):
        """(C, n): the full channel list at arbitrary points -- u, u_x, u_xx in 1-D; u, u_x, u_y (u_t), u_xx, u_yy (u_tt) in 2-D
        (hpv_eval_points; one forward launch)."""
        X = _points(X, self.layers[0], "evaluation points")
        out = np.empty((1 + 2 * self.layers[0], X.shape[0]))
        self._chk(self.lib.hpv_eval_points(self._h, _p(X), X.shape[0], _p(out), out.size))
        return out

    def residual_points(self, X, f=None):
        """(n,): the strong residual at arbitrary points (formulas: hpv_set_collocation); f None = zero right-hand side."""
        X, f = _points(X, self.layers[0], "residual points"), (None if f is None else _c(f).reshape(-1))
        if f is not None and f.size != X.shape[0]:
            raise ValueError("one right-hand-side value per residual point")
        out = np.empty(X.shape[0])
        self._chk(self.lib.hpv_residual_points(self._h, _p(X), _p(f), X.shape[0], _p(out)))
        return out

    def set_validation(self, X, u, du=None):
        """The validation set (uploaded once): points, exact values, optionally exact gradients (n, dim).  X None clears it."""
        if X is None:
            self._chk(self.lib.hpv_set_validation(self._h, None, None, None, 0))
            return
        X, u = _points(X, self.layers[0], "validation points"), _c(u).reshape(-1)
        if u.size != X.shape[0]:
            raise ValueError("one exact value per validation point")
        if du is not None:
            du = _points(du, self.layers[0], "exact gradients")
            if du.shape[0] != X.shape[0]:
                raise ValueError("one exact gradient per validation point")
        self._chk(self.lib.hpv_set_validation(self._h, _p(X), _p(u), _p(du), X.shape[0]))

    def validate(self):
        """{sum (u^-u)^2, sum u^2, max |u^-u|, sum |grad u^ - grad u|^2, sum |grad u|^2, n} on the validation set (hpv_validate)."""
        out = np.empty(6)
        self._chk(self.lib.hpv_validate(self._h, _p(out)))
        return out

    def validation_reset(self):
        self._chk(self.lib.hpv_validation_reset(self._h))

    def validate_enqueue(self):
        """Forward + reduction on the handle's stream, appended to the device-side history; no synchronisation."""
        self._chk(self.lib.hpv_validate_enqueue(self._h))

    def validation_read(self, n):
        out = np.empty((int(n), 6))
        self._chk(self.lib.hpv_validation_read(self._h, int(n), _p(out)))
        return out

    def step_validate(self, n_iters, every):
        """n_iters Adam iterations, a validation enqueued after every `every`-th update, one read at the end:
        (n_iters // every, 6)."""
        every = int(every)
        out = np.empty((max(int(n_iters), 0) // every if every >= 1 else 0, 6))
        self._chk(self.lib.hpv_step_validate(self._h, int(n_iters), every, _p(out), out.size))
        return out

    def channels(self, n_points, n_channels):
        """(C, n_points): the network value and its input-derivative channels at this handle's quadrature points,
        element-major (one forward launch; hpv_eval_channels)."""
        out = np.empty((int(n_channels), int(n_points)))
        self._chk(self.lib.hpv_eval_channels(self._h, _p(out), out.size))
        return out

    def set_active_tests(self, n_active):
        """per-element number of active test functions (1-D p-refinement); None = all."""
        if n_active is None:
            self._chk(self.lib.hpv_set_active_tests(self._h, None, 0))
            return
        a = np.ascontiguousarray(n_active, dtype=np.int32).reshape(-1)
        self._chk(self.lib.hpv_set_active_tests(self._h, a.ctypes.data_as(C.POINTER(C.c_int)), a.size))

    def set_active_tests_2d(self, nax, nay=None):
        """per-element numbers of active test functions per direction (2-D p-refinement, P2:72-73 / P3:112-113): one entry per
        element of the WHOLE grid, flattened e = ex * ney + ey; None = all."""
        if nax is None and nay is None:
            self._chk(self.lib.hpv_set_active_tests_2d(self._h, None, None, 0))
            return
        if nax is None or nay is None:
            raise ValueError("nax and nay are given together (or both None)")
        a = np.ascontiguousarray(nax, dtype=np.int32).reshape(-1)
        b = np.ascontiguousarray(nay, dtype=np.int32).reshape(-1)
        if a.size != b.size:
            raise ValueError("nax and nay must have one entry per element each")
        ip = C.POINTER(C.c_int)
        self._chk(self.lib.hpv_set_active_tests_2d(self._h, a.ctypes.data_as(ip), b.ctypes.data_as(ip), a.size))

    def residuals(self, n):
        out = np.empty(n)
        self._chk(self.lib.hpv_get_residuals(self._h, _p(out), out.size))
        return out

    def backend_in_use(self):
        rc = int(self.lib.hpv_backend_in_use(self._h))
        if rc < 0:
            self._chk(rc)
        return rc

    def enable_timing(self, on=True):
        self._chk(self.lib.hpv_enable_timing(self._h, 1 if on else 0))

    def kernel_time_ms(self, which):
        ms, n = C.c_double(), C.c_long()
        self._chk(self.lib.hpv_kernel_time_ms(self._h, int(which), C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def time_iteration_kernel(self, reps):
        """Average ms of `reps` back-to-back launches of the whole-iteration kernel between ONE hipEvent pair (HpvError -4 when the
        handle's iteration is not one such launch)."""
        ms = C.c_double()
        self._chk(self.lib.hpv_time_iteration_kernel(self._h, int(reps), C.byref(ms)))
        return ms.value

    def get_state(self):
        out = np.empty(3 * self.num_params() + 2)
        self._chk(self.lib.hpv_get_state(self._h, _p(out), out.size))
        return out

    def set_state(self, state):
        state = _c(state).reshape(-1)
        self._chk(self.lib.hpv_set_state(self._h, _p(state), state.size))

    def assemble_rhs(self, f_quad, n_out):
        f_quad = _c(f_quad).reshape(-1)
        out = np.empty(int(n_out))
        self._chk(self.lib.hpv_assemble_rhs(self._h, _p(f_quad), f_quad.size, _p(out), out.size))
        return out

    def step_record(self, n):
        """n Adam iterations; ((n, 3) array {loss, lossb, lossv}, (n,) epsilon) after each update (one extra forward pass
        in total)."""
        out, eps = np.empty((int(n), 3)), np.empty(int(n))
        self._chk(self.lib.hpv_step_record(self._h, int(n), _p(out), _p(eps)))
        return out, eps

    def history_reset(self):
        self._chk(self.lib.hpv_history_reset(self._h))

    def history_read(self, n):
        out, eps = np.empty((int(n), 3)), np.empty(int(n))
        self._chk(self.lib.hpv_history_read(self._h, int(n), _p(out), _p(eps)))
        return out, eps

    def rccl_available(self):
        """librccl can be loaded in this process (local check, no collective)."""
        return int(self.lib.hpv_rccl_available()) == 1

    def rccl_unique_id(self):
        buf = C.create_string_buffer(128)
        self._chk(self.lib.hpv_rccl_unique_id(self._h, buf))
        return buf.raw

    def rccl_connect(self, world, rank, uid):
        self._chk(self.lib.hpv_rccl_connect(self._h, int(world), int(rank), bytes(uid)))

    def rccl_selftest(self, n):
        out = np.empty(int(n))
        self._chk(self.lib.hpv_rccl_selftest(self._h, _p(out), out.size))
        return out

    def kernel_variant(self):
        """Name(s) of the kernel instantiation(s) the most recent reverse-mode pass launched (hpv_kernel_variant)."""
        buf = C.create_string_buffer(320)
        self._chk(self.lib.hpv_kernel_variant(self._h, buf, 320))
        return buf.value.decode()

    def build_info(self):
        return build_info(self.lib)

    def rccl_info(self):
        """(world, rank) as the connected communicator itself reports them (ncclCommCount / ncclCommUserRank); (0, -1): none."""
        w, r = C.c_int(0), C.c_int(-1)
        self._chk(self.lib.hpv_rccl_info(self._h, C.byref(w), C.byref(r)))
        return w.value, r.value

    def rccl_time_allreduce(self, reps=200):
        """Microseconds per eager all-reduce of a packed-buffer-sized scratch buffer (the collective alone).  Collective call."""
        us = C.c_double(0.0)
        self._chk(self.lib.hpv_rccl_time_allreduce(self._h, int(reps), C.byref(us)))
        return us.value

    def rccl_abandon(self):
        """Thread-safe: stop waiting for a blocking rccl_connect / rccl_selftest that runs on a helper thread."""
        self.lib.hpv_rccl_abandon(self._h)

    def leak(self):
        """Never destroy this handle (a helper thread may still be inside the library with it)."""
        _LEAKED.append(self._h)
        self._h = None

    def pass_structure(self):
        """'separate' | 'fused-reverse' | 'whole-iteration' | 'whole-iteration-split' | 'whole-iteration-tile' | 'whole-iteration-tall' |
        'whole-iteration-element' (or None)."""
        return {0: "separate", 1: "fused-reverse", 2: "whole-iteration", 3: "whole-iteration-split",
                4: "whole-iteration-tile", 5: "whole-iteration-tall", 6: "whole-iteration-element"}.get(int(self.lib.hpv_pass_structure(self._h)))

    def graphs_in_use(self):
        """hpv_step replays captured iteration graphs (False: eager launches, e.g. a collective that refused stream capture)."""
        return int(self.lib.hpv_graphs_in_use(self._h)) == 1

    def updates_applied(self):
        """Parameter updates applied through this handle so far (synchronises)."""
        n = C.c_longlong(0)
        self._chk(self.lib.hpv_updates_applied(self._h, C.byref(n)))
        return int(n.value)

    def lbfgs_step(self, max_iter, history=20, lr=1.0, tolerance_grad=1e-7, tolerance_change=1e-9, max_eval=None):
        """hpv_lbfgs_step: ((iters + 1, 3) array {loss, lossb, lossv} at the start and after every accepted iteration,
        {"iters", "func_evals", "pairs_skipped", "reason"})."""
        o = HpvLbfgsOpts(int(history), int(max_iter), 0 if max_eval is None else int(max_eval), float(lr), float(tolerance_grad),
                         float(tolerance_change))
        if max_eval is not None and int(max_eval) < 1:
            raise ValueError("max_eval must be at least 1")
        hist = np.zeros((max(int(max_iter), 0) + 1, 3))
        info = (C.c_int * 4)()
        self._chk(self.lib.hpv_lbfgs_step(self._h, C.byref(o), _p(hist), info))
        return hist[:info[0] + 1], {"iters": int(info[0]), "func_evals": int(info[1]), "pairs_skipped": int(info[2]),
                                    "reason": LBFGS_REASONS[info[3]]}

    def lbfgs_reset(self):
        self._chk(self.lib.hpv_lbfgs_reset(self._h))

    def shared_element_kernels(self):
        """False once the handle stays on launch structures without an in-kernel exchange (set, or after a timeout fallback)."""
        return int(self.lib.hpv_shared_element_kernels(self._h)) == 1

    def set_shared_element_kernels(self, on):
        """False: only launch structures without an in-kernel exchange from now on (what HPV_FUSE=s selects at creation)."""
        self._chk(self.lib.hpv_set_shared_element_kernels(self._h, 1 if on else 0))

    def rccl_disconnect(self):
        self._chk(self.lib.hpv_rccl_disconnect(self._h))

    def exchange_in_use(self):
        return {0: "none", 1: "rccl", 2: "p2p"}[int(self.lib.hpv_exchange_in_use(self._h))]

    def p2p_export(self, world, rank):
        buf = C.create_string_buffer(128)
        self._chk(self.lib.hpv_p2p_export(self._h, int(world), int(rank), buf))
        return buf.raw

    def p2p_connect(self, handles):
        self._chk(self.lib.hpv_p2p_connect(self._h, bytes(handles)))

    def p2p_selftest(self, n):
        out, flag = np.empty(int(n)), C.c_int(0)
        self._chk(self.lib.hpv_p2p_selftest(self._h, _p(out), out.size, C.byref(flag)))
        return out, int(flag.value)

    def p2p_disconnect(self):
        self._chk(self.lib.hpv_p2p_disconnect(self._h))

    def gll_rule(self, q):
        """(nodes, weights) of the q-point Gauss-Lobatto-Legendre rule, computed on the device."""
        xi, w = np.empty(int(q)), np.empty(int(q))
        self._chk(self.lib.hpv_gll_rule(self._h, int(q), _p(xi), _p(w)))
        return xi, w

    def test_tables(self, ntest, xi):
        """(3, ntest, q): phi, phi', phi'' of the Legendre-difference test functions at `xi`, computed on the device."""
        xi = _c(xi).reshape(-1)
        tab = np.empty((3, int(ntest), xi.size))
        self._chk(self.lib.hpv_test_tables(self._h, int(ntest), _p(xi), xi.size, _p(tab)))
        return tab

    def debug_activation(self, x):
        x = _c(x).reshape(-1)
        a, a1, ref = np.empty_like(x), np.empty_like(x), np.empty_like(x)
        self._chk(self.lib.hpv_debug_activation(self._h, _p(x), x.size, _p(a), _p(a1), _p(ref)))
        return a, a1, ref

    def bench_checksums(self, n_elem, do_adjoint=True):
        """Checksums of one stand-alone projection launch on the seeded synthetic batch (hpv_bench_residual_checksums)."""
        out = np.empty(6)
        self._chk(self.lib.hpv_bench_residual_checksums(self._h, int(n_elem), 1 if do_adjoint else 0, _p(out)))
        return out

    def bench_projection(self, n_elem, reps=10, do_adjoint=True):
        ms, by = C.c_double(), C.c_double()
        self._chk(self.lib.hpv_bench_residual(self._h, int(n_elem), int(reps), 1 if do_adjoint else 0, C.byref(ms), C.byref(by)))
        return ms.value, by.value
