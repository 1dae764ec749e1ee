"""A stand-in for the 24 `tensorflow` (1.x) symbols the three reference scripts use -- a BUILD-MACHINE TOOL of
tests/golden/make_golden.py, our own text, not TensorFlow and not product code.

What it is: a lazy expression graph.  Every `tf.*` call and every Python operator on a `Tensor` only records a node; `Session.run`
evaluates the fetched nodes with torch in float64, leaves (placeholders, constants, variables) as fresh `requires_grad` tensors.
`gradients(y, x)` is a node as well -- d(sum y)/dx by `torch.autograd.grad(..., create_graph=True)` -- so it can be differentiated
again (the classes differentiate twice, Adam a third time), with respect to placeholders and constants as much as variables.

What it stands in for, by documentation (checked by the shim tests of tests/test_oracle.py, never against TensorFlow itself):
  * numpy-style broadcasting of the element-wise operators, `matmul`, full `reduce_sum` / `reduce_mean`, `reshape`, `concat`, `stack`,
    `convert_to_tensor` of nested lists of tensors (a stack per nesting level);
  * `gradients(y, x)` = [d(sum y)/dx], [None] where no path leads from x to y;
  * `train.AdamOptimizer(lr, beta1=0.9, beta2=0.999, epsilon=1e-8).minimize(loss)` over every `Variable` created so far that the
    loss is connected to, with the TF1 rule: lr_t = lr sqrt(1 - beta2^t) / (1 - beta1^t); m <- beta1 m + (1 - beta1) g;
    v <- beta2 v + (1 - beta2) g^2; var <- var - lr_t m / (sqrt(v) + epsilon) -- epsilon OUTSIDE the bias correction; the two beta
    powers are running products updated after the variables; every gradient is taken before any variable moves;
  * `global_variables_initializer()` puts every variable back to its initial value and every optimizer back to t = 0;
  * `truncated_normal` returns zeros: initial parameters are an input of every comparison (`Variable.load`, usable at any time).

It imports nothing of this repository: an independent path from the reference's class text to numbers.
"""
import sys
import types

import numpy as np
import torch

float64 = torch.float64
_F = torch.float64

_VARIABLES = []       # every Variable of the default graph, in creation order
_OPTIMIZERS = []


def reset_default_graph():
    del _VARIABLES[:]
    del _OPTIMIZERS[:]


def set_random_seed(seed):
    return None


class Tensor:
    """A node: `op` names the rule of `_eval`, `args` are the inputs (nodes or plain values), `kw` its constants."""
    __array_priority__ = 1000      # numpy arrays and scalars on the left hand the operator over to the reflected methods below
    __array_ufunc__ = None

    def __init__(self, op, args=(), **kw):
        self.op, self.args, self.kw = op, tuple(args), kw

    # ---- operators ----
    def __add__(self, o): return Tensor("add", (self, o))
    def __radd__(self, o): return Tensor("add", (o, self))
    def __sub__(self, o): return Tensor("sub", (self, o))
    def __rsub__(self, o): return Tensor("sub", (o, self))
    def __mul__(self, o): return Tensor("mul", (self, o))
    def __rmul__(self, o): return Tensor("mul", (o, self))
    def __truediv__(self, o): return Tensor("div", (self, o))
    def __rtruediv__(self, o): return Tensor("div", (o, self))
    def __neg__(self): return Tensor("neg", (self,))
    def __getitem__(self, idx): return Tensor("getitem", (self,), idx=idx)
    __hash__ = object.__hash__

    @property
    def shape(self):
        """static shape, where the node carries one (constants, variables, placeholders)"""
        if "value" in self.kw:
            return tuple(np.shape(self.kw["value"]))
        if "shape" in self.kw:
            return tuple(self.kw["shape"])
        raise AttributeError("no static shape on a '%s' node" % self.op)

    def inputs(self):
        return [a for a in _flat(self.args) if isinstance(a, Tensor)]


def _flat(x):
    if isinstance(x, (list, tuple)):
        for v in x:
            for w in _flat(v):
                yield w
    else:
        yield x


def _value(v, shape=None):
    a = np.array(v, dtype=np.float64)
    if shape is not None:
        a = np.broadcast_to(a, tuple(int(s) for s in shape)).copy() if a.ndim == 0 else a.reshape(tuple(int(s) for s in shape))
    return a


def constant(value, dtype=None, shape=None, name=None):
    return Tensor("const", value=_value(value, shape))


def zeros(shape, dtype=None):
    return Tensor("const", value=np.zeros([int(s) for s in shape]))


def ones(shape, dtype=None):
    return Tensor("const", value=np.ones([int(s) for s in shape]))


def truncated_normal(shape, mean=0.0, stddev=1.0, dtype=None, seed=None):
    return zeros(shape)


def placeholder(dtype, shape=None, name=None):
    return Tensor("placeholder", shape=shape)


class Variable(Tensor):
    def __init__(self, initial_value, dtype=None, trainable=True, name=None):
        if isinstance(initial_value, Tensor):
            initial_value = _run([initial_value], {})[0]
        init = np.array(initial_value, dtype=np.float64)
        Tensor.__init__(self, "variable", value=init.copy())
        self.initial_value = init
        _VARIABLES.append(self)

    @property
    def value(self):
        return self.kw["value"]

    def load(self, value, session=None):
        """set the current value from outside (any time after construction, also after the initializer has run)"""
        v = np.array(value, dtype=np.float64)
        if v.shape != self.kw["value"].shape:
            raise ValueError("shape %s loaded into a variable of shape %s" % (v.shape, self.kw["value"].shape))
        self.kw["value"] = v.copy()


def convert_to_tensor(value, dtype=None):
    if isinstance(value, Tensor):
        return value
    if isinstance(value, (list, tuple)):
        return Tensor("stack", ([convert_to_tensor(v) for v in value],), axis=0)
    return constant(value)


def stack(values, axis=0):
    return Tensor("stack", ([convert_to_tensor(v) for v in values],), axis=axis)


def concat(values, axis):
    return Tensor("concat", ([convert_to_tensor(v) for v in values],), axis=axis)


def reshape(t, shape):
    return Tensor("reshape", (t,), shape=tuple(int(s) for s in shape))


def matmul(a, b): return Tensor("matmul", (a, b))
def add(a, b): return Tensor("add", (a, b))
def tanh(x): return Tensor("tanh", (x,))
def sin(x): return Tensor("sin", (x,))
def square(x): return Tensor("square", (x,))
def reduce_sum(x, axis=None): return Tensor("reduce_sum", (x,), axis=axis)
def reduce_mean(x, axis=None): return Tensor("reduce_mean", (x,), axis=axis)


def _ancestors(node):
    seen, todo = {}, [node]
    while todo:
        n = todo.pop()
        if id(n) in seen:
            continue
        seen[id(n)] = n
        todo.extend(n.inputs())
    return seen


def gradients(ys, xs):
    """[d(sum ys)/dx for x in xs]; None where x is not connected to ys"""
    xs = list(xs) if isinstance(xs, (list, tuple)) else [xs]
    if isinstance(ys, (list, tuple)):
        total = ys[0]
        for y in ys[1:]:
            total = total + y
        ys = total
    anc = _ancestors(ys)
    return [Tensor("grad", (ys, x)) if id(x) in anc else None for x in xs]


# ---- evaluation ---------------------------------------------------------------------------------------------------------------------
def _as_torch(v):
    return v if isinstance(v, torch.Tensor) else torch.as_tensor(np.asarray(v, dtype=np.float64))


def _eval(node, memo, feed):
    """torch value of `node`; iterative post-order (the element sums make long chains), memoised per run so that every use of a leaf
    sees the same torch tensor"""
    stack_ = [node]
    while stack_:
        n = stack_[-1]
        if id(n) in memo:
            stack_.pop()
            continue
        missing = [a for a in n.inputs() if id(a) not in memo]
        if missing:
            stack_.extend(missing)
            continue
        memo[id(n)] = _apply(n, memo, feed)
        stack_.pop()
    return memo[id(node)]


def _apply(n, memo, feed):
    def val(a):
        return memo[id(a)] if isinstance(a, Tensor) else _as_torch(a)
    op, a = n.op, n.args
    if op in ("const", "variable"):
        return torch.tensor(n.kw["value"], dtype=_F, requires_grad=True)
    if op == "placeholder":
        if n not in feed:
            raise ValueError("a placeholder the fetch depends on is not fed")
        return torch.tensor(np.asarray(feed[n], dtype=np.float64), dtype=_F, requires_grad=True)
    if op == "add": return val(a[0]) + val(a[1])
    if op == "sub": return val(a[0]) - val(a[1])
    if op == "mul": return val(a[0]) * val(a[1])
    if op == "div": return val(a[0]) / val(a[1])
    if op == "neg": return -val(a[0])
    if op == "getitem": return val(a[0])[n.kw["idx"]]
    if op == "matmul": return torch.matmul(val(a[0]), val(a[1]))
    if op == "tanh": return torch.tanh(val(a[0]))
    if op == "sin": return torch.sin(val(a[0]))
    if op == "square": return torch.square(val(a[0]))
    if op in ("reduce_sum", "reduce_mean"):
        f = torch.sum if op == "reduce_sum" else torch.mean
        return f(val(a[0])) if n.kw["axis"] is None else f(val(a[0]), dim=n.kw["axis"])
    if op == "reshape": return val(a[0]).reshape(n.kw["shape"])
    if op == "stack": return torch.stack([val(v) for v in a[0]], dim=n.kw["axis"])
    if op == "concat": return torch.cat([val(v) for v in a[0]], dim=n.kw["axis"])
    if op == "grad":
        y, x = val(a[0]), val(a[1])
        if not y.requires_grad:
            return torch.zeros_like(x)
        g, = torch.autograd.grad(y.sum(), x, create_graph=True, allow_unused=True)
        return torch.zeros_like(x) if g is None else g
    raise NotImplementedError(op)


def _run(nodes, feed):
    memo = {}
    with torch.enable_grad():
        return [_eval(n, memo, feed).detach().numpy().copy() for n in nodes]


class _Op:
    def __init__(self, fn):
        self.run = fn


def global_variables_initializer():
    variables, optimizers = list(_VARIABLES), list(_OPTIMIZERS)

    def init(feed):
        for v in variables:
            v.kw["value"] = v.initial_value.copy()
        for o in optimizers:
            o._reset()
    return _Op(init)


class ConfigProto:
    def __init__(self, **kw):
        self.kw = kw


class Session:
    def __init__(self, config=None):
        self.config = config

    def run(self, fetches, feed_dict=None):
        feed = dict(feed_dict or {})
        if isinstance(fetches, (list, tuple)):
            return [self.run(f, feed) for f in fetches]
        if isinstance(fetches, _Op):
            return fetches.run(feed)
        out = _run([fetches], feed)[0]
        return out[()] if out.ndim == 0 else out


class AdamOptimizer:
    def __init__(self, learning_rate=0.001, beta1=0.9, beta2=0.999, epsilon=1e-8):
        self.lr, self.beta1, self.beta2, self.epsilon = learning_rate, beta1, beta2, epsilon
        self.vars, self.grads = [], []
        _OPTIMIZERS.append(self)
        self._reset()

    def _reset(self):
        self.beta1_power, self.beta2_power = self.beta1, self.beta2
        self.m = [np.zeros_like(v.value) for v in self.vars]
        self.v = [np.zeros_like(v.value) for v in self.vars]

    def minimize(self, loss, var_list=None):
        candidates = list(_VARIABLES) if var_list is None else list(var_list)
        pairs = [(g, v) for g, v in zip(gradients(loss, candidates), candidates) if g is not None]
        if not pairs:
            raise ValueError("No gradients provided for any variable")
        self.grads, self.vars = [g for g, _ in pairs], [v for _, v in pairs]
        self._reset()

        def step(feed):
            gs = _run(self.grads, feed)                   # all of them before any variable moves
            lr_t = self.lr * np.sqrt(1.0 - self.beta2_power) / (1.0 - self.beta1_power)
            for i, (g, var) in enumerate(zip(gs, self.vars)):
                self.m[i] = self.beta1 * self.m[i] + (1.0 - self.beta1) * g
                self.v[i] = self.beta2 * self.v[i] + (1.0 - self.beta2) * g * g
                var.kw["value"] = var.value - lr_t * self.m[i] / (np.sqrt(self.v[i]) + self.epsilon)
            self.beta1_power *= self.beta1
            self.beta2_power *= self.beta2
        return _Op(step)


train = types.SimpleNamespace(AdamOptimizer=AdamOptimizer)


def install(name="tensorflow"):
    """make `import tensorflow as tf` resolve to this module"""
    sys.modules[name] = sys.modules[__name__]
    return sys.modules[__name__]
