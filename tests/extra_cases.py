"""Host restatement of one EXTRA round (dol_extra_csr_f32 / dol_extra_ring_f32,
ops.extra_csr / ops.extra_ring / ops.extra_ring_edges), shared by
tests/test_extra_host.py (CPU) and the test_extra_*_gpu.py files.  Built like
gt_cases.gt_round, from golden-pinned oracle calls and single numpy float32
operations:

  ax       oracle.mix_csr on X                      (+0 start, ascending e, no FMA)
  self w   gt_cases.add_self: ax = fl(ax + fl(d x))
  r        fl(x - ax)                               numpy float32
  x'       fl(gt_cases.sgd_step(ax, g(x, t), lr) - c): fmaf(-lr, g, ax), then one numpy float32 subtraction
  c'       gt_cases.sgd_step(c, r, -0.5): fmaf(0.5, r, c)

W = c + diag(d) is symmetric and doubly stochastic.  Matrices are agent-major
[n, P].  `grad` as in gt_cases.gt_round.  extra_round64 states the same round
in float64 on the dense W (the paper-equivalence test iterates it);
paper_recursion is the two-step recursion of Shi, Ling, Wu, Yin (2015).

Below: the graphs the tiers share (Metropolis weights on gt_cases' ring and
random 4-regular patterns), the DGD restatement the convergence tests compare
against, CPU entries with the ops' signatures for the sharded steps, and the
launch-free call builders of the host tier."""
import functools

import numpy as np
import torch

import gt_cases
import oracle
from gt_cases import F32, add_self, ls_grad, sgd_step


def finish(ax, X, C, T, lr, grad=ls_grad):
    """(X', C') from the mixed rows ax (self term included)."""
    with np.errstate(invalid="ignore", over="ignore"):
        r = (X - ax).astype(F32)
        Xn = (sgd_step(ax, grad(X, T), lr) - C).astype(F32)
    return Xn, sgd_step(C, r, -0.5)


def extra_round(X, C, T, c, d, lr, grad=ls_grad):
    """(X', C') of one round on agent-major X, C, T [n, P] with W = c + diag(d)."""
    X, C, T = (np.ascontiguousarray(a, F32) for a in (X, C, T))
    ax = add_self(oracle.mix_csr(X, c.rowptr, c.col, c.val), d, X)
    return finish(ax, X, C, T, lr, grad)


def dense64(c, d):
    """W = c + diag(d) as a float64 matrix."""
    W = c.dense().astype(np.float64)
    return W if d is None else W + np.diag(np.asarray(d, np.float64))


def extra_round64(X, C, T, W, lr):
    """extra_round's statements in float64 on the dense W, least squares."""
    ax = W @ X
    r = X - ax
    return (ax - lr * (X - T)) - C, C + 0.5 * r


def paper_recursion(X0, T, W, lr, rounds):
    """[x(0), ..., x(rounds)] of x(k+2) = (I + W) x(k+1) - W~ x(k) - lr [g(x(k+1)) - g(x(k))],
    x(1) = W x(0) - lr g(x(0)), W~ = (I + W) / 2, least squares, float64."""
    n = W.shape[0]
    eye = np.eye(n)
    Wt = (eye + W) / 2
    xs = [X0, W @ X0 - lr * (X0 - T)]
    for _ in range(rounds - 1):
        x1, x0 = xs[-1], xs[-2]
        xs.append((eye + W) @ x1 - Wt @ x0 - lr * ((x1 - T) - (x0 - T)))
    return xs


def dgd_round(X, T, c, d, lr):
    """The reference's round on the same W: consensus, then one plain SGD step (oracle.dgd_local)."""
    y = add_self(oracle.mix_csr(np.ascontiguousarray(X, F32), c.rowptr, c.col, c.val), d, X)
    return oracle.dgd_local(y, T, np.zeros_like(y), "least_squares", 1, lr, 0.0, False)[0]


@functools.lru_cache(maxsize=None)
def metropolis_ring(n):
    """(W_off, d, w_prev, w_next) of the Metropolis weights on the n-agent ring."""
    from dolhip import graph as G
    w_off, d = G.metropolis_weights(gt_cases.ring(n)[0])
    wp, wn = w_off.ring_weights()
    return w_off, d, wp, wn


@functools.lru_cache(maxsize=None)
def metropolis_regular(n):
    """(W_off, d) of the Metropolis weights on gt_cases.regular(n)'s random 4-regular pattern."""
    from dolhip import graph as G
    return G.metropolis_weights(gt_cases.regular(n)[0])


def replay(c, d, lr, rounds, P=8, seed=2028):
    """(X, C, T, X of dgd_round) after `rounds` float32 rounds from a zero start,
    targets standard normal from `seed`."""
    n = c.n_rows
    T = np.random.default_rng(seed).standard_normal((n, P)).astype(F32)
    X, C, Xd = np.zeros((n, P), F32), np.zeros((n, P), F32), np.zeros((n, P), F32)
    for _ in range(rounds):
        X, C = extra_round(X, C, T, c, d, lr)
        Xd = dgd_round(Xd, T, c, d, lr)
    return X, C, T, Xd


# ---------------------------------------------------------------------------
# CPU entries with the ops' signatures (the sharded steps under gloo)
# ---------------------------------------------------------------------------
def _np(t, rows, P):
    return np.ascontiguousarray(t[:rows, :P].numpy())


def _put(Y, corr, rows, P, xn, cn):
    Y[rows, :P] = torch.from_numpy(xn)
    corr[rows, :P] = torch.from_numpy(cn)


def cpu_extra_ring(X, Y, w_prev, w_next, target, corr, self_weight=None, objective="least_squares", lr=0.01,
                   halo_prev=None, halo_next=None, P=None, n_rows=None):
    """ops.extra_ring on CPU tensors: oracle.mix_ring (the ring mix's rounding), then finish()."""
    assert objective == "least_squares"
    n = n_rows
    x = _np(X, n, P)
    hp, hn = (None if h is None else h[:P].numpy() for h in (halo_prev, halo_next))
    d = None if self_weight is None else self_weight[:n].numpy()
    ax = add_self(oracle.mix_ring(x, w_prev[:n].numpy(), w_next[:n].numpy(), hp, hn), d, x)
    _put(Y, corr, slice(0, n), P, *finish(ax, x, _np(corr, n, P), _np(target, n, P), lr))
    return Y


def cpu_extra_ring_edges(X, Y, w_prev, w_next, target, corr, halo_prev, halo_next, self_weight=None,
                         objective="least_squares", lr=0.01, P=None, n_rows=None):
    """ops.extra_ring_edges on CPU tensors: rows 0 and n_rows - 1 only."""
    n = n_rows
    d = (lambda a, b: None) if self_weight is None else (lambda a, b: self_weight[a:b])
    for r in ([0] if n == 1 else [0, n - 1]):
        hp = halo_prev if r == 0 else X[r - 1]
        hn = halo_next if r == n - 1 else X[r + 1]
        cpu_extra_ring(X[r:r + 1], Y[r:r + 1], w_prev[r:r + 1], w_next[r:r + 1], target[r:r + 1], corr[r:r + 1],
                       self_weight=d(r, r + 1), objective=objective, lr=lr, halo_prev=hp, halo_next=hn, P=P, n_rows=1)
    return Y


def cpu_apply_extra(c):
    """extra_round with MixingPlan.apply_extra's signature."""
    def apply_extra(X, Y, target, corr, self_weight=None, objective="least_squares", lr=0.01, P=None):
        assert objective == "least_squares"
        n = c.n_rows
        d = None if self_weight is None else self_weight.numpy()
        _put(Y, corr, slice(0, n), P, *extra_round(_np(X, n, P), _np(corr, n, P), _np(target, n, P), c, d, lr))
        return Y
    return apply_extra


# ---------------------------------------------------------------------------
# the host tier: the three ops called without a launch
# ---------------------------------------------------------------------------
ORDER = {"extra_csr": ("X", "Y", "rowptr", "col", "val", "target", "corr"),
         "extra_ring": ("X", "Y", "w_prev", "w_next", "target", "corr"),
         "extra_ring_edges": ("X", "Y", "w_prev", "w_next", "target", "corr", "halo_prev", "halo_next")}


def host_args(op, dev, n=4, P=10, ld=12):
    """The tensor arguments of ops.<op> by name, zeros on dev: n agents x P,
    rows ld floats apart; extra_csr's W is the perfect matching 0 - 1, 2 - 3, ..."""
    from test_ops_args_gpu import mat, vec
    t = {k: mat(dev, n, P, ld) for k in ("X", "Y", "target", "corr")}
    if op == "extra_csr":
        t.update(rowptr=torch.arange(n + 1, dtype=torch.int32, device=dev),
                 col=torch.tensor([i ^ 1 for i in range(n)], dtype=torch.int32, device=dev), val=vec(dev, n))
    else:
        t.update(w_prev=vec(dev, n), w_next=vec(dev, n))
    if op == "extra_ring_edges":
        t.update(halo_prev=vec(dev, ld), halo_next=vec(dev, ld))
    return t


def host_call(op, t, **kw):
    from dolhip import ops
    return getattr(ops, op)(*(t[k] for k in ORDER[op]), **kw)
