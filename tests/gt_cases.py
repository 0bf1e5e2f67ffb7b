"""Host restatement of one gradient-tracking round (dol_gt_csr_pm_f32), shared
by tests/test_gt_host.py (CPU) and tests/test_gt_pm_gpu.py (GPU), built from
golden-pinned oracle calls and single numpy float32 operations:

  ax, as   oracle.mix_csr on X and on S           (+0 start, ascending e, no FMA)
  self w   ax = fl(ax + fl(d x)), as = fl(as + fl(d s))      numpy float32, one rounding each
  x'       oracle.prox_admm_sgd(w = ax, g = S, no theta, no alpha, momentum 0):
           w = fmaf(-lr, g, w), the reference's SGD.step
  s'       fl(fl(as + g(x', t)) - g(x, t))                    numpy float32

Matrices are agent-major [n, P] as the oracle takes them.  `grad` is the
gradient g(x, t): ls_grad here (fl(x - t), exact in numpy), or a callable that
evaluates the logistic gradient on the device (the host has no expf that
matches the device's bit for bit).  A plain module (no fixtures): tests import
it by name, tests/ being on sys.path.

Below the restatement, what the gradient-tracking test files of the three
layouts (parameter-major, agent-major ring, agent-major CSR, the last with its
push-sum form) share: the device helpers and graphs of the GPU tiers (same_bits
.. logistic_round) and the launch-free call builders of the host tiers
(ENTRIES, recorder, host_args, host_call)."""
import functools
from fractions import Fraction

import numpy as np
import torch

import oracle

F32 = np.float32


def ls_grad(x, t):
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.asarray(x, F32) - np.asarray(t, F32)).astype(F32)


def sgd_step(w, g, lr):
    """fmaf(-lr, g, w) elementwise: the oracle's plain SGD update."""
    return oracle.prox_admm_sgd(w, None, g, None, None, 0.0, lr, 0.0, False, write_grad=False)[0]


def add_self(a, d, v):
    """fl(a + fl(d_i * v_i)) row-wise, or a unchanged without self weights."""
    if d is None:
        return a
    with np.errstate(invalid="ignore", over="ignore"):
        prod = (np.asarray(d, F32)[:, None] * np.asarray(v, F32)).astype(F32)
        return (a + prod).astype(F32)


def gt_round(X, S, T, c, d, lr, grad=ls_grad):
    """(X', S') of one round on agent-major X, S, T [n, P] with W = c + diag(d)."""
    X, S, T = (np.ascontiguousarray(a, F32) for a in (X, S, T))
    ax = add_self(oracle.mix_csr(X, c.rowptr, c.col, c.val), d, X)
    as_ = add_self(oracle.mix_csr(S, c.rowptr, c.col, c.val), d, S)
    Xn = sgd_step(ax, S, lr)
    with np.errstate(invalid="ignore", over="ignore"):
        Sn = ((as_ + grad(Xn, T)).astype(F32) - grad(X, T)).astype(F32)
    return Xn, Sn


def with_diagonal(c, d):
    """The CSR of c + diag(d): the diagonal entry inserted in column order (c
    has a zero diagonal).  What SeparableDGDPM mixes with in the comparison."""
    from dolhip import graph as G
    n = c.n_rows
    rowptr, col, val = [0], [], []
    for i in range(n):
        a, b = int(c.rowptr[i]), int(c.rowptr[i + 1])
        cj = list(map(int, c.col[a:b])) + [i]
        vj = list(map(float, c.val[a:b])) + [float(d[i])]
        order = np.argsort(cj, kind="stable")
        col += [cj[k] for k in order]
        val += [vj[k] for k in order]
        rowptr.append(len(col))
    return G.CSR(n, n, np.asarray(rowptr, np.int32), np.asarray(col, np.int32), np.asarray(val, F32)).validate()


def fma_exact(a, b, c):
    """Correctly rounded float32 of a * b + c for finite float32 a, b, c, by
    exact rational arithmetic: the candidates are the float32 nearest the
    double nearest the exact value and its two neighbours; the closest wins,
    a tie goes to the even significand."""
    exact = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    if exact == 0:
        # a zero result: -0 only when product and addend are both -0 (round to nearest)
        prod_neg = (np.signbit(a) != np.signbit(b))
        if float(a) * float(b) == 0 and float(c) == 0:
            return F32(-0.0) if prod_neg and np.signbit(c) else F32(0.0)
        return F32(0.0)
    near = F32(float(exact))
    cands = {near, np.nextafter(near, F32(np.inf)), np.nextafter(near, F32(-np.inf))}
    best = None
    for v in cands:
        if not np.isfinite(v):
            continue
        err = abs(Fraction(float(v)) - exact)
        even = (int(np.asarray(v, F32).view(np.uint32)) & 1) == 0
        key = (err, 0 if even else 1)
        if best is None or key < best[0]:
            best = (key, v)
    return best[1]


# ---------------------------------------------------------------------------
# shared by the GPU tiers
# ---------------------------------------------------------------------------
def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def problem(n, P, seed):
    """Host X, S, T [n, P], standard normal."""
    rng = np.random.default_rng(seed)
    return tuple(rng.standard_normal((n, P)).astype(F32) for _ in range(3))


def logistic_problem(n, P):
    rng = np.random.default_rng(n + P)
    X, S, T = problem(n, P, n + 31)
    return X, S, np.where(rng.random(T.shape) < 0.5, -T, T).astype(F32)  # targets +-feature


@functools.lru_cache(maxsize=None)
def ring(n):
    """(the reference's stochastic circle W as a CSR, its w_prev, w_next, a self-weight vector)"""
    from dolhip import graph as G
    torch.manual_seed(2028 + n)
    c = G.communication_csr("circle", "stochastic", n)[0]
    wp, wn = c.ring_weights()
    return c, wp, wn, np.linspace(0.05, 0.45, n).astype(F32)


@functools.lru_cache(maxsize=None)
def regular(n):
    """(a random 4-regular W with its own 'stochastic' values, a self-weight vector)"""
    from dolhip import graph as G
    return G.random_regular_csr(n, 4, seed=n + 3), np.linspace(0.05, 0.45, n).astype(F32)


@functools.lru_cache(maxsize=None)
def irregular(n, values=True):
    """A symmetric pattern with rows of degree 0, 1, 2, 3, 4, 5 and >= 9, the
    degree-4 rows in the same 16-row blocks as the others: node 0 isolated; the
    path 1 - 2 - ... - 6 with the chord 3 - 5; node 7 a hub joined to every
    third node of the remainder (about 40 of them at most); the remainder 8 ..
    n - 1 the circulant +-1, +-2 (4-regular).  Random positive values, or ones
    (values=False: the pattern only)."""
    from dolhip import graph as G
    edges = {(i, i + 1) for i in range(1, 6)} | {(3, 5)}
    m = n - 8
    for i in range(m):
        for k in (1, 2):
            a, b = 8 + i, 8 + (i + k) % m
            edges.add((min(a, b), max(a, b)))
    for j in range(8, min(n, 8 + 120), 3):
        edges.add((7, j))
    A = np.zeros((n, n), F32)
    rng = np.random.default_rng(n)
    for a, b in edges:
        A[a, b], A[b, a] = rng.random(2).astype(F32) + F32(0.05) if values else (1.0, 1.0)
    return G.csr_from_dense(A).validate()


def csr_dev(c, gpu):
    return tuple(torch.as_tensor(np.asarray(a, t), device=gpu) for a, t in
                 ((c.rowptr, np.int32), (c.col, np.int32), (c.val, np.float32)))


def padded(A, ld, gpu, fill=float("nan"), off=0):
    """Device copy of host A [n, P] in a [n, ld] matrix, `fill` in the padding
    columns; off: the view starts `off` floats into each row."""
    t = torch.full((A.shape[0], ld), fill, dtype=torch.float32, device=gpu)
    t[:, off:off + A.shape[1]] = torch.as_tensor(A, device=gpu)
    return t


def pm(A, gpu, extra=0):
    """Parameter-major device copy of agent-major host A [n, P]: [P, round_up(n, 4) + extra], NaN padding."""
    n, P = A.shape
    t = torch.full((P, (n + 3) // 4 * 4 + extra), float("nan"), dtype=torch.float32, device=gpu)
    t[:, :n] = torch.as_tensor(np.ascontiguousarray(A.T), device=gpu)
    return t


def am(t, n):
    """Agent-major host copy [n, P] of a parameter-major device matrix."""
    return np.ascontiguousarray(t[:, :n].cpu().numpy().T)


def device_grad(gpu, objective):
    """g(x, t) on agent-major host arrays through ops.separable_grad."""
    from dolhip import ops

    def grad(x, t):
        xd, td = (torch.as_tensor(np.ascontiguousarray(a, F32), device=gpu) for a in (x, t))
        return ops.separable_grad(xd, td, None, objective).cpu().numpy()
    return grad


def logistic_round(mix, X, S, T, d, gpu, lr=0.1):
    """(x', s') of the logistic round as a device composition: mix(A) the
    layout's own device mix of host A [n, P]; the self-weight terms and x' on
    the host (one rounding each, an exact fma); g(x') and g(x) from
    ops.separable_grad; s' from two separate fp32 torch ops."""
    ax, as_ = (add_self(mix(A), d, A) for A in (X, S))
    want_x = sgd_step(ax, S, lr)
    grad = device_grad(gpu, "logistic")
    g1, g0, asd = (torch.as_tensor(a, device=gpu) for a in (grad(want_x, T), grad(X, T), as_))
    return want_x, torch.sub(torch.add(asd, g1), g0).cpu().numpy()


# ---------------------------------------------------------------------------
# shared by the host tiers: the four ops called without a launch
# ---------------------------------------------------------------------------
# per op: the names of its four state matrices, the agent count of host_args,
# its weight-vector arguments (positional ones first), the keywords its accepted call takes
ENTRIES = {
    "gt_csr_pm": dict(state=("XT", "ST", "XO", "SO"), n=2, vectors=("self_weight",), kw=dict(P=10, nseg=8)),
    "gt_ring": dict(state=("X", "S", "XO", "SO"), n=4, vectors=("w_prev", "w_next", "self_weight"),
                    kw=dict(P=10, n_rows=4)),
    "gt_csr": dict(state=("X", "S", "XO", "SO"), n=4, vectors=("self_weight",), kw=dict(P=10)),
    "gt_push_csr": dict(state=("U", "S", "UO", "SO"), n=4, vectors=("v", "v_out", "self_weight"), kw=dict(P=10)),
}


def recorder(monkeypatch):
    """ops._native.call replaced by a test_ops_args_gpu.Recorder, which is returned."""
    from dolhip import ops
    from test_ops_args_gpu import Recorder
    r = Recorder()
    monkeypatch.setattr(ops._native, "call", r)
    return r


def host_args(op, dev, n=None, P=10, ld=12):
    """The tensor arguments of ops.<op> by name, zeros on dev: n agents (the
    op's ENTRIES count when None) x P; agent-major rows are ld floats apart."""
    from test_ops_args_gpu import mat, vec
    n = ENTRIES[op]["n"] if n is None else n
    if op == "gt_csr_pm":
        ldn = (n + 3) // 4 * 4
        t = {k: mat(dev, P, n, ldn) for k in ("XT", "ST", "XO", "SO", "TT")}
    else:
        t = {k: mat(dev, n, P, ld) for k in ENTRIES[op]["state"] + ("target",)}
    if op == "gt_push_csr":
        t.update(v=vec(dev, n), v_out=vec(dev, n))
    if op == "gt_ring":
        t.update(w_prev=vec(dev, n), w_next=vec(dev, n))
    else:
        t.update(rowptr=vec(dev, n + 1, torch.int32), col=vec(dev, 4, torch.int32), val=vec(dev, 4))
    return t


def host_call(op, t, **kw):
    from dolhip import ops
    order = {"gt_csr_pm": ("XT", "ST", "XO", "SO", "rowptr", "col", "val", "TT"),
             "gt_ring": ("X", "S", "XO", "SO", "w_prev", "w_next", "target"),
             "gt_csr": ("X", "S", "XO", "SO", "rowptr", "col", "val", "target"),
             "gt_push_csr": ("U", "S", "UO", "SO", "rowptr", "col", "val", "target", "v", "v_out")}[op]
    return getattr(ops, op)(*(t[k] for k in order), **kw)
