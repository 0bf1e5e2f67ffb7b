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
it by name, tests/ being on sys.path."""
from fractions import Fraction

import numpy as np

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
