"""Host restatements of the gradient-FED rounds (dol_gt_grad_csr_f32 /
dol_extra_grad_csr_f32, ops.gt_grad_csr / ops.extra_grad_csr), shared by
tests/test_grad_rounds_host.py (CPU) and the test_grad_rounds_*gpu.py files.
Built like gt_cases.gt_round, from golden-pinned oracle calls and single numpy
float32 operations:

  ax, as   oracle.mix_csr on X and on S, gt_cases.add_self for the self weights
  s'       fl(fl(as + G) - Gprev)                           numpy float32
  x'       gt_cases.sgd_step(ax, s', lr): fmaf(-lr, s', ax)

and for EXTRA extra_cases.extra_round with a gradient callable that returns its
second argument: the row read in the target's place IS the gradient.

Below: the launch-free call builders of the host tier."""
import numpy as np
import torch

import extra_cases
import oracle
from gt_cases import F32, add_self, sgd_step


def gt_grad_round(X, S, G, Gp, c, d, lr):
    """(X', S') of one fed gradient-tracking round on agent-major [n, P] matrices with W = c + diag(d)."""
    X, S, G, Gp = (np.ascontiguousarray(a, F32) for a in (X, S, G, Gp))
    ax = add_self(oracle.mix_csr(X, c.rowptr, c.col, c.val), d, X)
    as_ = add_self(oracle.mix_csr(S, c.rowptr, c.col, c.val), d, S)
    with np.errstate(invalid="ignore", over="ignore"):
        Sn = ((as_ + G).astype(F32) - Gp).astype(F32)
    return sgd_step(ax, Sn, lr), Sn


def extra_grad_round(X, C, G, c, d, lr):
    """(X', C') of one fed EXTRA round: extra_cases.extra_round with g(x, t) = t."""
    return extra_cases.extra_round(X, C, G, c, d, lr, grad=lambda x, t: np.asarray(t, F32))


def problem4(n, P, seed):
    """Host X, S, G, Gprev [n, P], standard normal."""
    rng = np.random.default_rng(seed)
    return tuple(rng.standard_normal((n, P)).astype(F32) for _ in range(4))


# ---------------------------------------------------------------------------
# the host tier: the two ops called without a launch
# ---------------------------------------------------------------------------
ORDER = {"gt_grad_csr": ("X", "S", "XO", "SO", "rowptr", "col", "val", "G", "Gprev"),
         "extra_grad_csr": ("X", "Y", "rowptr", "col", "val", "G", "corr")}
MATRICES = {"gt_grad_csr": ("X", "S", "XO", "SO", "G", "Gprev"), "extra_grad_csr": ("X", "Y", "G", "corr")}


def host_args(op, dev, n=4, P=10, ld=12):
    """The tensor arguments of ops.<op> by name, zeros on dev: n agents x P,
    rows ld floats apart; W is the perfect matching 0 - 1, 2 - 3, ..."""
    from test_ops_args_gpu import mat, vec
    t = {k: mat(dev, n, P, ld) for k in MATRICES[op]}
    t.update(rowptr=torch.arange(n + 1, dtype=torch.int32, device=dev),
             col=torch.tensor([i ^ 1 for i in range(n)], dtype=torch.int32, device=dev), val=vec(dev, n))
    return t


def host_call(op, t, **kw):
    from dolhip import ops
    return getattr(ops, op)(*(t[k] for k in ORDER[op]), **kw)
