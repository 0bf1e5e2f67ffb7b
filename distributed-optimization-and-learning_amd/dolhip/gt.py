"""Gradient tracking (DIGing / NEXT) for BASELINE config 3 on the
parameter-major bank: one round in one HBM pass (dol_gt_csr_pm_f32) and the
device gradient of the separable losses (dol_separable_grad_f32) that starts
the trackers.  ops re-exports both calls as ops.gt_csr_pm /
ops.separable_grad.

  x_i' = sum_j W_ij x_j - lr s_i
  s_i' = sum_j W_ij s_j + grad f_i(x_i') - grad f_i(x_i)       s_i(0) = grad f_i(x_i(0))

Not in the reference: its decentralised round is consensus + local step
(DIST/simulators.py:147-162), which with a constant step size settles at a
biased fixed point; the mix inside this round is its consensus
(DIST/clients.py:61-69) in mix_csr_pm's rounding.  The argument rules are the
validators of ops.py (_check_rows, _check_csr, _check_array) and pm_steps'
square-W check, plus the four stated here: a known objective, at most
ops.GT_MAX_AGENTS agents, four distinct state matrices and a self-weight
vector of n floats; tests/test_gt_host.py pins them without a launch.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _native
from . import ops as _ops
from .pm_steps import _check_square


def _check_objective(name: str, objective: str) -> int:
    if objective not in _ops.OBJECTIVES:
        raise ValueError(f"{name}: objective must be one of {sorted(_ops.OBJECTIVES)}")
    return _ops.OBJECTIVES[objective]


def gt_csr_pm(XT: torch.Tensor, ST: torch.Tensor, XO: torch.Tensor, SO: torch.Tensor, rowptr: torch.Tensor,
              col: torch.Tensor, val: torch.Tensor, TT: torch.Tensor, self_weight: Optional[torch.Tensor] = None,
              objective: str = "least_squares", lr: float = 0.01, P: Optional[int] = None,
              nseg: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """One gradient-tracking round with W = W_off + diag(self_weight): XT the
    parameters, ST the trackers, TT the targets, all [P, >= n] like
    mix_csr_pm's XT (n = rowptr length - 1, W_off the square CSR, normally
    with a zero diagonal); XO / SO receive x' / s'.  Per coordinate
      ax = mix of x, as = mix of s                     (mix_csr_pm's sums)
      ax = fl(ax + fl(d_i x_i)), as = fl(as + fl(d_i s_i))     with self_weight
      x' = fma(-lr, s_i, ax);  s' = fl(fl(as + g(x', t_i)) - g(x_i, t_i))
    with g the gradient separable_grad computes.  The four state matrices
    must be distinct (a Jacobi update of both); at most ops.GT_MAX_AGENTS
    agents.  nseg as mix_csr_pm (None: the order tuned for the XT / XO pair on
    the plain mix, which only writes XO).  Returns (XO, SO)."""
    obj = _check_objective("gt_csr_pm", objective)
    n = rowptr.shape[0] - 1
    if n > _ops.GT_MAX_AGENTS:
        raise ValueError(f"gt_csr_pm: the gradient-tracking round takes at most {_ops.GT_MAX_AGENTS} agents (got {n})")
    state = (("XT", XT), ("ST", ST), ("XO", XO), ("SO", SO))
    for i, (na, a) in enumerate(state):
        for nb, b in state[i + 1:]:
            if a is b or a.data_ptr() == b.data_ptr():
                raise ValueError(f"gt_csr_pm: {na} and {nb} alias: the Jacobi update of x and s needs four buffers")
    if self_weight is not None:
        _ops._check_array("self_weight", self_weight, torch.float32, n, XT.device)
    P = XT.shape[0] if P is None else P
    ldx, ld_s, ldxo, ldso, ldt = (
        _ops._check_rows(nm, t, None, P, f"{nm}: expected [>= {P}, >= {n}] on {{}}", n, XT.device)
        for nm, t in state + (("TT", TT),))
    _ops._check_csr(rowptr, col, val, XT.device, same_length=False)
    _check_square(rowptr, col, n)
    if nseg is None:
        nseg = _ops._pm_auto(_ops._pm_mix(XT, XO, rowptr, col, val, ldx, ldxo, n, n, P), XT, XO, ldx, ldxo, n, n, P)
    _native.call("dol_gt_csr_pm_ex_f32", XT.data_ptr(), ldx, ST.data_ptr(), ld_s, XO.data_ptr(), ldxo, SO.data_ptr(),
                 ldso, n, P, rowptr.data_ptr(), _ops._ptr_unless_empty(col), _ops._ptr_unless_empty(val),
                 _ops._ptr(self_weight), TT.data_ptr(), ldt, obj, float(lr), int(nseg), _ops._stream(XT))
    return XO, SO


def separable_grad(X: torch.Tensor, T: torch.Tensor, out: Optional[torch.Tensor] = None,
                   objective: str = "least_squares") -> torch.Tensor:
    """out = g(X, T) elementwise, the gradient of config 3's separable losses
    with the device code of the DGD and gradient-tracking rounds:
    "least_squares" fl(x - t), "logistic" -t / (1 + exp(t x)).  X, T, out are
    row matrices of one shape (either bank layout; out allocated when None)."""
    obj = _check_objective("separable_grad", objective)
    ldx = _ops._check_rows("X", X)
    rows, cols = X.shape
    ldt = _ops._check_rows("T", T, cols, rows, f"T: expected >= {rows} rows on {{}}", 0, X.device)
    if out is None:
        out = torch.empty((rows, ldx), dtype=torch.float32, device=X.device)[:, :cols]
    ldg = _ops._check_rows("out", out, cols, rows, f"out: expected >= {rows} rows on {{}}", 0, X.device)
    _native.call("dol_separable_grad_f32", X.data_ptr(), ldx, T.data_ptr(), ldt, out.data_ptr(), ldg, rows, cols, obj,
                 _ops._stream(X))
    return out
