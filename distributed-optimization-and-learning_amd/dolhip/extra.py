"""EXTRA (Shi, Ling, Wu, Yin, SIAM J. Optim. 25(2), 2015) for BASELINE config
3: one round in one HBM pass on the agent-major bank with any sparse W
(dol_extra_csr_f32), on the agent-major ring (dol_extra_ring_f32, wrap-around
or the blocks of a sharded ring through its halo form) and on a ring block's
two boundary rows (dol_extra_ring_edges_f32), and on the parameter-major bank
with any sparse W up to ops.PM_DGD_MAX_AGENTS agents (dol_extra_csr_pm_f32).
ops re-exports the calls as ops.extra_csr / ops.extra_ring /
ops.extra_ring_edges / ops.extra_csr_pm.  extra_grad_csr
(dol_extra_grad_csr_f32, ops.extra_grad_csr) is extra_csr's round with the
gradient fed as a row matrix, for agents whose gradients are not a separable
loss of a target row (the per-agent MLPs of config 5); its rules are pinned by
tests/test_grad_rounds_host.py.

With W~ = (I + W) / 2 the paper's recursion
  x(k+2) = (I + W) x(k+1) - W~ x(k) - lr [grad f(x(k+1)) - grad f(x(k))],   x(1) = W x(0) - lr grad f(x(0))
is the pair
  x_i' = sum_j W_ij x_j - lr grad f_i(x_i) - c_i
  c_i' = c_i + (x_i - sum_j W_ij x_j) / 2                          c_i(0) = 0
which mixes ONLY x: the correction c_i is the agent's own row, never gathered,
updated in place.  A round therefore moves the five streams of the DGD round
with momentum (x gathered, c and the targets in, x' and c' out), where a
gradient-tracking round (gt.py) mixes two matrices; and a sharded ring
exchanges the halo rows of x alone, the exchange dgd_step already does.

Not in the reference: its decentralised round is consensus + local step
(DIST/simulators.py:147-162), which with a constant step size settles at a
biased fixed point; the mix inside this round is its consensus
(DIST/clients.py:61-69) in mix_csr's / mix_ring's rounding.  W is the one the
gradient-tracking rounds take: symmetric, doubly stochastic, positive diagonal
(graph.metropolis_weights, synthetic.ring_gt_weights), passed as its
off-diagonal part plus `self_weight`.

The argument rules are the validators of ops.py and gt.py (_ring_args,
_csr_args, _pm_args, _check_halos, _leading_dims, _check_objective, pm_steps'
square-W check) plus one stated here: corr is none of X, Y, target.
tests/test_extra_host.py and tests/test_extra_pm_host.py pin them without a
launch.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _native
from . import ops as _ops
from .gt import _check_objective, _leading_dims
from .pm_steps import _check_square


def _extra_rules(name: str, X, Y, target, corr, objective) -> int:
    """The rules that need no layout, first: a known objective (its code is
    returned), target and corr given, corr none of X, Y, target."""
    obj = _check_objective(name, objective)
    for nm, t in (("target", target), ("corr", corr)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name}: {nm}: expected a torch.Tensor")
    for nm, t in (("X", X), ("Y", Y), ("target", target)):
        if corr is t or (isinstance(t, torch.Tensor) and corr.data_ptr() == t.data_ptr()):
            raise ValueError(f"{name}: corr and {nm} alias: the correction is updated in place")
    return obj


def _extra_rows(X, target, corr, self_weight, P: int, n: int):
    """(ldt, ldc) of a round on n agents of P parameters whose X / Y pair the
    caller has checked; the self weights are n floats."""
    _, ldc, ldt = _leading_dims((("X", X), ("corr", corr)), ("target", target), P, n)
    if self_weight is not None:
        _ops._check_array("self_weight", self_weight, torch.float32, n, X.device)
    return ldt, ldc


def extra_csr(X: torch.Tensor, Y: torch.Tensor, rowptr: torch.Tensor, col: torch.Tensor, val: torch.Tensor,
              target: torch.Tensor, corr: torch.Tensor, self_weight: Optional[torch.Tensor] = None,
              objective: str = "least_squares", lr: float = 0.01, P: Optional[int] = None) -> torch.Tensor:
    """One EXTRA round on the agent-major bank (dol_extra_csr_f32) with W =
    W_off + diag(self_weight), W_off the square CSR (normally with a zero
    diagonal): X the parameters, target the targets, corr the corrections
    (zero before the first round), [>= n, >= P] like mix_csr's X (n = rowptr
    length - 1); Y receives x', corr is updated in place.  Per coordinate, all
    fp32, one rounding each
      ax = mix of x                                    (mix_csr's sum)
      ax = fl(ax + fl(d_i x_i))                        with self_weight
      r  = fl(x_i - ax)
      x' = fl(fma(-lr, g(x_i, t_i), ax) - c_i);  c' = fma(0.5, r, c_i)
    with g the gradient separable_grad computes.  The rules of this op: a
    known objective; Y is not X (a Jacobi mix); corr is none of X, Y, target;
    a self-weight vector of n floats; a square W.  Returns Y."""
    obj = _extra_rules("extra_csr", X, Y, target, corr, objective)
    P, n, ldx, ldy = _ops._csr_args(X, Y, rowptr, col, val, P, same_length=False)
    ldt, ldc = _extra_rows(X, target, corr, self_weight, P, n)
    _check_square(rowptr, col, n)
    _native.call("dol_extra_csr_f32", X.data_ptr(), ldx, Y.data_ptr(), ldy, n, P, rowptr.data_ptr(),
                 _ops._ptr_unless_empty(col), _ops._ptr_unless_empty(val), _ops._ptr(self_weight), target.data_ptr(),
                 ldt, corr.data_ptr(), ldc, obj, float(lr), _ops._stream(X))
    return Y


def extra_grad_csr(X: torch.Tensor, Y: torch.Tensor, rowptr: torch.Tensor, col: torch.Tensor, val: torch.Tensor,
                   G: torch.Tensor, corr: torch.Tensor, self_weight: Optional[torch.Tensor] = None, lr: float = 0.01,
                   P: Optional[int] = None) -> torch.Tensor:
    """extra_csr's round with the gradient FED as the row matrix G
    (dol_extra_grad_csr_f32), read where extra_csr reads the target: for agents
    whose gradients something else computes (BatchedMLP.forward_backward writes
    them into the bank's grad rows).  Per coordinate
      ax, the self term and r as extra_csr
      x' = fl(fma(-lr, g_i, ax) - c_i);  c' = fma(0.5, r, c_i)
    the bits of extra_csr when G holds g(x_i, t_i).  corr is zero before the
    first round and updated in place.  The rules of this op are extra_csr's
    without an objective, with G in target's place (Y is not X; corr is none of
    X, Y, G; a self-weight vector of n floats; a square W), and: G is not Y.
    Returns Y."""
    for nm, t in (("G", G), ("corr", corr)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"extra_grad_csr: {nm}: expected a torch.Tensor")
    for nm, t in (("X", X), ("Y", Y), ("G", G)):
        if corr is t or (isinstance(t, torch.Tensor) and corr.data_ptr() == t.data_ptr()):
            raise ValueError(f"extra_grad_csr: corr and {nm} alias: the correction is updated in place")
    if G is Y or (isinstance(Y, torch.Tensor) and G.data_ptr() == Y.data_ptr()):
        raise ValueError("extra_grad_csr: G and Y alias: the gradient rows are read while Y is written")
    P, n, ldx, ldy = _ops._csr_args(X, Y, rowptr, col, val, P, same_length=False)
    _, ldc, ldg = _leading_dims((("X", X), ("corr", corr)), ("G", G), P, n)
    if self_weight is not None:
        _ops._check_array("self_weight", self_weight, torch.float32, n, X.device)
    _check_square(rowptr, col, n)
    _native.call("dol_extra_grad_csr_f32", X.data_ptr(), ldx, Y.data_ptr(), ldy, n, P, rowptr.data_ptr(),
                 _ops._ptr_unless_empty(col), _ops._ptr_unless_empty(val), _ops._ptr(self_weight), G.data_ptr(), ldg,
                 corr.data_ptr(), ldc, float(lr), _ops._stream(X))
    return Y


def extra_csr_pm(XT: torch.Tensor, YT: torch.Tensor, rowptr: torch.Tensor, col: torch.Tensor, val: torch.Tensor,
                 TT: torch.Tensor, corr: torch.Tensor, self_weight: Optional[torch.Tensor] = None,
                 objective: str = "least_squares", lr: float = 0.01, P: Optional[int] = None,
                 nseg: Optional[int] = None) -> torch.Tensor:
    """extra_csr's round on the parameter-major bank (dol_extra_csr_pm_f32):
    XT the parameters, TT the targets, corr the corrections (zero before the
    first round), all [P, >= n] like mix_csr_pm's XT (n = rowptr length - 1);
    YT receives x', corr is updated in place.  ax is mix_csr_pm's sum and the
    rest as extra_csr: the bits of extra_csr on the transposed matrices.  The
    rules of this op are extra_csr's, on mix_csr_pm's layout, and at most
    ops.PM_DGD_MAX_AGENTS agents.  nseg as mix_csr_pm (None: the order tuned
    for the XT / YT pair on the plain mix, which only writes YT).  Returns YT."""
    obj = _extra_rules("extra_csr_pm", XT, YT, TT, corr, objective)
    n = rowptr.shape[0] - 1
    if n > _ops.PM_DGD_MAX_AGENTS:
        raise ValueError(f"extra_csr_pm: the EXTRA round takes at most {_ops.PM_DGD_MAX_AGENTS} agents (got {n})")
    P, n, _, ldx, ldy = _ops._pm_args(XT, YT, rowptr, col, val, n, P)
    _, ldc, ldt = _leading_dims((("XT", XT), ("corr", corr)), ("TT", TT), P, n, pmajor=True)
    if self_weight is not None:
        _ops._check_array("self_weight", self_weight, torch.float32, n, XT.device)
    _check_square(rowptr, col, n)
    if nseg is None:
        nseg = _ops._pm_auto(_ops._pm_mix(XT, YT, rowptr, col, val, ldx, ldy, n, n, P), XT, YT, ldx, ldy, n, n, P)
    _native.call("dol_extra_csr_pm_ex_f32", XT.data_ptr(), ldx, YT.data_ptr(), ldy, n, P, rowptr.data_ptr(),
                 _ops._ptr_unless_empty(col), _ops._ptr_unless_empty(val), _ops._ptr(self_weight), TT.data_ptr(), ldt,
                 corr.data_ptr(), ldc, obj, float(lr), int(nseg), _ops._stream(XT))
    return YT


def extra_ring(X: torch.Tensor, Y: torch.Tensor, w_prev: torch.Tensor, w_next: torch.Tensor, target: torch.Tensor,
               corr: torch.Tensor, self_weight: Optional[torch.Tensor] = None, objective: str = "least_squares",
               lr: float = 0.01, halo_prev: Optional[torch.Tensor] = None, halo_next: Optional[torch.Tensor] = None,
               P: Optional[int] = None, n_rows: Optional[int] = None) -> torch.Tensor:
    """extra_csr's round on the agent-major ring (dol_extra_ring_f32): W = the
    ring stencil (w_prev, w_next [n_rows], as mix_ring) + diag(self_weight),
      ax = fl(fl(+0 + fl(w_prev x[r-1])) + fl(w_next x[r+1]))
    and the rest as extra_csr: the bits of extra_csr on the ring's CSR.
    halo_prev / halo_next: the rows of X before and after the local block
    ([>= P] each; both or neither), or the wrap-around ring inside X without
    them (at least 3 rows then).  Only X has halos: target and corr are the
    block's own rows.  Returns Y."""
    obj = _extra_rules("extra_ring", X, Y, target, corr, objective)
    P, n, ldx, ldy = _ops._ring_args(X, Y, w_prev, w_next, P, n_rows)
    if not _ops._check_halos(halo_prev, halo_next, P, X.device) and n < 3:
        raise ValueError("a wrap-around ring needs >= 3 rows (use extra_csr)")
    ldt, ldc = _extra_rows(X, target, corr, self_weight, P, n)
    _native.call("dol_extra_ring_f32", X.data_ptr(), ldx, Y.data_ptr(), ldy, n, P, _ops._ptr(halo_prev),
                 _ops._ptr(halo_next), w_prev.data_ptr(), w_next.data_ptr(), _ops._ptr(self_weight), target.data_ptr(),
                 ldt, corr.data_ptr(), ldc, obj, float(lr), _ops._stream(X))
    return Y


def extra_ring_edges(X: torch.Tensor, Y: torch.Tensor, w_prev: torch.Tensor, w_next: torch.Tensor,
                     target: torch.Tensor, corr: torch.Tensor, halo_prev: torch.Tensor, halo_next: torch.Tensor,
                     self_weight: Optional[torch.Tensor] = None, objective: str = "least_squares", lr: float = 0.01,
                     P: Optional[int] = None, n_rows: Optional[int] = None) -> torch.Tensor:
    """Rows 0 and n_rows-1 of extra_ring with halos, in one launch
    (dol_extra_ring_edges_f32): the second half of a sharded ring's round.
    The weight vectors, target and corr are the whole block's."""
    obj = _extra_rules("extra_ring_edges", X, Y, target, corr, objective)
    P, n, ldx, ldy = _ops._ring_args(X, Y, w_prev, w_next, P, n_rows)
    _ops._check_halos(halo_prev, halo_next, P, X.device, required_by="extra_ring_edges")
    ldt, ldc = _extra_rows(X, target, corr, self_weight, P, n)
    _native.call("dol_extra_ring_edges_f32", X.data_ptr(), ldx, Y.data_ptr(), ldy, n, P, halo_prev.data_ptr(),
                 halo_next.data_ptr(), w_prev.data_ptr(), w_next.data_ptr(), _ops._ptr(self_weight), target.data_ptr(),
                 ldt, corr.data_ptr(), ldc, obj, float(lr), _ops._stream(X))
    return Y
