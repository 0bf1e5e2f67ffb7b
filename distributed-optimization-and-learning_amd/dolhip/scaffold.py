"""The SCAFFOLD least-squares server round in one pass
(dol_scaffold_ls_round_f32), beside the FedAvg / FedProx / FedADMM rounds of
fed_ls.py.  ops re-exports the call as ops.scaffold_ls_round.

The client is the reference's commented-out sketch, Scaffold_Client
(DEC/clients.py:146-170), on f_a(w) = 1/2 ||w - t_a||^2: every local gradient
is corrected by the server's control variate minus the client's own,
  g' = fl(fl(g + c) - c_a)                                  (:155)
and after the local steps the client's variate becomes
  c_a' = fl(fl(c_a - c) - fl(fl(w - theta) / (local_steps * lr)))   (:162-165)
The server step is not in the reference; it is Karimireddy et al. 2020,
Algorithm 1: theta += global_lr * mean over the sampled clients of (w - theta),
c += (1 / N) * sum over the sampled clients of (c_a' - c_a), N = ALL clients.

SCAFFOLD is not a fourth value of ops.FED_ALGORITHMS (those three share one
Server.run and one argument list; this round has a second server vector and a
second output), so it has its own entry point.  The argument rules are the
validators of ops.py plus those stated here; tests/test_scaffold_host.py pins
them without a launch.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _native
from . import ops as _ops


def inv_steps_lr(local_steps: int, lr: float) -> float:
    """1 / (local_steps * lr) in double (DEC/clients.py:164); the entry point
    takes it as one float, rounded once."""
    return 1.0 / (int(local_steps) * float(lr))


def scaffold_ls_round(w: torch.Tensor, ci: torch.Tensor, target: torch.Tensor, theta: torch.Tensor, c: torch.Tensor,
                      agents: Optional[torch.Tensor] = None, first: Optional[torch.Tensor] = None,
                      buf: Optional[torch.Tensor] = None, lr: float = 0.1, momentum: float = 0.0,
                      local_steps: int = 1, global_lr: float = 1.0, theta_out: Optional[torch.Tensor] = None,
                      c_out: Optional[torch.Tensor] = None, scale_w: Optional[float] = None,
                      n_total: Optional[int] = None, resid_total: Optional[torch.Tensor] = None,
                      work: Optional[torch.Tensor] = None, P: Optional[int] = None,
                      validate: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
    """One SCAFFOLD round for the sampled rows `agents` (int32 device [m],
    DISTINCT, in the sampled order; None = rows 0..n-1): every client's local
    steps from theta with the corrected gradient, its new control variate, and
    the server's step on theta and c, in ONE pass.  Returns (theta_out, c_out).
    w: [n, ld] rows, only written.  ci: the clients' control variates, shaped
    as w.  c: the server's, [P].  first / buf / momentum: as
    ops.admm_ls_round_mean.  local_steps >= 1.  scale_w: what the summed client
    deltas are divided by (None = m, the mean; 1.0 = the raw ordered sum).
    n_total: N of the 1 / N in the step on c (None = n, the rows of w).
    theta_out may be theta and c_out may be c; neither may be a row matrix.
    resid_total: float64 [2], the round's sums of ||w_k - theta||^2 and
    ||c_k'||^2.  validate: the host check that `agents` are distinct rows of w;
    it is not made while the stream is being captured into a graph."""
    if int(local_steps) < 1:
        raise ValueError("scaffold_ls_round: local_steps must be >= 1 (c_a' divides by local_steps * lr)")
    if not float(lr) > 0.0:
        raise ValueError("scaffold_ls_round: lr must be > 0 (c_a' divides by local_steps * lr)")
    P, n, ldw, ldc, ldt, ldb = _ops._ls_round_args(w, ci, target, theta, agents, buf, momentum, local_steps, P)
    _ops._check_vec("c", c, P, w.device)
    m = _ops._check_distinct_agents("scaffold_ls_round", agents, n, validate)
    (theta_out, c_out), work = _ops._one_pass_outputs(w, m, P, first, (("theta_out", theta_out), ("c_out", c_out)),
                                                      resid_total, work)
    rows = [w, ci, target] + ([buf] if ldb else [])
    for name, out in (("theta_out", theta_out), ("c_out", c_out)):
        if any(out.data_ptr() == r.data_ptr() for r in rows):
            raise ValueError(f"scaffold_ls_round: {name} aliases the rows")
    if theta_out.data_ptr() == c_out.data_ptr():
        raise ValueError("scaffold_ls_round: theta_out and c_out alias")
    n_total = n if n_total is None else int(n_total)
    scale_w = float(m if scale_w is None else scale_w)
    if n_total < 1 or not scale_w > 0.0:
        raise ValueError("scaffold_ls_round: n_total must be >= 1 and scale_w > 0")
    _native.call("dol_scaffold_ls_round_f32", w.data_ptr(), ldw, _ops._ptr(buf) if ldb else None, ldb, ci.data_ptr(),
                 ldc, target.data_ptr(), ldt, theta.data_ptr(), c.data_ptr(), _ops._ptr(agents), _ops._ptr(first), m, P,
                 float(lr), float(momentum), int(local_steps), inv_steps_lr(local_steps, lr), float(global_lr),
                 theta_out.data_ptr(), scale_w, c_out.data_ptr(), float(n_total), _ops._ptr(resid_total),
                 _ops._ptr(work) if resid_total is not None else None, _ops._stream(w))
    return theta_out, c_out
