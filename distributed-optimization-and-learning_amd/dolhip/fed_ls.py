"""The least-squares server round of all three algorithms of the reference's
primal/dual half (DEC/servers.py:50-81 drives FedAvg, FedProx and FedADMM
through one Server.run): dol_fed_ls_round_f32 and, fused with the server's
ordered average, dol_fed_ls_round_mean_f32.  ops re-exports both calls as
ops.fed_ls_round / ops.fed_ls_round_mean.

  "fedavg"   g' = g = fl(w - t)                            (DEC/clients.py:85-95)
  "fedprox"  g' = fl(g + fl(rho * fl(w - theta)))          (:101-115)
  "fedadmm"  ops.admm_ls_round / ops.admm_ls_round_mean, bit for bit (:125-144)

FedAvg and FedProx keep no duals: alpha is None, no dual row is read or
written, and a round moves t (, buf) in and w (, buf) out per sampled agent.
FedAvg is not FedADMM with rho = 0 and zero duals (the extra additions turn a
gradient of -0 into +0).  The argument rules are the validators of ops.py
(_ls_round_args, _check_distinct_agents, ...) plus the two stated here: a
known algorithm, and duals exactly where the algorithm has them;
tests/test_fed_ls_host.py pins them without a launch.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import ops as _ops


def _algorithm(name: str, algorithm: str, alpha: Optional[torch.Tensor]) -> int:
    """DOL_FED_* of `algorithm`; alpha is there exactly for "fedadmm"."""
    if algorithm not in _ops.FED_ALGORITHMS:
        raise ValueError(f"{name}: algorithm must be one of {sorted(_ops.FED_ALGORITHMS)}")
    alg = _ops.FED_ALGORITHMS[algorithm]
    if alg == 2 and alpha is None:
        raise ValueError(f"{name}: 'fedadmm' needs alpha")
    if alg != 2 and alpha is not None:
        raise ValueError(f"{name}: '{algorithm}' has no duals (alpha must be None)")
    return alg


def fed_ls_round(w: torch.Tensor, alpha: Optional[torch.Tensor], target: torch.Tensor, theta: torch.Tensor,
                 algorithm: str = "fedadmm", agents: Optional[torch.Tensor] = None,
                 first: Optional[torch.Tensor] = None, buf: Optional[torch.Tensor] = None, rho: float = 0.1,
                 lr: float = 0.1, momentum: float = 0.0, local_steps: int = 1,
                 resid_sq: Optional[torch.Tensor] = None, alpha_sq: Optional[torch.Tensor] = None,
                 work: Optional[torch.Tensor] = None, P: Optional[int] = None) -> None:
    """One client round of `algorithm` on f_a(w) = 1/2 ||w - t_a||^2 for the
    sampled rows `agents` (dol_fed_ls_round_f32): w = theta, `local_steps` x
    (LS gradient + the algorithm's term + momentum SGD), and for "fedadmm" the
    dual ascent.  The arguments are ops.admm_ls_round's; alpha is None unless
    the algorithm is "fedadmm".  resid_sq: float64 [m], ||w_k - theta||^2 (the
    client drift); it may be passed alone for "fedavg" / "fedprox", which take
    no alpha_sq.  rho is not used by "fedavg".
    Reference: DEC/clients.py:36-53 with update_model :85-95 / :101-115 /
    :125-139 and update_duals :58-59 / :141-144."""
    alg = _algorithm("fed_ls_round", algorithm, alpha)
    if alg != 2 and alpha_sq is not None:
        raise ValueError(f"fed_ls_round: '{algorithm}' has no duals (alpha_sq must be None)")
    _ops._ls_round("dol_fed_ls_round_f32", alg, w, alpha, target, theta, agents, first, buf, rho, lr, momentum,
                   local_steps, resid_sq, alpha_sq, work, P)


def fed_ls_round_mean(w: torch.Tensor, alpha: Optional[torch.Tensor], target: torch.Tensor, theta: torch.Tensor,
                      algorithm: str = "fedadmm", agents: Optional[torch.Tensor] = None,
                      first: Optional[torch.Tensor] = None, buf: Optional[torch.Tensor] = None, rho: float = 0.1,
                      lr: float = 0.1, momentum: float = 0.0, local_steps: int = 1,
                      out: Optional[torch.Tensor] = None, scale: Optional[float] = None,
                      resid_total: Optional[torch.Tensor] = None, work: Optional[torch.Tensor] = None,
                      P: Optional[int] = None, validate: bool = True) -> torch.Tensor:
    """fed_ls_round + the server's ordered average in ONE pass
    (dol_fed_ls_round_mean_f32): the whole round of DEC/servers.py:50-81 for
    `algorithm`.  The arguments are ops.admm_ls_round_mean's; alpha is None
    unless the algorithm is "fedadmm".  resid_total: float64 [2], the round's
    sums of ||w - theta||^2 and ||alpha||^2 (0 for "fedavg" / "fedprox").
    validate (default): the host check that `agents` are distinct rows of w;
    it is not made while the stream is being captured into a graph."""
    alg = _algorithm("fed_ls_round_mean", algorithm, alpha)
    return _ops._ls_round_mean("fed_ls_round_mean", "dol_fed_ls_round_mean_f32", alg, w, alpha, target, theta, agents,
                               first, buf, rho, lr, momentum, local_steps, out, scale, resid_total, work, P, validate)
