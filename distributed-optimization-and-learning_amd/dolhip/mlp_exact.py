"""Exact decentralised rounds for the per-agent MLPs of BASELINE config 5.

TimeVaryingMLPGossip runs the reference's round (local step, then consensus),
which with a constant step size settles away from the optimum on heterogeneous
data.  ExactMLPGossip is its single-GPU sibling on a FIXED doubly stochastic W
with the two exact rounds of config 3, gradient tracking and EXTRA, fed with
the gradients BatchedMLP.forward_backward writes into the bank's grad rows:

  round = dol_mlp_step_f32 with update == 0 (forward, CrossEntropyLoss and
          backward of every agent in one kernel, the raw gradients into the
          grad rows), then ONE gradient-fed round in one pass over the bank
          (dol_gt_grad_csr_f32 or dol_extra_grad_csr_f32).

Not a reference algorithm: the reference's decentralised round is
DIST/simulators.py:147-162 (local_update, then consensus).
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from .bank import AgentBank
from .graph import MixingPlan
from .mlp import BatchedMLP, mlp_layout

METHODS = ("gt", "extra")


def _check_weights(plan: MixingPlan, d: np.ndarray) -> None:
    """W = plan's CSR + diag(d): symmetric, rows summing to one, a positive
    diagonal (checked on the host CSR when the plan has one)."""
    if not (d > 0).all():
        raise ValueError("ExactMLPGossip: self_weight must be positive (W needs a positive diagonal)")
    c = plan.csr
    if c is None:
        return
    n = c.n_rows
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(c.rowptr))
    cols = np.asarray(c.col, np.int64)
    vals = np.asarray(c.val, np.float32)
    a, b = np.argsort(rows * n + cols, kind="stable"), np.argsort(cols * n + rows, kind="stable")
    if not (np.array_equal((rows * n + cols)[a], (cols * n + rows)[b]) and np.array_equal(vals[a], vals[b])):
        raise ValueError("ExactMLPGossip: W must be symmetric (graph.metropolis_weights gives such weights)")
    sums = np.bincount(rows, weights=vals.astype(np.float64), minlength=n) + d.astype(np.float64)
    if np.abs(sums - 1.0).max() > 1e-5:
        raise ValueError("ExactMLPGossip: the rows of W = plan + diag(self_weight) must sum to one "
                         "(graph.metropolis_weights gives such weights)")


class ExactMLPGossip:
    """N agents, each an nn.Sequential(Linear(d, h), ReLU(), Linear(h, c)) row
    of the bank (TimeVaryingMLPGossip's agents), on a fixed W, one exact round
    per call: method "gt" is gradient tracking (DIGing with the tracker update
    at the front of the round: s(k) = W s(k-1) + G(k) - G(k-1), x(k+1) = W x(k)
    - lr s(k); plan.apply_gt_grad), method "extra" is EXTRA (Shi, Ling, Wu,
    Yin, SIAM J. Optim. 25(2), 2015: x(k+1) = W x(k) - lr G(k) - c(k), c(k+1) =
    c(k) + (x(k) - W x(k)) / 2; plan.apply_extra_grad), G(k) the agents'
    gradients at x(k) on their current batches.  Not a reference algorithm.

    The weight rule: plan is a CSR plan (MixingPlan(..., allow_ring=False)
    where the pattern is a ring) holding the off-diagonal part of W, and W =
    plan + diag(self_weight) must be symmetric and doubly stochastic with a
    positive diagonal, which graph.metropolis_weights gives from any symmetric
    pattern.  self_weight is therefore required.  Step size: gradient tracking
    needs lr small against the spectral gap of W (SeparableGTCSR: on 16 agents,
    random 4-regular, Metropolis weights, least squares, 0.1 converges and 0.3
    diverges; the gap shrinks as 1 / n^2 on a ring); EXTRA's condition is lr <
    2 lambda_min(W~) / L with W~ = (I + W) / 2 and L the gradient's Lipschitz
    constant (SeparableEXTRA), which does not shrink with the gap.  Both are
    statements about convex losses; the MLP's loss is not convex, and on the
    8-agent ring of tests/test_grad_rounds_gpu.py lr 0.05 holds where 0.3 does
    not (float32 CPU simulations).

    The bank holds x / y (parameters in and out), grad (this round's
    gradients) and, for "gt", s / s_out (trackers) and grad_prev, for "extra",
    corr (the corrections, updated in place); s, s_out, grad_prev and corr are
    zero at the start, so the first round gives s = G(0) with no separate
    initialisation.  The initial rows come from one seeded normal stream of
    standard deviation init_std, as TimeVaryingMLPGossip draws them.

    batch(X, y): per-agent batches ([N, B, d] float32, [N, B] int64), kept
    until replaced."""

    def __init__(self, plan: MixingPlan, d: int, h: int, c: int, method: str = "gt", lr: float = 0.05,
                 self_weight=None, seed: int = 2028, init_std: float = 0.05, bank: Optional[AgentBank] = None):
        if method not in METHODS:
            raise ValueError(f"method must be one of {METHODS}")
        if plan.kind != "csr":
            raise ValueError(f"ExactMLPGossip runs on a CSR plan (got kind {plan.kind!r}); build it with "
                             "allow_ring=False")
        if plan.n_rows != plan.n_cols:
            raise ValueError("ExactMLPGossip needs a square W")
        if self_weight is None:
            raise ValueError("ExactMLPGossip: self_weight is required (W needs a positive diagonal)")
        self.plan, self.method, self.lr = plan, method, float(lr)
        self.N, self.d, self.h, self.c = plan.n_rows, int(d), int(h), int(c)
        self.device = plan.device
        w = torch.as_tensor(self_weight, dtype=torch.float32)
        if w.shape != (self.N,):
            raise ValueError(f"self_weight: expected {self.N} weights")
        _check_weights(plan, w.cpu().numpy())
        self.self_weight = w.to(self.device).contiguous()
        self.bank = bank if bank is not None else AgentBank(self.N, mlp_layout(d, h, c), self.device)
        self.P = self.bank.P
        self.mlp = BatchedMLP(self.bank, d, h, c)
        g = torch.Generator(device=self.device).manual_seed(int(seed))
        self.bank.rows()[:] = torch.empty(self.N, self.P, device=self.device).normal_(0, init_std, generator=g)
        self.bank.buffer("y").zero_()
        self.bank.buffer("grad").zero_()
        for name in (("s", "s_out", "grad_prev") if method == "gt" else ("corr",)):
            self.bank.buffer(name).zero_()
        self.X = self.y = None
        self.rounds = 0
        self.last_loss = None  # the latest round's per-agent losses (round() returns them too)

    def batch(self, X: torch.Tensor, y: torch.Tensor) -> None:
        if X.shape[:1] != (self.N,) or y.shape[:1] != (self.N,) or X.shape[-1] != self.d:
            raise ValueError(f"batch: expected X [{self.N}, B, {self.d}] and y [{self.N}, B]")
        self.X, self.y = X, y

    def round(self) -> torch.Tensor:
        """One exact round: every agent's gradient at its current parameters
        into the grad rows (one kernel), then the gradient-fed round (one
        pass); swaps x / y and, for "gt", s / s_out and grad / grad_prev.
        Returns the per-agent losses at the parameters before the round."""
        if self.X is None:
            raise RuntimeError("ExactMLPGossip.round: call batch() first")
        b = self.bank
        loss = self.mlp.forward_backward(self.X, self.y)
        if self.method == "gt":
            self.plan.apply_gt_grad(b.buffer("x"), b.buffer("s"), b.buffer("y"), b.buffer("s_out"), b.buffer("grad"),
                                    b.buffer("grad_prev"), self_weight=self.self_weight, lr=self.lr, P=self.P)
            b.swap("s", "s_out")
            b.swap("grad", "grad_prev")
        else:
            self.plan.apply_extra_grad(b.buffer("x"), b.buffer("y"), b.buffer("grad"), b.buffer("corr"),
                                       self_weight=self.self_weight, lr=self.lr, P=self.P)
        b.swap("x", "y")
        self.rounds += 1
        self.last_loss = loss
        return loss

    def params(self) -> torch.Tensor:
        return self.bank.rows()

    def tracker(self) -> torch.Tensor:
        """The trackers s_i ("gt"): after a round, mean_i s_i = mean_i G_i of that round."""
        if self.method != "gt":
            raise ValueError('tracker(): method "extra" keeps corrections, not trackers')
        return self.bank.rows("s")

    def correction(self) -> torch.Tensor:
        """The corrections c_i ("extra")."""
        if self.method != "extra":
            raise ValueError('correction(): method "gt" keeps trackers, not corrections')
        return self.bank.rows("corr")

    def gradients(self) -> torch.Tensor:
        """The gradients the latest round was fed (G(k) at the parameters before it)."""
        return self.bank.rows("grad_prev" if self.method == "gt" else "grad")

    def consensus_error(self) -> float:
        x = self.params()
        return float((x - x.mean(0, keepdim=True)).norm() / max(1, x.shape[0]) ** 0.5)
