"""Synthetic separable objectives for BASELINE config 3 (decentralised
gradient descent at 1024+ agents x 2^20 parameters, mixing-bound).

Agent i minimises f_i(x) over its own row of the bank; one round is the
reference's gossip round order (DIST/simulators.py:147-162: consensus with
W[t], then local_update = `local_steps` iterations of torch.optim.SGD(lr,
momentum), DIST/clients.py:43-49) with the local loss replaced by a
separable synthetic one, so the whole round fuses into one pass
(dol_dgd_ring_f32 / dol_dgd_csr_f32):

  least_squares  f_i(x) = 1/2 ||x - t_i||^2      (t_i = target row; optimum of
                                                  sum_i f_i is mean_i t_i)
  logistic       f_i(x) = sum_p log(1 + exp(-t_ip x_p))   (t = label * feature,
                                                  the diagonal-feature variant)

Not a reference model: the reference trains CNNs on MNIST (SURVEY §8d names
these objectives as the config-3 workload).  The momentum buffer persists
across rounds like the reference's optimizer state.
"""
from __future__ import annotations

from typing import Optional

import torch

from .bank import AgentBank
from .graph import MixingPlan


def _seeded_draw(x: torch.Tensor, t: torch.Tensor, objective: str, seed: int, dev) -> None:
    """The seeded init of every config-3 problem, from one generator on dev in
    this order: x standard normal, t standard normal, and for the logistic loss
    a random sign on t (t = label (+-1) * feature)."""
    g = torch.Generator(device=dev).manual_seed(seed)
    x.normal_(generator=g)
    t.normal_(generator=g)
    if objective == "logistic":
        t.copy_(torch.where(torch.rand(t.shape, generator=g, device=dev) < 0.5, -t, t))


def _gt_rules(objective: str, self_weight, n: int, dev) -> Optional[torch.Tensor]:
    """The rules of both gradient-tracking problems: a known objective, and n
    self weights (or None), returned as a contiguous float32 vector on dev."""
    from . import ops
    if objective not in ops.OBJECTIVES:
        raise ValueError(f"objective must be one of {sorted(ops.OBJECTIVES)}")
    if self_weight is None:
        return None
    w = torch.as_tensor(self_weight, dtype=torch.float32).to(dev).contiguous()
    if w.shape != (n,):
        raise ValueError(f"self_weight: expected {n} weights")
    return w


def _distance_to_mean_target(x: torch.Tensor, t: torch.Tensor, agent_axis: int, objective: str) -> float:
    """max over agents and coordinates of |x_ip - mean_j t_jp| (the mean in
    fp64, over the agent axis): least squares only, whose optimum is the mean of
    the targets."""
    if objective != "least_squares":
        raise ValueError("distance_to_optimum: the optimum is known in closed form for least squares only")
    return float((x.double() - t.double().mean(agent_axis, keepdim=True)).abs().max())


class SeparableDGD:
    def __init__(self, plan: MixingPlan, P: int, objective: str = "least_squares", lr: float = 0.01,
                 momentum: float = 0.0, local_steps: int = 1, seed: int = 2028, device=None,
                 bank: Optional[AgentBank] = None):
        self.plan = plan
        self.objective = objective
        self.lr, self.mu, self.local_steps = float(lr), float(momentum), int(local_steps)
        dev = plan.device if device is None else torch.device(device)
        self.bank = bank if bank is not None else AgentBank(plan.n_rows, P, dev)
        self.P = self.bank.P
        _seeded_draw(self.bank.buffer("x"), self.bank.buffer("target"), objective, seed, dev)
        self.bank.buffer("y")
        if self.mu != 0.0:
            self.bank.buffer("mom", zero=True)
        self.first = True
        self.rounds = 0

    def params(self) -> torch.Tensor:
        return self.bank.rows("x")

    def targets(self) -> torch.Tensor:
        return self.bank.rows("target")

    def momentum_rows(self) -> Optional[torch.Tensor]:
        return self.bank.rows("mom") if self.mu != 0.0 else None

    def round(self) -> None:
        """X <- W X, then the local steps; swaps the Jacobi buffers (no copy)."""
        b = self.bank
        self.plan.apply_dgd(b.buffer("x"), b.buffer("y"), b.buffer("target"),
                            mom=b.buffer("mom") if self.mu != 0.0 else None, objective=self.objective,
                            steps=self.local_steps, lr=self.lr, momentum=self.mu, first_step=self.first,
                            P=self.P)
        b.swap("x", "y")
        self.first = False
        self.rounds += 1

    def loss(self) -> torch.Tensor:
        """Per-agent local loss f_i(x_i) (diagnostic, torch ops)."""
        x, t = self.params(), self.targets()
        if self.objective == "least_squares":
            return 0.5 * ((x - t) ** 2).sum(1)
        return torch.nn.functional.softplus(-t * x).sum(1)

    def consensus_error(self) -> float:
        x = self.params()
        return float((x - x.mean(0, keepdim=True)).norm() / max(1, x.shape[0]) ** 0.5)


class SeparableADMM:
    """FedADMM on the separable least-squares objective f_k(w) = 1/2 ||w - t_k||^2
    over stacked agent rows (BASELINE config 4's primal/dual side).

    One round is the reference's Server.run body (DEC/servers.py:50-81) with
    the CNN loss replaced by least squares:
      m = max(int(frac * N), 1); order = np.random.choice(range(N), m, replace=False)
      every sampled client: FedAdmm_Client.update_weights(theta) (DEC/clients.py:36-53)
        = w <- theta, local_steps x (update_model :125-139 + SGD.step :44), update_duals :141-144
        -> one fused kernel over the sampled rows (dol_admm_ls_round_f32)
      theta <- average_weights(new w in sampled order) (DEC/servers.py:42-48)
        -> dol_ordered_mean_f32, or across ranks parallel.global_mean_exact
           ("exact", bit-identical to one process) / parallel.global_mean
           ("fast": local ordered sums + all_reduce(SUM), then / m).
    The reference's server averages the primal rows only (no alpha/rho term in
    theta, DEC/servers.py:42-48), so its iteration does NOT reach the optimum
    mean_k t_k of sum_k f_k: with every client sampled each round, sum_k alpha_k
    = rho*N*(theta - theta_0) holds after every round, and the fixed point
    (w_k = theta, grad = 0 => alpha_k = t_k - theta) is
        theta* = (mean_k t_k + rho*theta_0) / (1 + rho)          (fixed_point())
    which the engine reproduces, bias included.
    Each client's momentum buffer persists across rounds (the reference's
    per-client torch.optim.SGD is never reset); its first step ever sets
    buf = g'.  Metrics per round: sum over sampled clients of
    ||w_k - theta||^2 (primal residual, pre-round theta) and ||alpha_k||^2.

    Sharded (torch.distributed initialised), two ways:
      shard="agents": rank r owns the contiguous agent block
        parallel.shard_bounds(N, world, r); every rank draws the same order
        (same seed), runs its local sampled rows, and the mean is the only
        collective ("exact": parallel.global_mean_exact, "fast": all_reduce).
      shard="columns" (VERDICT r05 item 6): rank r owns EVERY
        agent x the parameter columns parallel.column_bounds(P, world, r).  The
        objective is separable per coordinate, so each rank runs the fused round
        + ordered mean (dol_admm_ls_round_mean_f32) over all sampled agents on
        its columns, in the global sampled order: theta's block is exactly
        DEC/servers.py:42-48's mean with NO collective on the round path.  The
        residual metrics are per-rank partials, summed across ranks when
        `history` is read (a collective: every rank reads it).
    `round_fn` / `ordered_sum` inject CPU checkers in tests.

    algorithm = "fedavg" / "fedprox" (SeparableFedAvg / SeparableFedProx) runs
    the same Server.run with the other two clients of the reference
    (FedAvg_Client / FedProx_Client, DEC/clients.py:85-95 / :101-115; their
    update_duals is the base class's no-op, :58-59) through
    dol_fed_ls_round_f32 / dol_fed_ls_round_mean_f32.  They keep no duals:
    `alpha` is None and never allocated, `round_fn` is called with alpha=None
    and alpha_sq=None, and `history` keeps its keys with dual_sq 0.0.  Sharding,
    both means and the fused / two-kernel choice work as for FedADMM.
    """

    def __init__(self, n_agents: int, P: int, rho: float = 0.1, lr: float = 0.1, momentum: float = 0.5,
                 local_steps: int = 1, frac: float = 1.0, seed: int = 2028, device=None, mean: str = "exact",
                 group=None, metrics: bool = True, round_fn=None, ordered_sum=None, fused: Optional[bool] = None,
                 shard: str = "agents", algorithm: str = "fedadmm"):
        import functools

        import numpy as np
        import torch.distributed as dist

        from . import ops, parallel
        from .bank import row_stride
        if mean not in ("exact", "fast"):
            raise ValueError("mean must be 'exact' or 'fast'")
        if shard not in ("agents", "columns"):
            raise ValueError("shard must be 'agents' or 'columns'")
        if algorithm not in ops.FED_ALGORITHMS:
            raise ValueError(f"algorithm must be one of {sorted(ops.FED_ALGORITHMS)}")
        self.algorithm = algorithm
        self.duals = algorithm == "fedadmm"
        self.shard = shard
        self.N, self.P = int(n_agents), int(P)
        self.rho, self.lr, self.mu, self.local_steps = float(rho), float(lr), float(momentum), int(local_steps)
        self.m = max(int(frac * self.N), 1)
        self.mean_mode, self.group, self.metrics = mean, group, metrics
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        self.rank = dist.get_rank(group) if dist.is_initialized() else 0
        if shard == "columns":
            # every agent, this rank's parameter columns [c0, c1): the kernels see Pl columns
            self.lo, self.hi = 0, self.N
            self.c0, self.c1 = parallel.column_bounds(self.P, self.world, self.rank)
            mean = self.mean_mode = "exact"  # each column block's mean IS the reference's order
        else:
            self.lo, self.hi = parallel.shard_bounds(self.N, self.world, self.rank)
            self.c0, self.c1 = 0, self.P
        self.Pl = self.c1 - self.c0
        self.n = self.hi - self.lo
        self.device = torch.device(device) if device is not None else torch.device("cuda")
        if self.duals:
            own_round, own_round_mean = ops.admm_ls_round, ops.admm_ls_round_mean
        else:
            own_round = functools.partial(ops.fed_ls_round, algorithm=algorithm)
            own_round_mean = functools.partial(ops.fed_ls_round_mean, algorithm=algorithm)
        self._round = round_fn if round_fn is not None else own_round
        self._osum = ordered_sum if ordered_sum is not None else ops.ordered_sum
        # the client round and the mean in one pass (dol_admm_ls_round_mean_f32)
        # wherever the mean is this rank's ordered sum of its own rows: one
        # process, or the 'fast' mean's local part; off with injected checkers
        # or DOL_ADMM_FUSED_MEAN=0
        import os
        auto = fused is None
        if fused is None:
            fused = os.environ.get("DOL_ADMM_FUSED_MEAN", "1") != "0"
        self.fused = bool(fused) and round_fn is None and ordered_sum is None and \
            (self.world == 1 or mean == "fast" or shard == "columns")
        if auto and self.fused and shard == "columns" and self.world > 1 and self.device.type == "cuda":
            # the one-pass kernel's parallelism is its column strips: below ~1024 lanes
            # per CU the two-kernel round (row-major client round, then the ordered
            # sum) is faster -- 5.15 vs 7.4 ms at 8192 x 2^17, a rank's block at 8
            # ranks (profiles/r06c_admm_narrow_ab.jsonl); same bits either way
            n_cu = torch.cuda.get_device_properties(self.device).multi_processor_count
            self.fused = self.Pl >= 4 * 1024 * n_cu
        self._round_mean = own_round_mean
        self._parallel = parallel
        self.rs = np.random.RandomState(seed)  # the reference's np.random.choice stream (setup_seed)
        ld = row_stride(max(self.Pl, 1))
        dev = self.device
        self.w = torch.zeros(max(self.n, 1), ld, dtype=torch.float32, device=dev)
        self.alpha = torch.zeros_like(self.w) if self.duals else None
        self.target = torch.empty_like(self.w)
        self.mom = torch.zeros_like(self.w) if self.mu != 0.0 else None
        # per-row seeds over the whole row: identical rows (and column blocks) for every sharding
        full_row = torch.empty(self.P, dtype=torch.float32, device=dev) if shard == "columns" else None
        for k in range(self.lo, self.hi):
            g = torch.Generator(device=dev).manual_seed(seed * 1000003 + k + 1)
            if full_row is None:
                self.target[k - self.lo, :self.P].normal_(generator=g)
            else:
                full_row.normal_(generator=g)
                self.target[k - self.lo, :self.Pl].copy_(full_row[self.c0:self.c1])
        del full_row
        g = torch.Generator(device=dev).manual_seed(seed)
        self.theta = torch.zeros(ld, dtype=torch.float32, device=dev)
        th = torch.empty(self.P, dtype=torch.float32, device=dev).normal_(generator=g)
        self.theta[:self.Pl].copy_(th[self.c0:self.c1])
        del th
        self.theta0 = self.theta.clone()
        self._theta_next = torch.zeros_like(self.theta)
        self.mom_started = np.zeros(max(self.n, 1), dtype=bool)
        self.rounds = 0
        self._pending = []  # per-round device metrics, read lazily (no sync on the round path)
        self._history = []

    def sample(self):
        """The sampled clients of the next round, in the reference's order."""
        return self.rs.choice(range(self.N), self.m, replace=False)

    def round(self, order=None) -> None:
        import numpy as np
        order = np.asarray(self.sample() if order is None else order, dtype=np.int64)
        if order.size < 1 or order.min() < 0 or order.max() >= self.N or len(set(order.tolist())) != order.size:
            raise ValueError(f"order must be distinct agent ids in [0, {self.N})")
        local = [int(g) - self.lo for g in order if self.lo <= g < self.hi]
        dev = self.device
        ml = len(local)
        rw = ra = None
        if self.shard == "columns":
            return self._column_round(order)
        if self.fused:
            return self._fused_round(order, local)
        if ml:
            rows = torch.as_tensor(local, dtype=torch.int32, device=dev)
            first = None
            if self.mom is not None:
                first = torch.as_tensor(~self.mom_started[local], dtype=torch.int32, device=dev)
            if self.metrics:
                rw = torch.empty(ml, dtype=torch.float64, device=dev)
                ra = torch.empty(ml, dtype=torch.float64, device=dev) if self.duals else None
            self._round(self.w, self.alpha, self.target, self.theta, agents=rows, first=first, buf=self.mom,
                        rho=self.rho, lr=self.lr, momentum=self.mu, local_steps=self.local_steps, resid_sq=rw,
                        alpha_sq=ra, P=self.P)
            if self.mom is not None and self.local_steps > 0:
                self.mom_started[local] = True
        par = self._parallel
        if self.mean_mode == "exact":
            par.global_mean_exact(self.w, self.lo, self.hi, [int(g) for g in order], self.P, group=self.group,
                                  out=self._theta_next, ordered_sum=self._osum)
        else:
            par.global_mean(self.w, local, self.m, self.P, group=self.group, out=self._theta_next,
                            ordered_sum=self._osum)
        self.theta, self._theta_next = self._theta_next, self.theta
        if self.metrics:
            s = torch.zeros(2, dtype=torch.float64, device=dev)
            if ml:
                s[0] = rw.sum()
                if ra is not None:
                    s[1] = ra.sum()
            if self.world > 1:
                self._all_reduce(s)
            self._pending.append((self.rounds, s))
        self.rounds += 1

    def _all_reduce(self, s: torch.Tensor) -> torch.Tensor:
        """all_reduce(SUM) in place (gloo: device tensors staged through host memory)."""
        import torch.distributed as dist
        if s.device.type == "cuda" and self._parallel._backend(self.group) == "gloo":
            h = s.cpu()
            dist.all_reduce(h, group=self.group)
            s.copy_(h)
        else:
            dist.all_reduce(s, group=self.group)
        return s

    def _column_round(self, order) -> None:
        """shard="columns": every sampled agent's client round and the server's
        ordered mean on this rank's parameter columns, in the global sampled
        order, with no collective (the round and the mean of DEC/servers.py:
        50-81 are per coordinate; theta's block is the reference's bits)."""
        dev = self.device
        m = int(order.size)
        s = torch.zeros(2, dtype=torch.float64, device=dev) if self.metrics else None
        if self.Pl > 0:
            rows = torch.as_tensor(order, dtype=torch.int32, device=dev)
            first = None
            if self.mom is not None:
                first = torch.as_tensor(~self.mom_started[order], dtype=torch.int32, device=dev)
            if self.fused:
                self._round_mean(self.w, self.alpha, self.target, self.theta, agents=rows, first=first, buf=self.mom,
                                 rho=self.rho, lr=self.lr, momentum=self.mu, local_steps=self.local_steps,
                                 out=self._theta_next, scale=float(m), resid_total=s, P=self.Pl, validate=False)
            else:  # two passes (injected checkers / DOL_ADMM_FUSED_MEAN=0): the client round, then the ordered mean
                rw = ra = None
                if self.metrics:
                    rw = torch.empty(m, dtype=torch.float64, device=dev)
                    ra = torch.empty(m, dtype=torch.float64, device=dev) if self.duals else None
                self._round(self.w, self.alpha, self.target, self.theta, agents=rows, first=first, buf=self.mom,
                            rho=self.rho, lr=self.lr, momentum=self.mu, local_steps=self.local_steps, resid_sq=rw,
                            alpha_sq=ra, P=self.Pl)
                self._osum(self.w, rows, out=self._theta_next, scale=float(m), P=self.Pl)
                if self.metrics:
                    s[0] = rw.sum()
                    if ra is not None:
                        s[1] = ra.sum()
        if self.mom is not None and self.local_steps > 0:
            self.mom_started[order] = True
        self.theta, self._theta_next = self._theta_next, self.theta
        if self.metrics:
            self._pending.append((self.rounds, s))  # this rank's columns only: summed in `history`
        self.rounds += 1

    def full_theta(self) -> torch.Tensor:
        """theta over all P columns on every rank (shard="columns": one
        all_gather of the column blocks; diagnostics and checkpoints, not on the
        round path)."""
        if self.shard != "columns" or self.world == 1:
            return self.theta[:self.P]
        return self._gather_columns(self.theta[:self.Pl])

    def _gather_columns(self, v: torch.Tensor) -> torch.Tensor:
        par = self._parallel
        bounds = [par.column_bounds(self.P, self.world, q) for q in range(self.world)]
        width = max(max(b - a for a, b in bounds), 1)
        pad = torch.zeros(width, dtype=v.dtype, device=v.device)
        pad[:v.numel()] = v
        parts = par._all_gather(pad, self.group)
        return torch.cat([parts[q][:b - a] for q, (a, b) in enumerate(bounds)])

    def _fused_round(self, order, local) -> None:
        """round() on dol_admm_ls_round_mean_f32: the client round and this
        rank's ordered sum of its new rows in one pass (one process: the mean
        itself, bit-identical to the two-kernel round; 'fast' mean: the local
        sum, then all_reduce + / m).  The residual metrics come as the round's
        totals (fp64, another fixed summation order than the per-agent path's:
        equal to ~1e-15 relative)."""
        dev = self.device
        ml = len(local)
        s = torch.zeros(2, dtype=torch.float64, device=dev) if self.metrics else None
        if ml:
            rows = torch.as_tensor(local, dtype=torch.int32, device=dev)
            first = None
            if self.mom is not None:
                first = torch.as_tensor(~self.mom_started[local], dtype=torch.int32, device=dev)
            self._round_mean(self.w, self.alpha, self.target, self.theta, agents=rows, first=first, buf=self.mom,
                             rho=self.rho, lr=self.lr, momentum=self.mu, local_steps=self.local_steps,
                             out=self._theta_next, scale=float(self.m) if self.world == 1 else 1.0,
                             resid_total=s, P=self.P, validate=False)
            if self.mom is not None and self.local_steps > 0:
                self.mom_started[local] = True
        else:  # a rank without sampled rows ('fast' mean): contributes zeros
            self._theta_next.zero_()
        if self.world > 1:
            self._parallel.global_mean_finish(self._theta_next, self.m, self.P, group=self.group)
        self.theta, self._theta_next = self._theta_next, self.theta
        if self.metrics:
            if self.world > 1:
                self._all_reduce(s)
            self._pending.append((self.rounds, s))
        self.rounds += 1

    @property
    def history(self):
        """Per-round metrics: {"round", "primal_resid_sq", "dual_sq"} (sums over
        the sampled clients).  shard="columns" at world > 1: the pending
        per-rank partials are summed across ranks here, in one all_reduce --
        every rank must read `history` at the same point."""
        if self._pending:
            if self.shard == "columns" and self.world > 1:
                stacked = self._all_reduce(torch.stack([s for _, s in self._pending]))
                self._pending = [(r, stacked[i]) for i, (r, _) in enumerate(self._pending)]
            for r, s in self._pending:
                v = s.cpu().tolist()
                self._history.append({"round": r, "primal_resid_sq": v[0], "dual_sq": v[1]})
        self._pending = []
        return self._history

    def optimum(self) -> torch.Tensor:
        """mean_k t_k in fp64 (the minimiser of sum_k f_k); all ranks (diagnostic)."""
        if self.shard == "columns":
            s = self.target[:self.n, :self.Pl].double().sum(0)
            return (s if self.world == 1 else self._gather_columns(s)) / self.N
        s = self.target[:self.n, :self.P].double().sum(0)
        if self.world > 1:
            self._all_reduce(s)
        return s / self.N

    def distance_to_optimum(self) -> float:
        """||theta - mean_k t_k|| / sqrt(P)."""
        return float((self.full_theta().double() - self.optimum()).norm() / self.P ** 0.5)

    def fixed_point(self) -> torch.Tensor:
        """theta* = (mean_k t_k + rho*theta_0) / (1 + rho): where the reference's
        iteration settles under full participation (see the class docstring).
        FedAvg / FedProx: optimum().  With every client sampled the round is
        the same affine map of (theta, t_k, buf_k) for every client, so the
        mean of the rows follows one client's iteration on mean_k t_k, and
        theta = mean_k t_k with zero mean momentum is stationary."""
        if not self.duals:
            return self.optimum()
        theta0 = self.theta0[:self.P] if self.shard != "columns" or self.world == 1 else \
            self._gather_columns(self.theta0[:self.Pl])
        return (self.optimum() + self.rho * theta0.double()) / (1.0 + self.rho)

    def distance_to_fixed_point(self) -> float:
        """||theta - theta*|| / sqrt(P) (full participation)."""
        return float((self.full_theta().double() - self.fixed_point()).norm() / self.P ** 0.5)


class SeparableFedAvg(SeparableADMM):
    """SeparableADMM's round with the reference's FedAvg client: plain local
    momentum SGD on the least-squares loss (DEC/clients.py:85-95), no duals.
    rho is not used."""

    def __init__(self, n_agents: int, P: int, **kw):
        super().__init__(n_agents, P, algorithm="fedavg", **kw)


class SeparableFedProx(SeparableADMM):
    """SeparableADMM's round with the reference's FedProx client: the proximal
    term rho * (w - theta) on every local gradient (DEC/clients.py:101-115), no
    duals."""

    def __init__(self, n_agents: int, P: int, **kw):
        super().__init__(n_agents, P, algorithm="fedprox", **kw)


class SeparableScaffold:
    """SCAFFOLD on the separable least-squares objective f_k(w) = 1/2 ||w - t_k||^2
    over stacked agent rows: the server round of SeparableADMM with the
    reference's fourth client, the commented-out Scaffold_Client sketch
    (DEC/clients.py:146-170), and the server step of Karimireddy et al. 2020,
    Algorithm 1, which the reference never wrote.  One round, in one pass
    (dol_scaffold_ls_round_f32):
      m = max(int(frac * N), 1); order = np.random.choice(range(N), m, replace=False)
      every sampled client: w <- theta, local_steps x momentum SGD on the
        gradient corrected by c - c_k (:155), then c_k <- c_k - c - (w - theta)
        / (local_steps * lr) (:162-165)
      theta <- theta + global_lr * mean over the sampled of (w - theta)
      c     <- c + (1 / N) * sum over the sampled of the change of c_k
    The control variates remove the client drift and the sampling error that
    keep FedAvg's theta moving under frac < 1 and that bias FedADMM's fixed
    point (SeparableADMM.fixed_point): theta reaches optimum() = mean_k t_k.

    A standalone class, not an `algorithm=` of SeparableADMM: there is a second
    server vector, the server step is not an ordered mean of the rows, and no
    two-kernel or sharded variant exists (single process only).  Targets and
    theta are seeded as SeparableADMM's; c_k and c start at zero; the sampling
    replays the reference's np.random.choice stream; each client's momentum
    buffer persists across rounds (`mom_started`).  `history` has
    SeparableADMM's keys: primal_resid_sq = sum over the sampled clients of
    ||w_k - theta||^2 (pre-round theta), dual_sq = that of ||c_k||^2.
    `round_fn` injects a CPU checker with ops.scaffold_ls_round's signature."""

    def __init__(self, n_agents: int, P: int, lr: float = 0.1, momentum: float = 0.5, local_steps: int = 1,
                 frac: float = 1.0, global_lr: float = 1.0, seed: int = 2028, device=None, metrics: bool = True,
                 round_fn=None):
        import numpy as np
        import torch.distributed as dist

        from . import ops
        from .bank import row_stride
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise ValueError("SeparableScaffold runs in one process (no sharded SCAFFOLD round)")
        if int(local_steps) < 1:
            raise ValueError("local_steps must be >= 1")
        self.N, self.P = int(n_agents), int(P)
        self.lr, self.mu, self.local_steps = float(lr), float(momentum), int(local_steps)
        self.global_lr = float(global_lr)
        self.m = max(int(frac * self.N), 1)
        self.metrics = metrics
        self.device = dev = torch.device(device) if device is not None else torch.device("cuda")
        self._round = round_fn if round_fn is not None else ops.scaffold_ls_round
        self.rs = np.random.RandomState(seed)  # the reference's np.random.choice stream (setup_seed)
        ld = row_stride(max(self.P, 1))
        self.w = torch.zeros(self.N, ld, dtype=torch.float32, device=dev)
        self.ci = torch.zeros_like(self.w)
        self.target = torch.empty_like(self.w)
        self.mom = torch.zeros_like(self.w) if self.mu != 0.0 else None
        for k in range(self.N):  # SeparableADMM's per-row seeds
            g = torch.Generator(device=dev).manual_seed(seed * 1000003 + k + 1)
            self.target[k, :self.P].normal_(generator=g)
        g = torch.Generator(device=dev).manual_seed(seed)
        self.theta = torch.zeros(ld, dtype=torch.float32, device=dev)
        self.theta[:self.P].copy_(torch.empty(self.P, dtype=torch.float32, device=dev).normal_(generator=g))
        self.c =torch.zeros_like(self.theta)
        self.mom_started = np.zeros(self.N, dtype=bool)
        self.rounds = 0
        self._pending = []  # per-round device metrics, read lazily (no sync on the round path)
        self._history = []

    def sample(self):
        """The sampled clients of the next round, in the reference's order."""
        return self.rs.choice(range(self.N), self.m, replace=False)

    def round(self, order=None) -> None:
        import numpy as np
        order = np.asarray(self.sample() if order is None else order, dtype=np.int64)
        if order.size < 1 or order.min() < 0 or order.max() >= self.N or len(set(order.tolist())) != order.size:
            raise ValueError(f"order must be distinct agent ids in [0, {self.N})")
        dev = self.device
        rows = torch.as_tensor(order, dtype=torch.int32, device=dev)
        first = None
        if self.mom is not None:
            first = torch.as_tensor(~self.mom_started[order], dtype=torch.int32, device=dev)
        s = torch.zeros(2, dtype=torch.float64, device=dev) if self.metrics else None
        # theta and c are stepped in place: each column is read before it is written
        self._round(self.w, self.ci, self.target, self.theta, self.c, agents=rows, first=first, buf=self.mom,
                    lr=self.lr, momentum=self.mu, local_steps=self.local_steps, global_lr=self.global_lr,
                    theta_out=self.theta, c_out=self.c, n_total=self.N, resid_total=s, P=self.P, validate=False)
        if self.mom is not None:
            self.mom_started[order] = True
        if self.metrics:
            self._pending.append((self.rounds, s))
        self.rounds += 1

    @property
    def history(self):
        """Per-round metrics: {"round", "primal_resid_sq", "dual_sq"} (sums over the sampled clients)."""
        for r, s in self._pending:
            v = s.cpu().tolist()
            self._history.append({"round": r, "primal_resid_sq": v[0], "dual_sq": v[1]})
        self._pending = []
        return self._history

    def optimum(self) -> torch.Tensor:
        """mean_k t_k in fp64 (the minimiser of sum_k f_k)."""
        return self.target[:, :self.P].double().sum(0) / self.N

    def distance_to_optimum(self) -> float:
        """||theta - mean_k t_k|| / sqrt(P)."""
        return float((self.theta[:self.P].double() - self.optimum()).norm() / self.P ** 0.5)


class SeparableDGDPM:
    """Config 3 on the parameter-major bank: the round of SeparableDGD (same
    objectives, same round order, bit-identical values) with every state
    matrix stored transposed, XT[p][i] = agent i's parameter p ([P, ld], ld =
    round_up(N, 4)), so that any sparse W streams the bank once
    (dol_dgd_csr_pm_f32).  Build it from a SeparableDGD
    (`from_agent_major`, which transposes that problem's current state) or
    fresh (random init drawn directly in this layout).  At most
    ops.PM_DGD_MAX_AGENTS agents.  consensus_steps = k > 1 makes the round
    FedLCon's (DIST/simulators.py:190-196): X <- W^k X, then the local steps,
    still one kernel and one pass over the bank (dol_dgd_csr_pm_steps_f32; W
    must be square); 1 is the round above, through the same call as ever."""

    def __init__(self, plan: MixingPlan, P: int, objective: str = "least_squares", lr: float = 0.01,
                 momentum: float = 0.0, local_steps: int = 1, seed: int = 2028, _state=None,
                 consensus_steps: int = 1):
        from . import ops
        if int(consensus_steps) < 1:
            raise ValueError("consensus_steps must be >= 1")
        self.consensus_steps = int(consensus_steps)
        if plan.n_rows > ops.PM_DGD_MAX_AGENTS:
            raise ValueError(f"the parameter-major round takes at most {ops.PM_DGD_MAX_AGENTS} agents")
        if plan.kind == "dense":
            raise ValueError("the parameter-major round mixes a sparse (CSR) W")
        self.plan, self.P, self.objective = plan, int(P), objective
        self.lr, self.mu, self.local_steps = float(lr), float(momentum), int(local_steps)
        self.N = plan.n_rows
        self.ld = (self.N + 3) // 4 * 4
        dev = plan.device
        shape = (self.P, self.ld)
        self.XT = torch.zeros(shape, dtype=torch.float32, device=dev)
        self.YT = torch.zeros_like(self.XT)
        self.TT = torch.zeros_like(self.XT)
        self.MT = torch.zeros_like(self.XT) if self.mu != 0.0 else None
        self.first, self.rounds = True, 0
        if _state is None:
            _seeded_draw(self.XT[:, :self.N], self.TT[:, :self.N], objective, seed, dev)

    @classmethod
    def from_agent_major(cls, prob: "SeparableDGD", consensus_steps: int = 1) -> "SeparableDGDPM":
        """Transpose prob's current state (x, targets, momentum, first-step flag)."""
        from . import ops
        self = cls(prob.plan, prob.P, prob.objective, prob.lr, prob.mu, prob.local_steps, _state=True,
                   consensus_steps=consensus_steps)
        ops.transpose(prob.params(), self.XT, prob.plan.n_rows, prob.P)
        ops.transpose(prob.targets(), self.TT, prob.plan.n_rows, prob.P)
        if self.MT is not None:
            ops.transpose(prob.momentum_rows(), self.MT, prob.plan.n_rows, prob.P)
        self.first, self.rounds = prob.first, prob.rounds
        return self

    def round(self) -> None:
        """X <- W^consensus_steps X, then the local steps (one kernel); swaps XT / YT."""
        from . import ops
        p = self.plan
        if self.consensus_steps == 1:
            ops.dgd_csr_pm(self.XT, self.YT, p.rowptr, p.col, p.val, self.TT, self.MT, objective=self.objective,
                           steps=self.local_steps, lr=self.lr, momentum=self.mu, first_step=self.first, P=self.P)
            self.XT, self.YT = self.YT, self.XT
        else:
            self._keep(ops.dgd_csr_pm_steps(self.XT, self.YT, p.rowptr, p.col, p.val, self.TT, self.MT,
                                            objective=self.objective, mix_steps=self.consensus_steps,
                                            steps=self.local_steps, lr=self.lr, momentum=self.mu,
                                            first_step=self.first, P=self.P))
        self.first = False
        self.rounds += 1

    def mix(self, steps: int = 1) -> None:
        """X <- W^steps X, plain consensus with no local step: the inner loop of
        FedLCon.run on this bank, one pass per ops.PM_MAX_FUSED_STEPS steps."""
        from . import ops
        p = self.plan
        self._keep(ops.mix_csr_pm_steps(self.XT, self.YT, p.rowptr, p.col, p.val, steps, P=self.P))

    def _keep(self, holder: torch.Tensor) -> None:
        """Make the buffer a multi-pass call left its result in the current XT."""
        if holder is self.YT:
            self.XT, self.YT = self.YT, self.XT

    def params(self) -> torch.Tensor:
        """Agent-major copy [N, P] of the current parameters (diagnostic)."""
        return self.XT[:, :self.N].T.contiguous()

    def momentum_rows(self) -> Optional[torch.Tensor]:
        return None if self.MT is None else self.MT[:, :self.N].T.contiguous()

    def consensus_error(self) -> float:
        x = self.XT[:, :self.N]
        return float((x - x.mean(1, keepdim=True)).norm() / max(1, self.N) ** 0.5)


class SeparableGTPM:
    """Config 3 with gradient tracking (DIGing / NEXT) on the parameter-major
    bank, SeparableDGDPM's sibling: every agent carries a tracker s_i of the
    average gradient beside x_i, and one round

      x_i' = sum_j W_ij x_j - lr s_i
      s_i' = sum_j W_ij s_j + grad f_i(x_i') - grad f_i(x_i)     s_i(0) = grad f_i(x_i(0))

    is one kernel and one pass over X, S and the targets (dol_gt_csr_pm_f32).
    Where the DGD round with a constant lr leaves every agent at a biased fixed
    point, every agent here reaches the optimum of sum_i f_i with the same
    constant lr.  Not a reference algorithm (the reference's decentralised
    round is consensus + local step, DIST/simulators.py:147-162).

    W = plan's CSR + diag(self_weight) must be doubly stochastic with a
    positive self weight for the method to converge: on a zero-diagonal ring
    of even size (-1 is an eigenvalue of W) the iterates grow without bound.
    graph.metropolis_weights builds such a W from any symmetric pattern.  lr
    must be small against the spectral gap of W: on a random 4-regular graph
    of 16 agents with Metropolis weights, least squares, 0.1 converges and 0.3
    diverges (a float32 CPU simulation of this arithmetic).

    XT / XO, ST / SO and TT are [P, ld] like SeparableDGDPM's matrices, with
    the same seeded init; ST starts as ops.separable_grad(XT, TT).  Dense
    plans and more than ops.GT_MAX_AGENTS agents are refused."""

    def __init__(self, plan: MixingPlan, P: int, objective: str = "least_squares", lr: float = 0.01,
                 self_weight=None, seed: int = 2028):
        from . import ops
        if plan.n_rows > ops.GT_MAX_AGENTS:
            raise ValueError(f"the gradient-tracking round takes at most {ops.GT_MAX_AGENTS} agents")
        if plan.kind == "dense":
            raise ValueError("the gradient-tracking round mixes a sparse (CSR) W")
        self.plan, self.P, self.objective, self.lr = plan, int(P), objective, float(lr)
        self.N = plan.n_rows
        self.ld = (self.N + 3) // 4 * 4
        dev = plan.device
        self.self_weight = _gt_rules(objective, self_weight, self.N, dev)
        self.XT = torch.zeros((self.P, self.ld), dtype=torch.float32, device=dev)
        self.XO, self.ST, self.SO, self.TT = (torch.zeros_like(self.XT) for _ in range(4))
        _seeded_draw(self.XT[:, :self.N], self.TT[:, :self.N], objective, seed, dev)
        ops.separable_grad(self.XT, self.TT, self.ST, objective)
        self.rounds = 0

    @classmethod
    def from_agent_major(cls, prob: "SeparableGT") -> "SeparableGTPM":
        """The problem of a SeparableGT on this bank: its plan, self weights and
        lr, and its current parameters, trackers and targets transposed (the
        two layouts draw their seeded init in different element orders)."""
        from . import ops
        self = cls(prob.plan, prob.P, prob.objective, prob.lr, self_weight=prob.self_weight)
        for src, dst in ((prob.params(), self.XT), (prob.tracker(), self.ST), (prob.targets(), self.TT)):
            ops.transpose(src, dst, prob.N, prob.P)
        self.rounds = prob.rounds
        return self

    def round(self) -> None:
        """One gradient-tracking round (one kernel); swaps XT / XO and ST / SO."""
        from . import ops
        p = self.plan
        ops.gt_csr_pm(self.XT, self.ST, self.XO, self.SO, p.rowptr, p.col, p.val, self.TT,
                      self_weight=self.self_weight, objective=self.objective, lr=self.lr, P=self.P)
        self.XT, self.XO = self.XO, self.XT
        self.ST, self.SO = self.SO, self.ST
        self.rounds += 1

    def params(self) -> torch.Tensor:
        """Agent-major copy [N, P] of the current parameters (diagnostic)."""
        return self.XT[:, :self.N].T.contiguous()

    def tracker(self) -> torch.Tensor:
        """Agent-major copy [N, P] of the gradient trackers s_i (diagnostic)."""
        return self.ST[:, :self.N].T.contiguous()

    def consensus_error(self) -> float:
        x = self.XT[:, :self.N]
        return float((x - x.mean(1, keepdim=True)).norm() / max(1, self.N) ** 0.5)

    def distance_to_optimum(self) -> float:
        """_distance_to_mean_target of the parameters (agents along axis 1)."""
        return _distance_to_mean_target(self.XT[:, :self.N], self.TT[:, :self.N], 1, self.objective)


def ring_gt_weights(ring_csr):
    """(w_prev, w_next, w_self), float32 [n] each, as ops.gt_ring and
    SeparableGT take them: graph.metropolis_weights on the pattern of
    `ring_csr` (row i = {i - 1, i + 1} mod n, n >= 3; its values are not
    used), the off-diagonal part through CSR.ring_weights.  On a ring every
    degree is 2: each edge weighs fl(1/3) and w_self = fl(1 - fl(1/3 + 1/3)),
    a symmetric doubly stochastic W with a positive diagonal."""
    from .graph import metropolis_weights
    w_off, d = metropolis_weights(ring_csr)
    ring = w_off.ring_weights()
    if ring is None:
        raise ValueError("ring_gt_weights: the pattern is not a ring (row i = {i - 1, i + 1} mod n, n >= 3)")
    return ring[0], ring[1], d


class SeparableGTCSR:
    """Config 3 with gradient tracking on the agent-major bank, SeparableGTPM's
    sibling on SeparableDGD's bank: the same round (see SeparableGTPM), one
    kernel and one pass over X, S and the targets through plan.apply_gt
    (dol_gt_csr_f32 on a CSR plan, dol_gt_ring_f32 on a ring plan), for any
    sparse W and any number of agents -- the parameter-major round stops at
    ops.GT_MAX_AGENTS.  Not a reference algorithm.

    plan is any non-dense plan; W = its W + diag(self_weight) must be doubly
    stochastic with a positive diagonal, which graph.metropolis_weights gives
    from any symmetric pattern.  lr must be small against the spectral gap of
    W (SeparableGTPM's docstring has the 16-agent random 4-regular numbers).

    The bank holds x / y (parameters in and out), s / s_out (trackers) and
    target, with SeparableDGD's seeded init; s starts as ops.separable_grad(x,
    target).  With the same seed and shape it is the problem of SeparableDGD
    and of SeparableGT, bit for bit.  The parameter-major draw of SeparableGTPM
    is another element order: SeparableGTPM.from_agent_major makes the same
    problem there."""

    _IN, _OUT = "x", "y"  # the bank's names for the parameters in and out

    def __init__(self, plan: MixingPlan, P: int, objective: str = "least_squares", lr: float = 0.01,
                 self_weight=None, seed: int = 2028, bank: Optional[AgentBank] = None):
        from . import ops
        self._check_plan(plan)
        self.plan, self.objective, self.lr = plan, objective, float(lr)
        self.N = plan.n_rows
        dev = plan.device
        self.self_weight = _gt_rules(objective, self_weight, self.N, dev)
        self.bank = bank if bank is not None else AgentBank(self.N, P, dev)
        self.P = self.bank.P
        _seeded_draw(self.bank.buffer(self._IN), self.bank.buffer("target"), objective, seed, dev)
        for name in (self._OUT, "s", "s_out"):
            self.bank.buffer(name, zero=True)
        ops.separable_grad(self.bank.rows(self._IN), self.bank.rows("target"), self.bank.rows("s"), objective)
        self.rounds = 0

    @staticmethod
    def _check_plan(plan) -> None:
        if plan.kind == "dense":
            raise ValueError("the gradient-tracking round mixes a sparse (CSR) W")

    def round(self) -> None:
        """One gradient-tracking round (one kernel); swaps x / y and s / s_out."""
        b = self.bank
        self.plan.apply_gt(b.buffer("x"), b.buffer("s"), b.buffer("y"), b.buffer("s_out"), b.buffer("target"),
                           self_weight=self.self_weight, objective=self.objective, lr=self.lr, P=self.P)
        b.swap("x", "y")
        b.swap("s", "s_out")
        self.rounds += 1

    def params(self) -> torch.Tensor:
        return self.bank.rows(self._IN)

    def tracker(self) -> torch.Tensor:
        return self.bank.rows("s")

    def targets(self) -> torch.Tensor:
        return self.bank.rows("target")

    def consensus_error(self) -> float:
        x = self.params()
        return float((x - x.mean(0, keepdim=True)).norm() / max(1, x.shape[0]) ** 0.5)

    def distance_to_optimum(self) -> float:
        """_distance_to_mean_target of the parameters (agents along axis 0)."""
        return _distance_to_mean_target(self.params(), self.targets(), 0, self.objective)


class SeparableGT(SeparableGTCSR):
    """SeparableGTCSR on the agent-major ring only: one kernel and one pass
    over X, S and the targets (dol_gt_ring_f32), for any number of agents.
    Not a reference algorithm.

    plan must be a ring plan (plan.kind == "ring": its w_prev / w_next are the
    stencil); W = that stencil + diag(self_weight) must be doubly stochastic
    with a positive diagonal, which ring_gt_weights gives.  lr must be small
    against the spectral gap of W, which shrinks as 1 / n^2 on a ring: on 9
    agents with Metropolis weights, least squares, 0.1 converges in 200 rounds
    and 0.3 diverges; 33 agents need far more rounds (a float32 CPU simulation
    of this arithmetic).  Bank, init and accessors are SeparableGTCSR's."""

    @staticmethod
    def _check_plan(plan) -> None:
        from . import ops
        if plan.kind != "ring":
            raise ValueError(f"SeparableGT runs on a ring plan (got kind {plan.kind!r}); SeparableGTPM takes any "
                             f"sparse W of up to {ops.GT_MAX_AGENTS} agents")


class SeparableGTPush(SeparableGTCSR):
    """Config 3 with push-sum gradient tracking (ADD-OPT / Push-DIGing) on the
    agent-major bank: SeparableGTCSR's sibling for weights that are
    column-stochastic only, one call and one pass over U, S and the targets per
    round through plan.apply_gt_push (dol_gt_push_csr_f32).  Not a reference
    algorithm.

    plan is a CSR plan (MixingPlan(..., allow_ring=False) where the pattern is
    a ring); C = its matrix + diag(self_weight) must be column-stochastic with
    a positive diagonal on a strongly connected graph: graph.push_sum_weights
    gives that from any directed pattern, and CSR.transpose() of the
    reference's row-stochastic W, halved, with self weights 1/2, from its own
    graphs.  On such weights SeparableGTCSR settles at a biased point.

    The bank holds u / u_out (the push-sum numerators in and out), s / s_out
    (trackers) and target, with SeparableDGD's seeded init (u starts as x(0));
    v / v_out are the push-sum weights, n floats each, starting at 1; s starts
    as ops.separable_grad(x(0), target).  The estimate every agent holds is
    params() = u / v.  Bank set-up, tracker start and the other accessors are
    SeparableGTCSR's, on u / u_out."""

    _IN, _OUT = "u", "u_out"

    def __init__(self, plan: MixingPlan, P: int, objective: str = "least_squares", lr: float = 0.01,
                 self_weight=None, seed: int = 2028, bank: Optional[AgentBank] = None):
        super().__init__(plan, P, objective, lr, self_weight, seed, bank)
        self.v = torch.ones(self.N, dtype=torch.float32, device=plan.device)
        self.v_out = torch.ones(self.N, dtype=torch.float32, device=plan.device)

    @staticmethod
    def _check_plan(plan) -> None:
        SeparableGTCSR._check_plan(plan)
        if plan.kind == "ring":
            raise ValueError("SeparableGTPush runs on a CSR plan (got kind 'ring'); build it with allow_ring=False")

    def round(self) -> None:
        """One push-sum gradient-tracking round (one call); swaps u / u_out, s / s_out and v / v_out."""
        b = self.bank
        self.plan.apply_gt_push(b.buffer("u"), b.buffer("s"), b.buffer("u_out"), b.buffer("s_out"), b.buffer("target"),
                                self.v, self.v_out, self_weight=self.self_weight, objective=self.objective, lr=self.lr,
                                P=self.P)
        b.swap("u", "u_out")
        b.swap("s", "s_out")
        self.v, self.v_out = self.v_out, self.v
        self.rounds += 1

    def params(self) -> torch.Tensor:
        """The agents' estimates z = u / v (a read-out: torch's division)."""
        return self.bank.rows("u") / self.v[:, None]

    def weights(self) -> torch.Tensor:
        return self.v


class SeparableEXTRA:
    """Config 3 with EXTRA (Shi, Ling, Wu, Yin, SIAM J. Optim. 25(2), 2015) on
    the agent-major bank: the exact round that mixes the parameters only, one
    kernel and one pass over X, the corrections and the targets through
    plan.apply_extra (dol_extra_csr_f32 on a CSR plan, dol_extra_ring_f32 on a
    ring plan), for any sparse W and any number of agents.  Not a reference
    algorithm.

    plan is any non-dense plan; W = its W + diag(self_weight) must be symmetric
    and doubly stochastic with a positive diagonal, SeparableGTCSR's weights
    (graph.metropolis_weights, ring_gt_weights).  Step size: with W~ = (I +
    W) / 2 the paper's condition is lr < 2 lambda_min(W~) / L, L the gradient's
    Lipschitz constant (1 for least squares): lambda_min(W~) = (1 +
    lambda_min(W)) / 2 is positive for any W with a positive diagonal, and the
    bound does not shrink with the spectral gap as gradient tracking's does.
    A float32 CPU simulation of this arithmetic (numpy, not a GPU run;
    Metropolis weights, least squares, max |x - mean t| after 200 rounds):
    9-agent ring, lr 0.1: 2.1e-6 (gradient tracking 5.6e-7, DGD 0.66); lr 0.3:
    5.3e-7 (gradient tracking diverges, DGD 1.34); random 4-regular 16 agents,
    lr 0.1: 4.7e-6 (3.1e-7, 0.43); lr 0.3: 6.8e-7 (diverges, 1.08); random
    4-regular 37 agents, lr 0.1: 3.3e-6 (2.1e-7, 0.57).  The floor is |sum_i
    c_i| / (n lr), the fp32 drift of the invariant sum_i c_i = 0; it stops
    moving once the iterates have converged.

    The bank holds x / y (parameters in and out), target and corr (the
    corrections, zero at the start, updated in place), with SeparableGTCSR's
    seeded draw: with the same seed and shape it is that problem bit for bit."""

    def __init__(self, plan: MixingPlan, P: int, objective: str = "least_squares", lr: float = 0.01,
                 self_weight=None, seed: int = 2028, bank: Optional[AgentBank] = None):
        if plan.kind == "dense":
            raise ValueError("the EXTRA round mixes a sparse (CSR) W")
        self.plan, self.objective, self.lr = plan, objective, float(lr)
        self.N = plan.n_rows
        dev = plan.device
        self.self_weight = _gt_rules(objective, self_weight, self.N, dev)
        self.bank = bank if bank is not None else AgentBank(self.N, P, dev)
        self.P = self.bank.P
        _seeded_draw(self.bank.buffer("x"), self.bank.buffer("target"), objective, seed, dev)
        for name in ("y", "corr"):
            self.bank.buffer(name, zero=True)
        self.rounds = 0

    def round(self) -> None:
        """One EXTRA round (one kernel); corr is updated in place; swaps x / y."""
        b = self.bank
        self.plan.apply_extra(b.buffer("x"), b.buffer("y"), b.buffer("target"), b.buffer("corr"),
                              self_weight=self.self_weight, objective=self.objective, lr=self.lr, P=self.P)
        b.swap("x", "y")
        self.rounds += 1

    def params(self) -> torch.Tensor:
        return self.bank.rows("x")

    def correction(self) -> torch.Tensor:
        return self.bank.rows("corr")

    def targets(self) -> torch.Tensor:
        return self.bank.rows("target")

    def consensus_error(self) -> float:
        x = self.params()
        return float((x - x.mean(0, keepdim=True)).norm() / max(1, x.shape[0]) ** 0.5)

    def distance_to_optimum(self) -> float:
        """_distance_to_mean_target of the parameters (agents along axis 0)."""
        return _distance_to_mean_target(self.params(), self.targets(), 0, self.objective)


class SeparableEXTRAPM:
    """Config 3 with EXTRA on the parameter-major bank, SeparableGTPM's sibling
    and SeparableEXTRA's round on that layout: one kernel and one pass over X,
    the corrections and the targets (dol_extra_csr_pm_f32), the five streams of
    SeparableDGDPM's round with momentum, for any sparse W.  Not a reference
    algorithm.  The weights W = plan's CSR + diag(self_weight) and the step
    size are SeparableEXTRA's: see its docstring.

    XT / YT (parameters in and out), TT and CT (the corrections, zero at the
    start, updated in place) are [P, ld], ld = round_up(N, 4), like
    SeparableGTPM's matrices, with the same seeded init.  Dense plans and more
    than ops.PM_DGD_MAX_AGENTS agents are refused."""

    def __init__(self, plan: MixingPlan, P: int, objective: str = "least_squares", lr: float = 0.01,
                 self_weight=None, seed: int = 2028, _state=None):
        from . import ops
        if plan.n_rows > ops.PM_DGD_MAX_AGENTS:
            raise ValueError(f"the EXTRA round on the parameter-major bank takes at most {ops.PM_DGD_MAX_AGENTS} agents")
        if plan.kind == "dense":
            raise ValueError("the EXTRA round mixes a sparse (CSR) W")
        self.plan, self.P, self.objective, self.lr = plan, int(P), objective, float(lr)
        self.N = plan.n_rows
        self.ld = (self.N + 3) // 4 * 4
        dev = plan.device
        self.self_weight = _gt_rules(objective, self_weight, self.N, dev)
        self.XT = torch.zeros((self.P, self.ld), dtype=torch.float32, device=dev)
        self.YT, self.TT, self.CT = (torch.zeros_like(self.XT) for _ in range(3))
        if _state is None:
            _seeded_draw(self.XT[:, :self.N], self.TT[:, :self.N], objective, seed, dev)
        self.rounds = 0

    @classmethod
    def from_agent_major(cls, prob: "SeparableEXTRA") -> "SeparableEXTRAPM":
        """The problem of a SeparableEXTRA on this bank: its plan, self weights
        and lr, and its current parameters, targets and corrections transposed
        (the two layouts draw their seeded init in different element orders)."""
        from . import ops
        self = cls(prob.plan, prob.P, prob.objective, prob.lr, self_weight=prob.self_weight, _state=True)
        for src, dst in ((prob.params(), self.XT), (prob.targets(), self.TT), (prob.correction(), self.CT)):
            ops.transpose(src, dst, prob.N, prob.P)
        self.rounds = prob.rounds
        return self

    def round(self) -> None:
        """One EXTRA round (one kernel); CT is updated in place; swaps XT / YT."""
        from . import ops
        p = self.plan
        ops.extra_csr_pm(self.XT, self.YT, p.rowptr, p.col, p.val, self.TT, self.CT, self_weight=self.self_weight,
                         objective=self.objective, lr=self.lr, P=self.P)
        self.XT, self.YT = self.YT, self.XT
        self.rounds += 1

    def params(self) -> torch.Tensor:
        """Agent-major copy [N, P] of the current parameters (diagnostic)."""
        return self.XT[:, :self.N].T.contiguous()

    def correction(self) -> torch.Tensor:
        """Agent-major copy [N, P] of the corrections c_i (diagnostic)."""
        return self.CT[:, :self.N].T.contiguous()

    def consensus_error(self) -> float:
        x = self.XT[:, :self.N]
        return float((x - x.mean(1, keepdim=True)).norm() / max(1, self.N) ** 0.5)

    def distance_to_optimum(self) -> float:
        """_distance_to_mean_target of the parameters (agents along axis 1)."""
        return _distance_to_mean_target(self.XT[:, :self.N], self.TT[:, :self.N], 1, self.objective)


class TimeVaryingMLPGossip:
    """BASELINE config 5 as a first-class round: N agents, each an
    nn.Sequential(Linear(d, h), ReLU(), Linear(h, c)) row of the bank, a new
    Erdos-Renyi p W drawn every round ('stochastic' weighting,
    DIST/simulators.py:65-70), one local momentum-SGD step per agent on its
    batch (DIST/clients.py:34-59: forward, CrossEntropyLoss, backward, step;
    the fused dol_mlp_step_f32), then the synchronous consensus round with that
    W (DIST/clients.py:61-69, bit-exact: device Neighbors + the LDS-gather CSR
    kernel).  One process per GPU: with torch.distributed initialised, rank r
    owns the agent block shard_bounds(N, world, r) and the mix runs through
    parallel.AgentColumnTranspose (bit-identical to one GPU).  The round's W
    draw + CSR build runs on a side stream, overlapped with the local step.

    batch(X, y): per-agent batches for this rank's agents ([n_local, B, d] float32,
    [n_local, B] int64), kept until replaced."""

    def __init__(self, n_agents: int, d: int = 784, h: int = 128, c: int = 10, p_edge: float = 0.1,
                 lr: float = 0.05, momentum: float = 0.5, seed: int = 2028, device=None, group=None,
                 init_std: float = 0.05, overlap_chunks: int = 2):
        import torch.distributed as dist
        from . import parallel
        from .mlp import BatchedMLP, mlp_layout
        self.N, self.d, self.h, self.c = int(n_agents), d, h, c
        self.p_edge, self.lr, self.mu, self.seed = float(p_edge), float(lr), float(momentum), int(seed)
        self.device = torch.device("cuda" if device is None else device)
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        self.rank = dist.get_rank(group) if dist.is_initialized() else 0
        self.lo, self.hi = parallel.shard_bounds(self.N, self.world, self.rank)
        self.n_local = self.hi - self.lo
        self.bank = AgentBank(self.n_local, mlp_layout(d, h, c), self.device)
        self.P = self.bank.P
        self.mlp = BatchedMLP(self.bank, d, h, c)
        # every agent's initial row from one global stream: the same model whatever the sharding
        g = torch.Generator(device=self.device).manual_seed(self.seed)
        full = torch.empty(self.N, self.P, device=self.device).normal_(0, init_std, generator=g)
        self.bank.rows()[:] = full[self.lo:self.hi]
        del full
        self.bank.buffer("y").zero_()
        if self.mu != 0.0:
            self.bank.buffer("mom", zero=True)
        self.tr = parallel.AgentColumnTranspose(self.N, self.P, self.device, group) if self.world > 1 else None
        self.overlap_chunks = max(1, int(overlap_chunks))  # pieces of the local step overlapped with the exchange
        self._W = torch.empty(self.N, self.N, device=self.device)
        self._plan = None
        self._side = torch.cuda.Stream(self.device)
        self.X = self.y = None
        self.rounds = 0
        self.last_loss = None  # the latest round's per-agent losses (round() returns them too)

    def batch(self, X: torch.Tensor, y: torch.Tensor) -> None:
        if X.shape[:1] != (self.n_local,) or y.shape[:1] != (self.n_local,) or X.shape[-1] != self.d:
            raise ValueError(f"batch: expected X [{self.n_local}, B, {self.d}] and y [{self.n_local}, B]")
        self.X, self.y = X, y

    def round_seed(self, r: int) -> int:
        return self.seed * 1000003 + r + 1

    def round(self) -> torch.Tensor:
        """One round; returns this rank's per-agent losses (device tensor)."""
        from . import graph as G
        if self.X is None:
            raise RuntimeError("TimeVaryingMLPGossip.round: call batch() first")
        main = torch.cuda.current_stream(self.device)
        self._side.wait_stream(main)  # the previous round's mix has consumed the old plan
        with torch.cuda.stream(self._side):
            W = G.erdos_renyi_stochastic_hip(self.N, self.p_edge, self.round_seed(self.rounds), self.device,
                                             out=self._W)
            # balanced pack: it runs here, on the side stream, under the local step
            self._plan = G.MixingPlan.from_dense(W, dense_kernel="csr", reuse=self._plan, balance=True)
        if self.tr is None:
            loss = self.mlp.step(self.X, self.y, lr=self.lr, momentum=self.mu, first_step=(self.rounds == 0))
            self._plan_ready(main)
            self.bank.mix(self._plan)
        else:
            # the local steps in pieces, each piece's first exchange posted while
            # the next piece steps (parallel.AgentColumnTranspose.mix_with_local_steps)
            loss = torch.empty(self.n_local, dtype=torch.float32, device=self.device)

            def step_rows(a, b):
                self.mlp.step(self.X, self.y, lr=self.lr, momentum=self.mu, first_step=(self.rounds == 0),
                              rows=slice(a, b), loss=loss)

            def before_mix():
                self._plan_ready(main)
                self.tr.set_plan(self._plan)
            self.tr.mix_with_local_steps(self.bank.rows(), step_rows, chunks=self.overlap_chunks,
                                         before_mix=before_mix)
        self.rounds += 1
        self.last_loss = loss
        return loss

    def _plan_ready(self, main) -> None:
        """The compute stream waits for the side stream's W draw + plan build."""
        main.wait_stream(self._side)
        # the plan's buffers were allocated on the side stream and are read on the
        # main one: tell the caching allocator, so freeing them never races the mix
        for t in (self._plan.rowptr, self._plan.col, self._plan.val, self._plan.ent, self._plan.hdr):
            if t is not None:
                t.record_stream(main)

    def params(self) -> torch.Tensor:
        return self.bank.rows()
