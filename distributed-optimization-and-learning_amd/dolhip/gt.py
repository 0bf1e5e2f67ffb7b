"""Gradient tracking (DIGing / NEXT) for BASELINE config 3: one round in one
HBM pass on the parameter-major bank (dol_gt_csr_pm_f32, any sparse W, at most
ops.GT_MAX_AGENTS agents), on the agent-major ring (dol_gt_ring_f32, any
number of agents, and the blocks of a sharded ring through its halo form, with
dol_gt_ring_edges_f32 for a block's two boundary rows: ops.gt_ring_edges,
rules pinned by tests/test_gt_sharded_host.py) and on the agent-major bank with any sparse W (dol_gt_csr_f32, any number of
agents, and the column blocks of a column-sharded bank), and the device
gradient of the separable losses (dol_separable_grad_f32) that starts the
trackers.  ops re-exports the calls as ops.gt_csr_pm / ops.gt_ring /
ops.gt_csr / ops.separable_grad.

  x_i' = sum_j W_ij x_j - lr s_i
  s_i' = sum_j W_ij s_j + grad f_i(x_i') - grad f_i(x_i)       s_i(0) = grad f_i(x_i(0))

Not in the reference: its decentralised round is consensus + local step
(DIST/simulators.py:147-162), which with a constant step size settles at a
biased fixed point; the mix inside this round is its consensus
(DIST/clients.py:61-69) in mix_csr_pm's rounding.  The argument rules are the
validators of ops.py (_check_rows, _check_csr, _check_array) and pm_steps'
square-W check, plus the four stated here: a known objective, at most
ops.GT_MAX_AGENTS agents (gt_csr_pm), four distinct state matrices
(_distinct_state) and weight vectors of n floats; tests/test_gt_host.py pins
them for the three ops without a launch.  gt_ring's own rules are in its
docstring and in tests/test_gt_ring_host.py, gt_csr's in its docstring and in
tests/test_gt_csr_gpu.py (the ones a CPU tensor does not reach, with the
library call recorded).

gt_push_csr (dol_gt_push_csr_f32, ops.gt_push_csr) is the push-sum form of
gt_csr's round for weights that are column-stochastic only (ADD-OPT /
Push-DIGing): one more scalar per agent and the gradients taken at U / v; its
arithmetic and rules are in its docstring, pinned by tests/test_gt_push_host.py.

gt_grad_csr (dol_gt_grad_csr_f32, ops.gt_grad_csr) is gt_csr's round with the
gradient fed as a row matrix, for agents whose gradients are not a separable
loss of a target row (the per-agent MLPs of config 5); its arithmetic and rules
are in its docstring, pinned by tests/test_grad_rounds_host.py.
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


def _distinct_state(name: str, state) -> None:
    """state: the four (name, matrix) pairs a round reads and writes."""
    for i, (na, a) in enumerate(state):
        for nb, b in state[i + 1:]:
            if a is b or a.data_ptr() == b.data_ptr():
                raise ValueError(f"{name}: {na} and {nb} alias: the Jacobi update of x and s needs four buffers")


def _leading_dims(state, target, P: int, n: int, pmajor: bool = False):
    """The leading dimensions of the four state matrices and the targets ((name,
    matrix) pairs) on the first one's device: [>= n, >= P] row matrices on the
    agent-major bank, [>= P, >= n] on the parameter-major one."""
    cols, rows, want, width = (None, P, f"[>= {P}, >= {n}]", n) if pmajor else (P, n, f">= {n} rows", 0)
    return tuple(_ops._check_rows(nm, t, cols, rows, f"{nm}: expected {want} on {{}}", width, state[0][1].device)
                 for nm, t in state + (target,))


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
    _distinct_state("gt_csr_pm", state)
    if self_weight is not None:
        _ops._check_array("self_weight", self_weight, torch.float32, n, XT.device)
    P = XT.shape[0] if P is None else P
    ldx, ld_s, ldxo, ldso, ldt = _leading_dims(state, ("TT", TT), P, n, pmajor=True)
    _ops._check_csr(rowptr, col, val, XT.device, same_length=False)
    _check_square(rowptr, col, n)
    if nseg is None:
        nseg = _ops._pm_auto(_ops._pm_mix(XT, XO, rowptr, col, val, ldx, ldxo, n, n, P), XT, XO, ldx, ldxo, n, n, P)
    _native.call("dol_gt_csr_pm_ex_f32", XT.data_ptr(), ldx, ST.data_ptr(), ld_s, XO.data_ptr(), ldxo, SO.data_ptr(),
                 ldso, n, P, rowptr.data_ptr(), _ops._ptr_unless_empty(col), _ops._ptr_unless_empty(val),
                 _ops._ptr(self_weight), TT.data_ptr(), ldt, obj, float(lr), int(nseg), _ops._stream(XT))
    return XO, SO


def gt_ring(X: torch.Tensor, S: torch.Tensor, XO: torch.Tensor, SO: torch.Tensor, w_prev: torch.Tensor,
            w_next: torch.Tensor, target: torch.Tensor, self_weight: Optional[torch.Tensor] = None,
            objective: str = "least_squares", lr: float = 0.01, halos=None, P: Optional[int] = None,
            n_rows: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """gt_csr_pm's round on the agent-major ring (dol_gt_ring_f32), for any
    number of agents and for the blocks of a sharded ring: X the parameters, S
    the trackers, target the targets, [>= n_rows, >= P] like mix_ring's X; XO /
    SO receive x' / s'.  W = the ring stencil (w_prev, w_next [n_rows], as
    mix_ring) + diag(self_weight).  Per coordinate
      ax = fl(fl(+0 + fl(w_prev x[r-1])) + fl(w_next x[r+1])), as the same over s
      ax = fl(ax + fl(d_r x_r)), as = fl(as + fl(d_r s_r))     with self_weight
      x' = fma(-lr, s_r, ax);  s' = fl(fl(as + g(x', t_r)) - g(x_r, t_r))
    the bits of gt_csr_pm on the ring's CSR.  halos: (x_prev, x_next, s_prev,
    s_next), the rows of X and S before and after the local block ([>= P]
    each), or None for the wrap-around ring inside X and S.  The rules of this
    op: a known objective; the four state matrices distinct (a Jacobi update
    of both); all four halos or None; without halos at least 3 rows; a
    self-weight vector of n_rows floats.  Returns (XO, SO)."""
    obj = _check_objective("gt_ring", objective)
    P = X.shape[1] if P is None else P
    n = X.shape[0] if n_rows is None else n_rows
    state = (("X", X), ("S", S), ("XO", XO), ("SO", SO))
    _distinct_state("gt_ring", state)
    for nm, w in (("w_prev", w_prev), ("w_next", w_next)) + ((("self_weight", self_weight),) if self_weight is not None
                                                              else ()):
        _ops._check_array(nm, w, torch.float32, n, X.device)
    if halos is not None:
        if len(halos) != 4 or any(h is None for h in halos):
            raise ValueError("gt_ring: halos are (x_prev, x_next, s_prev, s_next), all four or None")
    elif n < 3:
        raise ValueError("gt_ring: a wrap-around ring needs >= 3 rows (pass halos, or use gt_csr_pm)")
    ldx, ld_s, ldxo, ldso, ldt = _leading_dims(state, ("target", target), P, n)
    for nm, h in zip(("x_prev", "x_next", "s_prev", "s_next"), halos or ()):
        _ops._check_vec(f"halos {nm}", h, P, X.device)
    hp = [None] * 4 if halos is None else [h.data_ptr() for h in halos]
    _native.call("dol_gt_ring_f32", X.data_ptr(), ldx, S.data_ptr(), ld_s, XO.data_ptr(), ldxo, SO.data_ptr(), ldso, n,
                 P, hp[0], hp[1], hp[2], hp[3], w_prev.data_ptr(), w_next.data_ptr(), _ops._ptr(self_weight),
                 target.data_ptr(), ldt, obj, float(lr), _ops._stream(X))
    return XO, SO


def gt_ring_edges(X: torch.Tensor, S: torch.Tensor, XO: torch.Tensor, SO: torch.Tensor, w_prev: torch.Tensor,
                  w_next: torch.Tensor, target: torch.Tensor, halos, self_weight: Optional[torch.Tensor] = None,
                  objective: str = "least_squares", lr: float = 0.01, P: Optional[int] = None,
                  n_rows: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Rows 0 and n_rows - 1 of gt_ring's halo form in one launch
    (dol_gt_ring_edges_f32): the second half of a sharded ring's round, once
    the halo rows have arrived.  Arguments as gt_ring, the matrices and weight
    vectors the whole block's; halos: (x_prev, x_next, s_prev, s_next), all
    four required.  Only rows 0 and n_rows - 1 of XO / SO are written, with
    the bits gt_ring writes there.  Returns (XO, SO)."""
    obj = _check_objective("gt_ring_edges", objective)
    P = X.shape[1] if P is None else P
    n = X.shape[0] if n_rows is None else n_rows
    state = (("X", X), ("S", S), ("XO", XO), ("SO", SO))
    _distinct_state("gt_ring_edges", state)
    for nm, w in (("w_prev", w_prev), ("w_next", w_next)) + ((("self_weight", self_weight),) if self_weight is not None
                                                              else ()):
        _ops._check_array(nm, w, torch.float32, n, X.device)
    if halos is None or len(halos) != 4 or any(h is None for h in halos):
        raise ValueError("gt_ring_edges needs all four halos")
    ldx, ld_s, ldxo, ldso, ldt = _leading_dims(state, ("target", target), P, n)
    for nm, h in zip(("x_prev", "x_next", "s_prev", "s_next"), halos):
        _ops._check_vec(f"halos {nm}", h, P, X.device)
    _native.call("dol_gt_ring_edges_f32", X.data_ptr(), ldx, S.data_ptr(), ld_s, XO.data_ptr(), ldxo, SO.data_ptr(),
                 ldso, n, P, *(h.data_ptr() for h in halos), w_prev.data_ptr(), w_next.data_ptr(),
                 _ops._ptr(self_weight), target.data_ptr(), ldt, obj, float(lr), _ops._stream(X))
    return XO, SO


def _csr_round_args(name: str, state, rowptr, col, val, target, self_weight, objective, lr, P, vectors=(),
                    then=None) -> tuple:
    """The rules gt_csr and gt_push_csr share, in the order they fire, and the
    arguments their native calls start with (everything up to lr).  state: the
    four (name, matrix) pairs; vectors: the op's own (name, n floats) pairs,
    checked ahead of self_weight; then(): the op's own rule on them."""
    obj = _check_objective(name, objective)
    n = rowptr.shape[0] - 1
    _distinct_state(name, state)
    X = state[0][1]
    for nm, w in tuple(vectors) + ((("self_weight", self_weight),) if self_weight is not None else ()):
        _ops._check_array(nm, w, torch.float32, n, X.device)
    if then is not None:
        then()
    P = X.shape[1] if P is None else P
    lds = _leading_dims(state, ("target", target), P, n)
    _ops._check_csr(rowptr, col, val, X.device, same_length=False)
    _check_square(rowptr, col, n)
    rows = tuple(a for (_, t), ld in zip(state, lds) for a in (t.data_ptr(), ld))
    return rows + (n, P, rowptr.data_ptr(), _ops._ptr_unless_empty(col), _ops._ptr_unless_empty(val),
                   _ops._ptr(self_weight), target.data_ptr(), lds[4], obj, float(lr))


def gt_csr(X: torch.Tensor, S: torch.Tensor, XO: torch.Tensor, SO: torch.Tensor, rowptr: torch.Tensor,
           col: torch.Tensor, val: torch.Tensor, target: torch.Tensor, self_weight: Optional[torch.Tensor] = None,
           objective: str = "least_squares", lr: float = 0.01,
           P: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """gt_csr_pm's round on the agent-major bank (dol_gt_csr_f32), for any
    sparse W and any number of agents: X the parameters, S the trackers, target
    the targets, [>= n, >= P] like mix_csr's X (n = rowptr length - 1); XO / SO
    receive x' / s'.  W = W_off + diag(self_weight), W_off the square CSR
    (normally with a zero diagonal).  Per coordinate
      ax = mix of x, as = mix of s                     (mix_csr's sums)
      ax = fl(ax + fl(d_i x_i)), as = fl(as + fl(d_i s_i))     with self_weight
      x' = fma(-lr, s_i, ax);  s' = fl(fl(as + g(x', t_i)) - g(x_i, t_i))
    the bits of gt_csr_pm on the same CSR and of gt_ring on a ring's CSR.  The
    rules of this op: a known objective; the four state matrices distinct (a
    Jacobi update of both); a self-weight vector of n floats; a square W.
    Returns (XO, SO)."""
    call = _csr_round_args("gt_csr", (("X", X), ("S", S), ("XO", XO), ("SO", SO)), rowptr, col, val, target,
                           self_weight, objective, lr, P)
    _native.call("dol_gt_csr_f32", *call, _ops._stream(X))
    return XO, SO


def gt_push_csr(U: torch.Tensor, S: torch.Tensor, UO: torch.Tensor, SO: torch.Tensor, rowptr: torch.Tensor,
                col: torch.Tensor, val: torch.Tensor, target: torch.Tensor, v: torch.Tensor, v_out: torch.Tensor,
                self_weight: Optional[torch.Tensor] = None, objective: str = "least_squares", lr: float = 0.01,
                P: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """One push-sum gradient-tracking round (ADD-OPT / Push-DIGing,
    dol_gt_push_csr_f32) on the agent-major bank, for weights that are
    column-stochastic only -- a directed graph, or the reference's
    row-stochastic W transposed -- where gt_csr settles at a biased point.  U
    the push-sum numerators, S the trackers, target the targets, [>= n, >= P]
    like gt_csr's X; v the push-sum weights, n floats; UO / SO / v_out receive
    u' / s' / v'.  C = C_off + diag(self_weight) is column-stochastic, C_off
    the square CSR whose row i lists i's in-neighbours
    (graph.push_sum_weights).  Per coordinate, all fp32, one rounding each
      au = mix of u, as = mix of s                     (mix_csr's sums)
      av = the same mix of the n-vector v
      au = fl(au + fl(d_i u_i)), as = fl(as + fl(d_i s_i)), av = fl(av + fl(d_i v_i))     with self_weight
      u' = fma(-lr, s_i, au)
      z = u_i / v_i;  z' = u' / av                     (correctly rounded divisions)
      s' = fl(fl(as + g(z', t_i)) - g(z, t_i));  v'_i = av
    with g the gradient separable_grad computes.  The estimate z = U / v is not
    stored.  Start from v = 1, U = x(0), S = g(x(0), t).  With v = 1 and av = 1
    in every row the bits of gt_csr.  The rules of this op are gt_csr's (a
    known objective; the four state matrices distinct; a self-weight vector of
    n floats; a square C) and: v and v_out are n float32 values on the device,
    and distinct.  Values are not checked: a zero v_i divides like IEEE.
    Returns (UO, SO, v_out)."""
    def distinct_v():
        if v is v_out or v.data_ptr() == v_out.data_ptr():
            raise ValueError("gt_push_csr: v and v_out alias: every v' reads its neighbours' v")

    call = _csr_round_args("gt_push_csr", (("U", U), ("S", S), ("UO", UO), ("SO", SO)), rowptr, col, val, target,
                           self_weight, objective, lr, P, vectors=(("v", v), ("v_out", v_out)), then=distinct_v)
    _native.call("dol_gt_push_csr_f32", *call, v.data_ptr(), v_out.data_ptr(), _ops._stream(U))
    return UO, SO, v_out


def gt_grad_csr(X: torch.Tensor, S: torch.Tensor, XO: torch.Tensor, SO: torch.Tensor, rowptr: torch.Tensor,
                col: torch.Tensor, val: torch.Tensor, G: torch.Tensor, Gprev: torch.Tensor,
                self_weight: Optional[torch.Tensor] = None, lr: float = 0.01,
                P: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """One gradient-tracking round on the agent-major bank with the gradient
    FED as a row matrix (dol_gt_grad_csr_f32), for agents whose gradients
    something else computes (BatchedMLP.forward_backward writes them into the
    bank's grad rows): X the parameters, S the trackers, G this round's
    gradients, Gprev the previous round's, [>= n, >= P] like gt_csr's X; XO / SO
    receive x' / s'.  W = W_off + diag(self_weight) as gt_csr's.  DIGing with
    the tracker update at the front of the round, per coordinate, all fp32, one
    rounding each
      ax = mix of x, as = mix of s                     (mix_csr's sums)
      ax = fl(ax + fl(d_i x_i)), as = fl(as + fl(d_i s_i))     with self_weight
      s' = fl(fl(as + g_i) - gprev_i);  x' = fma(-lr, s', ax)
    x' takes the agent's own new tracker, so the round is one pass.  Start from
    S = 0 and Gprev = 0 (the first round then gives s = G: no separate
    initialisation) and swap G and Gprev after every call.  The rules of this
    op are gt_csr's without an objective (the four state matrices distinct; a
    self-weight vector of n floats; a square W), with G and Gprev in target's
    place, and: neither G nor Gprev is XO or SO.  Returns (XO, SO)."""
    name = "gt_grad_csr"
    n = rowptr.shape[0] - 1
    state = (("X", X), ("S", S), ("XO", XO), ("SO", SO))
    _distinct_state(name, state)
    for ng, g in (("G", G), ("Gprev", Gprev)):
        for no, o in state[2:]:
            if g is o or (isinstance(g, torch.Tensor) and g.data_ptr() == o.data_ptr()):
                raise ValueError(f"{name}: {ng} and {no} alias: the gradient rows are read while the outputs are written")
    if self_weight is not None:
        _ops._check_array("self_weight", self_weight, torch.float32, n, X.device)
    P = X.shape[1] if P is None else P
    lds = _leading_dims(state + (("G", G),), ("Gprev", Gprev), P, n)
    _ops._check_csr(rowptr, col, val, X.device, same_length=False)
    _check_square(rowptr, col, n)
    rows = tuple(a for (_, t), ld in zip(state, lds) for a in (t.data_ptr(), ld))
    _native.call("dol_gt_grad_csr_f32", *rows, n, P, rowptr.data_ptr(), _ops._ptr_unless_empty(col),
                 _ops._ptr_unless_empty(val), _ops._ptr(self_weight), G.data_ptr(), lds[4], Gprev.data_ptr(), lds[5],
                 float(lr), _ops._stream(X))
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
