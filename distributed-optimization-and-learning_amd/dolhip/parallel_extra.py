"""The EXTRA rounds of the two sharded layouts (parallel.ShardedRing.extra_step,
parallel.ColumnSharded.extra_step).  They live here, not in parallel.py, for
parallel_gt.py's reason: tests/test_parallel_gloo.py::
test_every_rccl_line_runs_under_gloo holds every statement of parallel.py's
functions to its own fixed list of calls.  Both are exercised over gloo by
tests/test_extra_host.py (with CPU entries passed in) and on the GPU by
tests/test_extra_csr_gpu.py.  The kernel entry is resolved inside each
function: the HIP op (or the plan's apply_extra), or the entry passed in.

EXTRA mixes the parameters only, so the sharded ring exchanges exactly the
halo rows dgd_step exchanges; the corrections and targets never leave their
rank."""
from __future__ import annotations


def sharded_ring_extra_step(sh, target, corr, self_w=None, extra_ring=None, extra_edges=None, **kw):
    """One EXTRA round (dol_extra_ring_f32) on this rank's block of the ring,
    with dgd_step's halo schedule: the interior rows while the halo rows of x
    travel, then the two boundary rows in one launch.  target / corr: the LOCAL
    [n_local, >= P] rows (corr updated in place, zero before the first round);
    self_w: the LOCAL [n_local] self weights or None.  extra_ring / extra_edges:
    the entries (default: the HIP ops; with an injected extra_ring and no
    injected edge entry the boundary rows go through extra_ring, one row each).
    Swaps x / y; bit-identical to the single-GPU round."""
    from . import ops
    ring = extra_ring if extra_ring is not None else ops.extra_ring
    edges = extra_edges if extra_edges is not None else (ops.extra_ring_edges if extra_ring is None else None)
    x, y = sh.x, sh.y
    n, P = sh.n_local, sh.P
    d = (lambda a, b: None) if self_w is None else (lambda a, b: self_w[a:b])
    if sh.world == 1:
        ring(x, y, sh.w_prev, sh.w_next, target, corr, self_weight=self_w, P=P, n_rows=n, **kw)
    else:
        reqs = sh._exchange(x)
        if n > 2:  # interior rows 1..n-2: their neighbours are all local
            ring(x[1:], y[1:], sh.w_prev[1:], sh.w_next[1:], target[1:], corr[1:], self_weight=d(1, n - 1),
                 halo_prev=x[0], halo_next=x[n - 1], P=P, n_rows=n - 2, **kw)
        sh._finish_exchange(reqs)
        if edges is not None:
            edges(x, y, sh.w_prev, sh.w_next, target, corr, sh.halo_prev, sh.halo_next, self_weight=self_w, P=P,
                  n_rows=n, **kw)
        else:
            ring(x[0:1], y[0:1], sh.w_prev[0:1], sh.w_next[0:1], target[0:1], corr[0:1], self_weight=d(0, 1),
                 halo_prev=sh.halo_prev, halo_next=x[1], P=P, n_rows=1, **kw)
            ring(x[n - 1:n], y[n - 1:n], sh.w_prev[n - 1:n], sh.w_next[n - 1:n], target[n - 1:n], corr[n - 1:n],
                 self_weight=d(n - 1, n), halo_prev=x[n - 2], halo_next=sh.halo_next, P=P, n_rows=1, **kw)
    sh.x, sh.y = sh.y, sh.x


def column_sharded_extra_step(sh, target, corr, apply_extra=None, **kw):
    """One EXTRA round on this rank's column block (the plan's apply_extra, or
    the entry passed as apply_extra).  target / corr: local [N, >= Pl] blocks
    like sh.x (corr updated in place).  No collective: the round is per
    column.  Swaps x / y as step() does."""
    entry = apply_extra if apply_extra is not None else sh.plan.apply_extra
    if sh.Pl > 0:
        entry(sh.x, sh.y, target, corr, P=sh.Pl, **kw)
    sh.x, sh.y = sh.y, sh.x
