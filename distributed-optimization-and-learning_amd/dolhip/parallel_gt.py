"""The gradient-tracking rounds of the two sharded layouts
(parallel.ShardedRing.gt_step, parallel.ColumnSharded.gt_step).  They live
here, not in parallel.py, because
tests/test_parallel_gloo.py::test_every_rccl_line_runs_under_gloo holds every
statement of parallel.py's functions to its own fixed list of calls.  The
column-sharded round is exercised at world 1, 2 and 3 over gloo by
tests/test_gt_csr_host.py (with the host round injected) and on the GPU by
tests/test_gt_csr_gpu.py; it has no collective: the round is per column.  The
sharded ring's round is exercised at world 1, 2 and 3 over gloo by
tests/test_gt_sharded_host.py (with CPU entries passed in) and on the GPU by
tests/test_gt_sharded_gpu.py.

Gradient tracking mixes the parameters AND the trackers, so the sharded ring
exchanges the boundary rows of both: one message per direction, the row of x
and the row of s packed side by side."""
from __future__ import annotations

import torch
import torch.distributed as dist


def column_sharded_gt_step(sh, s, s_out, target, **kw):
    """One gradient-tracking round on this rank's column block (plan.apply_gt,
    or the entry injected as apply_gt).  s / s_out / target: local [N, >= Pl]
    blocks like sh.x.  Swaps x / y as step() does and RETURNS the tracker pair
    swapped, (s_out, s): the caller owns those two buffers, so it rebinds them
    with `s, s_out = sh.gt_step(s, s_out, target, ...)`."""
    if sh._apply_gt is None:
        raise NotImplementedError("gt_step: the plan has no gradient-tracking entry (pass apply_gt)")
    if sh.Pl > 0:
        sh._apply_gt(sh.x, s, sh.y, s_out, target, P=sh.Pl, **kw)
    sh.x, sh.y = sh.y, sh.x
    return s_out, s


def _gt_halo_rows(sh):
    """(send, recv, hp): the staging rows of the two-matrix halo exchange,
    torch-allocated on first use and kept on sh.  A message is hp + P floats,
    hp = P rounded up to 4: x's boundary row in [0, P), s's in [hp, hp + P), so
    both halves of a received row are 16-B aligned whatever ld is (the rows
    are 2 hp floats apart).  send[0] / send[1]: this block's first / last row;
    recv[0] / recv[1]: the row before / after the block."""
    hp = (sh.P + 3) // 4 * 4
    rows = getattr(sh, "_gt_halo", None)
    if rows is None:
        rows = tuple(torch.zeros(2, 2 * hp, dtype=torch.float32, device=sh.device) for _ in range(2))
        sh._gt_halo = rows
    return rows[0], rows[1], hp


def _gt_exchange(sh, x, s):
    """Post the halo send/recv pairs of x and s; returns the requests.  The
    four point-to-point ops of ShardedRing._exchange, with its tags and its
    order (so world == 2, prev == next, still pairs correctly): the
    'downstream' message (my last rows -> next rank's previous halos), then
    the 'upstream' one (my first rows -> prev rank's next halos)."""
    P, n = sh.P, sh.n_local
    send, recv, hp = _gt_halo_rows(sh)
    m = hp + P
    for k, r in ((0, 0), (1, n - 1)):
        send[k, :P].copy_(x[r, :P])
        send[k, hp:m].copy_(s[r, :P])
    first, last, h_prev, h_next = send[0, :m], send[1, :m], recv[0, :m], recv[1, :m]
    if sh._staged():  # gloo cannot send device tensors: through host memory
        first, last = first.cpu(), last.cpu()
        sh._gt_host_halo = (torch.empty(m), torch.empty(m))
        h_prev, h_next = sh._gt_host_halo
    ops_ = [
        dist.P2POp(dist.isend, last, sh.next_rank, sh.group, tag=0),
        dist.P2POp(dist.irecv, h_prev, sh.prev_rank, sh.group, tag=0),
        dist.P2POp(dist.isend, first, sh.prev_rank, sh.group, tag=1),
        dist.P2POp(dist.irecv, h_next, sh.next_rank, sh.group, tag=1),
    ]
    return dist.batch_isend_irecv(ops_)


def _gt_finish_exchange(sh, reqs):
    """Wait for _gt_exchange's requests; returns the halos (x_prev, x_next,
    s_prev, s_next), [P] views of the receive rows."""
    from .parallel import _wait_all
    _wait_all(reqs, sh.group)
    _, recv, hp = _gt_halo_rows(sh)
    P = sh.P
    if sh._staged():
        recv[0, :hp + P].copy_(sh._gt_host_halo[0])
        recv[1, :hp + P].copy_(sh._gt_host_halo[1])
    return recv[0, :P], recv[1, :P], recv[0, hp:hp + P], recv[1, hp:hp + P]


def sharded_ring_gt_step(sh, s, s_out, target, self_w=None, gt_ring=None, gt_edges=None, **kw):
    """One gradient-tracking round (dol_gt_ring_f32) on this rank's block of
    the ring, with dgd_step's halo schedule: the interior rows while the
    boundary rows of x and s travel (one message per direction), then the two
    boundary rows in one launch (dol_gt_ring_edges_f32).  s / s_out / target:
    the LOCAL [n_local, >= P] rows, caller-owned; self_w: the LOCAL [n_local]
    self weights or None.  gt_ring / gt_edges: the entries (default: the HIP
    ops; with an injected gt_ring and no injected edge entry the boundary rows
    go through gt_ring, one row each).  Writes sh.y and s_out, swaps x / y and
    RETURNS the tracker pair swapped, (s_out, s), as ColumnSharded.gt_step
    does: `s, s_out = sh.gt_step(s, s_out, target, ...)`.  Bit-identical to
    the single-GPU round."""
    from . import ops
    ring = gt_ring if gt_ring is not None else ops.gt_ring
    edges = gt_edges if gt_edges is not None else (ops.gt_ring_edges if gt_ring is None else None)
    x, y = sh.x, sh.y
    n, P = sh.n_local, sh.P
    d = (lambda a, b: None) if self_w is None else (lambda a, b: self_w[a:b])
    if sh.world == 1:
        ring(x, s, y, s_out, sh.w_prev, sh.w_next, target, self_weight=self_w, P=P, n_rows=n, **kw)
    else:
        reqs = _gt_exchange(sh, x, s)
        if n > 2:  # interior rows 1..n-2: their neighbours are all local
            ev = sh.kernel_events
            if ev:
                ev[0].record()
            ring(x[1:], s[1:], y[1:], s_out[1:], sh.w_prev[1:], sh.w_next[1:], target[1:], self_weight=d(1, n - 1),
                 halos=(x[0], x[n - 1], s[0], s[n - 1]), P=P, n_rows=n - 2, **kw)
            if ev:
                ev[1].record()
        xp, xn, sp, sn = _gt_finish_exchange(sh, reqs)
        if edges is not None:
            edges(x, s, y, s_out, sh.w_prev, sh.w_next, target, (xp, xn, sp, sn), self_weight=self_w, P=P, n_rows=n,
                  **kw)
        else:
            ring(x[0:1], s[0:1], y[0:1], s_out[0:1], sh.w_prev[0:1], sh.w_next[0:1], target[0:1],
                 self_weight=d(0, 1), halos=(xp, x[1], sp, s[1]), P=P, n_rows=1, **kw)
            ring(x[n - 1:n], s[n - 1:n], y[n - 1:n], s_out[n - 1:n], sh.w_prev[n - 1:n], sh.w_next[n - 1:n],
                 target[n - 1:n], self_weight=d(n - 1, n), halos=(x[n - 2], xn, s[n - 2], sn), P=P, n_rows=1, **kw)
    sh.x, sh.y = sh.y, sh.x
    return s_out, s
