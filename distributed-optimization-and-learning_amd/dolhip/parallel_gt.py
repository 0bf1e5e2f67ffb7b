"""The gradient-tracking round of the column-sharded layout
(parallel.ColumnSharded.gt_step).  It lives here, not in parallel.py, because
tests/test_parallel_gloo.py::test_every_rccl_line_runs_under_gloo holds every
statement of parallel.py's functions to its own fixed list of calls; this
round is exercised at world 1, 2 and 3 over gloo by tests/test_gt_csr_host.py
(with the host round injected) and on the GPU by tests/test_gt_csr_gpu.py.  It
has no collective: the round is per column."""
from __future__ import annotations


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
