"""What the two tiers of the sharded ring's gradient-tracking round share
(tests/test_gt_sharded_host.py, tests/test_gt_sharded_gpu.py): CPU entries
with the signatures of ops.gt_ring and ops.gt_ring_edges, built like
extra_cases.cpu_extra_ring from oracle.mix_ring with halos (the ring mix's
rounding) and gt_cases' single-rounding pieces; the restatement iterated on the
whole ring's CSR; and the process plumbing of the gloo runs."""
import os
import socket

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import gt_cases
import oracle
from gt_cases import F32, add_self, ls_grad, sgd_step


def _np(t, rows, P):
    return np.ascontiguousarray(t[:rows, :P].numpy())


def cpu_gt_ring(X, S, XO, SO, w_prev, w_next, target, self_weight=None, objective="least_squares", lr=0.01,
                halos=None, P=None, n_rows=None):
    """ops.gt_ring on CPU tensors: oracle.mix_ring over X and over S, then
    gt_cases.gt_round's finish (add_self, sgd_step, two float32 operations)."""
    assert objective == "least_squares"
    n = n_rows
    x, s, t = (_np(A, n, P) for A in (X, S, target))
    xp, xn, sp, sn = (None,) * 4 if halos is None else (h[:P].numpy() for h in halos)
    wp, wn = w_prev[:n].numpy(), w_next[:n].numpy()
    d = None if self_weight is None else self_weight[:n].numpy()
    ax = add_self(oracle.mix_ring(x, wp, wn, xp, xn), d, x)
    as_ = add_self(oracle.mix_ring(s, wp, wn, sp, sn), d, s)
    xo = sgd_step(ax, s, lr)
    so = ((as_ + ls_grad(xo, t)).astype(F32) - ls_grad(x, t)).astype(F32)
    XO[:n, :P] = torch.from_numpy(xo)
    SO[:n, :P] = torch.from_numpy(so)
    return XO, SO


def cpu_gt_ring_edges(X, S, XO, SO, w_prev, w_next, target, halos, self_weight=None, objective="least_squares",
                      lr=0.01, P=None, n_rows=None):
    """ops.gt_ring_edges on CPU tensors: rows 0 and n_rows - 1 only."""
    n = n_rows
    xp, xn, sp, sn = halos
    d = (lambda a, b: None) if self_weight is None else (lambda a, b: self_weight[a:b])
    for r in ([0] if n == 1 else [0, n - 1]):
        h = (xp if r == 0 else X[r - 1], xn if r == n - 1 else X[r + 1],
             sp if r == 0 else S[r - 1], sn if r == n - 1 else S[r + 1])
        cpu_gt_ring(X[r:r + 1], S[r:r + 1], XO[r:r + 1], SO[r:r + 1], w_prev[r:r + 1], w_next[r:r + 1],
                    target[r:r + 1], self_weight=d(r, r + 1), objective=objective, lr=lr, halos=h, P=P, n_rows=1)
    return XO, SO


def unsharded(X, S, T, c, d, lr, rounds):
    """(X, S) after `rounds` rounds of gt_cases.gt_round on the whole ring's CSR."""
    for _ in range(rounds):
        X, S = gt_cases.gt_round(X, S, T, c, d, lr)
    return X, S


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def gloo_worker(rank, world, port, body, args, q):
    """body(*args) under a gloo group of `world` ranks; its result goes to q."""
    from dolhip import parallel
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    parallel.init_process_group("gloo", rank=rank, world_size=world, timeout_s=120)
    try:
        q.put(body(*args))
    finally:
        dist.destroy_process_group()


def spawn(body, world, *args, timeout=120):
    """body(*args) on `world` spawned gloo ranks; the results in arrival order."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=gloo_worker, args=(r, world, port, body, args, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=timeout) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return res


class CountedBatches:
    """dist.batch_isend_irecv wrapped: the (op count, [floats per op]) of every call."""

    def __init__(self):
        self.calls = []
        self._real = dist.batch_isend_irecv

    def __enter__(self):
        def counted(ops_):
            self.calls.append((len(ops_), [int(o.tensor.numel()) for o in ops_]))
            return self._real(ops_)
        dist.batch_isend_irecv = counted
        return self

    def __exit__(self, *exc):
        dist.batch_isend_irecv = self._real
        return False
