"""ShardedRing.gt_step with the REAL HIP kernels on one GPU: 2 and 3 ranks on
cuda:0 under gloo, in the manner of
test_parallel_gpu.test_sharded_dgd_ring_real_kernels_on_one_gpu (the packed
halo rows of x and s are staged through host memory -- the only difference from
the RCCL path is the transport).  The interior rows go through dol_gt_ring_f32
with the block's own boundary rows as halos, the boundary rows through
dol_gt_ring_edges_f32 with the received ones; (3, 6) leaves two rows per rank,
so no interior launch.  The concatenated parameters and trackers after three
rounds carry the bits of tests/gt_cases.py::gt_round iterated on the whole
ring's CSR.  At world 1 gt_step is one ops.gt_ring call."""
import numpy as np
import pytest
import torch

import extra_cases as E
import gt_cases
import gt_sharded_cases as C
from gt_cases import same_bits
from oracle import bits_equal
from dolhip import ops, parallel

pytestmark = pytest.mark.gpu

P, ROUNDS, LR = 4096 + 12, 3, 0.1


def _rounds(N):
    """This rank's rank and its rows of (x, s) after ROUNDS gt_step rounds on cuda:0."""
    dev = torch.device("cuda:0")
    _, d, wp, wn = E.metropolis_ring(N)
    X, S, T = gt_cases.problem(N, P, 13)
    sh = parallel.ShardedRing(N, P, wp, wn, dev)
    rows = slice(sh.lo, sh.hi)
    sh.x[:, :P] = torch.from_numpy(X[rows]).to(dev)
    s, t, dl = (torch.from_numpy(np.ascontiguousarray(a[rows])).to(dev) for a in (S, T, d))
    s_out = torch.zeros_like(s)
    for _ in range(ROUNDS):
        s, s_out = sh.gt_step(s, s_out, t, dl, lr=LR)
    torch.cuda.synchronize()
    return sh.rank, sh.x[:, :P].cpu().numpy(), s.cpu().numpy()


@pytest.mark.parametrize("world,N", [(2, 64), (3, 50), (3, 6)])
def test_sharded_gt_ring_real_kernels_on_one_gpu(world, N):
    c, d = E.metropolis_ring(N)[:2]
    want_x, want_s = C.unsharded(*gt_cases.problem(N, P, 13), c, d, LR, ROUNDS)
    res = sorted(C.spawn(_rounds, world, N, timeout=240), key=lambda r: r[0])
    assert bits_equal(np.concatenate([r[1] for r in res]), want_x)
    assert bits_equal(np.concatenate([r[2] for r in res]), want_s)


def test_gt_step_at_world_one_is_the_ring_op(gpu):
    N = 9
    _, d, wp, wn = E.metropolis_ring(N)
    X, S, T = gt_cases.problem(N, P, 13)
    sh = parallel.ShardedRing(N, P, wp, wn, gpu)
    assert sh.world == 1
    sh.x[:, :P] = torch.from_numpy(X).to(gpu)
    s, t, dl = (torch.from_numpy(a).to(gpu) for a in (S, T, d))
    s_out = torch.zeros_like(s)
    XO, SO = torch.zeros(N, P, device=gpu), torch.zeros(N, P, device=gpu)
    ops.gt_ring(sh.x, s, XO, SO, sh.w_prev, sh.w_next, t, self_weight=dl, lr=LR, P=P)
    x_before = sh.x
    got_s, got_s_out = sh.gt_step(s, s_out, t, dl, lr=LR)
    torch.cuda.synchronize()
    assert got_s is s_out and got_s_out is s and sh.y is x_before
    assert same_bits(sh.x[:, :P].contiguous(), XO) and same_bits(got_s, SO)
