"""dol_gt_push_csr_f32 is stream-ordered and neither allocates nor synchronises
(like dol_gt_csr_f32, tests/test_gt_csr_graph_capture_gpu.py), so push-sum
gradient-tracking rounds capture into a hipGraph: three ping-pong rounds (U, S
and v each alternate between two buffers; every round is the small v' kernel
followed by the main kernels) captured into one graph on one stream and
replayed give the eager rounds' bits, on the XCD-pinned kernel (n = 520, P =
1031: pinned tiles, a left-over f4 and a scalar tail) and on the small-n kernel
(n = 33, P = 7: scalar columns only).  One stream, no parallel branches."""
import numpy as np
import pytest
import torch

import gt_push_cases
from dolhip import graph as G
from dolhip import ops

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("objective", ["least_squares", "logistic"])
@pytest.mark.parametrize("n,P", [(520, 1031), (33, 7)], ids=["n=520 P=1031 pinned kernel", "n=33 P=7 small-n kernel"])
def test_three_captured_rounds_replay_bit_identically(n, P, objective, gpu):
    c, d = G.push_sum_weights(gt_push_cases.digraph(n))
    rp, col, val = (torch.as_tensor(np.asarray(a, t), device=gpu) for a, t in
                    ((c.rowptr, np.int32), (c.col, np.int32), (c.val, np.float32)))
    ws = torch.as_tensor(d, device=gpu)
    g = torch.Generator(device=gpu).manual_seed(5)
    ld = (P + 3) // 4 * 4 + 4
    U0, S0, T = (torch.randn(n, ld, generator=g, device=gpu)[:, :P] for _ in range(3))
    v0 = torch.linspace(0.5, 2.0, n, device=gpu)
    A = [torch.zeros(n, ld, device=gpu)[:, :P] for _ in range(4)]  # U, S and their partners
    V = [torch.zeros(n, device=gpu) for _ in range(2)]

    def reset():
        A[0].copy_(U0)
        A[1].copy_(S0)
        A[2].zero_()
        A[3].zero_()
        V[0].copy_(v0)
        V[1].zero_()

    def rounds():
        u, s, uo, so, v, vo = A[0], A[1], A[2], A[3], V[0], V[1]
        for _ in range(3):
            ops.gt_push_csr(u, s, uo, so, rp, col, val, T, v, vo, self_weight=ws, objective=objective, lr=0.1, P=P)
            u, uo, s, so, v, vo = uo, u, so, s, vo, v
        return u, s, v  # after three rounds: A[2], A[3], V[1]

    reset()
    out = rounds()  # eager reference (and the square-W check, which reads the indices back once)
    torch.cuda.synchronize()
    assert out[0] is A[2] and out[1] is A[3] and out[2] is V[1]
    want = [t.clone() for t in out]
    reset()
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=gpu)
    s.wait_stream(torch.cuda.current_stream(gpu))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            rounds()
    torch.cuda.current_stream(gpu).wait_stream(s)
    reset()  # capture does not execute; restore the start state and replay
    graph.replay()
    torch.cuda.synchronize()
    assert want[0].abs().sum() > 0 and not torch.equal(want[2], v0)
    for got, w in zip(out, want):
        assert torch.equal(got.view(torch.int32), w.view(torch.int32))
