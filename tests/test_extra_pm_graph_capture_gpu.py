"""dol_extra_csr_pm_ex_f32 is stream-ordered and neither allocates nor
synchronises (like dol_extra_csr_f32, tests/test_extra_graph_capture_gpu.py), so
EXTRA rounds on the parameter-major bank capture into a hipGraph: three
ping-pong rounds under an explicit stage order (nseg = 8: nothing is tuned
inside the capture; XT alternates between two buffers; the correction is
updated in place, so it is reset before every run) captured into one graph on
one stream and replayed give the eager rounds' bits.  1000 agents (a dead quad
lane group beside the live ones) x 777 p-rows (a ragged last stage).  One
stream, no parallel branches."""
import pytest
import torch

import extra_cases as E
from gt_cases import csr_dev
from dolhip import ops

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("objective", ["least_squares", "logistic"])
def test_three_captured_rounds_replay_bit_identically(objective, gpu):
    n, P = 1000, 777
    c, d = E.metropolis_regular(n)
    w = csr_dev(c, gpu)
    ws = torch.as_tensor(d, device=gpu)
    g = torch.Generator(device=gpu).manual_seed(5)
    ld = (n + 3) // 4 * 4 + 4
    X0, C0, T = (torch.randn(P, ld, generator=g, device=gpu)[:, :n] for _ in range(3))
    A = [torch.zeros(P, ld, device=gpu)[:, :n] for _ in range(3)]  # XT, its partner, corr

    def reset():
        A[0].copy_(X0)
        A[1].zero_()
        A[2].copy_(C0)

    def rounds():
        x, y = A[0], A[1]
        for _ in range(3):
            ops.extra_csr_pm(x, y, *w, T, A[2], self_weight=ws, objective=objective, lr=0.1, nseg=8)
            x, y = y, x
        return x  # after three rounds: A[1]

    reset()
    out = rounds()  # eager reference (and the square-W check, which reads the indices back once)
    torch.cuda.synchronize()
    assert out is A[1]
    want = [out.clone(), A[2].clone()]
    reset()
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=gpu)
    s.wait_stream(torch.cuda.current_stream(gpu))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            rounds()
    torch.cuda.current_stream(gpu).wait_stream(s)
    reset()  # capture does not execute; restore the start state (corr among it) and replay
    graph.replay()
    torch.cuda.synchronize()
    assert want[0].abs().sum() > 0 and not torch.equal(want[1], C0)
    for got, w_ in zip((out, A[2]), want):
        assert torch.equal(got.view(torch.int32), w_.view(torch.int32))
    reset()  # and once more: the correction starts from C0 again
    graph.replay()
    torch.cuda.synchronize()
    for got, w_ in zip((out, A[2]), want):
        assert torch.equal(got.view(torch.int32), w_.view(torch.int32))
