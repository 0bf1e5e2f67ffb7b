"""dol_gt_ring_f32 is stream-ordered and neither allocates nor synchronises
(like the entries of tests/test_graph_capture_gpu.py), so a gradient-tracking
round on the ring captures into a hipGraph: one captured and replayed
ops.gt_ring call gives the eager call's bits, f4 body and scalar tail alike."""
import pytest
import torch

from dolhip import ops

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("objective", ["least_squares", "logistic"])
def test_captured_gt_ring_replays_bit_identically(objective, gpu):
    n, P = 9, 2055
    g = torch.Generator(device=gpu).manual_seed(5)
    X, S, T = (torch.randn(n, P + 1, generator=g, device=gpu)[:, :P] for _ in range(3))
    wp, wn, ws = (torch.rand(n, generator=g, device=gpu) for _ in range(3))
    XO, SO = torch.zeros(n, P + 1, device=gpu), torch.zeros(n, P + 1, device=gpu)

    def round_():
        ops.gt_ring(X, S, XO, SO, wp, wn, T, self_weight=ws, objective=objective, lr=0.1, P=P)

    round_()  # eager reference
    torch.cuda.synchronize()
    want = (XO.clone(), SO.clone())
    s = torch.cuda.Stream(device=gpu)
    s.wait_stream(torch.cuda.current_stream(gpu))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            round_()
    torch.cuda.current_stream(gpu).wait_stream(s)
    XO.zero_()  # capture does not execute; clear the eager result and replay
    SO.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert want[0].abs().sum() > 0
    for got, w in zip((XO, SO), want):
        assert torch.equal(got.view(torch.int32), w.view(torch.int32))
