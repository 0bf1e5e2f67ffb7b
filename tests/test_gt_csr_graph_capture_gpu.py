"""dol_gt_csr_f32 is stream-ordered and neither allocates nor synchronises
(like the entries of tests/test_graph_capture_gpu.py), so a gradient-tracking
round on the agent-major CSR bank captures into a hipGraph: one captured and
replayed ops.gt_csr call gives the eager call's bits, on the XCD-pinned kernel
(n = 520) and on the small-n kernel (n = 17), f4 body and scalar tail alike.
One stream, no parallel branches."""
import numpy as np
import pytest
import torch

from dolhip import graph as G
from dolhip import ops

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("objective", ["least_squares", "logistic"])
@pytest.mark.parametrize("n", [520, 17], ids=["n=520 pinned kernel", "n=17 small-n kernel"])
def test_captured_gt_csr_replays_bit_identically(n, objective, gpu):
    P = 1031
    c = G.random_regular_csr(n, 4, seed=n + 3)
    rp, col, val = (torch.as_tensor(np.asarray(a, t), device=gpu) for a, t in
                    ((c.rowptr, np.int32), (c.col, np.int32), (c.val, np.float32)))
    g = torch.Generator(device=gpu).manual_seed(5)
    X, S, T = (torch.randn(n, P + 1, generator=g, device=gpu)[:, :P] for _ in range(3))
    ws = torch.rand(n, generator=g, device=gpu)
    XO, SO = torch.zeros(n, P + 1, device=gpu), torch.zeros(n, P + 1, device=gpu)

    def round_():
        ops.gt_csr(X, S, XO, SO, rp, col, val, T, self_weight=ws, objective=objective, lr=0.1, P=P)

    round_()  # eager reference (and the square-W check, which reads the indices back once)
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
