"""dol_gt_grad_csr_f32 and dol_extra_grad_csr_f32 are stream-ordered and neither
allocate nor synchronise (like dol_gt_csr_f32,
tests/test_gt_csr_graph_capture_gpu.py), so a gradient-fed round captures into
a hipGraph: one captured and replayed call of each op gives the eager call's
bits, on the XCD-pinned kernel (n = 520) and on the small-n kernel (n = 17), f4
body and scalar tail alike.  One stream, no parallel branches."""
import numpy as np
import pytest
import torch

from dolhip import graph as G
from dolhip import ops

pytestmark = pytest.mark.gpu


def _capture_and_replay(gpu, round_, outputs):
    round_()  # eager reference (and the square-W check, which reads the indices back once)
    torch.cuda.synchronize()
    want = [t.clone() for t in outputs]
    s = torch.cuda.Stream(device=gpu)
    s.wait_stream(torch.cuda.current_stream(gpu))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            round_()
    torch.cuda.current_stream(gpu).wait_stream(s)
    return graph, want


def _problem(n, P, gpu, count):
    c = G.random_regular_csr(n, 4, seed=n + 3)
    csr = tuple(torch.as_tensor(np.asarray(a, t), device=gpu) for a, t in
                ((c.rowptr, np.int32), (c.col, np.int32), (c.val, np.float32)))
    g = torch.Generator(device=gpu).manual_seed(5)
    mats = [torch.randn(n, P + 1, generator=g, device=gpu)[:, :P] for _ in range(count)]
    return csr, mats, torch.rand(n, generator=g, device=gpu)


@pytest.mark.parametrize("self_w", [False, True], ids=["no self weights", "self weights"])
@pytest.mark.parametrize("n", [520, 17], ids=["n=520 pinned kernel", "n=17 small-n kernel"])
def test_captured_gt_grad_csr_replays_bit_identically(n, self_w, gpu):
    P = 1031
    (rp, col, val), (X, S, Gr, Gp), ws = _problem(n, P, gpu, 4)
    XO, SO = torch.zeros(n, P + 1, device=gpu), torch.zeros(n, P + 1, device=gpu)

    def round_():
        ops.gt_grad_csr(X, S, XO, SO, rp, col, val, Gr, Gp, self_weight=ws if self_w else None, lr=0.1, P=P)

    graph, want = _capture_and_replay(gpu, round_, (XO, SO))
    XO.zero_()  # capture does not execute; clear the eager result and replay
    SO.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert want[0].abs().sum() > 0
    for got, w in zip((XO, SO), want):
        assert torch.equal(got.view(torch.int32), w.view(torch.int32))


@pytest.mark.parametrize("self_w", [False, True], ids=["no self weights", "self weights"])
@pytest.mark.parametrize("n", [520, 17], ids=["n=520 pinned kernel", "n=17 small-n kernel"])
def test_captured_extra_grad_csr_replays_bit_identically(n, self_w, gpu):
    P = 1031
    (rp, col, val), (X, Gr, C0), ws = _problem(n, P, gpu, 3)
    Y, corr = torch.zeros(n, P + 1, device=gpu), torch.zeros(n, P + 1, device=gpu)
    corr[:, :P] = C0

    def round_():
        ops.extra_grad_csr(X, Y, rp, col, val, Gr, corr, self_weight=ws if self_w else None, lr=0.1, P=P)

    graph, want = _capture_and_replay(gpu, round_, (Y, corr))
    Y.zero_()
    corr[:, :P] = C0  # corr is updated in place: restore the round's input before the replay
    graph.replay()
    torch.cuda.synchronize()
    assert want[0].abs().sum() > 0
    for got, w in zip((Y, corr), want):
        assert torch.equal(got.view(torch.int32), w.view(torch.int32))
