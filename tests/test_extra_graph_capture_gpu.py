"""dol_extra_csr_f32 and dol_extra_ring_f32 are stream-ordered and neither
allocate nor synchronise (like dol_gt_push_csr_f32,
tests/test_gt_push_graph_capture_gpu.py), so EXTRA rounds capture into a
hipGraph: three ping-pong rounds (X alternates between two buffers; the
correction is updated in place, so it is reset before every run) captured into
one graph on one stream and replayed give the eager rounds' bits, on the
XCD-pinned CSR kernel (n = 520, P = 1031: pinned tiles, a left-over f4 and a
scalar tail), on the small-n CSR kernel (n = 33, P = 7: scalar columns only)
and on the ring (n = 9, P = 1031).  One stream, no parallel branches."""
import pytest
import torch

import extra_cases as E
from gt_cases import csr_dev
from dolhip import ops

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("objective", ["least_squares", "logistic"])
@pytest.mark.parametrize("layout,n,P", [("csr", 520, 1031), ("csr", 33, 7), ("ring", 9, 1031)],
                         ids=["csr n=520 P=1031 pinned kernel", "csr n=33 P=7 small-n kernel", "ring n=9 P=1031"])
def test_three_captured_rounds_replay_bit_identically(layout, n, P, objective, gpu):
    if layout == "csr":
        c, d = E.metropolis_regular(n)
        w = csr_dev(c, gpu)
        op = ops.extra_csr
    else:
        _, d, wp, wn = E.metropolis_ring(n)
        w = (torch.as_tensor(wp, device=gpu), torch.as_tensor(wn, device=gpu))
        op = ops.extra_ring
    ws = torch.as_tensor(d, device=gpu)
    g = torch.Generator(device=gpu).manual_seed(5)
    ld = (P + 3) // 4 * 4 + 4
    X0, C0, T = (torch.randn(n, ld, generator=g, device=gpu)[:, :P] for _ in range(3))
    A = [torch.zeros(n, ld, device=gpu)[:, :P] for _ in range(3)]  # X, its partner, corr

    def reset():
        A[0].copy_(X0)
        A[1].zero_()
        A[2].copy_(C0)

    def rounds():
        x, y = A[0], A[1]
        for _ in range(3):
            op(x, y, *w, T, A[2], self_weight=ws, objective=objective, lr=0.1, P=P)
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
