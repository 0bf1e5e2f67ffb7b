"""The EXTRA round on the agent-major ring (dol_extra_ring_f32,
dol_extra_ring_edges_f32, ops.extra_ring, ops.extra_ring_edges,
MixingPlan.apply_extra on a ring plan).

Least squares is bit-exact against tests/extra_cases.py::extra_round on the
ring's CSR (the reference's stochastic circle W: unequal weights, so a swapped
neighbour shows), with a nonzero correction.  The round runs ring.hip's mixing
kernels with the ExtraEpi epilogue (4-row LDS-DMA tiles of 256 f4 columns;
4-row register tiles for scalar columns):
  n  3 fewer rows than a tile, 4 one tile, 5 / 7 / 9 ragged tiles;
  P  1 and 7 scalar tail only, 1024 one full column tile, 1031 a full tile then
     one f4 and a 3-float tail, 2055 two tiles and a partial one.
Split rings: the 9-agent ring cut into blocks, each block one halo-form call
(one- and two-row blocks among them), or its interior rows through the halo
form and its two boundary rows through the edges entry, give the bits of the
wrap-around call, for both objectives.  The same bits as ops.extra_csr on the
ring's CSR for both objectives, and a ring plan and a CSR plan of one W agree
through apply_extra."""
import functools

import numpy as np
import pytest
import torch

import extra_cases as E
from gt_cases import csr_dev, logistic_problem, padded, problem, ring, same_bits
from oracle import bits_equal
from dolhip import graph as G
from dolhip import ops

pytestmark = pytest.mark.gpu

F32 = np.float32


def run_ring(X, C, T, wp, wn, ws, gpu, objective="least_squares", lr=0.1, blocks=None, edges=False):
    """One round through ops.extra_ring on host X, C, T [n, P]; returns host
    (X', C').  blocks: the ring cut at these row bounds, with the neighbouring
    blocks' boundary rows as halos; each block is one halo-form call, or
    (edges) its interior rows through the halo form and rows 0 and b - a - 1
    through ops.extra_ring_edges.  None: the wrap-around call.  The padding
    columns and guard rows of Y and corr must still hold 7.0 and X and T must
    be untouched."""
    n, P = X.shape
    ld = (P + 3) // 4 * 4
    Xd, Td = (padded(A, ld, gpu) for A in (X, T))
    keep = [t.clone() for t in (Xd, Td)]
    YG, CG = (torch.full((n + 2, ld), 7.0, device=gpu) for _ in range(2))
    Y, Cd = YG[1:n + 1], CG[1:n + 1]
    Cd[:, :P] = torch.as_tensor(C, device=gpu)
    wpd, wnd = torch.as_tensor(wp, device=gpu), torch.as_tensor(wn, device=gpu)
    wsd = None if ws is None else torch.as_tensor(ws, device=gpu)
    cut = lambda a, b: None if wsd is None else wsd[a:b]  # noqa: E731
    kw = dict(objective=objective, lr=lr, P=P)
    if blocks is None:
        assert ops.extra_ring(Xd, Y, wpd, wnd, Td, Cd, self_weight=wsd, **kw) is Y
    else:
        for a, b in zip(blocks[:-1], blocks[1:]):
            hp, hn = Xd[(a - 1) % n, :P], Xd[b % n, :P]
            if not edges:
                ops.extra_ring(Xd[a:b], Y[a:b], wpd[a:b], wnd[a:b], Td[a:b], Cd[a:b], self_weight=cut(a, b),
                               halo_prev=hp, halo_next=hn, n_rows=b - a, **kw)
                continue
            if b - a > 2:
                ops.extra_ring(Xd[a + 1:b - 1], Y[a + 1:b - 1], wpd[a + 1:b - 1], wnd[a + 1:b - 1], Td[a + 1:b - 1],
                               Cd[a + 1:b - 1], self_weight=cut(a + 1, b - 1), halo_prev=Xd[a, :P],
                               halo_next=Xd[b - 1, :P], n_rows=b - a - 2, **kw)
            ops.extra_ring_edges(Xd[a:b], Y[a:b], wpd[a:b], wnd[a:b], Td[a:b], Cd[a:b], hp, hn, self_weight=cut(a, b),
                                 n_rows=b - a, **kw)
    torch.cuda.synchronize()
    for G_ in (YG, CG):
        assert (G_[0] == 7.0).all() and (G_[n + 1] == 7.0).all(), "wrote into a guard row"
        assert (G_[:, P:] == 7.0).all(), "wrote past column P"
    for t, k in zip((Xd, Td), keep):
        assert same_bits(t, k), "an input changed"
    return Y[:, :P].cpu().numpy(), Cd[:, :P].cpu().numpy()


@functools.lru_cache(maxsize=None)
def ls_case(n, P, self_w):
    c, wp, wn, d = ring(n)
    d = d if self_w else None
    X, C, T = problem(n, P, 7 * n + P)
    return X, C, T, wp, wn, d, E.extra_round(X, C, T, c, d, 0.1)


@pytest.mark.parametrize("self_w", [False, True], ids=["no self weights", "self weights"])
@pytest.mark.parametrize("P", [1, 7, 1024, 1031, 2055])
@pytest.mark.parametrize("n", [3, 4, 5, 7, 9])
def test_least_squares_vs_host_restatement(n, P, self_w, gpu):
    X, C, T, wp, wn, d, (want_x, want_c) = ls_case(n, P, self_w)
    got_x, got_c = run_ring(X, C, T, wp, wn, d, gpu)
    assert bits_equal(got_x, want_x)
    assert bits_equal(got_c, want_c)


@pytest.mark.parametrize("edges", [False, True], ids=["halo form", "interior + edges entry"])
@pytest.mark.parametrize("blocks", [(0, 4, 9), (0, 1, 3, 9), (0, 2, 3, 8, 9)],
                         ids=["[0,4) [4,9)", "1, 2 and 6 rows", "2, 1, 5 and 1 rows"])
@pytest.mark.parametrize("P", [1031, 7])
@pytest.mark.parametrize("self_w", [False, True], ids=["no self weights", "self weights"])
def test_split_ring_equals_the_wrap_around_call(self_w, P, blocks, edges, gpu):
    X, C, T, wp, wn, d, (want_x, want_c) = ls_case(9, P, self_w)
    whole = run_ring(X, C, T, wp, wn, d, gpu)
    parts = run_ring(X, C, T, wp, wn, d, gpu, blocks=blocks, edges=edges)
    assert bits_equal(parts[0], whole[0]) and bits_equal(parts[1], whole[1])
    assert bits_equal(parts[0], want_x) and bits_equal(parts[1], want_c)


@pytest.mark.parametrize("self_w", [False, True], ids=["no self weights", "self weights"])
@pytest.mark.parametrize("objective", ["least_squares", "logistic"])
@pytest.mark.parametrize("n", [9, 64])
def test_same_bits_as_the_csr_round_on_the_rings_csr(n, objective, self_w, gpu):
    c, wp, wn, d = ring(n)
    d = d if self_w else None
    P = 1031
    X, C, T = logistic_problem(n, P)
    got_x, got_c = run_ring(X, C, T, wp, wn, d, gpu, objective=objective)
    Xd, Td, Cd = (padded(A, 1032, gpu) for A in (X, T, C))
    Y = torch.zeros(n, 1032, device=gpu)
    ops.extra_csr(Xd, Y, *csr_dev(c, gpu), Td, Cd, self_weight=None if d is None else torch.as_tensor(d, device=gpu),
                  objective=objective, lr=0.1, P=P)
    torch.cuda.synchronize()
    assert np.abs(got_x).sum() > 0
    assert bits_equal(got_x, Y[:, :P].cpu().numpy()) and bits_equal(got_c, Cd[:, :P].cpu().numpy())


@pytest.mark.parametrize("edges", [False, True], ids=["halo form", "interior + edges entry"])
@pytest.mark.parametrize("self_w", [False, True], ids=["no self weights", "self weights"])
def test_logistic_split_ring_equals_the_wrap_around_call(self_w, edges, gpu):
    """The logistic instantiations of the halo form and of the edges entry (f4
    columns and the scalar tail): the bits of the wrap-around call, which the
    test above ties to ops.extra_csr."""
    c, wp, wn, d = ring(9)
    d = d if self_w else None
    X, C, T = logistic_problem(9, 1031)
    whole = run_ring(X, C, T, wp, wn, d, gpu, objective="logistic")
    parts = run_ring(X, C, T, wp, wn, d, gpu, objective="logistic", blocks=(0, 2, 3, 8, 9), edges=edges)
    assert np.abs(whole[0]).sum() > 0
    assert bits_equal(parts[0], whole[0]) and bits_equal(parts[1], whole[1])


@pytest.mark.parametrize("objective", ["least_squares", "logistic"])
def test_apply_extra_ring_plan_and_csr_plan_of_one_w_agree(objective, gpu):
    n, P = 64, 1031
    torch.manual_seed(2028)
    c = G.communication_csr("circle", "stochastic", n)[0]
    plans = G.MixingPlan(c, gpu), G.MixingPlan(c, gpu, allow_ring=False)
    assert plans[0].kind == "ring" and plans[1].kind == "csr"
    g = torch.Generator(device=gpu).manual_seed(3)
    X, T, C0 = (torch.randn(n, 1032, generator=g, device=gpu)[:, :P] for _ in range(3))
    d = torch.linspace(0.05, 0.45, n, device=gpu)
    outs = []
    for plan in plans:
        Y, C = (torch.zeros(n, 1032, device=gpu)[:, :P] for _ in range(2))
        C.copy_(C0)
        assert plan.apply_extra(X, Y, T, C, self_weight=d, objective=objective, lr=0.1) is Y
        outs.append((Y, C))
    torch.cuda.synchronize()
    assert outs[0][0].abs().sum() > 0 and not same_bits(outs[0][1], C0)
    assert same_bits(outs[0][0], outs[1][0]) and same_bits(outs[0][1], outs[1][1])
