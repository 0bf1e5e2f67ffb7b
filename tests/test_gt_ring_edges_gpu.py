"""The two boundary rows of a sharded ring block's gradient-tracking round in
one launch (dol_gt_ring_edges_f32, ops.gt_ring_edges).

The kernel runs gt_ring.hip's own lane on rows 0 and n - 1 of a block, so it
is held bit for bit to tests/gt_cases.py::gt_round on the whole ring's CSR
(least squares) and to ops.gt_ring's halo form on the same block (both
objectives: logistic calls expf, so the device round is its reference).  The
9-agent ring is cut into blocks of 1, 2 and more rows, one call per block with
the neighbouring blocks' boundary rows as halos; P covers scalar tail only, one
full 1024-float column tile, a tile + one f4 + a 3-float tail, and two tiles
and a partial one.  Buffers as test_gt_ring_gpu.run_ring: NaN in the inputs'
padding columns, 7.0 in the outputs and in a guard row before and after them;
every row that is no block's edge, the padding and the guards must still hold
7.0, and the three inputs keep their bits.  Further: every column down the
scalar kernel (an odd ld; halos one float off 16 B), an edge row past element
2^31, NaN / Inf / -0 / denormal inputs, and a captured and replayed call."""
import functools

import numpy as np
import pytest
import torch

import gt_cases
from gt_cases import logistic_problem, padded, problem, ring, same_bits
from oracle import bits_equal
from dolhip import ops

pytestmark = pytest.mark.gpu

F32 = np.float32
CUTS = [(0, 4, 9), (0, 1, 3, 9), (0, 2, 3, 8, 9)]
CUT_IDS = ["[0,4) [4,9)", "1, 2 and 6 rows", "2, 1, 5 and 1 rows"]


def edge_rows(blocks):
    return sorted({a for a in blocks[:-1]} | {b - 1 for b in blocks[1:]})


def run_edges(X, S, T, wp, wn, ws, gpu, blocks, objective="least_squares", lr=0.1, ld=None, halo_off=0,
              against_ring=True):
    """One ops.gt_ring_edges call per block of the ring cut at `blocks`, on
    host X, S, T [n, P], the neighbouring rows as halos (halo_off: the halos
    are copies that start this many floats into a 16-B aligned buffer).
    Returns host (X', S') [n, P], of which only edge_rows(blocks) were
    written: every other row, the padding columns and the guard rows must still
    hold 7.0, and the three inputs must be untouched.  against_ring: the edge
    rows must carry the bits ops.gt_ring's halo form writes on the same block."""
    n, P = X.shape
    ld = (P + 3) // 4 * 4 if ld is None else ld
    Xd, Sd, Td = (padded(A, ld, gpu) for A in (X, S, T))
    keep = [t.clone() for t in (Xd, Sd, Td)]
    XG, SG, XR, SR = (torch.full((n + 2, ld), 7.0, device=gpu) for _ in range(4))
    XO, SO = XG[1:n + 1], SG[1:n + 1]
    wpd, wnd = torch.as_tensor(wp, device=gpu), torch.as_tensor(wn, device=gpu)
    wsd = None if ws is None else torch.as_tensor(ws, device=gpu)
    for a, b in zip(blocks[:-1], blocks[1:]):
        prev, nxt = (a - 1) % n, b % n
        halos = (Xd[prev, :P], Xd[nxt, :P], Sd[prev, :P], Sd[nxt, :P])
        if halo_off:
            buf = torch.full((4, (P + halo_off + 3) // 4 * 4), float("nan"), device=gpu)
            for k, h in enumerate(halos):
                buf[k, halo_off:halo_off + P] = h
            halos = tuple(buf[k, halo_off:halo_off + P] for k in range(4))
            assert all(h.data_ptr() % 16 == 4 * halo_off % 16 for h in halos)
        kw = dict(self_weight=None if wsd is None else wsd[a:b], objective=objective, lr=lr, P=P, n_rows=b - a)
        out = ops.gt_ring_edges(Xd[a:b], Sd[a:b], XO[a:b], SO[a:b], wpd[a:b], wnd[a:b], Td[a:b], halos, **kw)
        assert out[0].data_ptr() == XO[a:b].data_ptr() and out[1].data_ptr() == SO[a:b].data_ptr()
        if against_ring:
            ops.gt_ring(Xd[a:b], Sd[a:b], XR[1 + a:1 + b], SR[1 + a:1 + b], wpd[a:b], wnd[a:b], Td[a:b], halos=halos,
                        **kw)
    torch.cuda.synchronize()
    edge = edge_rows(blocks)
    inner = [r for r in range(n) if r not in edge]
    for G_ in (XG, SG):
        assert (G_[0] == 7.0).all() and (G_[n + 1] == 7.0).all(), "wrote into a guard row"
        assert (G_[:, P:] == 7.0).all(), "wrote past column P"
        assert (G_[1:n + 1][inner] == 7.0).all(), "wrote a row that is no block's edge"
    for t, k in zip((Xd, Sd, Td), keep):
        assert same_bits(t, k), "an input changed"
    if against_ring:
        assert same_bits(XO[edge, :P].contiguous(), XR[1:n + 1][edge, :P].contiguous()), "x' differs from ops.gt_ring"
        assert same_bits(SO[edge, :P].contiguous(), SR[1:n + 1][edge, :P].contiguous()), "s' differs from ops.gt_ring"
    return XO[:, :P].cpu().numpy(), SO[:, :P].cpu().numpy()


@functools.lru_cache(maxsize=None)
def ls_case(P, self_w):
    """The 9-agent ring problem and one round of the host restatement on its CSR."""
    c, wp, wn, d = ring(9)
    d = d if self_w else None
    X, S, T = problem(9, P, 63 + P)
    return X, S, T, wp, wn, d, gt_cases.gt_round(X, S, T, c, d, 0.1)


# ---------------------------------------------------------------------------
# least squares against the host restatement and against ops.gt_ring
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("self_w", [False, True], ids=["no self weights", "self weights"])
@pytest.mark.parametrize("P", [1, 7, 1024, 1031, 2055])
@pytest.mark.parametrize("blocks", CUTS, ids=CUT_IDS)
def test_least_squares_vs_host_restatement(blocks, P, self_w, gpu):
    X, S, T, wp, wn, d, (want_x, want_s) = ls_case(P, self_w)
    got_x, got_s = run_edges(X, S, T, wp, wn, d, gpu, blocks)
    edge = edge_rows(blocks)
    assert bits_equal(got_x[edge], want_x[edge])
    assert bits_equal(got_s[edge], want_s[edge])


# ---------------------------------------------------------------------------
# the scalar path
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("self_w", [False, True], ids=["no self weights", "self weights"])
@pytest.mark.parametrize("how", [dict(ld=2057), dict(halo_off=1)], ids=["odd ld", "halos one float off 16 B"])
def test_scalar_path_gives_the_aligned_bits(how, self_w, gpu):
    """An odd ld leaves no row but the first 16-B aligned; halos that start one
    float into a buffer are not aligned either: every column then goes down
    the scalar kernel, to the bits of the aligned call (f4 body + 3-float tail)."""
    X, S, T, wp, wn, d, (want_x, want_s) = ls_case(2055, self_w)
    blocks = (0, 2, 3, 8, 9)
    aligned = run_edges(X, S, T, wp, wn, d, gpu, blocks)
    got = run_edges(X, S, T, wp, wn, d, gpu, blocks, **how)
    edge = edge_rows(blocks)
    assert bits_equal(got[0][edge], aligned[0][edge]) and bits_equal(got[1][edge], aligned[1][edge])
    assert bits_equal(got[0][edge], want_x[edge]) and bits_equal(got[1][edge], want_s[edge])


# ---------------------------------------------------------------------------
# rows past element 2^31
# ---------------------------------------------------------------------------
def test_rows_past_element_2_pow_31(gpu):
    """The whole 5-agent ring as one block of ld = 2^29 + 64 floats, its own last
    and first rows as halos: edge row 4 starts past element 2^31, where 32-bit
    row arithmetic would wrap.  The five matrices are disjoint column ranges of
    ONE 10.7 GB allocation (never initialised beyond them)."""
    n, P, ld = 5, 1031, (1 << 29) + 64
    c, wp, wn, d = ring(n)
    X, S, T = problem(n, P, 5)
    want_x, want_s = gt_cases.gt_round(X, S, T, c, d, 0.1)
    big = torch.empty(n * ld, dtype=torch.float32, device=gpu).view(n, ld)
    Xd, Sd, Td, XO, SO = (big[:, k * 2048:k * 2048 + P] for k in range(5))
    for dst, src in ((Xd, X), (Sd, S), (Td, T)):
        dst.copy_(torch.as_tensor(src, device=gpu))
    big[:, 3 * 2048:5 * 2048] = 7.0
    ops.gt_ring_edges(Xd, Sd, XO, SO, *(torch.as_tensor(a, device=gpu) for a in (wp, wn)), Td,
                      (Xd[4], Xd[0], Sd[4], Sd[0]), self_weight=torch.as_tensor(d, device=gpu), lr=0.1)
    torch.cuda.synchronize()
    edge = [0, 4]
    assert bits_equal(XO.cpu().numpy()[edge], want_x[edge]) and bits_equal(SO.cpu().numpy()[edge], want_s[edge])
    assert (big[1:4, 3 * 2048:5 * 2048] == 7.0).all(), "wrote a row that is no edge"
    assert (big[:, 3 * 2048 + P:4 * 2048] == 7.0).all() and (big[:, 4 * 2048 + P:5 * 2048] == 7.0).all()
    del Xd, Sd, Td, XO, SO, big
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------
# non-finite and signed-zero inputs
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("self_w", [False, True], ids=["no self weights", "self weights"])
@pytest.mark.parametrize("P", [1031, 7])
def test_nonfinite_and_signed_zero_inputs(P, self_w, gpu):
    """test_gt_ring_gpu's inputs (NaN, +-Inf, -0 and denormals in X, S and T;
    -0 in column 0 of every row of X, +0 in S) on a ring cut into blocks of at
    most two rows, so every row is some block's edge row and the whole output
    is compared: like the host's, NaN for NaN, and +0 where the mix starts."""
    n = 9
    c, wp, wn, d = ring(n)
    d = d if self_w else None
    X, S, T = problem(n, P, 11)
    for A, k in ((X, 1), (S, 2), (T, 3)):
        A[0, k], A[2, k], A[4, k], A[6, k], A[8, k] = np.nan, np.inf, -np.inf, -0.0, 1e-40
        A[1, 4], A[5, 5] = F32(-1e-42), F32(0.0)
    X[:, 0], S[:, 0] = -0.0, 0.0
    blocks = (0, 2, 4, 5, 7, 9)
    assert edge_rows(blocks) == list(range(n))
    got_x, got_s = run_edges(X, S, T, wp, wn, d, gpu, blocks)
    want_x, want_s = gt_cases.gt_round(X, S, T, c, d, 0.1)
    assert np.isnan(want_x).any() and np.isinf(want_x).any() and np.isnan(want_s).any()
    assert np.array_equal(np.isnan(got_x), np.isnan(want_x)) and np.array_equal(np.isnan(got_s), np.isnan(want_s))
    assert bits_equal(got_x, want_x) and bits_equal(got_s, want_s)
    assert (got_x[:, 0].view(np.uint32) == 0).all(), "-0 inputs must mix to +0"


# ---------------------------------------------------------------------------
# logistic: against ops.gt_ring's halo form (the same device separable_grad)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("self_w", [False, True], ids=["no self weights", "self weights"])
@pytest.mark.parametrize("n", [2, 9])
def test_logistic_vs_the_ring_entry(n, self_w, gpu):
    """A block of n rows inside an (n + 2)-agent ring: rows 1 .. n, with rows 0
    and n + 1 as halos.  _block_inside holds the edge rows to ops.gt_ring."""
    N, P = n + 2, 1031
    _, wp, wn, d = ring(N)
    X, S, T = logistic_problem(N, P)
    got_x, got_s = _block_inside(X, S, T, wp, wn, d if self_w else None, gpu, n)
    assert np.isfinite(got_x).all() and np.isfinite(got_s).all()
    assert np.abs(got_x).max() > 0 and (got_x != 7.0).all() and (got_s != 7.0).all()


def _block_inside(X, S, T, wp, wn, d, gpu, n):
    """ops.gt_ring_edges and ops.gt_ring (logistic) on rows 1 .. n of the host
    matrices with rows 0 and n + 1 as halos; returns the two edge rows of
    (x', s') after asserting that both entries wrote the same bits there and
    that the edge call wrote nothing else."""
    P = X.shape[1]
    ld = (P + 3) // 4 * 4
    Xd, Sd, Td = (padded(A, ld, gpu) for A in (X, S, T))
    XO, SO, XR, SR = (torch.full((n + 2, ld), 7.0, device=gpu) for _ in range(4))
    wpd, wnd = torch.as_tensor(wp, device=gpu), torch.as_tensor(wn, device=gpu)
    wsd = None if d is None else torch.as_tensor(d, device=gpu)[1:n + 1]
    halos = (Xd[0, :P], Xd[n + 1, :P], Sd[0, :P], Sd[n + 1, :P])
    kw = dict(self_weight=wsd, objective="logistic", lr=0.1, P=P, n_rows=n)
    blk = slice(1, n + 1)
    ops.gt_ring_edges(Xd[blk], Sd[blk], XO[blk], SO[blk], wpd[blk], wnd[blk], Td[blk], halos, **kw)
    ops.gt_ring(Xd[blk], Sd[blk], XR[blk], SR[blk], wpd[blk], wnd[blk], Td[blk], halos=halos, **kw)
    torch.cuda.synchronize()
    edge = [1, n]
    inner = [r for r in range(n + 2) if r not in edge]
    for G_, R_ in ((XO, XR), (SO, SR)):
        assert same_bits(G_[edge, :P].contiguous(), R_[edge, :P].contiguous())
        assert (G_[inner] == 7.0).all() and (G_[:, P:] == 7.0).all()
    return XO[edge, :P].cpu().numpy(), SO[edge, :P].cpu().numpy()


# ---------------------------------------------------------------------------
# graph capture
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("objective", ["least_squares", "logistic"])
def test_captured_gt_ring_edges_replays_bit_identically(objective, gpu):
    """The entry is stream-ordered and neither allocates nor synchronises: one
    captured and replayed call (f4 body, then the scalar tail, on one stream)
    gives the eager call's bits."""
    n, P = 9, 2055
    g = torch.Generator(device=gpu).manual_seed(5)
    X, S, T = (torch.randn(n, P + 1, generator=g, device=gpu)[:, :P] for _ in range(3))
    H = torch.randn(4, P + 1, generator=g, device=gpu)
    halos = tuple(H[k, :P] for k in range(4))
    wp, wn, ws = (torch.rand(n, generator=g, device=gpu) for _ in range(3))
    XO, SO = torch.zeros(n, P + 1, device=gpu), torch.zeros(n, P + 1, device=gpu)

    def round_():
        ops.gt_ring_edges(X, S, XO, SO, wp, wn, T, halos, self_weight=ws, objective=objective, lr=0.1, P=P)

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
    assert want[0][0].abs().sum() > 0 and want[0][n - 1].abs().sum() > 0 and not want[0][1:n - 1].any()
    for got, w in zip((XO, SO), want):
        assert torch.equal(got.view(torch.int32), w.view(torch.int32))
