"""The gradient-tracking round on the agent-major ring (dol_gt_ring_f32,
ops.gt_ring, SeparableGT).

Least squares is bit-exact against tests/gt_cases.py::gt_round, the host
restatement built from the golden-pinned oracle, on the ring's CSR (every
operation has one rounding on both sides; the ring's previous-then-next sum
and the CSR's ascending-column sum agree because fl(fl(+0 + a) + b) commutes):
with and without self weights, with fewer rows than a tile, exactly one tile
and ragged tiles, with column counts that are scalar tail only, one full
1024-float column tile, a full tile + one f4 + a 3-float tail, and two tiles
and a partial one; with an odd ld (every row down the scalar kernel), with
ld = P + 8, and with rows that start past element 2^31.  A ring cut into
blocks that see each other's boundary rows as halos gives the bits of the
wrap-around call, down to blocks of one row.  Logistic calls expf, so it is
held to ops.gt_csr_pm on the same ring CSR (the same device separable_grad)
and to a composition of ops.mix_ring, ops.separable_grad and single fp32
operations.  Buffers: NaN in the inputs' padding columns, 7.0 in the outputs'
padding columns and in a guard row before and after each output; the padding
must survive and the three inputs keep their bits."""
import functools

import numpy as np
import pytest
import torch

import gt_cases
from gt_cases import am, csr_dev, logistic_problem, padded, pm, problem, ring, same_bits
from oracle import bits_equal
from dolhip import graph as G
from dolhip import ops
from dolhip.synthetic import SeparableDGD, SeparableGT, SeparableGTPM, ring_gt_weights

pytestmark = pytest.mark.gpu

F32 = np.float32


def run_ring(X, S, T, wp, wn, ws, gpu, objective="least_squares", lr=0.1, ld=None, blocks=None):
    """One round through ops.gt_ring on host X, S, T [n, P]; returns host
    (X', S').  blocks: the ring cut at these row bounds, one call per block
    with the neighbouring blocks' boundary rows as halos; None: the
    wrap-around call.  The outputs' padding columns and guard rows must still
    hold 7.0 and the three inputs must be untouched."""
    n, P = X.shape
    ld = (P + 3) // 4 * 4 if ld is None else ld
    Xd, Sd, Td = (padded(A, ld, gpu) for A in (X, S, T))
    keep = [t.clone() for t in (Xd, Sd, Td)]
    XG, SG = (torch.full((n + 2, ld), 7.0, device=gpu) for _ in range(2))
    XO, SO = XG[1:n + 1], SG[1:n + 1]
    wpd, wnd = torch.as_tensor(wp, device=gpu), torch.as_tensor(wn, device=gpu)
    wsd = None if ws is None else torch.as_tensor(ws, device=gpu)
    if blocks is None:
        out = ops.gt_ring(Xd, Sd, XO, SO, wpd, wnd, Td, self_weight=wsd, objective=objective, lr=lr, P=P)
        assert out[0] is XO and out[1] is SO
    else:
        for a, b in zip(blocks[:-1], blocks[1:]):
            prev, nxt = (a - 1) % n, b % n
            ops.gt_ring(Xd[a:b], Sd[a:b], XO[a:b], SO[a:b], wpd[a:b], wnd[a:b], Td[a:b],
                        self_weight=None if wsd is None else wsd[a:b], objective=objective, lr=lr,
                        halos=(Xd[prev, :P], Xd[nxt, :P], Sd[prev, :P], Sd[nxt, :P]), P=P, n_rows=b - a)
    torch.cuda.synchronize()
    for G_ in (XG, SG):
        assert (G_[0] == 7.0).all() and (G_[n + 1] == 7.0).all(), "wrote into a guard row"
        assert (G_[:, P:] == 7.0).all(), "wrote past column P"
    for t, k in zip((Xd, Sd, Td), keep):
        assert same_bits(t, k), "an input changed"
    return XO[:, :P].cpu().numpy(), SO[:, :P].cpu().numpy()


@functools.lru_cache(maxsize=None)
def ls_case(n, P, self_w):
    c, wp, wn, d = ring(n)
    d = d if self_w else None
    X, S, T = problem(n, P, 7 * n + P)
    return X, S, T, wp, wn, d, gt_cases.gt_round(X, S, T, c, d, 0.1)


# ---------------------------------------------------------------------------
# least squares against the host restatement
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("self_w", [False, True], ids=["no self weights", "self weights"])
@pytest.mark.parametrize("P", [1, 7, 1024, 1031, 2055])
@pytest.mark.parametrize("n", [3, 4, 5, 7, 9])
def test_least_squares_vs_host_restatement(n, P, self_w, gpu):
    """n = 3 is fewer rows than a tile, 4 one tile, 5 / 7 / 9 ragged tiles; P =
    1 and 7 are scalar tail only, 1024 one full column tile, 1031 a full tile
    then one f4 and a 3-float tail, 2055 two tiles and a partial one."""
    X, S, T, wp, wn, d, (want_x, want_s) = ls_case(n, P, self_w)
    got_x, got_s = run_ring(X, S, T, wp, wn, d, gpu)
    assert bits_equal(got_x, want_x)
    assert bits_equal(got_s, want_s)


@pytest.mark.parametrize("ld", [2057, 2063], ids=["odd ld", "ld = P + 8"])
@pytest.mark.parametrize("self_w", [False, True], ids=["no self weights", "self weights"])
def test_row_strides(self_w, ld, gpu):
    """An odd ld leaves no row but the first 16-B aligned: every column goes
    down the scalar kernel.  ld = P + 8 = 2063 is odd as well; P = 2056 with ld
    = 2064 is the aligned form of 'eight more than P'."""
    X, S, T, wp, wn, d, (want_x, want_s) = ls_case(9, 2055, self_w)
    got_x, got_s = run_ring(X, S, T, wp, wn, d, gpu, ld=ld)
    assert bits_equal(got_x, want_x) and bits_equal(got_s, want_s)


def test_padded_aligned_rows(gpu):
    """ld = P + 8 with 16-B aligned rows: the f4 body on rows with a gap between them."""
    X, S, T, wp, wn, d, (want_x, want_s) = ls_case(7, 2056, True)
    got_x, got_s = run_ring(X, S, T, wp, wn, d, gpu, ld=2064)
    assert bits_equal(got_x, want_x) and bits_equal(got_s, want_s)


def test_rows_past_element_2_pow_31(gpu):
    """Five rows of ld = 2^29 + 64 floats: rows 4's elements start past 2^31,
    where 32-bit row arithmetic would wrap.  The five matrices are disjoint
    column ranges of ONE 10.7 GB allocation (never initialised beyond them)."""
    n, P, ld = 5, 1031, (1 << 29) + 64
    c, wp, wn, d = ring(n)
    X, S, T = problem(n, P, 5)
    want_x, want_s = gt_cases.gt_round(X, S, T, c, d, 0.1)
    big = torch.empty(n * ld, dtype=torch.float32, device=gpu).view(n, ld)
    Xd, Sd, Td, XO, SO = (big[:, k * 2048:k * 2048 + P] for k in range(5))
    for dst, src in ((Xd, X), (Sd, S), (Td, T)):
        dst.copy_(torch.as_tensor(src, device=gpu))
    big[:, 3 * 2048:5 * 2048] = 7.0
    ops.gt_ring(Xd, Sd, XO, SO, *(torch.as_tensor(a, device=gpu) for a in (wp, wn)), Td,
                self_weight=torch.as_tensor(d, device=gpu), lr=0.1)
    torch.cuda.synchronize()
    assert bits_equal(XO.cpu().numpy(), want_x) and bits_equal(SO.cpu().numpy(), want_s)
    assert (big[:, 3 * 2048 + P:4 * 2048] == 7.0).all() and (big[:, 4 * 2048 + P:5 * 2048] == 7.0).all()
    del Xd, Sd, Td, XO, SO, big
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------
# halos
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("blocks", [(0, 4, 9), (0, 1, 3, 9), (0, 2, 3, 8, 9)],
                         ids=["[0,4) [4,9)", "1, 2 and 6 rows", "2, 1, 5 and 1 rows"])
@pytest.mark.parametrize("P", [1031, 7])
@pytest.mark.parametrize("self_w", [False, True], ids=["no self weights", "self weights"])
def test_split_ring_equals_the_wrap_around_call(self_w, P, blocks, gpu):
    X, S, T, wp, wn, d, (want_x, want_s) = ls_case(9, P, self_w)
    whole = run_ring(X, S, T, wp, wn, d, gpu)
    parts = run_ring(X, S, T, wp, wn, d, gpu, blocks=blocks)
    assert bits_equal(parts[0], whole[0]) and bits_equal(parts[1], whole[1])
    assert bits_equal(parts[0], want_x) and bits_equal(parts[1], want_s)


# ---------------------------------------------------------------------------
# non-finite and signed-zero inputs
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("self_w", [False, True], ids=["no self weights", "self weights"])
@pytest.mark.parametrize("P", [1031, 7])
def test_nonfinite_and_signed_zero_inputs(P, self_w, gpu):
    """NaN, +-Inf, -0 and denormals in X, S and T come out like the host's, NaN
    for NaN.  Column 0 holds -0 in every row of X and +0 in S: the mix starts
    at +0, so x' is +0 there, not -0."""
    n = 9
    c, wp, wn, d = ring(n)
    d = d if self_w else None
    X, S, T = problem(n, P, 11)
    for A, k in ((X, 1), (S, 2), (T, 3)):
        A[0, k], A[2, k], A[4, k], A[6, k], A[8, k] = np.nan, np.inf, -np.inf, -0.0, 1e-40
        A[1, 4], A[5, 5] = F32(-1e-42), F32(0.0)
    X[:, 0], S[:, 0] = -0.0, 0.0
    got_x, got_s = run_ring(X, S, T, wp, wn, d, gpu)
    want_x, want_s = gt_cases.gt_round(X, S, T, c, d, 0.1)
    assert np.isnan(want_x).any() and np.isinf(want_x).any() and np.isnan(want_s).any()
    assert np.array_equal(np.isnan(got_x), np.isnan(want_x)) and np.array_equal(np.isnan(got_s), np.isnan(want_s))
    assert bits_equal(got_x, want_x) and bits_equal(got_s, want_s)
    assert (got_x[:, 0].view(np.uint32) == 0).all(), "-0 inputs must mix to +0"


# ---------------------------------------------------------------------------
# logistic: against the parameter-major round and against a device composition
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("self_w", [False, True], ids=["no self weights", "self weights"])
@pytest.mark.parametrize("objective", ["least_squares", "logistic"])
@pytest.mark.parametrize("n", [9, 64])
def test_same_bits_as_the_parameter_major_round(n, objective, self_w, gpu):
    c, wp, wn, d = ring(n)
    d = d if self_w else None
    P = 1031
    X, S, T = logistic_problem(n, P)
    got_x, got_s = run_ring(X, S, T, wp, wn, d, gpu, objective=objective)
    XT, ST, TT = (pm(A, gpu) for A in (X, S, T))
    XO, SO = torch.zeros_like(XT), torch.zeros_like(XT)
    ops.gt_csr_pm(XT, ST, XO, SO, *csr_dev(c, gpu), TT,
                  self_weight=None if d is None else torch.as_tensor(d, device=gpu), objective=objective, lr=0.1)
    torch.cuda.synchronize()
    assert bits_equal(got_x, am(XO, n))
    assert bits_equal(got_s, am(SO, n))


@pytest.mark.parametrize("self_w", [False, True], ids=["no self weights", "self weights"])
@pytest.mark.parametrize("n", [9, 64])
def test_logistic_vs_device_composition(n, self_w, gpu):
    """gt_cases.logistic_round with ax, as from ops.mix_ring."""
    c, wp, wn, d = ring(n)
    d = d if self_w else None
    P = 1031
    X, S, T = logistic_problem(n, P)
    got_x, got_s = run_ring(X, S, T, wp, wn, d, gpu, objective="logistic")
    wpd, wnd = torch.as_tensor(wp, device=gpu), torch.as_tensor(wn, device=gpu)

    def mix(A):
        Y = torch.empty(n, P, device=gpu)
        ops.mix_ring(torch.as_tensor(A, device=gpu), Y, wpd, wnd)
        return Y.cpu().numpy()
    want_x, want_s = gt_cases.logistic_round(mix, X, S, T, d, gpu)
    assert bits_equal(got_x, want_x)
    assert bits_equal(got_s, want_s)


# ---------------------------------------------------------------------------
# SeparableGT
# ---------------------------------------------------------------------------
def gt_problem(gpu, P, objective="least_squares", lr=0.1, seed=7, n=9):
    torch.manual_seed(2028)
    pattern = G.communication_csr("circle", "stochastic", n)[0]
    w_off, d = G.metropolis_weights(pattern)
    wp, wn, ws = ring_gt_weights(pattern)
    plan = G.MixingPlan(w_off, gpu)
    assert plan.kind == "ring" and np.array_equal(plan.w_prev.cpu().numpy(), wp) and np.array_equal(ws, d)
    return SeparableGT(plan, P, objective=objective, lr=lr, self_weight=ws, seed=seed), w_off, d


def test_problem_reaches_the_optimum_that_dgd_misses(gpu):
    """The 9-agent ring with Metropolis weights (1/3, 1/3, 1/3), least squares,
    lr 0.1, 200 rounds: every agent within 1e-5 of mean_i t_i; SeparableDGD on
    the same W (the diagonal as a CSR entry), lr, seed and so the same problem
    stays above 0.1 at its biased fixed point."""
    prob, w_off, d = gt_problem(gpu, 1031)
    assert same_bits(prob.tracker(), ops.separable_grad(prob.params(), prob.targets()))
    dgd = SeparableDGD(G.MixingPlan(gt_cases.with_diagonal(w_off, d), gpu), 1031, objective="least_squares", lr=0.1,
                       seed=7)
    assert same_bits(dgd.targets(), prob.targets()) and same_bits(dgd.params(), prob.params())  # the same problem
    opt = prob.targets().double().mean(0, keepdim=True)
    for _ in range(200):
        prob.round()
        dgd.round()
    torch.cuda.synchronize()
    err = float((prob.params().double() - opt).abs().max())
    err_dgd = float((dgd.params().double() - opt).abs().max())
    print(f"max |x - mean t| after 200 rounds: gradient tracking {err:.3g} (consensus error "
          f"{prob.consensus_error():.3g}), DGD {err_dgd:.3g}")
    assert prob.rounds == 200
    assert err <= 1e-5 and prob.distance_to_optimum() == err
    assert err_dgd > 0.1


@pytest.mark.parametrize("objective", ["least_squares", "logistic"])
def test_problem_rounds_equal_the_parameter_major_problem(objective, gpu):
    """After 5 rounds params() and tracker() have the bits of SeparableGTPM on
    the same problem (from_agent_major: the two layouts draw their seeded init
    in different element orders, so the state is transposed, not redrawn)."""
    prob, _, _ = gt_problem(gpu, 513, objective=objective)
    twin = SeparableGTPM.from_agent_major(prob)
    for _ in range(5):
        prob.round()
        twin.round()
    torch.cuda.synchronize()
    assert prob.rounds == twin.rounds == 5
    assert same_bits(prob.params().contiguous(), twin.params())
    assert same_bits(prob.tracker().contiguous(), twin.tracker())
