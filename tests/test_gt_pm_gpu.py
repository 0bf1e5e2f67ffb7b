"""The gradient-tracking round on the parameter-major bank (dol_gt_csr_pm_f32)
and the device gradient (dol_separable_grad_f32).

Least squares is bit-exact against tests/gt_cases.py, the host restatement
built from the golden-pinned oracle (every operation has one rounding on both
sides): at agent counts on both sides of every quad / p-row-group boundary up
to the 4096-agent limit, with and without self weights, with many stages per
workgroup, under every stage order, with long rows and non-finite values.
Logistic calls expf, so it is bit-exact against a composition of device ops
(ops.mix_csr_pm for the sums, ops.separable_grad for the gradients -- the same
device code -- and single fp32 torch ops), and ops.separable_grad itself is
held to the float64 formula at test_dgd_gpu.LOGISTIC_TOL.  Buffers as in
tests/test_pm_steps_gpu.py: NaN in the inputs' agent padding, 7.0 in the
outputs' padding and extra columns; the padding must survive and the inputs
stay untouched.  SeparableGTPM reaches the optimum that SeparableDGDPM, on the
same W and lr, does not."""
import functools

import numpy as np
import pytest
import torch

import gt_cases
from gt_cases import am, csr_dev, pm, problem, same_bits
from oracle import bits_equal
from dolhip import graph as G
from dolhip import ops
from test_dgd_gpu import LOGISTIC_TOL

pytestmark = pytest.mark.gpu

F32 = np.float32


def run_gt(X, S, T, c, d, gpu, objective="least_squares", lr=0.1, extra=0, nseg=None):
    """One round through ops.gt_csr_pm on agent-major host X, S, T; returns
    (X', S') agent-major.  The outputs' padding must still hold 7.0 and the
    three inputs must be untouched."""
    rp, col, val = csr_dev(c, gpu)
    n, P = X.shape
    XT, ST, TT = pm(X, gpu, extra), pm(S, gpu, extra), pm(T, gpu, extra)
    keep = [t.clone() for t in (XT, ST, TT)]
    XO, SO = (torch.full((P, (n + 3) // 4 * 4 + extra), 7.0, device=gpu) for _ in range(2))
    dw = None if d is None else torch.as_tensor(np.asarray(d, F32), device=gpu)
    out = ops.gt_csr_pm(XT, ST, XO, SO, rp, col, val, TT, self_weight=dw, objective=objective, lr=lr, nseg=nseg)
    torch.cuda.synchronize()
    assert out[0] is XO and out[1] is SO
    assert (XO[:, n:] == 7.0).all() and (SO[:, n:] == 7.0).all(), "wrote past the last agent"
    for t, k in zip((XT, ST, TT), keep):
        assert same_bits(t, k), "an input changed"
    return am(XO, n), am(SO, n)


@functools.lru_cache(maxsize=None)
def _regular(n):
    """(stochastic random 4-regular W, its Metropolis weights, their self weights)"""
    c = G.random_regular_csr(n, 4, seed=n + 3)
    return (c,) + G.metropolis_weights(c)


@functools.lru_cache(maxsize=None)
def _ls_case(n, P, self_w):
    c, m, d = _regular(n)
    W, d = (m, d) if self_w else (c, None)
    X, S, T = problem(n, P, n * 7 + P)
    return W, d, X, S, T, gt_cases.gt_round(X, S, T, W, d, 0.1)


@pytest.mark.parametrize("self_w", [False, True], ids=["no self weights", "self weights"])
@pytest.mark.parametrize("P", [1, 7, 300])
@pytest.mark.parametrize("n", [5, 64, 100, 257, 1000, 1024, 1025, 4096])
def test_least_squares_vs_host_restatement(n, P, self_w, gpu):
    """1024 / 1025 agents straddle a quads-per-p-row power of two, 4096 is the
    limit (one p-row per stage), 5 / 257 / 1025 end on a ragged quad; P = 1 and
    7 leave most of a stage's p-rows dead."""
    W, d, X, S, T, (want_x, want_s) = _ls_case(n, P, self_w)
    got_x, got_s = run_gt(X, S, T, W, d, gpu, extra=4 * (n % 3))
    assert bits_equal(got_x, want_x)
    assert bits_equal(got_s, want_s)


def test_many_stages_per_workgroup(gpu):
    """Every workgroup cycles its LDS-DMA ring several times and the last stage is ragged."""
    n, P = 1024, 4099
    _, W, d = _regular(n)
    X, S, T = problem(n, P, 17)
    got_x, got_s = run_gt(X, S, T, W, d, gpu)
    want_x, want_s = gt_cases.gt_round(X, S, T, W, d, 0.1)
    assert bits_equal(got_x, want_x) and bits_equal(got_s, want_s)


@functools.lru_cache(maxsize=None)
def _order_case():
    _, W, d = _regular(1000)
    X, S, T = problem(1000, 2500, 1)
    return W, d, X, S, T, gt_cases.gt_round(X, S, T, W, d, 0.1)


@pytest.mark.parametrize("nseg", [1, 8, 7])
def test_stage_orders_bit_identical(nseg, gpu):
    """The stage order is a speed choice only; 7 does not divide the grid and falls back to one sweep."""
    W, d, X, S, T, (want_x, want_s) = _order_case()
    got_x, got_s = run_gt(X, S, T, W, d, gpu, nseg=nseg)
    assert bits_equal(got_x, want_x) and bits_equal(got_s, want_s)


@pytest.mark.parametrize("self_w", [False, True], ids=["no self weights", "self weights"])
def test_long_rows_and_nonfinite(self_w, gpu):
    """The complete graph on 40 agents (degree 39): every row takes mix_quad's
    memory fallback for the X and for the S image.  Inf, NaN, -0 and a
    denormal in X and in S come out like the host's, NaN for NaN.  Without
    self weights nothing may be added (0 * Inf would be NaN)."""
    torch.manual_seed(2028)
    c = G.csr_from_dense(G.communication_graph("compelete", "stochastic", 40)[0])
    d = np.linspace(0.01, 0.4, 40).astype(F32) if self_w else None
    X, S, T = problem(40, 333, 5)
    X[3, 7], X[9, 8], X[11, 9], X[12, 10] = np.inf, np.nan, -0.0, 1e-40
    S[4, 7], S[10, 8], S[11, 9], S[13, 10] = -np.inf, np.nan, -0.0, 1e-40
    got_x, got_s = run_gt(X, S, T, c, d, gpu)
    want_x, want_s = gt_cases.gt_round(X, S, T, c, d, 0.1)
    assert np.isnan(want_x).any() and np.isinf(want_x).any() and np.isnan(want_s).any()
    assert np.array_equal(np.isnan(got_x), np.isnan(want_x)) and np.array_equal(np.isnan(got_s), np.isnan(want_s))
    assert bits_equal(got_x, want_x) and bits_equal(got_s, want_s)


def _logistic_case(n, P, self_w, gpu, extra=0):
    """The logistic round against the device composition
    (gt_cases.logistic_round) with ax, as from ops.mix_csr_pm.  Targets
    +-feature, as SeparableDGDPM draws them."""
    c, m, d = _regular(n)
    W, d = (m, d) if self_w else (c, None)
    rng = np.random.default_rng(n + P)
    X, S, T = problem(n, P, n + 31)
    T = np.where(rng.random(T.shape) < 0.5, -T, T).astype(F32)
    got_x, got_s = run_gt(X, S, T, W, d, gpu, objective="logistic", lr=0.1, extra=extra)
    rp, col, val = csr_dev(W, gpu)

    def mix(A):
        YT = torch.full((P, (n + 3) // 4 * 4), 7.0, device=gpu)
        ops.mix_csr_pm(pm(A, gpu), YT, rp, col, val)
        return am(YT, n)
    want_x, want_s = gt_cases.logistic_round(mix, X, S, T, d, gpu)
    assert bits_equal(got_x, want_x)
    assert bits_equal(got_s, want_s)


@pytest.mark.parametrize("self_w", [False, True], ids=["no self weights", "self weights"])
@pytest.mark.parametrize("n", [100, 1024])
def test_logistic_vs_device_composition(n, self_w, gpu):
    _logistic_case(n, 300, self_w, gpu, extra=4 * (n % 3))


def test_logistic_many_stages_per_workgroup(gpu):
    """The logistic kernel has a ring of its own (three buffers, two stages in
    flight): every workgroup cycles it and the last stage is ragged."""
    _logistic_case(1024, 4099, True, gpu)


@pytest.mark.parametrize("rows,cols,ld", [(64, 4096, 4100), (5, 1027, 1028), (7, 3, 3)],
                         ids=["f4, padded rows", "f4 + scalar tail", "scalar"])
@pytest.mark.parametrize("objective", ["least_squares", "logistic"])
def test_separable_grad(rows, cols, ld, objective, gpu):
    rng = np.random.default_rng(rows + cols)
    X, T = (rng.standard_normal((rows, cols)).astype(F32) * 3 for _ in range(2))
    Xd, Td, Gd = (torch.full((rows, ld), 7.0, device=gpu) for _ in range(3))
    Xd[:, :cols], Td[:, :cols] = torch.as_tensor(X, device=gpu), torch.as_tensor(T, device=gpu)
    out = ops.separable_grad(Xd[:, :cols], Td[:, :cols], Gd[:, :cols], objective)
    torch.cuda.synchronize()
    assert out.data_ptr() == Gd.data_ptr() and (Gd[:, cols:] == 7.0).all()
    got = Gd[:, :cols].cpu().numpy()
    if objective == "least_squares":
        assert bits_equal(got, X - T)
    else:
        T64, X64 = T.astype(np.float64), X.astype(np.float64)
        np.testing.assert_allclose(got, -T64 / (1.0 + np.exp(T64 * X64)), **LOGISTIC_TOL)
    fresh = ops.separable_grad(Xd[:, :cols], Td[:, :cols], None, objective)  # allocates its own output
    assert bits_equal(fresh.cpu().numpy(), got)


def test_entry_point_refuses_aliased_outputs_and_4097_agents(gpu):
    """Straight at the C-ABI (ops refuses both before it gets there): DOL_EINVAL, nothing launched."""
    stream = torch.cuda.current_stream(gpu).cuda_stream
    c = G.random_regular_csr(16, 4, seed=1)
    rp, col, val = csr_dev(c, gpu)
    XT, ST, XO, TT = (torch.zeros(3, 16, device=gpu) for _ in range(4))
    with pytest.raises(ops.DolNativeError, match="alias"):
        ops._native.call("dol_gt_csr_pm_f32", XT.data_ptr(), 16, ST.data_ptr(), 16, XO.data_ptr(), 16, XO.data_ptr(),
                         16, 16, 3, rp.data_ptr(), col.data_ptr(), val.data_ptr(), None, TT.data_ptr(), 16, 0, 0.1,
                         stream)
    big = G.random_regular_csr(4097, 4, seed=1)
    rpb, colb, valb = csr_dev(big, gpu)
    Z = [torch.zeros(3, 4100, device=gpu) for _ in range(5)]
    with pytest.raises(ops.DolNativeError, match="at most 4096 agents"):
        ops._native.call("dol_gt_csr_pm_ex_f32", Z[0].data_ptr(), 4100, Z[1].data_ptr(), 4100, Z[2].data_ptr(), 4100,
                         Z[3].data_ptr(), 4100, 4097, 3, rpb.data_ptr(), colb.data_ptr(), valb.data_ptr(), None,
                         Z[4].data_ptr(), 4100, 0, 0.1, 8, stream)
    torch.cuda.synchronize()
    assert not XO.any() and not Z[2].any() and not Z[3].any()


# --- SeparableGTPM ---

def _gt_problem(gpu, n=16, P=4096, lr=0.1, objective="least_squares", seed=7):
    from dolhip.synthetic import SeparableGTPM
    W, d = G.metropolis_weights(G.random_regular_csr(n, 4, seed=5))
    return SeparableGTPM(G.MixingPlan(W, gpu), P, objective=objective, lr=lr, self_weight=d, seed=seed), W, d


@pytest.mark.parametrize("objective", ["least_squares", "logistic"])
def test_problem_rounds_equal_manual_calls(objective, gpu):
    prob, W, d = _gt_problem(gpu, n=100, P=513, objective=objective)
    assert same_bits(prob.ST, ops.separable_grad(prob.XT, prob.TT, None, objective))
    rp, col, val = csr_dev(W, gpu)
    dw = torch.as_tensor(d, device=gpu)
    A, B = prob.XT.clone(), prob.ST.clone()
    Ao, Bo = torch.zeros_like(A), torch.zeros_like(B)
    for _ in range(5):
        prob.round()
        ops.gt_csr_pm(A, B, Ao, Bo, rp, col, val, prob.TT, self_weight=dw, objective=objective, lr=0.1)
        A, Ao, B, Bo = Ao, A, Bo, B
    torch.cuda.synchronize()
    assert prob.rounds == 5
    assert same_bits(prob.XT, A) and same_bits(prob.ST, B)
    assert bits_equal(prob.params().cpu().numpy(), am(A, 100)) and bits_equal(prob.tracker().cpu().numpy(), am(B, 100))


def test_problem_reaches_the_optimum_that_dgd_misses(gpu):
    """Random 4-regular, 16 agents x 4096, Metropolis weights, lr 0.1, least
    squares: after 200 rounds every agent is within atol 1e-5 (the N-term-mean
    atol of tests/test_dgd_gpu.py) of mean_i t_i; SeparableDGDPM on the same
    W + diag(d) (the diagonal as a CSR entry) and lr is not -- it sits at its
    biased fixed point -- although its agents' mean is."""
    from dolhip.synthetic import SeparableDGDPM
    prob, W, d = _gt_problem(gpu)
    opt = prob.TT[:, :16].double().mean(1)
    for _ in range(200):
        prob.round()
    torch.cuda.synchronize()
    x = prob.params().double()
    print(f"gradient tracking: max |x - mean t| = {float((x - opt).abs().max()):.3g}, "
          f"consensus error {prob.consensus_error():.3g}")
    torch.testing.assert_close(x, opt.expand_as(x), rtol=0, atol=1e-5)
    assert prob.distance_to_optimum() <= 1e-5
    dgd = SeparableDGDPM(G.MixingPlan(gt_cases.with_diagonal(W, d), gpu), 4096, objective="least_squares", lr=0.1,
                         seed=7)
    assert same_bits(dgd.TT, prob.TT)  # the same problem
    for _ in range(200):
        dgd.round()
    torch.cuda.synchronize()
    y = dgd.params().double()
    print(f"DGD: max |x - mean t| = {float((y - opt).abs().max()):.3g}")
    assert float((y - opt).abs().max()) > 1e-5
    torch.testing.assert_close(y.mean(0), opt, rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("objective", ["least_squares", "logistic"])
def test_tracking_invariant(objective, gpu):
    """W is doubly stochastic, so after a round mean_i s_i = mean_i g(x_i)."""
    prob, _, _ = _gt_problem(gpu, P=1000, objective=objective)
    prob.round()
    g = ops.separable_grad(prob.XT, prob.TT, None, objective)[:, :16]
    torch.testing.assert_close(prob.ST[:, :16].double().mean(1), g.double().mean(1), rtol=1e-4, atol=1e-5)
