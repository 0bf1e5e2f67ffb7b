"""The EXTRA round on the parameter-major bank (dol_extra_csr_pm_f32,
ops.extra_csr_pm, SeparableEXTRAPM).

Least squares is bit-exact against tests/extra_cases.py::extra_round, the host
restatement built from the golden-pinned oracle (every operation has one
rounding on both sides), through gt_cases.pm / am, from a nonzero correction (a
zero one would hide a mistake in it) with unequal weights: at agent counts on
both sides of every quad / p-row-group boundary up to the 4096-agent limit, with
and without self weights, with many stages per workgroup, under every stage
order, with long rows and non-finite values.  Logistic calls expf, so it is
bit-exact against test_extra_csr_gpu.logistic_round, the device composition,
with ax from ops.mix_csr_pm.  Both objectives equal ops.extra_csr on the
transposed problem bit for bit.  Buffers as in tests/test_gt_pm_gpu.py: NaN in
the agent padding of XT and TT, 7.0 in the padding and extra columns of YT and
of corr (an output too); the padding must survive and XT and TT keep their bits.

SeparableEXTRAPM: its rounds are ops.extra_csr_pm calls, and built from a
SeparableEXTRA (16 agents x 4096, random 4-regular, Metropolis weights, lr 0.1,
seed 7) its 200 rounds are that problem's own 200 rounds bit for bit, so every
agent ends within 1e-5 of mean_i t_i (tests/test_extra_csr_gpu.py's bound,
measured there at 8.2e-6) where SeparableDGDPM on the same W, lr and problem
stays more than 0.05 away."""
import functools

import numpy as np
import pytest
import torch

import extra_cases as E
import gt_cases
from gt_cases import am, csr_dev, pm, problem, same_bits
from oracle import bits_equal
from dolhip import graph as G
from dolhip import ops
from test_extra_csr_gpu import logistic_round

pytestmark = pytest.mark.gpu

F32 = np.float32


def run_extra(X, C, T, c, d, gpu, objective="least_squares", lr=0.1, extra=0, nseg=None):
    """One round through ops.extra_csr_pm on agent-major host X, C, T; returns
    (X', C') agent-major.  The padding of YT and corr must still hold 7.0 and XT
    and TT must be untouched."""
    rp, col, val = csr_dev(c, gpu)
    n, P = X.shape
    XT, TT = pm(X, gpu, extra), pm(T, gpu, extra)
    keep = [t.clone() for t in (XT, TT)]
    YT, CT = (torch.full((P, (n + 3) // 4 * 4 + extra), 7.0, device=gpu) for _ in range(2))
    CT[:, :n] = torch.as_tensor(np.ascontiguousarray(C.T), device=gpu)
    dw = None if d is None else torch.as_tensor(np.asarray(d, F32), device=gpu)
    out = ops.extra_csr_pm(XT, YT, rp, col, val, TT, CT, self_weight=dw, objective=objective, lr=lr, nseg=nseg)
    torch.cuda.synchronize()
    assert out is YT
    assert (YT[:, n:] == 7.0).all() and (CT[:, n:] == 7.0).all(), "wrote past the last agent"
    for t, k in zip((XT, TT), keep):
        assert same_bits(t, k), "an input changed"
    return am(YT, n), am(CT, n)


@functools.lru_cache(maxsize=None)
def _regular(n):
    """(stochastic random 4-regular W, its Metropolis weights, their self weights)"""
    c = G.random_regular_csr(n, 4, seed=n + 3)
    return (c,) + G.metropolis_weights(c)


def _weights(n, self_w):
    """Unequal weights either way: the Metropolis W with its self weights, or the pattern's own random values."""
    c, m, d = _regular(n)
    return (m, d) if self_w else (c, None)


@functools.lru_cache(maxsize=None)
def _ls_case(n, P, self_w):
    W, d = _weights(n, self_w)
    X, C, T = problem(n, P, n * 7 + P)
    return W, d, X, C, T, E.extra_round(X, C, T, W, d, 0.1)


@pytest.mark.parametrize("self_w", [False, True], ids=["no self weights", "self weights"])
@pytest.mark.parametrize("P", [1, 7, 300])
@pytest.mark.parametrize("n", [5, 64, 100, 257, 1000, 1024, 1025, 4096])
def test_least_squares_vs_host_restatement(n, P, self_w, gpu):
    """1024 / 1025 agents straddle a quads-per-p-row power of two, 4096 is the
    limit (one p-row per stage), 5 / 257 / 1025 end on a ragged quad; P = 1 and
    7 leave most of a stage's p-rows dead."""
    W, d, X, C, T, (want_x, want_c) = _ls_case(n, P, self_w)
    got_x, got_c = run_extra(X, C, T, W, d, gpu, extra=4 * (n % 3))
    assert bits_equal(got_x, want_x)
    assert bits_equal(got_c, want_c)


def test_many_stages_per_workgroup(gpu):
    """At 1024 agents a 48 KiB stage holds 4 p-rows of X, T and C, one per p-row
    group of the workgroup: 4099 p-rows are 1025 stages, four or five for each
    of 256 workgroups, so every one comes back to the first buffer of its
    three-buffer ring, and the last stage holds 3 of its 4 p-rows."""
    n, P = 1024, 4099
    _, W, d = _regular(n)
    X, C, T = problem(n, P, 17)
    got_x, got_c = run_extra(X, C, T, W, d, gpu)
    want_x, want_c = E.extra_round(X, C, T, W, d, 0.1)
    assert bits_equal(got_x, want_x) and bits_equal(got_c, want_c)


def test_every_workgroup_cycles_its_ring_four_times(gpu):
    """12399 p-rows of 1024 agents are 3100 stages of 4: under the default stage
    order (8 segments of 388 or 384 stages over 32 workgroups each, 256 CUs)
    every workgroup walks at least twelve stages, four times round its
    three-buffer ring, and the last stage holds 3 of its 4 p-rows."""
    n, P = 1024, 12399
    _, W, d = _regular(n)
    X, C, T = problem(n, P, 19)
    got_x, got_c = run_extra(X, C, T, W, d, gpu)
    want_x, want_c = E.extra_round(X, C, T, W, d, 0.1)
    assert bits_equal(got_x, want_x) and bits_equal(got_c, want_c)


@functools.lru_cache(maxsize=None)
def _order_case():
    _, W, d = _regular(1000)
    X, C, T = problem(1000, 2500, 1)
    return W, d, X, C, T, E.extra_round(X, C, T, W, d, 0.1)


@pytest.mark.parametrize("nseg", [1, 8, 7])
def test_stage_orders_bit_identical(nseg, gpu):
    """The stage order is a speed choice only; 7 does not divide the grid and falls back to one sweep."""
    W, d, X, C, T, (want_x, want_c) = _order_case()
    got_x, got_c = run_extra(X, C, T, W, d, gpu, nseg=nseg)
    assert bits_equal(got_x, want_x) and bits_equal(got_c, want_c)


@pytest.mark.parametrize("self_w", [False, True], ids=["no self weights", "self weights"])
def test_long_rows_and_nonfinite(self_w, gpu):
    """The complete graph on 40 agents (degree 39): every row takes mix_quad's
    memory fallback.  Inf, NaN, -0 and a denormal in X, C and T come out like
    the host's, NaN for NaN.  Without self weights nothing may be added (0 *
    Inf would be NaN)."""
    torch.manual_seed(2028)
    c = G.csr_from_dense(G.communication_graph("compelete", "stochastic", 40)[0])
    d = np.linspace(0.01, 0.4, 40).astype(F32) if self_w else None
    X, C, T = problem(40, 333, 5)
    for A, k in ((X, 7), (C, 17), (T, 27)):
        A[3, k], A[4, k + 1], A[9, k + 2], A[11, k + 3], A[12, k + 4] = np.inf, -np.inf, np.nan, -0.0, 1e-40
    got_x, got_c = run_extra(X, C, T, c, d, gpu)
    want_x, want_c = E.extra_round(X, C, T, c, d, 0.1)
    assert np.isnan(want_x).any() and np.isinf(want_x).any() and np.isnan(want_c).any()
    assert np.array_equal(np.isnan(got_x), np.isnan(want_x)) and np.array_equal(np.isnan(got_c), np.isnan(want_c))
    assert bits_equal(got_x, want_x) and bits_equal(got_c, want_c)


def _logistic_case(n, P, self_w, gpu, extra=0):
    """The logistic round against the device composition
    (test_extra_csr_gpu.logistic_round) with ax from ops.mix_csr_pm.  Targets
    +-feature, as the problems draw them."""
    W, d = _weights(n, self_w)
    X, C, T = gt_cases.logistic_problem(n, P)
    got_x, got_c = run_extra(X, C, T, W, d, gpu, objective="logistic", lr=0.1, extra=extra)
    rp, col, val = csr_dev(W, gpu)

    def mix(A):
        YT = torch.full((P, (n + 3) // 4 * 4), 7.0, device=gpu)
        ops.mix_csr_pm(pm(A, gpu), YT, rp, col, val)
        return am(YT, n)
    want_x, want_c = logistic_round(mix, X, C, T, d, gpu)
    assert bits_equal(got_x, want_x)
    assert bits_equal(got_c, want_c)


@pytest.mark.parametrize("self_w", [False, True], ids=["no self weights", "self weights"])
@pytest.mark.parametrize("n", [100, 1024])
def test_logistic_vs_device_composition(n, self_w, gpu):
    _logistic_case(n, 300, self_w, gpu, extra=4 * (n % 3))


def test_logistic_many_stages_per_workgroup(gpu):
    _logistic_case(1024, 4099, True, gpu)


@pytest.mark.parametrize("objective", ["least_squares", "logistic"])
@pytest.mark.parametrize("n,P", [(100, 513), (1024, 300)])
def test_the_bits_of_extra_csr_on_the_transposed_problem(n, P, objective, gpu):
    _, W, d = _regular(n)
    X, C, T = gt_cases.logistic_problem(n, P) if objective == "logistic" else problem(n, P, n + P)
    got_x, got_c = run_extra(X, C, T, W, d, gpu, objective=objective)
    Xd, Td, Cd = (torch.as_tensor(A, device=gpu) for A in (X, T, C))
    Yd = torch.zeros_like(Xd)
    ops.extra_csr(Xd, Yd, *csr_dev(W, gpu), Td, Cd, self_weight=torch.as_tensor(d, device=gpu), objective=objective,
                  lr=0.1)
    torch.cuda.synchronize()
    assert bits_equal(got_x, Yd.cpu().numpy())
    assert bits_equal(got_c, Cd.cpu().numpy())


def test_entry_point_refuses_aliased_corr_and_4097_agents_and_returns_on_empty(gpu):
    """Straight at the C-ABI (ops refuses the first two before it gets there):
    DOL_EINVAL, nothing launched; n = 0 and P = 0 are DOL_OK, nothing launched."""
    stream = torch.cuda.current_stream(gpu).cuda_stream
    c = G.random_regular_csr(16, 4, seed=1)
    rp, col, val = csr_dev(c, gpu)
    XT, YT, TT, CT = (torch.full((3, 16), float(k + 1), device=gpu) for k in range(4))
    keep = [t.clone() for t in (XT, YT, TT, CT)]

    def call(x, y, t, corr, n=16, P=3):
        ops._native.call("dol_extra_csr_pm_f32", x.data_ptr(), 16, y.data_ptr(), 16, n, P, rp.data_ptr(),
                         col.data_ptr(), val.data_ptr(), None, t.data_ptr(), 16, corr.data_ptr(), 16, 0, 0.1, stream)
    for corr in (XT, YT, TT):
        with pytest.raises(ops.DolNativeError, match="alias"):
            call(XT, YT, TT, corr)
    call(XT, YT, TT, CT, n=0)
    call(XT, YT, TT, CT, P=0)
    big = G.random_regular_csr(4097, 4, seed=1)
    rpb, colb, valb = csr_dev(big, gpu)
    Z = [torch.zeros(3, 4100, device=gpu) for _ in range(4)]
    with pytest.raises(ops.DolNativeError, match="at most 4096 agents"):
        ops._native.call("dol_extra_csr_pm_ex_f32", Z[0].data_ptr(), 4100, Z[1].data_ptr(), 4100, 4097, 3,
                         rpb.data_ptr(), colb.data_ptr(), valb.data_ptr(), None, Z[2].data_ptr(), 4100,
                         Z[3].data_ptr(), 4100, 0, 0.1, 8, stream)
    torch.cuda.synchronize()
    for t, k in zip((XT, YT, TT, CT), keep):
        assert same_bits(t, k)
    assert not Z[1].any() and not Z[3].any()


# --- SeparableEXTRAPM ---

def _extra_problem(gpu, n=16, P=4096, lr=0.1, objective="least_squares", seed=7):
    from dolhip.synthetic import SeparableEXTRAPM
    W, d = G.metropolis_weights(G.random_regular_csr(n, 4, seed=5))
    return SeparableEXTRAPM(G.MixingPlan(W, gpu), P, objective=objective, lr=lr, self_weight=d, seed=seed), W, d


@pytest.mark.parametrize("objective", ["least_squares", "logistic"])
def test_problem_rounds_equal_manual_calls(objective, gpu):
    prob, W, d = _extra_problem(gpu, n=100, P=513, objective=objective)
    assert prob.XT.shape == prob.YT.shape == prob.TT.shape == prob.CT.shape == (513, 100)
    assert not prob.CT.any() and not prob.correction().any()
    rp, col, val = csr_dev(W, gpu)
    dw = torch.as_tensor(d, device=gpu)
    A, Cm = prob.XT.clone(), prob.CT.clone()
    Ao = torch.zeros_like(A)
    for _ in range(5):
        prob.round()
        ops.extra_csr_pm(A, Ao, rp, col, val, prob.TT, Cm, self_weight=dw, objective=objective, lr=0.1)
        A, Ao = Ao, A
    torch.cuda.synchronize()
    assert prob.rounds == 5
    assert prob.CT.any() and same_bits(prob.XT, A) and same_bits(prob.CT, Cm)
    assert bits_equal(prob.params().cpu().numpy(), am(A, 100)) and bits_equal(prob.correction().cpu().numpy(), am(Cm, 100))


def test_trajectory_is_the_agent_major_problems_and_reaches_the_optimum_that_dgd_misses(gpu):
    """16 agents x 4096, random 4-regular, Metropolis weights, lr 0.1, least
    squares: 200 rounds of from_agent_major(SeparableEXTRA) equal that
    problem's own 200 rounds bit for bit, x and corr, so every agent is within
    1e-5 of mean_i t_i; SeparableDGDPM on W + diag(d) (the diagonal as a CSR
    entry), same lr and problem, stays more than 0.05 away at its biased fixed
    point."""
    from dolhip.synthetic import SeparableDGD, SeparableDGDPM, SeparableEXTRA, SeparableEXTRAPM
    W, d = G.metropolis_weights(G.random_regular_csr(16, 4, seed=5))
    plan = G.MixingPlan(W, gpu)
    assert plan.kind == "csr"
    am_prob = SeparableEXTRA(plan, 4096, objective="least_squares", lr=0.1, self_weight=d, seed=7)
    prob = SeparableEXTRAPM.from_agent_major(am_prob)
    assert prob.plan is plan and prob.lr == 0.1 and prob.rounds == 0 and same_bits(prob.self_weight, am_prob.self_weight)
    assert same_bits(prob.params(), am_prob.params().contiguous()) and not prob.CT.any()
    dgd = SeparableDGDPM.from_agent_major(
        SeparableDGD(G.MixingPlan(gt_cases.with_diagonal(W, d), gpu), 4096, objective="least_squares", lr=0.1, seed=7))
    assert same_bits(dgd.TT, prob.TT) and same_bits(dgd.XT, prob.XT)  # the same problem
    opt = am_prob.targets().double().mean(0, keepdim=True)
    for _ in range(200):
        am_prob.round()
        prob.round()
        dgd.round()
    torch.cuda.synchronize()
    assert prob.rounds == 200
    assert same_bits(prob.params(), am_prob.params().contiguous())
    assert same_bits(prob.correction(), am_prob.correction().contiguous())
    err = float((prob.params().double() - opt).abs().max())
    err_dgd = float((dgd.params().double() - opt).abs().max())
    print(f"max |x - mean t| after 200 rounds: EXTRA {err:.3g} (consensus error {prob.consensus_error():.3g}), "
          f"DGD {err_dgd:.3g}")
    assert prob.distance_to_optimum() == err and err <= 1e-5
    assert err_dgd > 0.05
