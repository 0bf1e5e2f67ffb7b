"""Multi-step consensus on the parameter-major bank (dol_mix_csr_pm_steps_f32,
dol_dgd_csr_pm_steps_f32): W^k X in one pass is bit-exact against the oracle's
mix applied k times and against k single-step launches, at agent counts on both
sides of every geometry boundary, on both LDS images a stage can end on, with
long and empty rows, non-finite values, every stage order and the fused local
steps of config 3.  Nothing here has a tolerance except the logistic round
against the glibc oracle (test_pmajor_gpu's rtol 2e-6, atol 1e-6)."""
import functools

import numpy as np
import pytest
import torch

import oracle
from oracle import bits_equal
from dolhip import graph as G
from dolhip import ops

pytestmark = pytest.mark.gpu


def csr_dev(c, gpu):
    return (torch.as_tensor(np.asarray(c.rowptr, np.int32), device=gpu),
            torch.as_tensor(np.asarray(c.col, np.int32), device=gpu),
            torch.as_tensor(np.asarray(c.val, np.float32), device=gpu))


def pm(X, gpu, extra=0):
    """Parameter-major device copy of agent-major X [n, P]: [P, round_up(n, 4) + extra], NaN padding."""
    n, P = X.shape
    t = torch.full((P, (n + 3) // 4 * 4 + extra), float("nan"), dtype=torch.float32, device=gpu)
    t[:, :n] = torch.as_tensor(np.ascontiguousarray(X.T), device=gpu)
    return t


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def oracle_steps(X, c, steps):
    for _ in range(steps):
        X = oracle.mix_csr(X, c.rowptr, c.col, c.val)
    return X


def run_steps(X, c, gpu, steps, extra=0, nseg=None):
    """W^steps X through ops.mix_csr_pm_steps, agent-major; YT's padding must
    still hold 7.0 and, for a single pass, XT must be untouched and YT the
    result."""
    rp, col, val = csr_dev(c, gpu)
    n = X.shape[0]
    XT = pm(X, gpu, extra)
    X0 = XT.clone()
    YT = torch.full((X.shape[1], (n + 3) // 4 * 4 + extra), 7.0, device=gpu)
    out = ops.mix_csr_pm_steps(XT, YT, rp, col, val, steps, nseg=nseg)
    torch.cuda.synchronize()
    assert (YT[:, n:] == 7.0).all(), "wrote past the last agent"
    if steps <= ops.PM_MAX_FUSED_STEPS:
        assert out is YT
        assert same_bits(XT, X0), "XT changed"
    else:
        assert torch.isnan(XT[:, n:]).all(), "wrote past the last agent of XT"
    return np.ascontiguousarray(out[:, :n].cpu().numpy().T)


@functools.lru_cache(maxsize=None)
def _regular_case(n, P):
    """(W, X, {steps: W^steps X}) for the size sweep: one oracle chain per shape."""
    c = G.random_regular_csr(n, 4, seed=n + 3)
    X = np.random.default_rng(n * 7 + P).standard_normal((n, P)).astype(np.float32)
    want, Y = {}, X
    for k in range(1, 6):
        Y = oracle.mix_csr(Y, c.rowptr, c.col, c.val)
        want[k] = Y
    return c, X, want


@pytest.mark.parametrize("steps", [2, 3, 5])
@pytest.mark.parametrize("P", [1, 7, 300])
@pytest.mark.parametrize("n", [5, 64, 100, 257, 1000, 1024, 1025, 4096, 4097, 8192])
def test_steps_random_regular_vs_oracle(n, P, steps, gpu):
    """Steps 2 and 3 end on different LDS images (scratch / stage); 4096 and
    4097 agents straddle the two geometries; P = 1 and 7 leave most of a
    stage's p-rows dead."""
    c, X, want = _regular_case(n, P)
    assert bits_equal(run_steps(X, c, gpu, steps, extra=4 * (n % 3)), want[steps])


@pytest.mark.parametrize("n,P", [(1024, 4099), (4097, 3000)])
def test_steps_many_stages_per_workgroup(n, P, gpu):
    """Every workgroup cycles its LDS-DMA ring many times with the LDS-only
    barriers inside, and the last stage is ragged."""
    c = G.random_regular_csr(n, 4, seed=n + 11)
    X = np.random.default_rng(n + P).standard_normal((n, P)).astype(np.float32)
    assert bits_equal(run_steps(X, c, gpu, 3), oracle_steps(X, c, 3))


@functools.lru_cache(maxsize=None)
def _circle_case():
    torch.manual_seed(2028)
    c = G.communication_csr("circle", "stochastic", 1000)[0]
    X = np.random.default_rng(1).standard_normal((1000, 2500)).astype(np.float32)
    return c, X, oracle_steps(X, c, 3)


@pytest.mark.parametrize("nseg", [1, 8, 7])
def test_steps_stage_orders_bit_identical(nseg, gpu):
    """The stage order is a speed choice only; 7 does not divide the grid and
    falls back to one sweep."""
    c, X, want = _circle_case()
    assert bits_equal(run_steps(X, c, gpu, 3, nseg=nseg), want)


def test_one_step_is_the_plain_mix(gpu):
    c = G.random_regular_csr(777, 4, seed=5)
    X = np.random.default_rng(2).standard_normal((777, 1001)).astype(np.float32)
    rp, col, val = csr_dev(c, gpu)
    XT = pm(X, gpu)
    YT = torch.full_like(XT, 7.0)
    ops.mix_csr_pm(XT, YT, rp, col, val)
    assert bits_equal(run_steps(X, c, gpu, 1), np.ascontiguousarray(YT[:, :777].cpu().numpy().T))


def test_eight_steps_equal_eight_launches(gpu):
    c = G.random_regular_csr(777, 4, seed=5)
    X = np.random.default_rng(3).standard_normal((777, 1001)).astype(np.float32)
    rp, col, val = csr_dev(c, gpu)
    A, B = pm(X, gpu), torch.full((1001, 780), 7.0, device=gpu)
    for _ in range(8):
        ops.mix_csr_pm(A, B, rp, col, val)
        A, B = B, A
    assert bits_equal(run_steps(X, c, gpu, 8), np.ascontiguousarray(A[:, :777].cpu().numpy().T))


def test_steps_long_rows_and_nonfinite(gpu):
    """The complete graph (degree 39): every row takes the memory fallback at
    every step, gathering from the current LDS image; Inf, NaN, -0 and a
    denormal go through three steps like the oracle's."""
    torch.manual_seed(2028)
    c = G.csr_from_dense(G.communication_graph("compelete", "stochastic", 40)[0])
    X = np.random.default_rng(5).standard_normal((40, 333)).astype(np.float32)
    X[3, 7], X[9, 8], X[11, 9], X[12, 10] = np.inf, np.nan, -0.0, 1e-40
    assert bits_equal(run_steps(X, c, gpu, 3), oracle_steps(X, c, 3))


def test_steps_empty_rows(gpu):
    """The dynamic topology (one edge per step): empty rows give +0 at every
    step, and the zeros propagate."""
    torch.manual_seed(2028)
    rng = np.random.default_rng(6)
    for Wt in G.communication_graph("dynamic", "stochastic", 9)[:3]:
        c = G.csr_from_dense(Wt)
        X = rng.standard_normal((9, 50)).astype(np.float32)
        X[0, :5] = np.inf
        X[1, 5:9] = np.nan
        assert bits_equal(run_steps(X, c, gpu, 2), oracle_steps(X, c, 2))


@pytest.mark.parametrize("n,steps", [(6, 50), (6, 51), (5, 64)])
def test_steps_ring_parity(n, steps, gpu):
    """The even ring is bipartite, so 50 and 51 steps differ in kind; the odd
    ring runs the largest single pass."""
    torch.manual_seed(2028)
    c = G.communication_csr("circle", "stochastic", n)[0]
    X = np.random.default_rng(n + steps).standard_normal((n, 37)).astype(np.float32)
    assert bits_equal(run_steps(X, c, gpu, steps), oracle_steps(X, c, steps))


def test_steps_above_the_cap(gpu):
    """65 steps through ops are two passes (64 + 1) whose result ends in XT;
    the library itself refuses 65 and names the cap."""
    c = G.random_regular_csr(101, 4, seed=9)
    X = np.random.default_rng(8).standard_normal((101, 70)).astype(np.float32)
    assert ops.pm_steps_passes(101, 65) == [64, 1]
    assert bits_equal(run_steps(X, c, gpu, 65), oracle_steps(X, c, 65))
    rp, col, val = csr_dev(c, gpu)
    XT, YT = pm(X, gpu), torch.zeros(70, 104, device=gpu)
    with pytest.raises(ops.DolNativeError, match=r"outside \[1, 64\]"):
        ops._native.call("dol_mix_csr_pm_steps_f32", XT.data_ptr(), 104, YT.data_ptr(), 104, 101, 70, rp.data_ptr(),
                         col.data_ptr(), val.data_ptr(), 65, torch.cuda.current_stream(gpu).cuda_stream)


# --- the fused round: W^k, then config 3's local steps ---

MODES = [(0.0, False), (0.9, True), (0.9, False)]


def _dgd_steps(X, T, M, c, gpu, objective, mix_steps, steps, lr, momentum, first, extra=0):
    rp, col, val = csr_dev(c, gpu)
    n = X.shape[0]
    XT, TT = pm(X, gpu, extra), pm(T, gpu, extra)
    MT = pm(M, gpu, extra) if momentum else None
    X0 = XT.clone()
    YT = torch.full((X.shape[1], (n + 3) // 4 * 4 + extra), 7.0, device=gpu)
    out = ops.dgd_csr_pm_steps(XT, YT, rp, col, val, TT, MT, objective=objective, mix_steps=mix_steps, steps=steps,
                               lr=lr, momentum=momentum, first_step=first)
    torch.cuda.synchronize()
    assert out is YT and same_bits(XT, X0)
    assert (YT[:, n:] == 7.0).all(), "wrote past the last agent"
    Mo = None
    if momentum:
        assert torch.isnan(MT[:, n:]).all(), "momentum written past the last agent"
        Mo = np.ascontiguousarray(MT[:, :n].cpu().numpy().T)
    return np.ascontiguousarray(YT[:, :n].cpu().numpy().T), Mo


@pytest.mark.parametrize("momentum,first", MODES)
@pytest.mark.parametrize("P", [1, 300])
@pytest.mark.parametrize("n", [5, 1000, 1025, 4096])
def test_dgd_steps_least_squares_vs_oracle(n, P, momentum, first, gpu):
    c = G.random_regular_csr(n, 4, seed=n + 11)
    rng = np.random.default_rng(n + 13 * P)
    X, T, M = (rng.standard_normal((n, P)).astype(np.float32) for _ in range(3))
    got_y, got_m = _dgd_steps(X, T, M, c, gpu, "least_squares", 3, 2, 0.05, momentum, first, extra=4 * (n % 2))
    want_y, want_m = oracle.dgd_local(oracle_steps(X, c, 3), T, M if momentum else None, "least_squares", 2, 0.05,
                                      momentum, first)
    assert bits_equal(got_y, want_y)
    if momentum:
        assert bits_equal(got_m, want_m)


@pytest.mark.parametrize("momentum,first", MODES)
def test_dgd_steps_logistic_matches_agent_major_kernels(momentum, first, gpu):
    """Logistic calls expf: bit-identical to two ops.mix_csr and one
    ops.dgd_csr on the agent-major matrices (same device libm), and within
    test_pmajor_gpu's stated tolerance (rtol 2e-6, atol 1e-6) of the glibc
    oracle."""
    n, P = 1000, 257
    c = G.random_regular_csr(n, 4, seed=n)
    rng = np.random.default_rng(n + P)
    X, T, M = (rng.standard_normal((n, P)).astype(np.float32) for _ in range(3))
    got_y, got_m = _dgd_steps(X, T, M, c, gpu, "logistic", 3, 2, 0.1, momentum, first)
    rp, col, val = csr_dev(c, gpu)
    Xd, Td = (torch.as_tensor(a, device=gpu) for a in (X, T))
    Md = torch.as_tensor(M, device=gpu) if momentum else None
    Y1, Y2, Yd = (torch.empty_like(Xd) for _ in range(3))
    ops.mix_csr(Xd, Y1, rp, col, val)
    ops.mix_csr(Y1, Y2, rp, col, val)
    ops.dgd_csr(Y2, Yd, rp, col, val, Td, Md, objective="logistic", steps=2, lr=0.1, momentum=momentum,
                first_step=first)
    assert bits_equal(got_y, Yd.cpu().numpy())
    if momentum:
        assert bits_equal(got_m, Md.cpu().numpy())
    want_y, _ = oracle.dgd_local(oracle_steps(X, c, 3), T, M if momentum else None, "logistic", 2, 0.1, momentum,
                                 first)
    np.testing.assert_allclose(got_y, want_y, rtol=2e-6, atol=1e-6)


def test_separable_dgd_pm_consensus_steps(gpu):
    """consensus_steps = 3: four rounds equal, bit for bit, a second problem
    from the same state on which each round is two plain mixes and round();
    mix(5) equals five single mixes."""
    from dolhip.synthetic import SeparableDGD, SeparableDGDPM
    plan = G.MixingPlan(G.random_regular_csr(777, 4, seed=3), gpu)
    a = SeparableDGD(plan, 1001, objective="least_squares", lr=0.05, momentum=0.9, local_steps=2, seed=11)
    a.round()
    b = SeparableDGDPM.from_agent_major(a, consensus_steps=3)
    c = SeparableDGDPM.from_agent_major(a)

    def single_mix(p):
        ops.mix_csr_pm(p.XT, p.YT, plan.rowptr, plan.col, plan.val, P=p.P)
        p.XT, p.YT = p.YT, p.XT

    for _ in range(4):
        b.round()
        single_mix(c)
        single_mix(c)
        c.round()
    torch.cuda.synchronize()
    assert b.rounds == c.rounds == 5
    assert bits_equal(b.params().cpu().numpy(), c.params().cpu().numpy())
    assert bits_equal(b.momentum_rows().cpu().numpy(), c.momentum_rows().cpu().numpy())
    b.mix(5)
    for _ in range(5):
        single_mix(c)
    torch.cuda.synchronize()
    assert bits_equal(b.params().cpu().numpy(), c.params().cpu().numpy())


def test_captured_steps_replay_bit_identically(gpu):
    """One mix_csr_pm_steps call with the stage order given captures into a
    graph (the eager call before it has checked W) and replays the same bits."""
    c = G.random_regular_csr(300, 4, seed=4)
    rp, col, val = csr_dev(c, gpu)
    X = np.random.default_rng(4).standard_normal((300, 513)).astype(np.float32)
    XT, YT = pm(X, gpu), torch.zeros(513, 300, device=gpu)
    ops.mix_csr_pm_steps(XT, YT, rp, col, val, 3, nseg=8)
    torch.cuda.synchronize()
    want = YT.clone()
    YT.zero_()
    s = torch.cuda.Stream(device=gpu)
    s.wait_stream(torch.cuda.current_stream(gpu))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            ops.mix_csr_pm_steps(XT, YT, rp, col, val, 3, nseg=8)
    torch.cuda.current_stream(gpu).wait_stream(s)
    YT.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits(YT, want)
    assert bits_equal(np.ascontiguousarray(YT.cpu().numpy().T), oracle_steps(X, c, 3))


def test_steps_argument_errors(gpu, monkeypatch):
    """Every refusal comes before any launch (the library call is replaced by a recorder)."""
    calls = []
    monkeypatch.setattr(ops._native, "call", lambda name, *a: calls.append(name))
    c = G.random_regular_csr(16, 4, seed=1)
    rp, col, val = csr_dev(c, gpu)
    XT, YT = torch.zeros(10, 16, device=gpu), torch.zeros(10, 16, device=gpu)
    with pytest.raises(ValueError, match="steps must be >= 1"):
        ops.mix_csr_pm_steps(XT, YT, rp, col, val, 0)
    with pytest.raises(ValueError, match="steps must be >= 1"):
        ops.dgd_csr_pm_steps(XT, YT, rp, col, val, XT.clone(), mix_steps=0)
    with pytest.raises(ValueError, match="alias"):
        ops.mix_csr_pm_steps(XT, XT, rp, col, val, 2)
    with pytest.raises(ValueError, match="needs MT"):
        ops.dgd_csr_pm_steps(XT, YT, rp, col, val, XT.clone(), mix_steps=2, momentum=0.9)
    # a rectangular W (16 output agents gathering from 20): a column index >= n
    wide = col.clone()
    wide[3] = 17
    with pytest.raises(ValueError, match="square W"):
        ops.mix_csr_pm_steps(torch.zeros(10, 20, device=gpu), torch.zeros(10, 20, device=gpu), rp, wide, val, 2)
    big = G.random_regular_csr(4100, 4, seed=1)
    rpb, colb, valb = csr_dev(big, gpu)
    Z = torch.zeros(3, 4100, device=gpu)
    with pytest.raises(ValueError, match="at most 4096"):
        ops.dgd_csr_pm_steps(Z, Z.clone(), rpb, colb, valb, Z.clone(), mix_steps=2)
    assert calls == []
