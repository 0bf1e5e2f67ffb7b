"""FedAvg and FedProx on least squares on the GPU: dol_fed_ls_round_f32 and the
one-pass dol_fed_ls_round_mean_f32 (ops.fed_ls_round / fed_ls_round_mean,
dolhip.synthetic.SeparableFedAvg / SeparableFedProx).

* Bit for bit the composed oracle of tests/test_fed_ls_host.py (which replays
  the REFERENCE's FedAvg_Server.run / FedProx_Server.run) on
  test_admm_gpu.py's grid: the f4 path, the scalar path (rows off 16-byte
  alignment), the tail, full and partial prefetch groups, 256-lane strips.
* "fedadmm" through the new entry points is ops.admm_ls_round /
  admm_ls_round_mean, bit for bit.
* FedAvg is not FedADMM with rho = 0 (the sign of a zero says so).
* The problem classes replay tests/golden/fed_ls.npz, fused and two-kernel
  rounds agree, full participation converges to the optimum, theta_out may
  be theta, and the one-pass round captures into a graph."""
import numpy as np
import pytest
import torch

import oracle
from conftest import golden
from dolhip import ops
from oracle import bits_equal
from test_fed_ls_host import (ALGORITHMS, CASES, CONVERGENCE_BOUND, CONVERGENCE_KW, CONVERGENCE_ROUNDS,
                              convergence_problem, fed_ls_round_oracle, fixture_kw, problem_class, replay_problem)

pytestmark = pytest.mark.gpu

N = 9
ORDER = np.array([7, 2, 0, 8, 5, 3, 6, 4, 1], np.int32)
FIRST = np.array([1, 0, 1, 0, 0, 1, 1, 0, 0], np.int32)
GRID = [(4096, 0), (1031, 0), (1031, 1), (3, 0), (5000, 3), (70001, 0)]
MOM_STEPS = [(0.5, 3), (0.0, 1), (0.9, 0)]
RHO, LR = 0.1, 0.05


def _inputs(P, seed):
    """T, B, theta with the Inf / -0 / denormal targets of test_admm_gpu.py."""
    rng = np.random.default_rng(seed)
    T = rng.standard_normal((N, P)).astype(np.float32)
    B = rng.standard_normal((N, P)).astype(np.float32)
    th = rng.standard_normal(P).astype(np.float32)
    T[1, :3] = [np.inf, -0.0, 1e-40][:min(3, P)]
    return T, B, th


def _mat(a, ld, gpu):
    """a in a NaN-filled [N, ld] matrix (ld - P columns of padding)."""
    t = torch.full((a.shape[0], ld), float("nan"), device=gpu)
    t[:, :a.shape[1]] = torch.as_tensor(a, device=gpu)
    return t


def _check_rows(w, b, w1, b1, order, P, mom):
    wn = w.cpu().numpy()
    assert bits_equal(wn[order][:, :P], w1[order])
    rest = np.setdiff1d(np.arange(N), order)
    assert bits_equal(wn[rest][:, :P], np.zeros((rest.size, P), np.float32))  # rows not sampled: untouched
    assert np.isnan(wn[:, P:]).all()  # the padding stays NaN
    if mom:
        bn = b.cpu().numpy()
        assert bits_equal(bn[:, :P], b1)
        assert np.isnan(bn[:, P:]).all()


@pytest.mark.parametrize("P,extra", GRID)
@pytest.mark.parametrize("mom,steps", MOM_STEPS)
@pytest.mark.parametrize("algorithm", ALGORITHMS)
def test_fed_ls_round_vs_oracle(algorithm, P, extra, mom, steps, gpu):
    """dol_fed_ls_round_f32: rows bit-identical to the composed oracle, the
    drift ||w_k - theta||^2 within rtol 1e-12 (another fp64 summation order)."""
    T, B, th = _inputs(P, P + steps)
    m = 5
    order, first = ORDER[:m], FIRST[:m]
    w, b, t = _mat(np.zeros((N, P), np.float32), P + extra, gpu), _mat(B, P + extra, gpu), _mat(T, P + extra, gpu)
    rw = torch.full((m,), float("nan"), dtype=torch.float64, device=gpu)
    ops.fed_ls_round(w, None, t, torch.as_tensor(th, device=gpu), algorithm=algorithm,
                     agents=torch.as_tensor(order, device=gpu), first=torch.as_tensor(first, device=gpu),
                     buf=b if mom else None, rho=RHO, lr=LR, momentum=mom, local_steps=steps, resid_sq=rw, P=P)
    torch.cuda.synchronize()
    w1, b1, rw1 = fed_ls_round_oracle(algorithm, np.zeros((N, P), np.float32), B if mom else None, T, th, order,
                                      first, RHO, LR, mom, steps)
    _check_rows(w, b, w1, b1, order, P, mom)
    np.testing.assert_allclose(rw.cpu().numpy(), rw1, rtol=1e-12)


@pytest.mark.parametrize("P,extra", GRID)
@pytest.mark.parametrize("mom,steps", MOM_STEPS)
@pytest.mark.parametrize("m", [5, 1, 6, 9])
@pytest.mark.parametrize("algorithm", ALGORITHMS)
def test_fed_ls_round_mean_vs_oracle(algorithm, P, extra, mom, steps, m, gpu):
    """dol_fed_ls_round_mean_f32: rows bit-identical to the composed oracle,
    theta_out to oracle.ordered_mean (scale None) / ordered_sum (scale 1) of
    the new rows in the sampled order, resid_total[0] to the per-agent drifts
    summed (rtol 1e-12) and resid_total[1] exactly 0.  Groups of three agents
    in flight: m = 6 / 9 end on a full group, 5 / 1 on a partial one."""
    T, B, th = _inputs(P, P + 7 * steps + m)
    order, first = ORDER[:m], FIRST[:m]
    w1, b1, rw1 = fed_ls_round_oracle(algorithm, np.zeros((N, P), np.float32), B if mom else None, T, th, order,
                                      first, RHO, LR, mom, steps)
    for scale in (None, 1.0):
        w, b, t = _mat(np.zeros((N, P), np.float32), P + extra, gpu), _mat(B, P + extra, gpu), _mat(T, P + extra, gpu)
        tot = torch.full((2,), float("nan"), dtype=torch.float64, device=gpu)
        out = ops.fed_ls_round_mean(w, None, t, torch.as_tensor(th, device=gpu), algorithm=algorithm,
                                    agents=torch.as_tensor(order, device=gpu),
                                    first=torch.as_tensor(first, device=gpu), buf=b if mom else None, rho=RHO, lr=LR,
                                    momentum=mom, local_steps=steps, scale=scale, resid_total=tot, P=P)
        torch.cuda.synchronize()
        _check_rows(w, b, w1, b1, order, P, mom)
        want = oracle.ordered_mean(w1, order) if scale is None else oracle.ordered_sum(w1, order)
        assert bits_equal(out.cpu().numpy(), want)
        got = tot.cpu().numpy()
        np.testing.assert_allclose(got[0], rw1.sum(), rtol=1e-12)
        assert got[1] == 0.0


@pytest.mark.parametrize("P", [1031, 4096])
@pytest.mark.parametrize("mom", [0.5, 0.0])
def test_fedadmm_through_the_new_entry_points_is_the_admm_round(P, mom, gpu):
    """algorithm = "fedadmm": the rows, the duals, theta_out and both residuals
    of ops.admm_ls_round / admm_ls_round_mean, bit for bit."""
    T, B, th = _inputs(P, P)
    A = (0.1 * np.random.default_rng(P + 1).standard_normal((N, P))).astype(np.float32)
    m = 5
    agents = torch.as_tensor(ORDER[:m], device=gpu)
    first = torch.as_tensor(FIRST[:m], device=gpu)
    theta = torch.as_tensor(th, device=gpu)
    kw = dict(agents=agents, first=first, rho=RHO, lr=LR, momentum=mom, local_steps=3, P=P)

    def state():
        return [_mat(x, P, gpu) for x in (np.zeros((N, P), np.float32), A, T, B)]

    def res(n):
        return torch.full((n,), float("nan"), dtype=torch.float64, device=gpu)
    w0, a0, t0, b0 = state()
    w1, a1, t1, b1 = state()
    r0, s0, r1, s1 = res(m), res(m), res(m), res(m)
    ops.admm_ls_round(w0, a0, t0, theta, buf=b0 if mom else None, resid_sq=r0, alpha_sq=s0, **kw)
    ops.fed_ls_round(w1, a1, t1, theta, algorithm="fedadmm", buf=b1 if mom else None, resid_sq=r1, alpha_sq=s1, **kw)
    torch.cuda.synchronize()
    for x, y in ((w0, w1), (a0, a1), (b0, b1)):
        assert bits_equal(x.cpu().numpy(), y.cpu().numpy())
    assert np.array_equal(r0.cpu().numpy(), r1.cpu().numpy(), equal_nan=True)
    assert np.array_equal(s0.cpu().numpy(), s1.cpu().numpy(), equal_nan=True)
    w0, a0, t0, b0 = state()
    w1, a1, t1, b1 = state()
    tot0, tot1 = res(2), res(2)
    o0 = ops.admm_ls_round_mean(w0, a0, t0, theta, buf=b0 if mom else None, resid_total=tot0, **kw)
    o1 = ops.fed_ls_round_mean(w1, a1, t1, theta, algorithm="fedadmm", buf=b1 if mom else None, resid_total=tot1,
                               **kw)
    torch.cuda.synchronize()
    for x, y in ((w0, w1), (a0, a1), (b0, b1), (o0, o1)):
        assert bits_equal(x.cpu().numpy(), y.cpu().numpy())
    assert np.array_equal(tot0.cpu().numpy(), tot1.cpu().numpy(), equal_nan=True)


def test_fedavg_is_not_fedadmm_with_rho_zero(gpu):
    """A column with theta = -0.0 and t = +0.0, one step, no momentum:
    FedAvg's fma(-lr, fl(w - t), w) gives +0.0; the ADMM term with rho = 0 and
    alpha = 0, and the prox term with rho = 0, turn the -0 gradient into +0
    and give -0.0.  The oracle says the same."""
    P = 8
    T = np.zeros((2, P), np.float32)
    th = np.full(P, -0.0, np.float32)

    def run(algorithm, alpha):
        w = torch.ones(2, P, device=gpu)
        ops.fed_ls_round(w, alpha, torch.as_tensor(T, device=gpu), torch.as_tensor(th, device=gpu),
                         algorithm=algorithm, rho=0.0, lr=LR, momentum=0.0, local_steps=1)
        out = ops.fed_ls_round_mean(w.clone(), None if alpha is None else torch.zeros_like(alpha),
                                    torch.as_tensor(T, device=gpu), torch.as_tensor(th, device=gpu),
                                    algorithm=algorithm, rho=0.0, lr=LR, momentum=0.0, local_steps=1, scale=1.0,
                                    agents=torch.zeros(1, dtype=torch.int32, device=gpu))
        torch.cuda.synchronize()
        return w.cpu().numpy(), out.cpu().numpy()
    for algorithm, negative in (("fedavg", False), ("fedprox", True), ("fedadmm", True)):
        w, out = run(algorithm, torch.zeros(2, P, device=gpu) if algorithm == "fedadmm" else None)
        assert (w == 0).all() and (out == 0).all()
        assert (np.signbit(w) == negative).all(), algorithm
        assert (np.signbit(out) == negative).all(), algorithm
    order = np.arange(2)
    for algorithm, negative in (("fedavg", False), ("fedprox", True)):
        w1, _, _ = fed_ls_round_oracle(algorithm, np.ones((2, P), np.float32), None, T, th, order, None, 0.0, LR, 0.0, 1)
        assert (w1 == 0).all() and (np.signbit(w1) == negative).all()
    w1, _, _, _, _ = oracle.admm_ls_round(np.ones((2, P), np.float32), None, np.zeros((2, P), np.float32), T, th, order,
                                          None, 0.0, LR, 0.0, 1)
    assert (w1 == 0).all() and np.signbit(w1).all()


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("algorithm", ALGORITHMS)
def test_problem_classes_replay_reference_server(algorithm, case, fused, gpu):
    g = golden("fed_ls")
    n, P = g[f"{algorithm}__{case}__targets"].shape
    s = problem_class(algorithm)(n, P, device=gpu, fused=fused, **fixture_kw(g, algorithm, case))
    assert s.fused == fused and s.alpha is None
    replay_problem(s, g, algorithm, case)


@pytest.mark.parametrize("algorithm", ALGORITHMS)
def test_fused_matches_two_kernel_round(algorithm, gpu):
    kw = dict(rho=0.1, lr=0.1, momentum=0.5, local_steps=3, frac=0.5, seed=9, device=gpu)
    a = problem_class(algorithm)(37, 20003, fused=True, **kw)
    b = problem_class(algorithm)(37, 20003, fused=False, **kw)
    for _ in range(4):
        a.round()
        b.round()
    torch.cuda.synchronize()
    for x, y in ((a.theta, b.theta), (a.w, b.w), (a.mom, b.mom)):
        assert bits_equal(x.cpu().numpy(), y.cpu().numpy())
    for ha, hb in zip(a.history, b.history):
        np.testing.assert_allclose(ha["primal_resid_sq"], hb["primal_resid_sq"], rtol=1e-12)
        assert ha["dual_sq"] == 0.0 and hb["dual_sq"] == 0.0
    assert len(a.history) == 4


@pytest.mark.parametrize("algorithm", ALGORITHMS)
def test_full_participation_converges_to_the_optimum(algorithm, gpu):
    """The CPU tier's 64 x 10000 problem on the kernels: the same bound."""
    s = convergence_problem(problem_class(algorithm)(64, 10000, device=gpu, **CONVERGENCE_KW))
    assert s.fused
    for _ in range(CONVERGENCE_ROUNDS):
        s.round()
    d = s.distance_to_optimum()
    print(f"{algorithm}: distance_to_optimum {d:.4e} after {CONVERGENCE_ROUNDS} rounds")
    assert d < CONVERGENCE_BOUND[algorithm]
    assert s.distance_to_fixed_point() == pytest.approx(d, rel=1e-12)


@pytest.mark.parametrize("algorithm", ALGORITHMS)
def test_theta_out_may_be_theta(algorithm, gpu):
    rng = np.random.default_rng(3)
    n, P = 6, 2051
    T = torch.as_tensor(rng.standard_normal((n, P)).astype(np.float32), device=gpu)
    th = torch.as_tensor(rng.standard_normal(P).astype(np.float32), device=gpu)
    order = torch.as_tensor([4, 1, 3], dtype=torch.int32, device=gpu)
    w1, w2 = torch.zeros(n, P, device=gpu), torch.zeros(n, P, device=gpu)
    ref = ops.fed_ls_round_mean(w1, None, T, th, algorithm=algorithm, agents=order, local_steps=2, P=P)
    th2 = th.clone()
    ops.fed_ls_round_mean(w2, None, T, th2, algorithm=algorithm, agents=order, local_steps=2, out=th2, P=P)
    torch.cuda.synchronize()
    assert bits_equal(th2.cpu().numpy(), ref.cpu().numpy())
    assert bits_equal(w2.cpu().numpy(), w1.cpu().numpy())


def test_round_mean_captures_into_a_graph(gpu):
    """fed_ls_round_mean with `agents` given and the default validate, captured
    with torch.cuda.graph (the host check of the ids is a device-to-host copy:
    not made while capturing) as one linear chain and replayed twice: the
    eager call's bits each time."""
    rng = np.random.default_rng(12)
    n, P, m = 8, 5003, 5
    T = torch.as_tensor(rng.standard_normal((n, P)).astype(np.float32), device=gpu)
    th = torch.as_tensor(rng.standard_normal(P).astype(np.float32), device=gpu)
    B0 = torch.as_tensor(rng.standard_normal((n, P)).astype(np.float32), device=gpu)
    agents = torch.as_tensor([6, 0, 3, 7, 2], dtype=torch.int32, device=gpu)
    first = torch.as_tensor([0, 1, 0, 0, 1], dtype=torch.int32, device=gpu)

    def call(w, b, out, tot):
        return ops.fed_ls_round_mean(w, None, T, th, algorithm="fedprox", agents=agents, first=first, buf=b, rho=RHO,
                                     lr=LR, momentum=0.5, local_steps=3, out=out, resid_total=tot, P=P)
    w0, b0, o0 = torch.zeros(n, P, device=gpu), B0.clone(), torch.zeros(P, device=gpu)
    t0 = torch.zeros(2, dtype=torch.float64, device=gpu)
    call(w0, b0, o0, t0)  # eager; also sizes the shared workspace before the capture
    w, b, o = torch.zeros(n, P, device=gpu), B0.clone(), torch.zeros(P, device=gpu)
    tot = torch.zeros(2, dtype=torch.float64, device=gpu)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call(w, b, o, tot)
    for _ in range(2):
        w.zero_()
        o.zero_()
        tot.fill_(float("nan"))
        b.copy_(B0)
        graph.replay()
        torch.cuda.synchronize()
        for x, y in ((w, w0), (b, b0), (o, o0)):
            assert bits_equal(x.cpu().numpy(), y.cpu().numpy())
        assert np.array_equal(tot.cpu().numpy(), t0.cpu().numpy()) and tot[1].item() == 0.0
    with pytest.raises(ValueError, match="agents must be distinct"):  # eager: the check is made
        ops.fed_ls_round_mean(w, None, T, th, algorithm="fedprox",
                              agents=torch.as_tensor([1, 1], dtype=torch.int32, device=gpu), P=P)
