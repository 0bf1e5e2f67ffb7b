"""FedAvg and FedProx on least squares (the other two algorithms of BASELINE
config 4's server round), CPU tier.

* The REFERENCE's own FedAvg_Server.run / FedProx_Server.run on a least-squares
  model (tests/golden/fed_ls.npz, made by tests/golden/make_golden_fed_ls.py)
  is replayed bit for bit by a composition of golden-pinned oracle calls: per
  sampled agent w = theta, then local_steps x { g = fl(w - t) in numpy;
  oracle.prox_admm_sgd(theta = None | theta, alpha = None) }, then
  oracle.ordered_mean.  That composition (fed_ls_round_oracle below) is what
  the GPU tier holds dol_fed_ls_round_f32 / dol_fed_ls_round_mean_f32 to.
* dolhip.synthetic.SeparableFedAvg / SeparableFedProx with the composition
  injected as the arithmetic replay the same fixtures, keep no duals, and are
  bit-identical across shardings (gloo ranks, agent blocks and column blocks).
* The argument rules of ops.fed_ls_round / fed_ls_round_mean and of the two
  entry points, without a launch."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import oracle
from conftest import golden
from dolhip import _native, ops, parallel
from oracle import bits_equal
from test_admm_ls_host import _free_port, cpu_ordered_sum
from test_ops_args_gpu import Recorder

CASES = ("mini_mom", "flat_nomom", "mini_full")
ALGORITHMS = ("fedavg", "fedprox")


def fed_ls_round_oracle(algorithm, w, buf, target, theta, agents, first, rho, lr, momentum, local_steps):
    """One FedAvg / FedProx least-squares client round for the sampled rows
    `agents`, composed from the oracle's per-step call; returns (w', buf',
    resid_sq[m]) on copies (buf' None without momentum).  The agents whose
    first-step flags agree go through the oracle together (the step is
    row-wise)."""
    assert algorithm in ALGORITHMS
    w = np.array(w, np.float32)
    buf = None if buf is None or momentum == 0 else np.array(buf, np.float32)
    T = np.asarray(target, np.float32)
    theta = np.asarray(theta, np.float32)
    agents = np.asarray(agents, np.int64)
    first = np.zeros(len(agents), bool) if first is None else np.asarray(first) != 0
    th = theta if algorithm == "fedprox" else None
    for flag in (False, True):
        rows = agents[first == flag]
        if rows.size == 0:
            continue
        wk = np.repeat(theta[None, :], rows.size, axis=0)  # load_state_dict(theta), DEC/clients.py:37
        bk = None if buf is None else buf[rows]
        for step in range(int(local_steps)):
            with np.errstate(invalid="ignore"):  # Inf targets: Inf - Inf is the NaN the kernels give too
                g = (wk - T[rows]).astype(np.float32)
            wk, bk, _ = oracle.prox_admm_sgd(wk, bk, g, th, None, np.float32(rho), np.float32(lr),
                                             np.float32(momentum), flag and step == 0)
        w[rows] = wk
        if buf is not None:
            buf[rows] = bk
    d = (w[agents] - theta[None, :]).astype(np.float32).astype(np.float64)
    return w, buf, (d * d).sum(1)


def replay_oracle(g, algorithm, case):
    key = f"{algorithm}__{case}"
    N, frac, rounds, steps, lr, mom, rho = g[f"{key}__params"]
    N, rounds, steps = int(N), int(rounds), int(steps)
    T = g[f"{key}__targets"]
    P = T.shape[1]
    w = np.zeros((N, P), np.float32)
    buf = np.zeros((N, P), np.float32) if mom != 0 else None
    theta = g[f"{key}__theta0"].copy()
    started = np.zeros(N, bool)
    thetas = []
    for r in range(rounds):
        order = g[f"{key}__orders"][r]
        w, buf, _ = fed_ls_round_oracle(algorithm, w, buf, T, theta, order, ~started[order], rho, lr, mom, steps)
        started[order] = True
        theta = oracle.ordered_mean(w, order)
        thetas.append(theta)
    return np.stack(thetas), w, buf, started


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("algorithm", ALGORITHMS)
def test_composed_oracle_replays_reference_server(algorithm, case):
    g = golden("fed_ls")
    key = f"{algorithm}__{case}"
    thetas, w, buf, started = replay_oracle(g, algorithm, case)
    assert bits_equal(thetas, g[f"{key}__thetas"])
    # clients never sampled keep the global init in the reference; compare the sampled ones
    assert started.any() and bits_equal(w[started], g[f"{key}__w"][started])
    if buf is not None:
        assert bits_equal(buf, g[f"{key}__mom"])


def test_fixture_algorithms_differ():
    """The two fixtures are not one trajectory twice (rho != 0 in every case)."""
    g = golden("fed_ls")
    for case in CASES:
        assert not bits_equal(g[f"fedavg__{case}__thetas"], g[f"fedprox__{case}__thetas"])
        assert bits_equal(g[f"fedavg__{case}__orders"], g[f"fedprox__{case}__orders"])


# ---------------------------------------------------------------------------
# SeparableFedAvg / SeparableFedProx with the composition as the arithmetic
# ---------------------------------------------------------------------------
def cpu_fed_ls_round(algorithm):
    """A round_fn for SeparableADMM(algorithm=...) on CPU tensors: the
    signature of ops.admm_ls_round, called with alpha = alpha_sq = None."""
    def round_fn(w, alpha, target, theta, agents=None, first=None, buf=None, rho=0.1, lr=0.1, momentum=0.0,
                 local_steps=1, resid_sq=None, alpha_sq=None, work=None, P=None):
        assert alpha is None and alpha_sq is None
        P = w.shape[1] if P is None else P
        ag = agents.numpy() if agents is not None else np.arange(w.shape[0])
        fs = first.numpy() if first is not None else None
        wn, bn, rw = fed_ls_round_oracle(algorithm, w[:, :P].numpy(), None if buf is None else buf[:, :P].numpy(),
                                         target[:, :P].numpy(), theta[:P].numpy(), ag, fs, rho, lr, momentum,
                                         local_steps)
        w[:, :P] = torch.from_numpy(wn)
        if buf is not None and bn is not None:
            buf[:, :P] = torch.from_numpy(bn)
        if resid_sq is not None:
            resid_sq[:] = torch.from_numpy(rw)
    return round_fn


def problem_class(algorithm):
    from dolhip.synthetic import SeparableFedAvg, SeparableFedProx
    return {"fedavg": SeparableFedAvg, "fedprox": SeparableFedProx}[algorithm]


def cpu_problem(algorithm, N, P, **kw):
    return problem_class(algorithm)(N, P, device="cpu", round_fn=cpu_fed_ls_round(algorithm),
                                    ordered_sum=cpu_ordered_sum, **kw)


def _run(algorithm, N, P, rounds, **kw):
    s = cpu_problem(algorithm, N, P, **kw)
    for _ in range(rounds):
        s.round()
    return s


def replay_problem(s, g, algorithm, case):
    """Drive s (a SeparableFedAvg / SeparableFedProx of the fixture's shape,
    on any device) through the fixture's rounds; asserts every round's theta
    and the final rows."""
    key = f"{algorithm}__{case}"
    rounds = int(g[f"{key}__params"][2])
    mom = g[f"{key}__params"][5]
    T = g[f"{key}__targets"]
    N, P = T.shape
    s.target[:, :P] = torch.as_tensor(T, device=s.device)
    s.theta[:P] = torch.as_tensor(g[f"{key}__theta0"], device=s.device)
    sampled = np.zeros(N, bool)
    for r in range(rounds):
        order = g[f"{key}__orders"][r]
        s.round(order=order)
        sampled[order] = True
        assert bits_equal(s.theta[:P].cpu().numpy(), g[f"{key}__thetas"][r]), f"round {r}"
    assert bits_equal(s.w[:N, :P].cpu().numpy()[sampled], g[f"{key}__w"][sampled])
    if mom != 0:
        assert bits_equal(s.mom[:N, :P].cpu().numpy(), g[f"{key}__mom"])
    assert s.alpha is None
    h = s.history
    assert [sorted(e) for e in h] == [["dual_sq", "primal_resid_sq", "round"]] * rounds
    assert [e["round"] for e in h] == list(range(rounds))
    assert all(e["dual_sq"] == 0.0 and e["primal_resid_sq"] >= 0.0 for e in h)


def fixture_kw(g, algorithm, case):
    N, frac, rounds, steps, lr, mom, rho = g[f"{algorithm}__{case}__params"]
    return dict(rho=rho, lr=lr, momentum=mom, local_steps=int(steps), frac=frac)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("algorithm", ALGORITHMS)
def test_separable_problem_replays_reference_server(algorithm, case):
    g = golden("fed_ls")
    N, P = g[f"{algorithm}__{case}__targets"].shape
    replay_problem(cpu_problem(algorithm, N, P, **fixture_kw(g, algorithm, case)), g, algorithm, case)


KW = dict(rho=0.1, lr=0.1, momentum=0.5, local_steps=3, frac=0.6, seed=5)


@pytest.mark.parametrize("algorithm", ALGORITHMS)
def test_column_sharded_one_process_is_the_agent_path(algorithm):
    a = _run(algorithm, 11, 70, 3, **KW)
    b = _run(algorithm, 11, 70, 3, shard="columns", **KW)
    assert a.alpha is None and b.alpha is None
    assert bits_equal(b.theta[:70].numpy(), a.theta[:70].numpy())
    assert bits_equal(b.w[:11, :70].numpy(), a.w[:11, :70].numpy())
    assert bits_equal(b.mom[:11, :70].numpy(), a.mom[:11, :70].numpy())
    assert a.history == b.history and len(a.history) == 3
    assert a.algorithm == algorithm and not a.duals


def test_algorithm_argument():
    from dolhip.synthetic import SeparableADMM
    s = SeparableADMM(4, 8, device="cpu", round_fn=cpu_fed_ls_round("fedprox"), ordered_sum=cpu_ordered_sum,
                      algorithm="fedprox")
    assert s.alpha is None and s.algorithm == "fedprox"
    with pytest.raises(ValueError, match="algorithm"):
        SeparableADMM(4, 8, device="cpu", algorithm="scaffold")


# Full participation at 64 x 10000 (the GPU tier runs the same problem on the
# kernels, tests/test_fed_ls_gpu.py): distance_to_optimum() after
# CONVERGENCE_ROUNDS rounds, as this CPU replay gives it, and the bound both
# tiers assert, one decade above (the kernels produce the oracle's bits, so
# no other margin).  From 1.0 at theta_0: 2.8e-4 / 3.6e-4 after 10 rounds,
# these after 20, and theta's fp32 rounding floor, 2.1e-8, from 30 on.
CONVERGENCE_KW = dict(rho=0.1, lr=0.2, momentum=0.5, local_steps=2, frac=1.0, seed=4)
CONVERGENCE_ROUNDS = 20
CONVERGENCE_CPU = {"fedavg": 1.0917e-06, "fedprox": 7.1098e-07}
CONVERGENCE_BOUND = {k: 10.0 * v for k, v in CONVERGENCE_CPU.items()}


def convergence_problem(s):
    """The 64 x 10000 problem on s's device, from one numpy stream (the same
    targets and theta_0 whatever the device)."""
    rng = np.random.default_rng(64)
    s.target[:, :s.P] = torch.as_tensor(rng.standard_normal((s.N, s.P)).astype(np.float32), device=s.device)
    s.theta[:s.P] = torch.as_tensor(rng.standard_normal(s.P).astype(np.float32), device=s.device)
    return s


@pytest.mark.parametrize("algorithm", ALGORITHMS)
def test_full_participation_converges_to_the_optimum(algorithm):
    """fixed_point() is optimum() for FedAvg / FedProx: with every client
    sampled the mean follows one client's iteration on mean_k t_k."""
    s = convergence_problem(cpu_problem(algorithm, 64, 10000, **CONVERGENCE_KW))
    d0 = s.distance_to_optimum()
    for _ in range(CONVERGENCE_ROUNDS):
        s.round()
    d = s.distance_to_optimum()
    print(f"{algorithm}: distance_to_optimum {d0:.3e} -> {d:.3e} after {CONVERGENCE_ROUNDS} rounds")
    assert d < CONVERGENCE_BOUND[algorithm]
    assert s.distance_to_fixed_point() == pytest.approx(d, rel=1e-12)
    assert d == pytest.approx(CONVERGENCE_CPU[algorithm], rel=1e-3)  # the recorded value is this run's
    assert torch.equal(s.fixed_point(), s.optimum())


# ---------------------------------------------------------------------------
# over gloo ranks
# ---------------------------------------------------------------------------
def _worker(rank, world, port, N, P, rounds, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    parallel.init_process_group("gloo", rank=rank, world_size=world, timeout_s=120)
    try:
        out = {}
        for algorithm in ALGORITHMS:
            for mode, kw in (("exact", dict(mean="exact")), ("fast", dict(mean="fast")),
                             ("columns", dict(shard="columns"))):
                s = _run(algorithm, N, P, rounds, **kw, **KW)
                assert s.alpha is None
                cols = s.Pl if mode == "columns" else P
                out[algorithm, mode] = (s.lo, s.hi, s.c0, s.c1, s.w[:s.n, :cols].numpy().copy(),
                                        s.mom[:s.n, :cols].numpy().copy(), s.full_theta().numpy().copy(),
                                        [(h["primal_resid_sq"], h["dual_sq"]) for h in s.history])
        q.put((rank, out))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_rounds_match_single_process(world):
    """SeparableFedAvg / SeparableFedProx over gloo ranks: the 'exact' mean and
    shard="columns" are bit-identical to one process (rows, momentum, theta);
    the 'fast' mean is within test_admm_ls_host.py's tolerance of it."""
    N, P, rounds = 13, 45, 4
    ref = {a: _run(a, N, P, rounds, **KW) for a in ALGORITHMS}
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, N, P, rounds, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [out for _, out in sorted((q.get(timeout=180) for _ in range(world)), key=lambda x: x[0])]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for algorithm in ALGORITHMS:
        r0 = ref[algorithm]
        theta = r0.theta[:P].numpy()
        hist = [(h["primal_resid_sq"], h["dual_sq"]) for h in r0.history]
        for mode in ("exact", "fast", "columns"):
            parts = [out[algorithm, mode] for out in res]
            for p in parts:
                if mode == "fast":
                    np.testing.assert_allclose(p[6], theta, rtol=1e-5, atol=1e-6)
                else:
                    assert bits_equal(p[6], theta), (algorithm, mode)
                np.testing.assert_allclose(np.array(p[7]), np.array(hist), rtol=1e-4 if mode == "fast" else 1e-9)
                assert all(h[1] == 0.0 for h in p[7])
            if mode == "fast":
                continue
            axis = 1 if mode == "columns" else 0
            assert bits_equal(np.concatenate([p[4] for p in parts], axis=axis), r0.w[:N, :P].numpy())
            assert bits_equal(np.concatenate([p[5] for p in parts], axis=axis), r0.mom[:N, :P].numpy())


# ---------------------------------------------------------------------------
# argument rules, without a launch
# ---------------------------------------------------------------------------
@pytest.fixture
def rec(monkeypatch):
    r = Recorder()
    monkeypatch.setattr(ops._native, "call", r)
    return r


@pytest.mark.parametrize("op", [ops.fed_ls_round, ops.fed_ls_round_mean])
def test_ops_algorithm_rules(op, rec):
    w, th = torch.zeros(4, 8), torch.zeros(8)
    with pytest.raises(ValueError, match="algorithm must be one of"):
        op(w, None, w.clone(), th, algorithm="scaffold")
    with pytest.raises(ValueError, match="'fedadmm' needs alpha"):
        op(w, None, w.clone(), th, algorithm="fedadmm")
    with pytest.raises(ValueError, match="'fedavg' has no duals"):
        op(w, w.clone(), w.clone(), th, algorithm="fedavg")
    with pytest.raises(ops.DolNativeError, match="cpu"):  # and no CPU path either
        op(w, None, w.clone(), th, algorithm="fedprox")
    assert rec.calls == []


def test_ops_alpha_sq_is_refused_without_duals(rec):
    w, th = torch.zeros(4, 8), torch.zeros(8)
    with pytest.raises(ValueError, match="'fedprox' has no duals .alpha_sq must be None."):
        ops.fed_ls_round(w, None, w.clone(), th, algorithm="fedprox", resid_sq=torch.zeros(4, dtype=torch.float64),
                         alpha_sq=torch.zeros(4, dtype=torch.float64))
    assert rec.calls == []


class _OnGpu(torch.Tensor):
    """A host tensor that says it is on cuda:0, so that the wrappers' checks
    past "no CPU path" run without a GPU; nothing is launched on it."""
    device = property(lambda self: torch.device("cuda", 0))


def _gpu(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype).as_subclass(_OnGpu)


def _ids(*ids):
    return torch.tensor(ids, dtype=torch.int32).as_subclass(_OnGpu)


_F64 = torch.float64
# the argument errors of the round (first block) and round + mean (second) wrappers: what to pass wrong
ROUND_ERRORS = {
    "first_dtype": dict(first=_gpu(4)),
    "first_short": dict(first=_gpu(3, dtype=torch.int32)),
    "alpha_rows": dict(alpha=_gpu(3, 8)),
    "alpha_cols": dict(alpha=_gpu(4, 7)),
    "target_rows": dict(target=_gpu(3, 8)),
    "target_cols": dict(target=_gpu(4, 7)),
    "buf_missing": dict(momentum=0.5),
    "buf_rows": dict(momentum=0.5, buf=_gpu(3, 8)),
    "buf_cols": dict(momentum=0.5, buf=_gpu(4, 7)),
    "resid_alone": dict(resid_sq=_gpu(4, dtype=_F64)),
    "resid_sq_short": dict(resid_sq=_gpu(3, dtype=_F64), alpha_sq=_gpu(4, dtype=_F64)),
    "alpha_sq_dtype": dict(resid_sq=_gpu(4, dtype=_F64), alpha_sq=_gpu(4)),
}
MEAN_ERRORS = {k: v for k, v in ROUND_ERRORS.items() if "resid" not in k and "alpha_sq" not in k}
MEAN_ERRORS.update({
    "out_short": dict(out=_gpu(7)),
    "out_dtype": dict(out=_gpu(8, dtype=_F64)),
    "out_matrix": dict(out=_gpu(1, 8)),
    "resid_total_short": dict(resid_total=_gpu(1, dtype=_F64)),
    "resid_total_dtype": dict(resid_total=_gpu(2)),
    "no_agents": dict(agents=_ids()),
    "agents_repeated": dict(agents=_ids(1, 2, 1)),
    "agents_out_of_range": dict(agents=_ids(0, 4)),
    "agents_more_than_rows": dict(agents=_ids(0, 1, 2, 3, 0)),
})


@pytest.mark.parametrize("mean,case", [(False, c) for c in sorted(ROUND_ERRORS)] + [(True, c) for c in sorted(MEAN_ERRORS)])
def test_fedadmm_spelling_raises_what_admm_ls_round_raises(mean, case, rec, monkeypatch):
    """ops.admm_ls_round* and fed_ls_round*(..., "fedadmm") are two spellings
    of one body: every argument error is the same exception with the same
    text, apart from the wrapper's name."""
    import contextlib
    monkeypatch.setattr(torch.cuda, "device", lambda d: contextlib.nullcontext())  # the distinct-agents check: no GPU
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    kw = dict(alpha=_gpu(4, 8), target=_gpu(4, 8))
    if mean:
        kw["out"] = _gpu(8)  # given, so that no default is allocated on a GPU
    kw.update((MEAN_ERRORS if mean else ROUND_ERRORS)[case])
    alpha, target = kw.pop("alpha"), kw.pop("target")
    w, theta = _gpu(4, 8), _gpu(8)
    admm, fed = (ops.admm_ls_round_mean, ops.fed_ls_round_mean) if mean else (ops.admm_ls_round, ops.fed_ls_round)
    with pytest.raises(Exception) as a:
        admm(w, alpha, target, theta, **kw)
    with pytest.raises(Exception) as f:
        fed(w, alpha, target, theta, "fedadmm", **kw)
    assert type(a.value) is type(f.value) and isinstance(a.value, (ValueError, TypeError)), (a.value, f.value)
    assert str(a.value).replace("admm_ls_round", "NAME") == str(f.value).replace("fed_ls_round", "NAME")
    assert "NAME" not in str(a.value) and str(a.value)
    assert rec.calls == []


def test_ops_surface():
    assert ops.FED_ALGORITHMS == {"fedavg": 0, "fedprox": 1, "fedadmm": 2}
    assert {"dol_fed_ls_round_f32", "dol_fed_ls_round_mean_f32"} <= set(_native.SIGNATURES)


def test_entry_points_check_arguments_without_launch():
    L = _native.lib()
    fake = 1 << 20  # never dereferenced: every call below fails its argument check first
    A, B, T, TH, OUT = fake + (1 << 16), fake + (2 << 16), fake + (3 << 16), fake + (4 << 16), fake + (5 << 16)

    def rnd(alg, alpha, m=2, alpha_sq=None):
        return L.dol_fed_ls_round_f32(fake, 8, B, 8, alpha, 8, T, 8, TH, None, None, m, 8, alg, 0.1, 0.1, 0.5, 1,
                                      None, alpha_sq, None, None)

    def mean(alg, alpha, m=2, out=OUT):
        return L.dol_fed_ls_round_mean_f32(fake, 8, B, 8, alpha, 8, T, 8, TH, None, None, m, 8, alg, 0.1, 0.1, 0.5,
                                           1, out, 2.0, None, None, None)
    for call in (rnd, mean):
        for alg in (0, 1):
            assert call(alg, A) == -1 and b"alpha must be NULL" in L.dol_last_error()
        for alg in (3, -1):
            assert call(alg, None) == -1 and b"algorithm must be 0" in L.dol_last_error()
    assert rnd(1, None, alpha_sq=fake) == -1 and b"alpha_sq must be NULL" in L.dol_last_error()
    assert rnd(2, None) == -1 and b"null pointer" in L.dol_last_error()  # FedADMM needs its duals
    assert rnd(0, None, m=-1) == -1 and b"negative size" in L.dol_last_error()
    assert rnd(0, None, m=0) == 0  # nothing sampled: nothing to do
    for alg in (0, 1, 2):
        assert mean(alg, A if alg == 2 else None, m=0) == -1 and b"m must be >= 1" in L.dol_last_error()
    for alg, alpha in ((0, None), (1, None), (2, A)):
        for rows in (fake, T, B) + ((A,) if alg == 2 else ()):
            assert mean(alg, alpha, out=rows) == -1 and b"theta_out aliases the rows" in L.dol_last_error()
