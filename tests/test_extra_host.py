"""EXTRA on the agent-major ring and CSR banks (dol_extra_csr_f32,
dol_extra_ring_f32, dol_extra_ring_edges_f32, ops.extra_csr / extra_ring /
extra_ring_edges, MixingPlan.apply_extra, SeparableEXTRA,
ShardedRing.extra_step, ColumnSharded.extra_step), CPU tier: nothing is
launched.

* The surface: the SIGNATURES rows, the ops re-exports, the package export.
* The method: tests/extra_cases.py::extra_round64 (the restatement's statements
  in float64) iterated 20 rounds equals the paper's two-step recursion to
  1e-12 on the 9-agent ring and the 16-agent random 4-regular graph with
  Metropolis weights; one float32 round stays within fp32 rounding of it.
* Convergence of the float32 restatement (least squares, P = 8, zero start,
  targets standard normal from seed 2028, lr 0.1, 200 rounds): max |x - mean t|
  <= 1e-5 on both graphs (measured here: 7.0e-7 on the ring, 2.0e-6 on the
  4-regular graph; |sum_i c_i| / (n lr) is 7.3e-7 and 2.0e-6, so the error is
  the floor), where the DGD restatement on the same W, lr and seed stays more
  than 0.05 away (0.68 and 0.45).  After convergence mean_i x_i - mean_i t_i =
  -sum_i c_i / (n lr) to 1e-6 per coordinate (measured: 5.0e-8 and 3.9e-8).
* The entry points' argument rules, called through the library with addresses
  that are never dereferenced: null target / corr / X / Y / weights, short
  ldt / ldc, a bad objective, corr aliasing X, Y or target, X aliasing Y,
  halos passed singly, negative and empty sizes.
* The rules of the three ops with ops._native.call replaced by
  test_ops_args_gpu.Recorder: an unknown objective, a missing target or corr,
  corr aliasing X, Y or target (CPU tensors reach these).  A CPU matrix is
  refused before the layout rules are looked at, so short rows, a non-square W,
  halos passed singly and the accepted calls' argument tuples use device
  tensors: those tests carry the gpu marker, still with the Recorder and
  without a launch.
* MixingPlan.apply_extra's routing by kind and SeparableEXTRA's refusals.
* ShardedRing.extra_step (worlds 2 and 3 over gloo, N = 11, P = 130, with and
  without the one-launch edge entry) and ColumnSharded.extra_step (world 1
  in-process, world 2 over gloo) with CPU entries, bit-equal to the
  single-process restatement."""
import multiprocessing as mp
import os
import socket
import types

import numpy as np
import pytest
import torch
import torch.distributed as dist

import dolhip
import extra_cases as E
import gt_cases
import oracle
from dolhip import _native, extra, graph as G, ops, parallel
from dolhip.synthetic import SeparableEXTRA
from test_ops_args_gpu import named, vec

CPU = torch.device("cpu")
F32 = np.float32
OPS = ("extra_csr", "extra_ring", "extra_ring_edges")
GRAPHS = {"ring 9": lambda: E.metropolis_ring(9)[:2], "random 4-regular 16": lambda: E.metropolis_regular(16)}


# ---------------------------------------------------------------------------
# the surface
# ---------------------------------------------------------------------------
def test_surface():
    assert len(_native.SIGNATURES["dol_extra_csr_f32"]) == 17
    assert len(_native.SIGNATURES["dol_extra_ring_f32"]) == len(_native.SIGNATURES["dol_extra_ring_edges_f32"]) == 18
    for op in OPS:
        assert getattr(ops, op) is getattr(extra, op)
    assert dolhip.SeparableEXTRA is SeparableEXTRA
    assert callable(G.MixingPlan.apply_extra)
    assert callable(parallel.ShardedRing.extra_step) and callable(parallel.ColumnSharded.extra_step)


# ---------------------------------------------------------------------------
# the method
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("graph", list(GRAPHS))
def test_the_round_is_the_papers_recursion(graph):
    c, d = GRAPHS[graph]()
    W = E.dense64(c, d)
    assert np.abs(W - W.T).max() == 0 and np.abs(W.sum(1) - 1).max() <= 1e-7 and W.diagonal().min() > 0
    n = c.n_rows
    T, X0 = (np.random.default_rng(s).standard_normal((n, 8)) for s in (1, 2))
    want = E.paper_recursion(X0, T, W, 0.1, 20)
    X, C, worst = X0, np.zeros_like(X0), 0.0
    for k in range(20):
        X, C = E.extra_round64(X, C, T, W, 0.1)
        worst = max(worst, np.abs(X - want[k + 1]).max())
    print(f"{graph}: max |restatement - paper recursion| over 20 rounds {worst:.3g}")
    assert worst <= 1e-12


@pytest.mark.parametrize("graph", list(GRAPHS))
def test_the_float32_restatement_is_the_float64_one_rounded(graph):
    """One round from standard normal x, c, t: at most a dozen roundings of
    values below 16 per output, each <= 2^-24 relative: 12 * 16 * 6e-8 < 2e-5."""
    c, d = GRAPHS[graph]()
    X, C, T = gt_cases.problem(c.n_rows, 8, 5)
    xn, cn = E.extra_round(X, C, T, c, d, 0.1)
    x64, c64 = E.extra_round64(*(a.astype(np.float64) for a in (X, C, T)), E.dense64(c, d), float(F32(0.1)))
    assert np.abs(xn - x64).max() <= 2e-5 and np.abs(cn - c64).max() <= 2e-5


@pytest.mark.parametrize("graph", list(GRAPHS))
def test_host_round_reaches_the_optimum_where_dgd_is_biased(graph):
    c, d = GRAPHS[graph]()
    n, lr = c.n_rows, 0.1
    X, C, T, Xd = E.replay(c, d, lr, 200)
    opt = T.astype(np.float64).mean(0)
    err = np.abs(X.astype(np.float64) - opt).max()
    err_dgd = np.abs(Xd.astype(np.float64) - opt).max()
    floor = np.abs(C.astype(np.float64).sum(0)).max() / (n * lr)
    print(f"{graph}: max |x - mean t| after 200 rounds: EXTRA {err:.3g} (|sum c| / (n lr) = {floor:.3g}), DGD {err_dgd:.3g}")
    assert err <= 1e-5
    assert err_dgd > 0.05


@pytest.mark.parametrize("graph", list(GRAPHS))
def test_the_floor_is_the_drift_of_the_corrections_sum(graph):
    c, d = GRAPHS[graph]()
    n, lr = c.n_rows, 0.1
    X, C, T, _ = E.replay(c, d, lr, 200)
    gap = X.astype(np.float64).mean(0) - T.astype(np.float64).mean(0)
    want = -C.astype(np.float64).sum(0) / (n * lr)
    print(f"{graph}: max |(mean x - mean t) + sum c / (n lr)| {np.abs(gap - want).max():.3g}")
    assert np.abs(gap - want).max() <= 1e-6


# ---------------------------------------------------------------------------
# the entry points' argument rules, without a launch
# ---------------------------------------------------------------------------
FAKE = 1 << 20  # never dereferenced: every refused call returns from its argument checks
X_, Y_, T_, C_, RP, COL, VAL, WS, WP, WN, HP, HN = (FAKE + (k << 16) for k in range(12))


def _entry(name):
    L = _native.lib()

    def call(x=X_, y=Y_, n=8, P=8, ld=8, ldt=None, ldc=None, t=T_, c=C_, ws=None, objective=0, rp=RP, col=COL, val=VAL,
             wp=WP, wn=WN, hp=None, hn=None):
        ldt, ldc = (ld if v is None else v for v in (ldt, ldc))
        if name == "dol_extra_csr_f32":
            return L.dol_extra_csr_f32(x, ld, y, ld, n, P, rp, col, val, ws, t, ldt, c, ldc, objective, 0.1, None)
        return getattr(L, name)(x, ld, y, ld, n, P, hp, hn, wp, wn, ws, t, ldt, c, ldc, objective, 0.1, None)

    def refused(word, **kw):
        assert call(**kw) == -1, kw
        msg = L.dol_last_error()
        assert name.encode() in msg and word in msg, (kw, msg)
    return L, call, refused


@pytest.mark.parametrize("name", ["dol_extra_csr_f32", "dol_extra_ring_f32", "dol_extra_ring_edges_f32"])
def test_entry_points_check_arguments_without_launch(name):
    L, call, refused = _entry(name)
    both = dict(hp=HP, hn=HN) if name == "dol_extra_ring_edges_f32" else {}
    for ws in (None, WS):  # self_w alone may be null (and the ring's halos)
        refused(b"null target", t=None, ws=ws, **both)
        refused(b"null corr", c=None, ws=ws, **both)
        for kw in (dict(x=None), dict(y=None)) + ((dict(rp=None), dict(col=None), dict(val=None))
                                                  if name == "dol_extra_csr_f32" else (dict(wp=None), dict(wn=None))):
            refused(b"null pointer", ws=ws, **kw, **both)
    refused(b"ldt < P", ldt=7, **both)
    refused(b"ldc < P", ldc=7, **both)
    refused(b": ld < P", ld=7, ldt=8, ldc=8, **both)
    refused(b"objective must be 0", objective=2, **both)
    refused(b"objective must be 0", objective=-1, **both)
    for kw in (dict(c=X_), dict(c=Y_), dict(c=T_)):
        refused(b"corr aliases X, Y or target", **kw, **both)
    refused(b"X and Y alias", y=X_, **both)
    if name == "dol_extra_ring_f32":
        refused(b"pass both halos or neither", hp=HP)
        refused(b"pass both halos or neither", hn=HN)
        refused(b"n_rows >= 3", n=2)
    if name == "dol_extra_ring_edges_f32":
        refused(b"null pointer", hp=HP)
        refused(b"null pointer", hn=HN)
    refused(b"negative size", n=-1, **both)
    refused(b"negative size", P=-1, **both)
    refused(b"size above 2^40", P=(1 << 40) + 1, ld=(1 << 40) + 1, **both)
    # nothing to do: DOL_OK whatever else is passed, nothing launched
    assert call(n=0) == 0 and call(P=0) == 0 and call(n=0, t=None, c=None, objective=5) == 0
    assert L.dol_last_error() == b""


# ---------------------------------------------------------------------------
# the ops before the library is reached
# ---------------------------------------------------------------------------
@pytest.fixture
def rec(monkeypatch):
    return gt_cases.recorder(monkeypatch)


@pytest.mark.parametrize("op", OPS)
def test_unknown_objective_is_refused(op, rec):
    with pytest.raises(ValueError, match=f"{op}: objective must be one of"):
        E.host_call(op, E.host_args(op, CPU), objective="hinge")
    assert rec.calls == []


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("name", ["target", "corr"])
def test_a_missing_target_or_corr_is_refused(op, name, rec):
    t = E.host_args(op, CPU)
    t[name] = None
    with pytest.raises(TypeError, match=f"{op}: {name}: expected a torch.Tensor"):
        E.host_call(op, t)
    assert rec.calls == []


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("other", ["X", "Y", "target"])
def test_corr_aliasing_another_matrix_is_refused(op, other, rec):
    t = E.host_args(op, CPU)
    t["corr"] = t[other]
    with pytest.raises(ValueError, match=f"{op}: corr and {other} alias"):
        E.host_call(op, t)
    t["corr"] = t[other][:, :t[other].shape[1]]  # another view of the same rows
    with pytest.raises(ValueError, match=f"{op}: corr and {other} alias"):
        E.host_call(op, t)
    assert rec.calls == []


@pytest.mark.parametrize("op", OPS)
def test_cpu_tensors_are_refused(op, rec):
    with pytest.raises(ops.DolNativeError, match="cpu"):
        E.host_call(op, E.host_args(op, CPU), self_weight=vec(CPU, 4), objective="logistic", lr=0.5, P=10)
    assert rec.calls == []


@pytest.mark.gpu
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("name", ["target", "corr"])
def test_short_rows_are_refused(op, name, gpu, rec):
    t = E.host_args(op, gpu)
    t[name] = t[name][:, :9]  # 9 columns < P = 10
    with pytest.raises(ValueError, match=f"{name}: has 9 columns < P=10"):
        E.host_call(op, t)
    t = E.host_args(op, gpu)
    t[name] = t[name][:3]  # 3 rows < n = 4
    with pytest.raises(ValueError, match=f"{name}: expected >= 4 rows"):
        E.host_call(op, t)
    assert rec.calls == []


@pytest.mark.gpu
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("bad", [lambda dev: vec(dev, 3), lambda dev: vec(dev, 4, torch.float64),
                                 lambda dev: vec(dev, 8)[::2]], ids=["length", "dtype", "stride"])
def test_bad_self_weights_are_refused(op, bad, gpu, rec):
    with pytest.raises(ValueError, match=r"self_weight: expected contiguous float32 \[4\]"):
        E.host_call(op, E.host_args(op, gpu), self_weight=bad(gpu))
    assert rec.calls == []


@pytest.mark.gpu
def test_a_non_square_w_is_refused(gpu, rec):
    t = E.host_args("extra_csr", gpu)
    t["col"][2] = 4  # in place: the square-W check keeps its answers per (buffers, versions)
    with pytest.raises(ValueError, match="needs a square W"):
        E.host_call("extra_csr", t)
    assert rec.calls == []


@pytest.mark.gpu
def test_halos_passed_singly_are_refused(gpu, rec):
    t = E.host_args("extra_ring", gpu)
    for kw in (dict(halo_prev=vec(gpu, 12)), dict(halo_next=vec(gpu, 12))):
        with pytest.raises(ValueError, match="pass both halos or neither"):
            E.host_call("extra_ring", t, **kw)
    t = E.host_args("extra_ring_edges", gpu)
    t["halo_next"] = None
    with pytest.raises(ValueError, match="extra_ring_edges needs both halos"):
        E.host_call("extra_ring_edges", t)
    with pytest.raises(ValueError, match="wrap-around ring needs >= 3 rows"):
        E.host_call("extra_ring", E.host_args("extra_ring", gpu, n=2))
    assert rec.calls == []


@pytest.mark.gpu
def test_the_accepted_calls_reach_the_library_with_these_arguments(gpu, rec):
    t = E.host_args("extra_csr", gpu)
    t["self_weight"] = vec(gpu, 4)
    assert E.host_call("extra_csr", t, self_weight=t["self_weight"], objective="logistic", lr=0.5) is t["Y"]
    E.host_call("extra_csr", t, P=8)
    assert named(rec.calls, t, gpu) == [
        ("dol_extra_csr_f32", "X+0", 12, "Y+0", 12, 4, 10, "rowptr+0", "col+0", "val+0", "self_weight+0", "target+0",
         12, "corr+0", 12, 1, 0.5, "stream"),
        ("dol_extra_csr_f32", "X+0", 12, "Y+0", 12, 4, 8, "rowptr+0", "col+0", "val+0", None, "target+0", 12, "corr+0",
         12, 0, 0.01, "stream")]
    rec.calls.clear()
    t = E.host_args("extra_ring", gpu)
    t.update(self_weight=vec(gpu, 4), halo_prev=vec(gpu, 12), halo_next=vec(gpu, 12))
    assert E.host_call("extra_ring", t, self_weight=t["self_weight"], objective="logistic", lr=0.5) is t["Y"]
    E.host_call("extra_ring", t, halo_prev=t["halo_prev"], halo_next=t["halo_next"], P=8, n_rows=2)
    assert named(rec.calls, t, gpu) == [
        ("dol_extra_ring_f32", "X+0", 12, "Y+0", 12, 4, 10, None, None, "w_prev+0", "w_next+0", "self_weight+0",
         "target+0", 12, "corr+0", 12, 1, 0.5, "stream"),
        ("dol_extra_ring_f32", "X+0", 12, "Y+0", 12, 2, 8, "halo_prev+0", "halo_next+0", "w_prev+0", "w_next+0", None,
         "target+0", 12, "corr+0", 12, 0, 0.01, "stream")]
    rec.calls.clear()
    t = E.host_args("extra_ring_edges", gpu)
    t["self_weight"] = vec(gpu, 4)
    assert E.host_call("extra_ring_edges", t, self_weight=t["self_weight"], lr=0.5, n_rows=3) is t["Y"]
    assert named(rec.calls, t, gpu) == [
        ("dol_extra_ring_edges_f32", "X+0", 12, "Y+0", 12, 3, 10, "halo_prev+0", "halo_next+0", "w_prev+0", "w_next+0",
         "self_weight+0", "target+0", 12, "corr+0", 12, 0, 0.5, "stream")]


# ---------------------------------------------------------------------------
# MixingPlan.apply_extra and SeparableEXTRA
# ---------------------------------------------------------------------------
def test_apply_extra_routes_by_kind(monkeypatch, rec):
    seen = []
    monkeypatch.setattr(ops, "extra_csr", lambda *a, **k: seen.append(("csr", a, k)) or a[1])
    monkeypatch.setattr(ops, "extra_ring", lambda *a, **k: seen.append(("ring", a, k)) or a[1])
    c9 = gt_cases.ring(9)[0]
    t = E.host_args("extra_ring", CPU, n=9)
    four = tuple(t[k] for k in ("X", "Y", "target", "corr"))
    kw = dict(self_weight=vec(CPU, 9), objective="logistic", lr=0.5, P=10)

    csr = G.MixingPlan(c9, CPU, allow_ring=False)
    assert csr.kind == "csr" and csr.apply_extra(*four, **kw) is t["Y"]
    kind, a, k = seen.pop()
    want = (t["X"], t["Y"], csr.rowptr, csr.col, csr.val, t["target"], t["corr"])
    assert kind == "csr" and k == kw and len(a) == len(want) and all(x is y for x, y in zip(a, want))

    ring = G.MixingPlan(c9, CPU)
    assert ring.kind == "ring" and ring.apply_extra(*four, **kw) is t["Y"]
    kind, a, k = seen.pop()
    want = (t["X"], t["Y"], ring.w_prev, ring.w_next, t["target"], t["corr"])
    assert kind == "ring" and k == dict(kw, n_rows=9) and len(a) == len(want) and all(x is y for x, y in zip(a, want))

    with pytest.raises(NotImplementedError, match="EXTRA rounds are fused into the sparse mixes"):
        G.MixingPlan(c9, CPU, dense=True).apply_extra(*four)
    with pytest.raises(ValueError, match="X has 4 rows; W has 9 columns"):
        csr.apply_extra(t["X"][:4], *four[1:])
    csr._retire()
    with pytest.raises(RuntimeError, match="no longer holds its W"):
        csr.apply_extra(*four)
    assert seen == [] and rec.calls == []


def test_problem_class_refusals(rec):
    c = G.random_regular_csr(8, 4, seed=1)
    with pytest.raises(ValueError, match="sparse"):
        SeparableEXTRA(G.MixingPlan(c, CPU, dense=True), 8)
    with pytest.raises(ValueError, match="objective must be one of"):
        SeparableEXTRA(G.MixingPlan(c, CPU), 8, objective="hinge")
    with pytest.raises(ValueError, match="self_weight: expected 8 weights"):
        SeparableEXTRA(G.MixingPlan(c, CPU), 8, self_weight=np.zeros(9, F32))
    assert rec.calls == []


def test_problem_round_makes_one_call_and_swaps():
    """round() on stand-ins for the plan and the bank: one apply_extra call on
    (x, y, target, corr), then the one swap (corr is updated in place)."""
    calls = []
    prob = SeparableEXTRA.__new__(SeparableEXTRA)
    prob.plan = types.SimpleNamespace(apply_extra=lambda *a, **k: calls.append((a, k)))
    prob.bank = types.SimpleNamespace(buffer=lambda name: name, swap=lambda a, b: calls.append(("swap", a, b)))
    prob.self_weight, prob.objective, prob.lr, prob.P, prob.rounds = "d", "logistic", 0.5, 10, 0
    prob.round()
    assert calls == [(("x", "y", "target", "corr"), dict(self_weight="d", objective="logistic", lr=0.5, P=10)),
                     ("swap", "x", "y")]
    assert prob.rounds == 1


# ---------------------------------------------------------------------------
# the sharded steps with CPU entries
# ---------------------------------------------------------------------------
SH_ROUNDS = 3
RING_N, RING_P = 11, 130
COL_N, COL_P = 24, 130  # column cuts on 64 floats: (0, 130) / (0, 64, 130)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _problem(n, P, seed):
    rng = np.random.default_rng(seed)
    return tuple(rng.standard_normal((n, P)).astype(F32) for _ in range(3))  # X, C (a nonzero start), T


def _unsharded(c, d, n, P, seed):
    X, C, T = _problem(n, P, seed)
    for _ in range(SH_ROUNDS):
        X, C = E.extra_round(X, C, T, c, d, 0.1)
    return X, C


def _ring_rounds(edges):
    """This rank's rows of (x, corr) after SH_ROUNDS extra_step rounds, and its row range."""
    _, d, wp, wn = E.metropolis_ring(RING_N)
    X, C, T = _problem(RING_N, RING_P, 21)
    sh = parallel.ShardedRing(RING_N, RING_P, wp, wn, "cpu", ld=RING_P + 3)
    rows = slice(sh.lo, sh.hi)
    sh.x[:, :RING_P] = torch.from_numpy(X[rows])
    t, corr, dl = (torch.from_numpy(np.ascontiguousarray(a[rows])) for a in (T, C, d))
    for _ in range(SH_ROUNDS):
        x_before = sh.x
        sh.extra_step(t, corr, dl, extra_ring=E.cpu_extra_ring, extra_edges=E.cpu_extra_ring_edges if edges else None,
                      lr=0.1)
        assert sh.y is x_before
    return sh.lo, sh.hi, sh.x[:, :RING_P].numpy().copy(), corr.numpy().copy()


def _ring_worker(rank, world, port, edges, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    parallel.init_process_group("gloo", rank=rank, world_size=world, timeout_s=120)
    try:
        q.put(_ring_rounds(edges))
    finally:
        dist.destroy_process_group()


def _spawn(worker, world, *args):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=worker, args=(r, world, port) + args + (q,)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return res


def test_sharded_ring_extra_step_in_one_process():
    lo, hi, x, corr = _ring_rounds(edges=True)
    c, d = E.metropolis_ring(RING_N)[:2]
    want_x, want_c = _unsharded(c, d, RING_N, RING_P, 21)
    assert (lo, hi) == (0, RING_N) and oracle.bits_equal(x, want_x) and oracle.bits_equal(corr, want_c)


@pytest.mark.parametrize("edges", [True, False], ids=["edge entry", "edges through the ring entry"])
@pytest.mark.parametrize("world", [2, 3])
def test_sharded_ring_extra_step_over_gloo(world, edges):
    """Only the halo rows of x travel; corrections, targets and self weights are
    sliced per rank.  Every rank's rows are the single-process restatement's."""
    c, d = E.metropolis_ring(RING_N)[:2]
    want_x, want_c = _unsharded(c, d, RING_N, RING_P, 21)
    res = _spawn(_ring_worker, world, edges)
    assert sorted((lo, hi) for lo, hi, _, _ in res) == [parallel.shard_bounds(RING_N, world, r) for r in range(world)]
    for lo, hi, x, corr in res:
        assert oracle.bits_equal(x, want_x[lo:hi]) and oracle.bits_equal(corr, want_c[lo:hi])


def _column_rounds():
    """(x, corr) gathered on rank 0 (None elsewhere) after SH_ROUNDS extra_step rounds."""
    c, d = E.metropolis_regular(COL_N)
    X, C, T = _problem(COL_N, COL_P, 22)
    plan = types.SimpleNamespace(n_rows=COL_N, n_cols=COL_N, apply=lambda *a, **k: None, apply_dgd=lambda *a, **k: None)
    sh = parallel.ColumnSharded(plan, COL_P, "cpu")
    cut = lambda A: torch.from_numpy(np.ascontiguousarray(A[:, sh.c0:sh.c1]))  # noqa: E731
    sh.x[:, :sh.Pl] = cut(X)
    t, corr = cut(T), cut(C)
    for _ in range(SH_ROUNDS):
        x_before = sh.x
        sh.extra_step(t, corr, apply_extra=E.cpu_apply_extra(c), self_weight=torch.from_numpy(d), lr=0.1)
        assert sh.y is x_before
    return sh.gather(0), sh.gather(0, src=corr)


def _column_worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    parallel.init_process_group("gloo", rank=rank, world_size=world, timeout_s=120)
    try:
        x, corr = _column_rounds()
        q.put((rank, None if x is None else x.numpy(), None if corr is None else corr.numpy()))
    finally:
        dist.destroy_process_group()


def test_column_sharded_extra_step_in_one_process():
    x, corr = _column_rounds()
    want_x, want_c = _unsharded(*E.metropolis_regular(COL_N), COL_N, COL_P, 22)
    assert oracle.bits_equal(x.numpy(), want_x) and oracle.bits_equal(corr.numpy(), want_c)


def test_column_sharded_extra_step_uses_the_plans_entry():
    calls = []
    plan = types.SimpleNamespace(n_rows=6, n_cols=6, apply=lambda *a, **k: None, apply_dgd=lambda *a, **k: None,
                                 apply_extra=lambda *a, **k: calls.append((a, k)))
    sh = parallel.ColumnSharded(plan, 10, "cpu")
    x, y, z = sh.x, sh.y, torch.zeros(6, sh.ld)
    sh.extra_step(z, z.clone(), lr=0.5)
    assert len(calls) == 1 and all(a is b for a, b in zip(calls[0][0], (x, y, z))) and calls[0][1] == dict(P=10, lr=0.5)
    assert sh.x is y and sh.y is x


def test_column_sharded_extra_step_over_gloo():
    """Column cut at 64: every rank runs the round on its block, no data-path
    communication; the gathered result is the unsharded host round's."""
    res = {r: (x, c) for r, x, c in _spawn(_column_worker, 2)}
    want_x, want_c = _unsharded(*E.metropolis_regular(COL_N), COL_N, COL_P, 22)
    assert oracle.bits_equal(res[0][0], want_x) and oracle.bits_equal(res[0][1], want_c)
    assert res[1] == (None, None)
