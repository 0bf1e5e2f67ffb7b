"""Gradient tracking on the parameter-major bank, CPU tier (launch-free:
ops._native.call is replaced by test_ops_args_gpu.Recorder where an op is
called), and the rules the four ops share.

* The rules that ops.gt_csr_pm, ops.gt_ring, ops.gt_csr and ops.gt_push_csr
  state alike, each tested once over the four (gt_cases.ENTRIES): an unknown objective, each
  pair of the four state matrices aliased, bad weight vectors, CPU tensors.
  The rules of one layout are in tests/test_gt_ring_host.py and
  tests/test_gt_csr_host.py.
* The surface: ops re-exports, ops.GT_MAX_AGENTS, the three SIGNATURES rows.
* Every refusal of ops.gt_csr_pm / ops.separable_grad / SeparableGTPM comes
  before the library is reached, and the entry points themselves refuse bad
  arguments without a launch.
* graph.metropolis_weights gives a symmetric doubly stochastic W with a
  positive diagonal on regular and irregular graphs.
* tests/gt_cases.py, the float32 host restatement of the round that the GPU
  tier holds the kernel to: its x' update is an exact fma, it converges to the
  optimum with Metropolis weights (max |x - mean t| <= 1e-5 after 200 rounds,
  the atol tests/test_dgd_gpu.py uses for N-term means; the float32 CPU
  simulation of this arithmetic settled at 3.2e-7 from round 150 on), and it
  diverges on the zero-diagonal doubly stochastic circle of even size, where
  -1 is an eigenvalue of W."""
import types

import numpy as np
import pytest
import torch

import gt_cases
from dolhip import _native, graph as G, gt, ops
from dolhip.ops import DolNativeError
from test_ops_args_gpu import vec

CPU = torch.device("cpu")
I32 = torch.int32
F32 = np.float32


OPS = sorted(gt_cases.ENTRIES)


@pytest.fixture
def rec(monkeypatch):
    return gt_cases.recorder(monkeypatch)


def _args(dev):
    return gt_cases.host_args("gt_csr_pm", dev)


def _call(t, **kw):
    return gt_cases.host_call("gt_csr_pm", t, **kw)


# ---------------------------------------------------------------------------
# the surface
# ---------------------------------------------------------------------------
def test_surface():
    assert ops.gt_csr_pm is gt.gt_csr_pm and ops.separable_grad is gt.separable_grad
    assert ops.GT_MAX_AGENTS == 4096 and "GT_MAX_AGENTS" in ops.__all__
    from dolhip.synthetic import SeparableGTPM  # noqa: F401
    assert callable(G.metropolis_weights)


def test_native_table_carries_the_three_signatures():
    want = {"dol_gt_csr_pm_f32": 19, "dol_gt_csr_pm_ex_f32": 20, "dol_separable_grad_f32": 10}
    assert {k: len(_native.SIGNATURES[k]) for k in want} == want
    assert len(_native.SIGNATURES["dol_gt_csr_pm_ex_f32"]) == len(_native.SIGNATURES["dol_gt_csr_pm_f32"]) + 1


# ---------------------------------------------------------------------------
# refusals, before the library is reached
# ---------------------------------------------------------------------------
def test_more_than_4096_agents_are_refused(rec):
    t = _args(CPU)
    t["rowptr"] = vec(CPU, 4098, I32)
    with pytest.raises(ValueError, match="at most 4096 agents .got 4097."):
        _call(t)
    assert rec.calls == []


@pytest.mark.parametrize("op", OPS)
def test_unknown_objective_is_refused(op, rec):
    t = gt_cases.host_args(op, CPU)
    with pytest.raises(ValueError, match=f"{op}: objective must be one of"):
        gt_cases.host_call(op, t, objective="hinge")
    if op == "gt_csr_pm":
        with pytest.raises(ValueError, match="objective must be one of"):
            ops.separable_grad(t["XT"], t["TT"], t["XO"], "hinge")
    assert rec.calls == []


@pytest.mark.parametrize("op,a,b", [(op, e["state"][i], e["state"][j]) for op, e in sorted(gt_cases.ENTRIES.items())
                                    for i in range(4) for j in range(i + 1, 4)])
def test_two_state_matrices_the_same_tensor_are_refused(op, a, b, rec):
    t = gt_cases.host_args(op, CPU)
    t[b] = t[a]
    with pytest.raises(ValueError, match=f"{op}: {a} and {b} alias"):
        gt_cases.host_call(op, t)
    t = gt_cases.host_args(op, CPU)
    t[b] = t[a][:, :t[a].shape[1]]  # another view of the same rows
    with pytest.raises(ValueError, match=f"{op}: {a} and {b} alias"):
        gt_cases.host_call(op, t)
    assert rec.calls == []


@pytest.mark.parametrize("op,name", [(op, v) for op, e in sorted(gt_cases.ENTRIES.items()) for v in e["vectors"]])
@pytest.mark.parametrize("bad", [lambda n: vec(CPU, n - 1), lambda n: vec(CPU, n, torch.float64),
                                 lambda n: torch.zeros(n, device="meta"), lambda n: vec(CPU, 2 * n)[::2]],
                         ids=["length", "dtype", "device", "stride"])
def test_bad_weight_vectors_are_refused(op, name, bad, rec):
    n = gt_cases.ENTRIES[op]["n"]
    t, kw = gt_cases.host_args(op, CPU), {}
    if name == "self_weight":
        kw[name] = bad(n)
    else:
        t[name] = bad(n)
    with pytest.raises(ValueError, match=rf"{name}: expected contiguous float32 \[{n}\] on cpu"):
        gt_cases.host_call(op, t, **kw)
    assert rec.calls == []


@pytest.mark.parametrize("op", OPS)
def test_cpu_tensors_are_refused(op, rec):
    t, n = gt_cases.host_args(op, CPU), gt_cases.ENTRIES[op]["n"]
    with pytest.raises(DolNativeError, match="cpu"):
        gt_cases.host_call(op, t, self_weight=vec(CPU, n), objective="logistic", lr=0.5, **gt_cases.ENTRIES[op]["kw"])
    if op == "gt_csr_pm":
        with pytest.raises(DolNativeError, match="cpu"):
            ops.separable_grad(t["XT"], t["TT"], t["XO"], "logistic")
    assert rec.calls == []


def test_problem_class_refuses_dense_plans_and_too_many_agents(rec):
    from dolhip.synthetic import SeparableGTPM
    c = G.random_regular_csr(8, 4, seed=1)
    with pytest.raises(ValueError, match="sparse"):
        SeparableGTPM(G.MixingPlan(c, CPU, dense=True), 8)
    with pytest.raises(ValueError, match="at most 4096 agents"):
        SeparableGTPM(types.SimpleNamespace(n_rows=4097, kind="csr", device=CPU), 8)
    with pytest.raises(ValueError, match="objective must be one of"):
        SeparableGTPM(G.MixingPlan(c, CPU), 8, objective="hinge")
    assert rec.calls == []


def test_entry_points_check_arguments_without_launch():
    L = _native.lib()
    fake = 1 << 20  # never dereferenced: every call below fails its argument check first
    A, B, C, D, T, RP = (fake + (k << 16) for k in range(6))

    def gt_call(xt=A, st=B, xo=C, so=D, n=8, P=8, ld=8, objective=0, nseg=0, tt=T):
        return L.dol_gt_csr_pm_ex_f32(xt, ld, st, ld, xo, ld, so, ld, n, P, RP, RP, RP, None, tt, ld, objective, 0.1,
                                      nseg, None)
    for kw in (dict(st=A), dict(xo=A), dict(so=A), dict(xo=B), dict(so=B), dict(so=C)):
        assert gt_call(**kw) == -1 and b"alias" in L.dol_last_error()
    assert gt_call(n=4097, ld=4100) == -1 and b"at most 4096 agents" in L.dol_last_error()
    assert gt_call(objective=2) == -1 and b"objective must be 0 or 1" in L.dol_last_error()
    assert gt_call(ld=6) == -1 and b"multiples of 4" in L.dol_last_error()
    assert gt_call(n=9) == -1 and b"multiples of 4" in L.dol_last_error()  # ld 8 < round_up(9, 4)
    assert gt_call(xt=A + 4) == -1 and b"16-B aligned" in L.dol_last_error()
    assert gt_call(tt=None) == -1 and b"null pointer" in L.dol_last_error()
    assert gt_call(nseg=257) == -1 and b"stage order" in L.dol_last_error()
    assert gt_call(n=-1) == -1 and b"negative size" in L.dol_last_error()
    assert gt_call(n=0) == 0 and gt_call(P=0) == 0  # nothing to do: nothing launched
    assert L.dol_gt_csr_pm_f32(A, 8, A, 8, C, 8, D, 8, 8, 8, RP, RP, RP, None, T, 8, 0, 0.1, None) == -1

    def grad_call(x=A, t=B, g=C, rows=4, cols=8, ld=8, objective=0):
        return L.dol_separable_grad_f32(x, ld, t, ld, g, ld, rows, cols, objective, None)
    assert grad_call(objective=-1) == -1 and b"objective must be 0 or 1" in L.dol_last_error()
    assert grad_call(x=None) == -1 and b"null pointer" in L.dol_last_error()
    assert grad_call(cols=9) == -1 and b"ld < cols" in L.dol_last_error()
    assert grad_call(rows=-1) == -1 and b"negative size" in L.dol_last_error()
    assert grad_call(rows=0) == 0 and grad_call(cols=0) == 0


# ---------------------------------------------------------------------------
# Metropolis weights
# ---------------------------------------------------------------------------
def _star(n):
    return G.csr_from_dense(G.adjacency("star", n)[0])


def _graphs():
    torch.manual_seed(2028)
    return {"circle 8": G.communication_csr("circle", "stochastic", 8)[0],
            "random 4-regular 16": G.random_regular_csr(16, 4, seed=5),
            "star 5": _star(5)}


@pytest.mark.parametrize("name", ["circle 8", "random 4-regular 16", "star 5"])
def test_metropolis_weights_are_doubly_stochastic(name):
    c = _graphs()[name]
    w, d = G.metropolis_weights(c)
    w.validate()
    n = c.n_rows
    assert d.dtype == np.float32 and d.shape == (n,) and (d > 0).all()
    assert w.col.dtype == np.int32 and w.val.dtype == np.float32
    # the pattern is csr's, columns ascending, no diagonal
    assert np.array_equal(w.rowptr, c.rowptr) and np.array_equal(w.col, c.col)
    rows = np.repeat(np.arange(n), np.diff(w.rowptr))
    assert (rows != w.col).all() and all(np.all(np.diff(w.col[a:b]) > 0) for a, b in zip(w.rowptr[:-1], w.rowptr[1:]))
    deg = np.diff(w.rowptr)
    assert np.array_equal(w.val, (F32(1) / (1 + np.maximum(deg[rows], deg[w.col])).astype(F32)))
    W = w.dense().astype(np.float64) + np.diag(d.astype(np.float64))
    assert np.array_equal(W, W.T)
    tol = n * np.finfo(F32).eps  # 1 ulp per term
    assert np.abs(W.sum(1) - 1).max() <= tol and np.abs(W.sum(0) - 1).max() <= tol
    # d_i = fl(1 - sum), the sum in fp32 in ascending j
    for i in range(n):
        s = F32(0)
        for e in range(w.rowptr[i], w.rowptr[i + 1]):
            s = F32(s + w.val[e])
        assert d[i] == F32(F32(1) - s)


def test_metropolis_weights_use_the_pattern_only():
    """Values, diagonal entries and duplicates of the input do not matter; the
    star has unequal degrees (hub 4, leaves 1): every edge weighs 1/5."""
    star = _star(5)
    w, d = G.metropolis_weights(star)
    assert np.array_equal(w.val, np.full(8, F32(1) / F32(5)))
    assert np.array_equal(d, np.array([F32(1) - (F32(0.2) + F32(0.2) + F32(0.2) + F32(0.2))] + [F32(1) - F32(0.2)] * 4,
                                      F32))
    noisy = G.csr_from_dense(G.adjacency("star", 5)[0] * 7.5 + np.eye(5))
    w2, d2 = G.metropolis_weights(noisy)
    assert np.array_equal(w2.rowptr, w.rowptr) and np.array_equal(w2.col, w.col)
    assert np.array_equal(w2.val, w.val) and np.array_equal(d2, d)


def test_metropolis_weights_refuse_a_one_directional_pattern():
    a = np.zeros((4, 4))
    a[0, 1] = a[1, 0] = a[1, 2] = 1.0  # 1 -> 2 without 2 -> 1
    with pytest.raises(ValueError, match="not symmetric"):
        G.metropolis_weights(G.csr_from_dense(a))
    with pytest.raises(ValueError, match="square"):
        G.metropolis_weights(G.CSR(2, 3, np.array([0, 1, 2], np.int32), np.array([1, 0], np.int32), np.ones(2, F32)))


# ---------------------------------------------------------------------------
# the host restatement
# ---------------------------------------------------------------------------
def test_oracle_sgd_step_is_an_exact_fma():
    """x' = oracle.prox_admm_sgd(no theta, no alpha, momentum 0) is
    fmaf(-lr, g, w), one rounding: checked against exact rational arithmetic
    (this Python has no math.fma) on 3000 random triples, with products that
    cancel the addend among them."""
    rng = np.random.default_rng(11)
    n = 3000
    lr = rng.uniform(0.01, 2.0, n).astype(F32)
    g = rng.standard_normal(n).astype(F32)
    w = rng.standard_normal(n).astype(F32)
    w[::3] = (lr[::3] * g[::3]).astype(F32)  # w ~ lr * g: the fma's extra bits decide the result
    fused = 0
    for i in range(n):
        got = gt_cases.sgd_step(w[i:i + 1, None], g[i:i + 1, None], float(lr[i]))[0, 0]
        want = gt_cases.fma_exact(-lr[i], g[i], w[i])
        assert got.view(np.uint32) == np.asarray(want, F32).view(np.uint32), (lr[i], g[i], w[i], got, want)
        fused += got != F32(w[i] + F32(-lr[i] * g[i]))
    assert fused > 100, "the triples never told an fma from a rounded product"


def _ls_problem(n, P, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, P)).astype(F32)
    T = rng.standard_normal((n, P)).astype(F32)
    return X, gt_cases.ls_grad(X, T), T


def test_host_round_converges_with_metropolis_weights():
    c, d = G.metropolis_weights(G.random_regular_csr(16, 4, seed=5))
    X, S, T = _ls_problem(16, 64, 3)
    opt = T.astype(np.float64).mean(0)
    for _ in range(200):
        X, S = gt_cases.gt_round(X, S, T, c, d, 0.1)
    err = np.abs(X.astype(np.float64) - opt).max()
    print(f"max |x - mean t| after 200 rounds: {err:.3g}")
    assert err <= 1e-5


def test_host_round_diverges_on_the_zero_diagonal_even_circle():
    """The reference's doubly stochastic circle has a zero diagonal; with an
    even n the ring is bipartite, -1 is an eigenvalue of W, and on that mode
    the round's 2 x 2 iteration has an eigenvalue below -1 for every lr > 0."""
    torch.manual_seed(2028)
    c = G.csr_from_dense(G.communication_graph("circle", "double_stochastic", 8, sinkhorn_tol=1e-6)[0])
    assert (np.repeat(np.arange(8), np.diff(c.rowptr)) != c.col).all()
    X, S, T = _ls_problem(8, 64, 4)
    size = []
    for r in range(120):
        X, S = gt_cases.gt_round(X, S, T, c, None, 0.1)
        if r % 40 == 39:
            size.append(np.abs(X).max())
    print("max |x| after 40 / 80 / 120 rounds:", size)
    assert size[0] < size[1] < size[2] and size[2] > 1e10
