"""Push-sum gradient tracking on the agent-major CSR bank (dol_gt_push_csr_f32,
ops.gt_push_csr, CSR.transpose, graph.push_sum_weights,
MixingPlan.apply_gt_push, SeparableGTPush), CPU tier: nothing is launched.

* The surface: the SIGNATURES row, the ops re-export, the package export.
* The entry point's own argument rules beside dol_gt_csr_f32's, called through
  the library with addresses that are never dereferenced: null v / v_out, v and
  v_out aliased.
* The rules of ops.gt_push_csr with ops._native.call replaced by
  test_ops_args_gpu.Recorder: aliased state matrices, aliased v / v_out, a
  short or wrongly typed v or v_out (an unknown objective and CPU tensors: with
  the other ops in tests/test_gt_host.py).  A CPU matrix is refused before the
  square-C rule is looked at (as for ops.gt_csr), so the non-square C and the
  accepted call's argument tuple use device tensors: those two tests carry the
  gpu marker, still with the Recorder and without a launch.
* MixingPlan.apply_gt_push's routing by kind and SeparableGTPush's refusals.
* CSR.transpose() and graph.push_sum_weights.
* tests/gt_push_cases.py::gt_push_round replayed (least squares, P = 8, zero
  start, targets standard normal from seed 3): on digraph(9) with out-degree
  weights, lr 0.1, 200 rounds, and on the reference's 9-agent stochastic circle
  W as C = 1/2 (I + W^T), lr 0.05, 400 rounds, every agent's U / v ends within
  1e-5 of the mean of the targets (measured here: 2.1e-7 and 6.1e-7), where
  gt_cases.gt_round on the same weights stays more than 0.05 away (0.30 and
  0.61); after every round sum_i v_i = n and sum_i s_i = sum_i g(z_i)."""
import types

import numpy as np
import pytest
import torch

import dolhip
import gt_cases
import gt_push_cases
from dolhip import _native, graph as G, gt, ops
from dolhip.synthetic import SeparableGTPush
from test_ops_args_gpu import mat, named, vec

CPU = torch.device("cpu")
F32 = np.float32
I32 = torch.int32


# ---------------------------------------------------------------------------
# the surface
# ---------------------------------------------------------------------------
def test_surface():
    assert len(_native.SIGNATURES["dol_gt_push_csr_f32"]) == len(_native.SIGNATURES["dol_gt_csr_f32"]) + 2 == 21
    assert ops.gt_push_csr is gt.gt_push_csr and "gt_push_csr" not in ops.__all__
    assert dolhip.SeparableGTPush is SeparableGTPush
    assert callable(G.MixingPlan.apply_gt_push) and callable(G.push_sum_weights) and callable(G.CSR.transpose)


# ---------------------------------------------------------------------------
# the entry point's argument rules, without a launch
# ---------------------------------------------------------------------------
def test_entry_point_checks_arguments_without_launch():
    L = _native.lib()
    fake = 1 << 20  # never dereferenced: every call below returns from its argument checks
    U, S, UO, SO, T, RP, COL, VAL, WS, V, VO = (fake + (k << 16) for k in range(11))

    def call(u=U, s=S, uo=UO, so=SO, n=8, P=8, ld=8, rp=RP, col=COL, val=VAL, ws=None, t=T, objective=0, v=V, vo=VO):
        return L.dol_gt_push_csr_f32(u, ld, s, ld, uo, ld, so, ld, n, P, rp, col, val, ws, t, ld, objective, 0.1, v, vo,
                                     None)

    def refused(word, **kw):
        assert call(**kw) == -1, kw
        msg = L.dol_last_error()
        assert b"dol_gt_push_csr_f32" in msg and word in msg, (kw, msg)

    for name in ("u", "s", "uo", "so", "t", "rp", "col", "val", "v", "vo"):  # self_w alone may be null
        refused(b"null pointer", **{name: None})
        refused(b"null pointer", ws=WS, **{name: None})
    refused(b"ld < P", ld=7)
    for kw in (dict(s=U), dict(uo=U), dict(so=U), dict(uo=S), dict(so=S), dict(so=UO)):
        refused(b"alias", **kw)
    refused(b"v and v_out alias", vo=V)
    refused(b"v and v_out alias", vo=V, ws=WS)
    refused(b"objective must be 0 or 1", objective=2)
    refused(b"too large", n=1 << 20, P=1 << 40, ld=1 << 40)
    refused(b"too large", n=(1 << 28) + 16, P=1, ld=1)
    refused(b"negative size", n=-1)
    refused(b"negative size", P=-1)
    # nothing to do: DOL_OK whatever else is passed, nothing launched
    assert call(n=0) == 0 and call(P=0) == 0 and call(n=0, v=None, vo=None, objective=5) == 0
    assert L.dol_last_error() == b""


# ---------------------------------------------------------------------------
# ops.gt_push_csr before the library is reached
# ---------------------------------------------------------------------------
@pytest.fixture
def rec(monkeypatch):
    return gt_cases.recorder(monkeypatch)


STATE = ("U", "S", "UO", "SO")


def _args(dev, n=4):
    """gt_cases.host_args of gt_csr under this op's names, with v / v_out and a
    C that is square: the perfect matching 0 - 1, 2 - 3."""
    t = gt_cases.host_args("gt_csr", dev, n=n)
    t["U"], t["UO"] = t.pop("X"), t.pop("XO")
    t.update(v=vec(dev, n), v_out=vec(dev, n), rowptr=torch.tensor([0, 1, 2, 3, 4], dtype=I32, device=dev),
             col=torch.tensor([1, 0, 3, 2], dtype=I32, device=dev))
    return t


def _call(t, **kw):
    return ops.gt_push_csr(*(t[k] for k in STATE + ("rowptr", "col", "val", "target", "v", "v_out")), **kw)


@pytest.mark.parametrize("a,b", [(STATE[i], STATE[j]) for i in range(4) for j in range(i + 1, 4)])
def test_two_state_matrices_the_same_tensor_are_refused(a, b, rec):
    t = _args(CPU)
    t[b] = t[a]
    with pytest.raises(ValueError, match=f"gt_push_csr: {a} and {b} alias"):
        _call(t)
    t = _args(CPU)
    t[b] = t[a][:, :t[a].shape[1]]  # another view of the same rows
    with pytest.raises(ValueError, match=f"gt_push_csr: {a} and {b} alias"):
        _call(t)
    assert rec.calls == []


def test_v_and_v_out_the_same_vector_are_refused(rec):
    t = _args(CPU)
    t["v_out"] = t["v"]
    with pytest.raises(ValueError, match="gt_push_csr: v and v_out alias"):
        _call(t)
    t["v_out"] = t["v"][:4]  # another view of the same floats
    with pytest.raises(ValueError, match="gt_push_csr: v and v_out alias"):
        _call(t)
    assert rec.calls == []


@pytest.mark.parametrize("name", ["v", "v_out", "self_weight"])
@pytest.mark.parametrize("bad", [lambda n: vec(CPU, n - 1), lambda n: vec(CPU, n, torch.float64),
                                 lambda n: torch.zeros(n, device="meta"), lambda n: vec(CPU, 2 * n)[::2]],
                         ids=["length", "dtype", "device", "stride"])
def test_bad_weight_vectors_are_refused(name, bad, rec):
    t, kw = _args(CPU), {}
    if name == "self_weight":
        kw[name] = bad(4)
    else:
        t[name] = bad(4)
    with pytest.raises(ValueError, match=rf"{name}: expected contiguous float32 \[4\] on cpu"):
        _call(t, **kw)
    assert rec.calls == []


@pytest.mark.gpu
def test_a_non_square_c_is_refused(gpu, rec):
    t = _args(gpu)
    t["col"][2] = 4  # in place: the square-W check keeps its answers per (buffers, versions)
    with pytest.raises(ValueError, match="needs a square W"):
        _call(t)
    assert rec.calls == []


@pytest.mark.gpu
def test_the_accepted_call_reaches_the_library_with_these_arguments(gpu, rec):
    t = _args(gpu)
    t["self_weight"] = vec(gpu, 4)
    out = _call(t, self_weight=t["self_weight"], objective="logistic", lr=0.5)
    assert out[0] is t["UO"] and out[1] is t["SO"] and out[2] is t["v_out"]
    assert named(rec.calls, t, gpu) == [
        ("dol_gt_push_csr_f32", "U+0", 12, "S+0", 12, "UO+0", 12, "SO+0", 12, 4, 10, "rowptr+0", "col+0", "val+0",
         "self_weight+0", "target+0", 12, 1, 0.5, "v+0", "v_out+0", "stream")]
    rec.calls.clear()
    _call(t, P=8)
    assert named(rec.calls, t, gpu) == [
        ("dol_gt_push_csr_f32", "U+0", 12, "S+0", 12, "UO+0", 12, "SO+0", 12, 4, 8, "rowptr+0", "col+0", "val+0", None,
         "target+0", 12, 0, 0.01, "v+0", "v_out+0", "stream")]


# ---------------------------------------------------------------------------
# MixingPlan.apply_gt_push and SeparableGTPush
# ---------------------------------------------------------------------------
def test_apply_gt_push_routes_by_kind(monkeypatch, rec):
    seen = []
    monkeypatch.setattr(ops, "gt_push_csr", lambda *a, **k: seen.append((a, k)) or (a[2], a[3], a[9]))
    c9 = gt_cases.ring(9)[0]
    t = _args(CPU, n=9)
    d = vec(CPU, 9)
    kw = dict(self_weight=d, objective="logistic", lr=0.5, P=10)
    seven = tuple(t[k] for k in STATE + ("target", "v", "v_out"))

    csr = G.MixingPlan(c9, CPU, allow_ring=False)
    assert csr.kind == "csr"
    out = csr.apply_gt_push(*seven, **kw)
    assert out[0] is t["UO"] and out[1] is t["SO"] and out[2] is t["v_out"]
    a, k = seen.pop()
    assert k == kw
    want = tuple(t[k_] for k_ in STATE) + (csr.rowptr, csr.col, csr.val, t["target"], t["v"], t["v_out"])
    assert len(a) == len(want) and all(x is y for x, y in zip(a, want))

    ring = G.MixingPlan(c9, CPU)
    assert ring.kind == "ring"
    with pytest.raises(NotImplementedError, match="allow_ring=False"):
        ring.apply_gt_push(*seven, **kw)
    dense = G.MixingPlan(c9, CPU, dense=True)
    with pytest.raises(NotImplementedError, match="gradient-tracking rounds are fused into the sparse mixes"):
        dense.apply_gt_push(*seven)
    csr._retire()
    with pytest.raises(RuntimeError, match="no longer holds its W"):
        csr.apply_gt_push(*seven)
    assert seen == [] and rec.calls == []


def test_problem_class_refusals(rec):
    c = G.random_regular_csr(8, 4, seed=1)
    with pytest.raises(ValueError, match="sparse"):
        SeparableGTPush(G.MixingPlan(c, CPU, dense=True), 8)
    with pytest.raises(ValueError, match="allow_ring=False"):
        SeparableGTPush(G.MixingPlan(gt_cases.ring(9)[0], CPU), 8)
    with pytest.raises(ValueError, match="objective must be one of"):
        SeparableGTPush(G.MixingPlan(c, CPU), 8, objective="hinge")
    with pytest.raises(ValueError, match="self_weight: expected 8 weights"):
        SeparableGTPush(G.MixingPlan(c, CPU), 8, self_weight=np.zeros(9, F32))
    assert rec.calls == []


def test_problem_round_makes_one_call_and_swaps():
    """round() on stand-ins for the plan and the bank: one apply_gt_push call on
    (u, s, u_out, s_out, target, v, v_out), then the three swaps."""
    calls = []
    prob = SeparableGTPush.__new__(SeparableGTPush)
    prob.plan = types.SimpleNamespace(apply_gt_push=lambda *a, **k: calls.append((a, k)))
    prob.bank = types.SimpleNamespace(buffer=lambda name: name, swap=lambda a, b: calls.append(("swap", a, b)))
    prob.self_weight, prob.objective, prob.lr, prob.P, prob.rounds = "d", "logistic", 0.5, 10, 0
    prob.v, prob.v_out = "v", "v_out"
    prob.round()
    assert calls == [(("u", "s", "u_out", "s_out", "target", "v", "v_out"),
                      dict(self_weight="d", objective="logistic", lr=0.5, P=10)),
                     ("swap", "u", "u_out"), ("swap", "s", "s_out")]
    assert (prob.v, prob.v_out) == ("v_out", "v") and prob.rounds == 1


# ---------------------------------------------------------------------------
# CSR.transpose and push_sum_weights
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["digraph 9", "reference circle 9", "random 4-regular 16", "irregular 37", "3 x 5"])
def test_transposing_twice_gives_back_the_same_arrays(name):
    c = {"digraph 9": lambda: gt_push_cases.digraph(9), "reference circle 9": lambda: gt_cases.ring(9)[0],
         "random 4-regular 16": lambda: G.random_regular_csr(16, 4, seed=5),
         "irregular 37": lambda: gt_push_cases.irregular(37),
         "3 x 5": lambda: G.csr_from_dense(np.array([[0, 2, 0, 0, 3], [0, 0, 0, 0, 0], [1, 0, 4, 0, 5]], F32))}[name]()
    t = c.transpose()
    t.validate()
    assert (t.n_rows, t.n_cols) == (c.n_cols, c.n_rows)
    assert t.rowptr.dtype == np.int32 and t.col.dtype == np.int32 and t.val.dtype == np.float32
    assert all(np.all(np.diff(t.col[a:b]) > 0) for a, b in zip(t.rowptr[:-1], t.rowptr[1:]))  # ascending columns
    assert np.array_equal(t.dense(), c.dense().T)
    back = t.transpose()
    assert (back.n_rows, back.n_cols) == (c.n_rows, c.n_cols)
    for a, b in ((back.rowptr, c.rowptr), (back.col, c.col), (back.val, c.val)):
        assert a.dtype == b.dtype and np.array_equal(a, b)


def test_push_sum_weights_are_column_stochastic_only():
    pattern = gt_push_cases.digraph(9)
    c, d = G.push_sum_weights(pattern)
    c.validate()
    assert d.dtype == np.float32 and d.shape == (9,) and c.val.dtype == np.float32 and c.col.dtype == np.int32
    assert np.array_equal(c.rowptr, pattern.rowptr) and np.array_equal(c.col, pattern.col)
    outdeg = np.array([3 if i % 3 == 0 else 2 for i in range(9)])
    assert np.array_equal(np.bincount(pattern.col, minlength=9), outdeg)
    share = (F32(1) / (outdeg + 1).astype(F32)).astype(F32)  # fl(1 / (outdeg + 1))
    assert np.array_equal(d, share) and np.array_equal(c.val, share[c.col])
    C = c.dense().astype(np.float64) + np.diag(d.astype(np.float64))
    assert np.abs(C.sum(0) - 1).max() <= 1e-6
    assert np.abs(C.sum(1) - 1).max() > 0.1


def test_push_sum_weights_use_the_pattern_only():
    pattern = gt_push_cases.digraph(9)
    noisy = G.csr_from_dense(pattern.dense() * 7.5 + np.eye(9, dtype=F32))
    (c, d), (c2, d2) = G.push_sum_weights(pattern), G.push_sum_weights(noisy)
    for a, b in ((c.rowptr, c2.rowptr), (c.col, c2.col), (c.val, c2.val), (d, d2)):
        assert np.array_equal(a, b)
    with pytest.raises(ValueError, match="square"):
        G.push_sum_weights(G.CSR(2, 3, np.array([0, 1, 2], np.int32), np.array([1, 0], np.int32), np.ones(2, F32)))


# ---------------------------------------------------------------------------
# convergence and invariants, by replaying the host restatement
# ---------------------------------------------------------------------------
def _replay(c, d, lr, rounds, invariants=False):
    """(max |U / v - mean t| of the push-sum round, the same of gt_cases.gt_round on
    the same weights) from a zero start, P = 8, targets from seed 3."""
    n, P = c.n_rows, 8
    T = np.random.default_rng(3).standard_normal((n, P)).astype(F32)
    X0 = np.zeros((n, P), F32)
    opt = T.astype(np.float64).mean(0)
    U, S, v = X0, gt_cases.ls_grad(X0, T), np.ones(n, F32)
    X, Sg = X0, gt_cases.ls_grad(X0, T)
    for _ in range(rounds):
        U, S, v = gt_push_cases.gt_push_round(U, S, T, v, c, d, lr)
        X, Sg = gt_cases.gt_round(X, Sg, T, c, d, lr)
        if invariants:  # fp64 sums over fp32 values
            assert abs(v.astype(np.float64).sum() - n) <= 1e-5 * n
            z = (U / v[:, None]).astype(F32)
            g = gt_cases.ls_grad(z, T).astype(np.float64).sum(0)
            assert np.abs(S.astype(np.float64).sum(0) - g).max() <= 1e-4
    return np.abs(gt_push_cases.estimate(U, v) - opt).max(), np.abs(X.astype(np.float64) - opt).max()


def test_host_round_reaches_the_optimum_on_a_digraph_where_gradient_tracking_is_biased():
    c, d = G.push_sum_weights(gt_push_cases.digraph(9))
    err, err_gt = _replay(c, d, 0.1, 200, invariants=True)
    print(f"max |z - mean t| after 200 rounds: push-sum {err:.3g}, gt_round on the same weights {err_gt:.3g}")
    assert err <= 1e-5
    assert err_gt > 0.05


def test_host_round_reaches_the_optimum_on_the_reference_w_transposed():
    c, d = gt_push_cases.reference_ring_weights(9)
    C = c.dense().astype(np.float64) + np.diag(d.astype(np.float64))
    assert np.abs(C.sum(0) - 1).max() <= 1e-6 and np.abs(C.sum(1) - 1).max() > 0.1  # column-stochastic only
    err, err_gt = _replay(c, d, 0.05, 400)
    print(f"max |z - mean t| after 400 rounds: push-sum {err:.3g}, gt_round on the same weights {err_gt:.3g}")
    assert err <= 1e-5
    assert err_gt > 0.05
