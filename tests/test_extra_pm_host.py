"""ops.extra_csr_pm and SeparableEXTRAPM before the library is reached:
ops._native.call is replaced by test_ops_args_gpu.Recorder, so nothing is
launched -- not with good arguments and above all not with bad ones.

CPU tensors reach the rules that need no layout (an unknown objective, corr
aliasing XT, YT or TT, 4097 agents) and the refusal of a CPU tensor itself; a
CPU matrix is refused before the layout rules are looked at, so XT is YT, a
non-square W, a short self-weight vector, a short corr and the accepted call's
argument tuple use device tensors: those tests carry the gpu marker, still with
the Recorder and without a launch.  The entry points' own rules are called
through the library with addresses that are never dereferenced."""
import types

import numpy as np
import pytest
import torch

import gt_cases
from dolhip import _native, extra, graph as G, ops
from dolhip.synthetic import SeparableEXTRAPM
from test_ops_args_gpu import mat, named, vec

CPU = torch.device("cpu")
ORDER = ("XT", "YT", "rowptr", "col", "val", "TT", "corr")


@pytest.fixture
def rec(monkeypatch):
    return gt_cases.recorder(monkeypatch)


def host_args(dev, n=2, P=10):
    """The tensor arguments of ops.extra_csr_pm by name, zeros on dev: n agents
    x P, p-rows round_up(n, 4) floats apart; W is the perfect matching 0 - 1, 2 - 3, ..."""
    ldn = (n + 3) // 4 * 4
    t = {k: mat(dev, P, n, ldn) for k in ("XT", "YT", "TT", "corr")}
    t.update(rowptr=torch.arange(n + 1, dtype=torch.int32, device=dev),
             col=torch.tensor([i ^ 1 for i in range(n)], dtype=torch.int32, device=dev), val=vec(dev, n))
    return t


def host_call(t, **kw):
    return ops.extra_csr_pm(*(t[k] for k in ORDER), **kw)


def test_surface():
    assert len(_native.SIGNATURES["dol_extra_csr_pm_f32"]) == 17
    assert len(_native.SIGNATURES["dol_extra_csr_pm_ex_f32"]) == 18
    assert _native.SIGNATURES["dol_extra_csr_pm_f32"] == _native.SIGNATURES["dol_extra_csr_f32"]
    assert ops.extra_csr_pm is extra.extra_csr_pm
    assert "extra_csr_pm" not in ops.__all__


def test_unknown_objective_is_refused(rec):
    with pytest.raises(ValueError, match="extra_csr_pm: objective must be one of"):
        host_call(host_args(CPU), objective="hinge")
    assert rec.calls == []


@pytest.mark.parametrize("other,name", [("XT", "X"), ("YT", "Y"), ("TT", "target")])
def test_corr_aliasing_another_matrix_is_refused(other, name, rec):
    t = host_args(CPU)
    t["corr"] = t[other]
    with pytest.raises(ValueError, match=f"extra_csr_pm: corr and {name} alias"):
        host_call(t)
    t["corr"] = t[other][:, :2]  # another view of the same rows
    with pytest.raises(ValueError, match=f"extra_csr_pm: corr and {name} alias"):
        host_call(t)
    assert rec.calls == []


def test_4097_agents_are_refused(rec):
    t = host_args(CPU)
    t["rowptr"] = torch.zeros(4098, dtype=torch.int32)
    with pytest.raises(ValueError, match="extra_csr_pm: the EXTRA round takes at most 4096 agents .got 4097."):
        host_call(t)
    assert ops.PM_DGD_MAX_AGENTS == 4096 and rec.calls == []


def test_cpu_tensors_are_refused(rec):
    with pytest.raises(ops.DolNativeError, match="cpu"):
        host_call(host_args(CPU), self_weight=vec(CPU, 2), objective="logistic", lr=0.5, P=10, nseg=8)
    assert rec.calls == []


@pytest.mark.gpu
def test_xt_is_yt_is_refused(gpu, rec):
    t = host_args(gpu)
    t["YT"] = t["XT"]
    with pytest.raises(ValueError, match="XT and YT alias: the Jacobi mix needs two buffers"):
        host_call(t, nseg=8)
    assert rec.calls == []


@pytest.mark.gpu
def test_a_non_square_w_is_refused(gpu, rec):
    t = host_args(gpu, n=4)
    t["col"][2] = 4  # in place: the square-W check keeps its answers per (buffers, versions)
    with pytest.raises(ValueError, match="needs a square W"):
        host_call(t, nseg=8)
    assert rec.calls == []


@pytest.mark.gpu
@pytest.mark.parametrize("bad", [lambda dev: vec(dev, 1), lambda dev: vec(dev, 2, torch.float64),
                                 lambda dev: vec(dev, 4)[::2]], ids=["length", "dtype", "stride"])
def test_bad_self_weights_are_refused(bad, gpu, rec):
    with pytest.raises(ValueError, match=r"self_weight: expected contiguous float32 \[2\]"):
        host_call(host_args(gpu), self_weight=bad(gpu), nseg=8)
    assert rec.calls == []


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["corr", "TT"])
def test_a_short_corr_or_target_is_refused(name, gpu, rec):
    t = host_args(gpu)
    t[name] = t[name][:, :1]  # 1 agent column < n = 2
    with pytest.raises(ValueError, match=rf"{name}: expected \[>= 10, >= 2\]"):
        host_call(t, nseg=8)
    t = host_args(gpu)
    t[name] = t[name][:9]  # 9 parameter rows < P = 10
    with pytest.raises(ValueError, match=rf"{name}: expected \[>= 10, >= 2\]"):
        host_call(t, nseg=8)
    assert rec.calls == []


@pytest.mark.gpu
def test_the_accepted_call_reaches_the_library_with_these_arguments(gpu, rec):
    t = host_args(gpu)
    t["self_weight"] = vec(gpu, 2)
    assert host_call(t, self_weight=t["self_weight"], objective="logistic", lr=0.5, nseg=8) is t["YT"]
    host_call(t, P=8, nseg=16)
    assert named(rec.calls, t, gpu) == [
        ("dol_extra_csr_pm_ex_f32", "XT+0", 4, "YT+0", 4, 2, 10, "rowptr+0", "col+0", "val+0", "self_weight+0", "TT+0",
         4, "corr+0", 4, 1, 0.5, 8, "stream"),
        ("dol_extra_csr_pm_ex_f32", "XT+0", 4, "YT+0", 4, 2, 8, "rowptr+0", "col+0", "val+0", None, "TT+0", 4, "corr+0",
         4, 0, 0.01, 16, "stream")]


def test_problem_class_refusals(rec):
    c = G.random_regular_csr(8, 4, seed=1)
    with pytest.raises(ValueError, match="sparse"):
        SeparableEXTRAPM(G.MixingPlan(c, CPU, dense=True), 8)
    with pytest.raises(ValueError, match="at most 4096 agents"):
        SeparableEXTRAPM(types.SimpleNamespace(n_rows=4097, kind="csr", device=CPU), 8)
    with pytest.raises(ValueError, match="objective must be one of"):
        SeparableEXTRAPM(G.MixingPlan(c, CPU), 8, objective="hinge")
    with pytest.raises(ValueError, match="self_weight: expected 8 weights"):
        SeparableEXTRAPM(G.MixingPlan(c, CPU), 8, self_weight=np.zeros(9, np.float32))
    assert rec.calls == []


def test_problem_round_makes_one_call_and_swaps(monkeypatch):
    """round() on a stand-in plan: one ops.extra_csr_pm call on (XT, YT, W, TT,
    CT), then the one swap (CT is updated in place)."""
    calls = []
    monkeypatch.setattr(ops, "extra_csr_pm", lambda *a, **k: calls.append((a, k)))
    prob = SeparableEXTRAPM.__new__(SeparableEXTRAPM)
    prob.plan = types.SimpleNamespace(rowptr="rp", col="col", val="val")
    prob.XT, prob.YT, prob.TT, prob.CT = "x", "y", "t", "c"
    prob.self_weight, prob.objective, prob.lr, prob.P, prob.rounds = "d", "logistic", 0.5, 10, 0
    prob.round()
    assert calls == [(("x", "y", "rp", "col", "val", "t", "c"), dict(self_weight="d", objective="logistic", lr=0.5, P=10))]
    assert (prob.XT, prob.YT, prob.CT, prob.rounds) == ("y", "x", "c", 1)


# ---------------------------------------------------------------------------
# the entry points' argument rules, without a launch
# ---------------------------------------------------------------------------
FAKE = 1 << 20  # never dereferenced: every refused call returns from its argument checks
X_, Y_, T_, C_, RP, COL, VAL, WS = (FAKE + (k << 16) for k in range(8))


@pytest.mark.parametrize("ex", [False, True], ids=["dol_extra_csr_pm_f32", "dol_extra_csr_pm_ex_f32"])
def test_entry_points_check_arguments_without_launch(ex):
    L = _native.lib()

    def call(x=X_, y=Y_, n=8, P=8, ld=8, ldt=None, ldc=None, t=T_, c=C_, ws=None, objective=0, rp=RP, col=COL, val=VAL,
             nseg=8):
        ldt, ldc = (ld if v is None else v for v in (ldt, ldc))
        a = (x, ld, y, ld, n, P, rp, col, val, ws, t, ldt, c, ldc, objective, 0.1)
        return L.dol_extra_csr_pm_ex_f32(*a, nseg, None) if ex else L.dol_extra_csr_pm_f32(*a, None)

    def refused(word, **kw):
        assert call(**kw) == -1, kw
        msg = L.dol_last_error()
        assert b"dol_extra_csr_pm_f32" in msg and word in msg, (kw, msg)

    for ws in (None, WS):  # self_w alone may be null
        for kw in (dict(x=None), dict(y=None), dict(t=None), dict(c=None), dict(rp=None), dict(col=None),
                   dict(val=None)):
            refused(b"null pointer", ws=ws, **kw)
    refused(b"objective must be 0 or 1", objective=2)
    refused(b"objective must be 0 or 1", objective=-1)
    if ex:
        refused(b"stage order", nseg=-1)
        refused(b"stage order", nseg=257)
    refused(b"negative size", n=-1)
    refused(b"negative size", P=-1)
    refused(b"at most 4096 agents", n=4097, ld=4100)
    for kw in (dict(ld=7), dict(ld=6), dict(ldt=4), dict(ldc=12, n=13, ld=16), dict(ldc=10)):
        refused(b"multiples of 4 covering the rounded-up agent count", **kw)
    for kw in (dict(x=X_ + 4), dict(y=Y_ + 8), dict(t=T_ + 4), dict(c=C_ + 12)):
        refused(b"16-B aligned", **kw)
    refused(b"XT and YT alias", y=X_)
    for kw in (dict(c=X_), dict(c=Y_), dict(c=T_)):
        refused(b"CT aliases XT, YT or TT", **kw)
    refused(b"leading dimension too large", n=4096, ld=1 << 29, P=1)
    refused(b"size above 2^40", P=(1 << 40) + 1)
    # nothing to do: DOL_OK whatever else is passed, nothing launched
    assert call(n=0) == 0 and call(P=0) == 0 and call(n=0, t=None, c=None) == 0
    assert L.dol_last_error() == b""
