"""The gradient-fed exact rounds (dol_gt_grad_csr_f32 / dol_extra_grad_csr_f32,
ops.gt_grad_csr / ops.extra_grad_csr, MixingPlan.apply_gt_grad /
apply_extra_grad, ExactMLPGossip) before a kernel runs:

* the surface: both entries declared, bound and re-exported;
* the C-ABI's own refusals, called with fake pointers that no refused call
  dereferences: negative sizes, short leading dimensions (each name), null
  pointers (each name; self_w alone may be null), the aliases among X, S, XO, SO,
  G or Gprev aliasing an output, launches above 2^24 blocks, and n == 0 / P == 0
  giving DOL_OK; dol_extra_csr_f32 keeps refusing every objective but 0 and 1
  (the fed epilogue is reachable from the new entry only);
* the ops' rules that a CPU tensor reaches, with the library call recorded
  (gt_cases.recorder): the aliases, a self-weight vector of the wrong length;
  and, marked gpu because the row validators refuse a CPU tensor first, short
  matrices for each name, a non-square W and the accepted call's exact argument
  tuple;
* MixingPlan.apply_gt_grad / apply_extra_grad: CSR plans (a slab pack
  included) run the ops, ring and dense plans are refused;
* ExactMLPGossip's own refusals and its round() on stand-ins for plan and bank;
* the host restatement of the fed gradient-tracking round against
  gt_cases.gt_round: fed with the least-squares gradients it is that round with
  the tracker one round behind."""
import types

import numpy as np
import pytest
import torch

import dolhip
import extra_cases
import grad_rounds_cases as GR
import gt_cases
from dolhip import _native, extra, graph as G, gt, ops
from dolhip.mlp_exact import ExactMLPGossip
from oracle import bits_equal
from test_ops_args_gpu import mat, named, vec

CPU = torch.device("cpu")
F32 = np.float32
I32 = torch.int32
OPS = ("gt_grad_csr", "extra_grad_csr")


# ---------------------------------------------------------------------------
# the surface
# ---------------------------------------------------------------------------
def test_surface():
    assert len(_native.SIGNATURES["dol_gt_grad_csr_f32"]) == len(_native.SIGNATURES["dol_gt_csr_f32"]) + 1 == 20
    assert len(_native.SIGNATURES["dol_extra_grad_csr_f32"]) == len(_native.SIGNATURES["dol_extra_csr_f32"]) - 1 == 16
    assert ops.gt_grad_csr is gt.gt_grad_csr and ops.extra_grad_csr is extra.extra_grad_csr
    assert callable(G.MixingPlan.apply_gt_grad) and callable(G.MixingPlan.apply_extra_grad)
    assert dolhip.ExactMLPGossip is ExactMLPGossip
    L = _native.lib()
    assert hasattr(L, "dol_gt_grad_csr_f32") and hasattr(L, "dol_extra_grad_csr_f32")


# ---------------------------------------------------------------------------
# the entry points' argument rules, without a launch
# ---------------------------------------------------------------------------
FAKE = 1 << 20  # never dereferenced: every refused call returns from its argument checks
X_, S_, XO_, SO_, G_, GP_, C_, RP, COL, VAL, WS = (FAKE + (k << 16) for k in range(11))


def _refuser(L, call, name):
    def refused(word, **kw):
        assert call(**kw) == -1, kw
        msg = L.dol_last_error()
        assert name in msg and word in msg, (kw, msg)
    return refused


def test_gt_grad_entry_point_checks_arguments_without_launch():
    L = _native.lib()

    def call(x=X_, s=S_, xo=XO_, so=SO_, n=8, P=8, ld=8, lds=None, ldxo=None, ldso=None, ldg=None, ldgp=None, rp=RP,
             col=COL, val=VAL, ws=None, g=G_, gp=GP_):
        pick = lambda v: ld if v is None else v  # noqa: E731
        return L.dol_gt_grad_csr_f32(x, ld, s, pick(lds), xo, pick(ldxo), so, pick(ldso), n, P, rp, col, val, ws, g,
                                     pick(ldg), gp, pick(ldgp), 0.1, None)

    refused = _refuser(L, call, b"dol_gt_grad_csr_f32")
    for name in ("x", "s", "xo", "so", "g", "gp", "rp", "col", "val"):  # self_w alone may be null
        refused(b"null pointer", **{name: None})
        refused(b"null pointer", ws=WS, **{name: None})
    for name in ("ld", "lds", "ldxo", "ldso", "ldg", "ldgp"):
        refused(b"ld < P", **{name: 7})
    for kw in (dict(s=X_), dict(xo=X_), dict(so=X_), dict(xo=S_), dict(so=S_), dict(so=XO_)):
        refused(b"X, S, XO, SO alias", **kw)
    for kw in (dict(g=XO_), dict(g=SO_), dict(gp=XO_), dict(gp=SO_)):
        refused(b"G or Gprev aliases XO or SO", **kw)
    refused(b"too large", n=1 << 20, P=1 << 40, ld=1 << 40)  # 2^30 column tiles x 2^16 row groups
    refused(b"too large", n=(1 << 28) + 16, P=1, ld=1)  # the scalar kernel's grid: 1 x (2^24 + 1)
    refused(b"too large", n=(1 << 28) + 16, P=1, ld=1, ws=WS)
    refused(b"negative size", n=-1)
    refused(b"negative size", P=-1)
    refused(b"size above 2^40", ld=(1 << 40) + 4)
    # G == Gprev, G == X and G == S only read: accepted by the rules (no launch here: n == 0)
    # nothing to do: DOL_OK whatever else is passed, nothing launched
    assert call(n=0) == 0 and call(P=0) == 0 and call(n=0, x=None, g=None) == 0
    assert L.dol_last_error() == b""


def test_extra_grad_entry_point_checks_arguments_without_launch():
    L = _native.lib()

    def call(x=X_, y=XO_, n=8, P=8, ld=8, ldg=None, ldc=None, g=G_, c=C_, ws=None, rp=RP, col=COL, val=VAL):
        ldg, ldc = (ld if v is None else v for v in (ldg, ldc))
        return L.dol_extra_grad_csr_f32(x, ld, y, ld, n, P, rp, col, val, ws, g, ldg, c, ldc, 0.1, None)

    refused = _refuser(L, call, b"dol_extra_grad_csr_f32")
    for ws in (None, WS):  # self_w alone may be null
        refused(b"null G", g=None, ws=ws)
        refused(b"null corr", c=None, ws=ws)
        for kw in (dict(x=None), dict(y=None), dict(rp=None), dict(col=None), dict(val=None)):
            refused(b"null pointer", ws=ws, **kw)
    refused(b"ldg < P", ldg=7)
    refused(b"ldc < P", ldc=7)
    refused(b": ld < P", ld=7, ldg=8, ldc=8)
    for kw in (dict(c=X_), dict(c=XO_), dict(c=G_)):
        refused(b"corr aliases X, Y or G", **kw)
    refused(b"G aliases Y", g=XO_)
    refused(b"X and Y alias", y=X_)
    refused(b"negative size", n=-1)
    refused(b"negative size", P=-1)
    refused(b"size above 2^40", P=(1 << 40) + 1, ld=(1 << 40) + 1)
    assert call(n=0) == 0 and call(P=0) == 0 and call(n=0, g=None, c=None) == 0
    assert L.dol_last_error() == b""


def test_the_fed_epilogue_is_reachable_from_the_new_entry_only():
    """dol_extra_csr_f32 keeps refusing every objective but 0 and 1, with its message."""
    L = _native.lib()
    for objective in (2, 3, -1):
        assert L.dol_extra_csr_f32(X_, 8, XO_, 8, 8, 8, RP, COL, VAL, None, G_, 8, C_, 8, objective, 0.1, None) == -1
        assert b"dol_extra_csr_f32: objective must be 0 (least squares) or 1 (logistic)" in L.dol_last_error()
    with pytest.raises(ValueError, match="extra_csr: objective must be one of"):
        extra_cases.host_call("extra_csr", extra_cases.host_args("extra_csr", CPU), objective="gradient")


# ---------------------------------------------------------------------------
# the ops before the library is reached
# ---------------------------------------------------------------------------
@pytest.fixture
def rec(monkeypatch):
    return gt_cases.recorder(monkeypatch)


@pytest.mark.parametrize("a,b", [("X", "S"), ("X", "XO"), ("X", "SO"), ("S", "XO"), ("S", "SO"), ("XO", "SO")])
def test_aliased_state_is_refused(a, b, rec):
    t = GR.host_args("gt_grad_csr", CPU)
    t[b] = t[a]
    with pytest.raises(ValueError, match=f"gt_grad_csr: {a} and {b} alias: the Jacobi update of x and s needs four"):
        GR.host_call("gt_grad_csr", t)
    t[b] = t[a][:, :10]  # another view of the same rows
    with pytest.raises(ValueError, match=f"gt_grad_csr: {a} and {b} alias"):
        GR.host_call("gt_grad_csr", t)
    assert rec.calls == []


@pytest.mark.parametrize("out", ["XO", "SO"])
@pytest.mark.parametrize("g", ["G", "Gprev"])
def test_a_gradient_matrix_aliasing_an_output_is_refused(g, out, rec):
    t = GR.host_args("gt_grad_csr", CPU)
    t[g] = t[out]
    with pytest.raises(ValueError, match=f"gt_grad_csr: {g} and {out} alias: the gradient rows are read"):
        GR.host_call("gt_grad_csr", t)
    assert rec.calls == []


@pytest.mark.parametrize("other", ["X", "Y", "G"])
def test_corr_aliasing_another_matrix_is_refused(other, rec):
    t = GR.host_args("extra_grad_csr", CPU)
    t["corr"] = t[other]
    with pytest.raises(ValueError, match=f"extra_grad_csr: corr and {other} alias"):
        GR.host_call("extra_grad_csr", t)
    assert rec.calls == []


def test_extra_grad_other_refusals(rec):
    t = GR.host_args("extra_grad_csr", CPU)
    t["G"] = t["Y"]
    with pytest.raises(ValueError, match="extra_grad_csr: G and Y alias"):
        GR.host_call("extra_grad_csr", t)
    for name in ("G", "corr"):
        t = GR.host_args("extra_grad_csr", CPU)
        t[name] = None
        with pytest.raises(TypeError, match=f"extra_grad_csr: {name}: expected a torch.Tensor"):
            GR.host_call("extra_grad_csr", t)
    assert rec.calls == []


def test_a_self_weight_vector_of_the_wrong_length_is_refused(rec):
    with pytest.raises(ValueError, match=r"self_weight: expected contiguous float32 \[4\]"):
        GR.host_call("gt_grad_csr", GR.host_args("gt_grad_csr", CPU), self_weight=vec(CPU, 3))
    assert rec.calls == []


@pytest.mark.parametrize("op", OPS)
def test_cpu_tensors_are_refused(op, rec):
    with pytest.raises(ops.DolNativeError, match="cpu"):
        GR.host_call(op, GR.host_args(op, CPU), self_weight=vec(CPU, 4), lr=0.5, P=10)
    assert rec.calls == []


@pytest.mark.gpu
@pytest.mark.parametrize("op", OPS)
def test_bad_self_weights_are_refused_on_the_device(op, gpu, rec):
    for bad in (vec(gpu, 3), vec(gpu, 4, torch.float64), vec(gpu, 8)[::2]):
        with pytest.raises(ValueError, match=r"self_weight: expected contiguous float32 \[4\]"):
            GR.host_call(op, GR.host_args(op, gpu), self_weight=bad)
    assert rec.calls == []


@pytest.mark.gpu
@pytest.mark.parametrize("op,name", [(op, nm) for op in OPS for nm in GR.MATRICES[op]])
def test_short_matrices_are_refused(op, name, gpu, rec):
    t = GR.host_args(op, gpu)
    t[name] = mat(gpu, 3, 10, 12)
    # the mix's output pair is checked by extra_csr's own rule (ops._csr_args), with its wording
    rows = "Y has 3 rows < 4" if (op, name) == ("extra_grad_csr", "Y") else f"{name}: expected >= 4 rows"
    with pytest.raises(ValueError, match=rows):
        GR.host_call(op, t)
    t = GR.host_args(op, gpu)
    t[name] = mat(gpu, 4, 9, 12)
    with pytest.raises(ValueError, match=f"{name}: has 9 columns < P=10"):
        GR.host_call(op, t, P=10)
    assert rec.calls == []


@pytest.mark.gpu
@pytest.mark.parametrize("op", OPS)
def test_a_non_square_w_is_refused(op, gpu, rec):
    t = GR.host_args(op, gpu)
    t["col"][2] = 4  # in place: the square-W check keeps its answers per (buffers, versions)
    with pytest.raises(ValueError, match="needs a square W"):
        GR.host_call(op, t)
    assert rec.calls == []


@pytest.mark.gpu
def test_the_accepted_calls_reach_the_library_with_these_arguments(gpu, rec):
    t = GR.host_args("gt_grad_csr", gpu)
    t["self_weight"] = vec(gpu, 4)
    out = GR.host_call("gt_grad_csr", t, self_weight=t["self_weight"], lr=0.5)
    assert out[0] is t["XO"] and out[1] is t["SO"]
    GR.host_call("gt_grad_csr", t, P=8)
    assert named(rec.calls, t, gpu) == [
        ("dol_gt_grad_csr_f32", "X+0", 12, "S+0", 12, "XO+0", 12, "SO+0", 12, 4, 10, "rowptr+0", "col+0", "val+0",
         "self_weight+0", "G+0", 12, "Gprev+0", 12, 0.5, "stream"),
        ("dol_gt_grad_csr_f32", "X+0", 12, "S+0", 12, "XO+0", 12, "SO+0", 12, 4, 8, "rowptr+0", "col+0", "val+0", None,
         "G+0", 12, "Gprev+0", 12, 0.01, "stream")]
    rec.calls.clear()
    t = GR.host_args("extra_grad_csr", gpu)
    t["self_weight"] = vec(gpu, 4)
    assert GR.host_call("extra_grad_csr", t, self_weight=t["self_weight"], lr=0.5) is t["Y"]
    GR.host_call("extra_grad_csr", t, P=8)
    assert named(rec.calls, t, gpu) == [
        ("dol_extra_grad_csr_f32", "X+0", 12, "Y+0", 12, 4, 10, "rowptr+0", "col+0", "val+0", "self_weight+0", "G+0", 12,
         "corr+0", 12, 0.5, "stream"),
        ("dol_extra_grad_csr_f32", "X+0", 12, "Y+0", 12, 4, 8, "rowptr+0", "col+0", "val+0", None, "G+0", 12, "corr+0",
         12, 0.01, "stream")]


# ---------------------------------------------------------------------------
# MixingPlan.apply_gt_grad / apply_extra_grad
# ---------------------------------------------------------------------------
def _ring_pattern(n):
    torch.manual_seed(2028)
    return G.communication_csr("circle", "stochastic", n)[0]


def test_plans_route_by_kind(monkeypatch, rec):
    seen = []
    monkeypatch.setattr(ops, "gt_grad_csr", lambda *a, **k: seen.append(("gt_grad_csr", a, k)) or (a[2], a[3]))
    monkeypatch.setattr(ops, "extra_grad_csr", lambda *a, **k: seen.append(("extra_grad_csr", a, k)) or a[1])
    monkeypatch.setattr(ops, "mix_csr_slab", lambda *a, **k: seen.append(("slab", a, k)))
    c9 = _ring_pattern(9)
    t = GR.host_args("gt_grad_csr", CPU, n=9)
    e = GR.host_args("extra_grad_csr", CPU, n=9)
    d = vec(CPU, 9)
    kw = dict(self_weight=d, lr=0.5, P=10)
    six = tuple(t[k] for k in ("X", "S", "XO", "SO", "G", "Gprev"))
    four = tuple(e[k] for k in ("X", "Y", "G", "corr"))

    csr = G.MixingPlan(c9, CPU, allow_ring=False)
    assert csr.kind == "csr"
    for _ in range(2):  # the second time with a slab pack: still the fed ops, as apply_gt
        out = csr.apply_gt_grad(*six, **kw)
        assert out[0] is t["XO"] and out[1] is t["SO"]
        name, a, k = seen.pop()
        assert name == "gt_grad_csr" and k == kw
        assert all(x is y for x, y in zip(a, six[:4] + (csr.rowptr, csr.col, csr.val) + six[4:]))
        assert csr.apply_extra_grad(*four, **kw) is e["Y"]
        name, a, k = seen.pop()
        assert name == "extra_grad_csr" and k == kw
        assert all(x is y for x, y in zip(a, four[:2] + (csr.rowptr, csr.col, csr.val) + four[2:]))
        csr.ent = csr.hdr = vec(CPU, 4, I32)
    assert seen == []

    ring = G.MixingPlan(c9, CPU)
    assert ring.kind == "ring"
    with pytest.raises(NotImplementedError, match="runs on a CSR plan; build this one with allow_ring=False"):
        ring.apply_gt_grad(*six, **kw)
    with pytest.raises(NotImplementedError, match="runs on a CSR plan; build this one with allow_ring=False"):
        ring.apply_extra_grad(*four, **kw)
    dense = G.MixingPlan(c9, CPU, dense=True)
    with pytest.raises(NotImplementedError, match="fused into the sparse mixes; use a CSR plan"):
        dense.apply_gt_grad(*six)
    with pytest.raises(NotImplementedError, match="fused into the sparse mixes; use a CSR plan"):
        dense.apply_extra_grad(*four)
    with pytest.raises(ValueError, match="X has 4 rows; W has 9 columns"):
        csr.apply_gt_grad(*(mat(CPU, 4, 10, 12) for _ in range(6)))
    csr._retire()
    with pytest.raises(RuntimeError, match="no longer holds its W"):
        csr.apply_extra_grad(*four)
    assert seen == [] and rec.calls == []


# ---------------------------------------------------------------------------
# ExactMLPGossip
# ---------------------------------------------------------------------------
def test_exact_mlp_gossip_refusals(rec):
    w_off, d = G.metropolis_weights(_ring_pattern(8))
    csr = G.MixingPlan(w_off, CPU, allow_ring=False)
    with pytest.raises(ValueError, match="method must be one of"):
        ExactMLPGossip(csr, 8, 32, 4, method="dgd", self_weight=d)
    with pytest.raises(ValueError, match="runs on a CSR plan .got kind 'ring'.; build it with allow_ring=False"):
        ExactMLPGossip(G.MixingPlan(w_off, CPU), 8, 32, 4, self_weight=d)
    with pytest.raises(ValueError, match="runs on a CSR plan .got kind 'dense'"):
        ExactMLPGossip(G.MixingPlan(w_off, CPU, dense=True), 8, 32, 4, self_weight=d)
    with pytest.raises(ValueError, match="self_weight is required"):
        ExactMLPGossip(csr, 8, 32, 4)
    with pytest.raises(ValueError, match="self_weight: expected 8 weights"):
        ExactMLPGossip(csr, 8, 32, 4, self_weight=np.ones(9, F32))
    with pytest.raises(ValueError, match="self_weight must be positive"):
        ExactMLPGossip(csr, 8, 32, 4, self_weight=np.zeros(8, F32))
    with pytest.raises(ValueError, match="rows of W = plan . diag.self_weight. must sum to one"):
        ExactMLPGossip(csr, 8, 32, 4, self_weight=np.full(8, 0.5, F32))
    # the reference's row-stochastic ring weights are not symmetric
    ref = _ring_pattern(8)
    with pytest.raises(ValueError, match="W must be symmetric"):
        ExactMLPGossip(G.MixingPlan(ref, CPU, allow_ring=False), 8, 32, 4, self_weight=np.full(8, 0.25, F32))
    assert rec.calls == []


@pytest.mark.parametrize("method", ["gt", "extra"])
def test_exact_mlp_gossip_round_on_stand_ins(method):
    """round(): forward_backward on the batch, ONE fed round on the bank's named
    buffers, then the swaps: x / y and, for "gt", s / s_out and grad / grad_prev."""
    calls = []
    sim = ExactMLPGossip.__new__(ExactMLPGossip)
    sim.method, sim.lr, sim.P, sim.rounds, sim.self_weight = method, 0.5, 420, 0, "d"
    sim.X, sim.y = "X", "y"
    sim.mlp = types.SimpleNamespace(forward_backward=lambda X, y: calls.append(("fb", X, y)) or "loss")
    sim.plan = types.SimpleNamespace(apply_gt_grad=lambda *a, **k: calls.append(("gt", a, k)),
                                     apply_extra_grad=lambda *a, **k: calls.append(("extra", a, k)))
    sim.bank = types.SimpleNamespace(buffer=lambda name: name, swap=lambda a, b: calls.append(("swap", a, b)))
    assert sim.round() == "loss" and sim.rounds == 1 and sim.last_loss == "loss"
    kw = dict(self_weight="d", lr=0.5, P=420)
    if method == "gt":
        assert calls == [("fb", "X", "y"), ("gt", ("x", "s", "y", "s_out", "grad", "grad_prev"), kw),
                         ("swap", "s", "s_out"), ("swap", "grad", "grad_prev"), ("swap", "x", "y")]
    else:
        assert calls == [("fb", "X", "y"), ("extra", ("x", "y", "grad", "corr"), kw), ("swap", "x", "y")]
    sim.X = None
    with pytest.raises(RuntimeError, match="call batch.. first"):
        sim.round()


# ---------------------------------------------------------------------------
# the host restatement
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("self_w", [False, True], ids=["no self weights", "self weights"])
def test_fed_with_least_squares_gradients_the_round_is_gt_round_one_tracker_behind(self_w):
    """K = 5 rounds on a random 4-regular graph with G = fl(x - t) each round:
    from S = 0, Gprev = 0 the fed round's X equals gt_cases.gt_round's every
    round, and its S after round k + 1 equals gt_round's S after round k (gt_round
    starts from S = g(x(0))).  Standard normal inputs: no gradient is an exact
    zero (the S = 0 start turns a -0 gradient into +0)."""
    n, P, lr = 33, 17, 0.1
    c, d = gt_cases.regular(n)
    d = d if self_w else None
    X, _, T = gt_cases.problem(n, P, 3)
    Xg, Sg = X.copy(), gt_cases.ls_grad(X, T)
    Xf, Sf, Gp = X.copy(), np.zeros_like(X), np.zeros_like(X)
    for _ in range(5):
        Gk = gt_cases.ls_grad(Xf, T)
        s_before = Sg
        Xg, Sg = gt_cases.gt_round(Xg, Sg, T, c, d, lr)
        Xf_new, Sf = GR.gt_grad_round(Xf, Sf, Gk, Gp, c, d, lr)
        Xf, Gp = Xf_new, Gk
        assert bits_equal(Xf, Xg) and bits_equal(Sf, s_before)
