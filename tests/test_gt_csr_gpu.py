"""The gradient-tracking round on the agent-major bank with any sparse W
(dol_gt_csr_f32, ops.gt_csr, MixingPlan.apply_gt, SeparableGTCSR,
ColumnSharded.gt_step).

Least squares is bit-exact against tests/gt_cases.py::gt_round, the host
restatement built from the golden-pinned oracle (every operation has one
rounding on both sides), on random 4-regular graphs with their own unequal
values (equal weights would hide an ordering mistake).  The shapes name the
roles they play in csrc/gt_csr.hip's geometry (16 rows per block; 32-f4 = 512-B
XCD-pinned tiles from 512 rows; 256-thread 4 KiB tiles below that and for the
columns the pinned tiles leave over; scalar columns for P % 4 and for unaligned
rows):
  n  5 fewer rows than a block, 16 one block, 17 / 33 ragged blocks on the
     small-n kernel; 512 / 513 / 527 the pinned kernel, whole and ragged blocks;
  P  1 and 7 scalar tail only; 128 exactly one pinned tile; 131 one tile + a
     3-float tail; 300 two tiles + 11 left-over f4s on the 4 KiB-tile kernel;
     1031 eight tiles (one per XCD) + one f4 + a 3-float tail;
  4100 x 132: beyond the parameter-major cap, the case gt_csr_pm refuses.
Irregular degrees (0, 1, 2, 3, 4, 5 and >= 9 in one 16-row block) reach the
4-at-a-time loop, its remainder loop and the branch that leaves the degree-4
fast path.  Odd ld, ld = P + 8 and a base pointer off by one float; rows that
start past element 2^31 on both kernels; non-finite and signed-zero inputs.
The siblings' bits: ops.gt_ring on a ring's CSR, ops.gt_csr_pm on the
transposed problem, and for logistic at 4100 x 132, where no sibling exists, a
composition of ops.mix_csr, ops.separable_grad and single fp32 operations.
Buffers: NaN in the inputs' padding columns, 7.0 in the outputs' padding
columns and in a guard row before and after each output; the padding must
survive and the three inputs keep their bits.

The rules of ops.gt_csr that need device tensors to be reached (a non-square
W, short matrices) and the accepted call's exact argument tuple are here too,
with test_ops_args_gpu.Recorder in place of the library call: a CPU tensor is
refused before them (tests/test_gt_csr_host.py has the launch-free rest)."""
import functools

import numpy as np
import pytest
import torch

import gt_cases
from gt_cases import am, csr_dev, logistic_problem, padded, pm, problem, regular, same_bits
from oracle import bits_equal
from dolhip import graph as G
from dolhip import ops, parallel
from dolhip.synthetic import SeparableDGD, SeparableGT, SeparableGTCSR, SeparableGTPM
from test_ops_args_gpu import mat, named, vec

pytestmark = pytest.mark.gpu

F32 = np.float32
I32 = torch.int32


def run_csr(X, S, T, c, ws, gpu, objective="least_squares", lr=0.1, ld=None, off=0):
    """One round through ops.gt_csr on host X, S, T [n, P]; returns host (X',
    S').  off = 1: every matrix is the view M[:, 1:] of its buffer (a base
    pointer off by one float).  The outputs' padding columns and guard rows
    must still hold 7.0 and the three inputs must be untouched."""
    n, P = X.shape
    ld = (P + off + 3) // 4 * 4 if ld is None else ld
    Xd, Sd, Td = (padded(A, ld, gpu, off=off) for A in (X, S, T))
    keep = [t.clone() for t in (Xd, Sd, Td)]
    XG, SG = (torch.full((n + 2, ld), 7.0, device=gpu) for _ in range(2))
    XO, SO = XG[1:n + 1, off:], SG[1:n + 1, off:]
    wsd = None if ws is None else torch.as_tensor(ws, device=gpu)
    out = ops.gt_csr(Xd[:, off:], Sd[:, off:], XO, SO, *csr_dev(c, gpu), Td[:, off:], self_weight=wsd,
                     objective=objective, lr=lr, P=P)
    assert out[0] is XO and out[1] is SO
    torch.cuda.synchronize()
    for G_ in (XG, SG):
        assert (G_[0] == 7.0).all() and (G_[n + 1] == 7.0).all(), "wrote into a guard row"
        assert (G_[:, off + P:] == 7.0).all() and (G_[:, :off] == 7.0).all(), "wrote outside columns [0, P)"
    for t, k in zip((Xd, Sd, Td), keep):
        assert same_bits(t, k), "an input changed"
    return XO[:, :P].cpu().numpy(), SO[:, :P].cpu().numpy()


@functools.lru_cache(maxsize=None)
def ls_case(n, P, self_w):
    c, d = regular(n)
    d = d if self_w else None
    X, S, T = problem(n, P, 7 * n + P)
    return X, S, T, c, d, gt_cases.gt_round(X, S, T, c, d, 0.1)


# ---------------------------------------------------------------------------
# least squares against the host restatement
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("self_w", [False, True], ids=["no self weights", "self weights"])
@pytest.mark.parametrize("P", [1, 7, 128, 131, 300, 1031],
                         ids=["P=1 tail only", "P=7 tail only", "P=128 one pinned tile", "P=131 tile + 3-float tail",
                              "P=300 two tiles + 11 f4", "P=1031 eight tiles + f4 + tail"])
@pytest.mark.parametrize("n", [5, 16, 17, 33, 512, 513, 527],
                         ids=["n=5 under a block", "n=16 one block", "n=17 ragged", "n=33 ragged", "n=512 pinned",
                              "n=513 pinned ragged", "n=527 pinned ragged"])
def test_least_squares_vs_host_restatement(n, P, self_w, gpu):
    X, S, T, c, d, (want_x, want_s) = ls_case(n, P, self_w)
    got_x, got_s = run_csr(X, S, T, c, d, gpu)
    assert bits_equal(got_x, want_x)
    assert bits_equal(got_s, want_s)


@pytest.mark.parametrize("self_w", [False, True], ids=["no self weights", "self weights"])
def test_beyond_the_parameter_major_cap(self_w, gpu):
    """4100 agents x 132: more agents than ops.GT_MAX_AGENTS, which gt_csr_pm refuses."""
    n, P = 4100, 132
    assert n > ops.GT_MAX_AGENTS
    X, S, T, c, d, (want_x, want_s) = ls_case(n, P, self_w)
    got_x, got_s = run_csr(X, S, T, c, d, gpu)
    assert bits_equal(got_x, want_x) and bits_equal(got_s, want_s)
    z = torch.zeros(P, 4100, device=gpu)
    with pytest.raises(ValueError, match="at most 4096 agents"):
        ops.gt_csr_pm(z, z.clone(), z.clone(), z.clone(), *csr_dev(c, gpu), z.clone())


# ---------------------------------------------------------------------------
# irregular degrees
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [37, 520], ids=["n=37 small-n kernel", "n=520 pinned kernel"])
@pytest.mark.parametrize("P", [1031, 7])
def test_irregular_degrees(n, P, gpu):
    c = gt_cases.irregular(n)
    deg = np.diff(c.rowptr)
    assert {0, 1, 2, 3, 4, 5} <= set(deg.tolist()) and deg.max() >= 9
    assert 4 in deg[:16] and len(set(deg[:16].tolist())) >= 6 and (deg[n - 16:] == 4).any()
    d = np.linspace(0.05, 0.45, n).astype(F32)
    X, S, T = problem(n, P, n + P)
    want_x, want_s = gt_cases.gt_round(X, S, T, c, d, 0.1)
    got_x, got_s = run_csr(X, S, T, c, d, gpu)
    assert bits_equal(got_x, want_x) and bits_equal(got_s, want_s)


# ---------------------------------------------------------------------------
# strides
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [33, 520])
@pytest.mark.parametrize("ld", [1033, 1039], ids=["odd ld", "ld = P + 8"])
def test_odd_row_strides(n, ld, gpu):
    """An odd ld leaves no row but the first 16-B aligned: every column goes
    down the scalar kernel.  ld = P + 8 = 1039 is odd as well; the aligned
    form of 'eight more than P' is the next test."""
    X, S, T, c, d, (want_x, want_s) = ls_case(n, 1031, True)
    got_x, got_s = run_csr(X, S, T, c, d, gpu, ld=ld)
    assert bits_equal(got_x, want_x) and bits_equal(got_s, want_s)


@pytest.mark.parametrize("n", [33, 520])
def test_padded_aligned_rows(n, gpu):
    """ld = P + 8 with 16-B aligned rows: the f4 body on rows with a gap between them."""
    X, S, T, c, d, (want_x, want_s) = ls_case(n, 1032, True)
    got_x, got_s = run_csr(X, S, T, c, d, gpu, ld=1040)
    assert bits_equal(got_x, want_x) and bits_equal(got_s, want_s)


@pytest.mark.parametrize("n", [33, 520])
def test_base_pointer_off_by_one_float(n, gpu):
    """M[:, 1:] of 16-B aligned rows: unaligned bases, every column scalar."""
    X, S, T, c, d, (want_x, want_s) = ls_case(n, 1031, True)
    got_x, got_s = run_csr(X, S, T, c, d, gpu, off=1)
    assert bits_equal(got_x, want_x) and bits_equal(got_s, want_s)


# ---------------------------------------------------------------------------
# rows past element 2^31
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n,ld", [(5, (1 << 29) + 64), (520, (1 << 22) + 64)],
                         ids=["small-n kernel, 10.7 GB", "pinned kernel, 8.7 GB"])
def test_rows_past_element_2_pow_31(n, ld, gpu):
    """Rows whose elements start past 2^31 (row 4 of five at ld = 2^29 + 64; row
    519 of 520 at ld = 2^22 + 64), where 32-bit row arithmetic would wrap.  The
    five matrices are disjoint column ranges of ONE allocation (never
    initialised beyond them)."""
    P = 1031
    assert (n - 1) * ld >= 1 << 31
    c, d = regular(n)
    X, S, T = problem(n, P, n)
    want_x, want_s = gt_cases.gt_round(X, S, T, c, d, 0.1)
    big = torch.empty(n * ld, dtype=torch.float32, device=gpu).view(n, ld)
    Xd, Sd, Td, XO, SO = (big[:, k * 2048:k * 2048 + P] for k in range(5))
    for dst, src in ((Xd, X), (Sd, S), (Td, T)):
        dst.copy_(torch.as_tensor(src, device=gpu))
    big[:, 3 * 2048:5 * 2048] = 7.0
    ops.gt_csr(Xd, Sd, XO, SO, *csr_dev(c, gpu), Td, self_weight=torch.as_tensor(d, device=gpu), lr=0.1)
    torch.cuda.synchronize()
    assert bits_equal(XO.cpu().numpy(), want_x) and bits_equal(SO.cpu().numpy(), want_s)
    assert (big[:, 3 * 2048 + P:4 * 2048] == 7.0).all() and (big[:, 4 * 2048 + P:5 * 2048] == 7.0).all()
    del Xd, Sd, Td, XO, SO, big
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------
# non-finite and signed-zero inputs
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("self_w", [False, True], ids=["no self weights", "self weights"])
@pytest.mark.parametrize("P", [1031, 7])
@pytest.mark.parametrize("n", [33, 520])
def test_nonfinite_and_signed_zero_inputs(n, P, self_w, gpu):
    """NaN, +-Inf, -0 and denormals in X, S and T come out like the host's, NaN
    for NaN.  Column 0 holds -0 in every row of X and +0 in S: the mix starts
    at +0, so x' is +0 there, not -0."""
    c, d = regular(n)
    d = d if self_w else None
    X, S, T = problem(n, P, 11)
    for A, k in ((X, 1), (S, 2), (T, 3)):
        A[0, k], A[2, k], A[4, k], A[6, k], A[8, k] = np.nan, np.inf, -np.inf, -0.0, 1e-40
        A[1, 4], A[5, 5] = F32(-1e-42), F32(0.0)
    X[:, 0], S[:, 0] = -0.0, 0.0
    got_x, got_s = run_csr(X, S, T, c, d, gpu)
    want_x, want_s = gt_cases.gt_round(X, S, T, c, d, 0.1)
    assert np.isnan(want_x).any() and np.isinf(want_x).any() and np.isnan(want_s).any()
    assert np.array_equal(np.isnan(got_x), np.isnan(want_x)) and np.array_equal(np.isnan(got_s), np.isnan(want_s))
    assert bits_equal(got_x, want_x) and bits_equal(got_s, want_s)
    assert (got_x[:, 0].view(np.uint32) == 0).all(), "-0 inputs must mix to +0"


# ---------------------------------------------------------------------------
# the siblings' bits
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("self_w", [False, True], ids=["no self weights", "self weights"])
@pytest.mark.parametrize("objective", ["least_squares", "logistic"])
@pytest.mark.parametrize("n", [9, 64, 520])
def test_same_bits_as_the_ring_round_on_a_ring_csr(n, objective, self_w, gpu):
    c, wp, wn, d = gt_cases.ring(n)
    d = d if self_w else None
    P = 1031
    X, S, T = logistic_problem(n, P)
    got_x, got_s = run_csr(X, S, T, c, d, gpu, objective=objective)
    Xd, Sd, Td = (padded(A, 1032, gpu) for A in (X, S, T))
    XO, SO = torch.zeros(n, 1032, device=gpu), torch.zeros(n, 1032, device=gpu)
    ops.gt_ring(Xd, Sd, XO, SO, torch.as_tensor(wp, device=gpu), torch.as_tensor(wn, device=gpu), Td,
                self_weight=None if d is None else torch.as_tensor(d, device=gpu), objective=objective, lr=0.1, P=P)
    torch.cuda.synchronize()
    assert bits_equal(got_x, XO[:, :P].cpu().numpy()) and bits_equal(got_s, SO[:, :P].cpu().numpy())


@pytest.mark.parametrize("objective", ["least_squares", "logistic"])
@pytest.mark.parametrize("n", [100, 1024])
def test_same_bits_as_the_parameter_major_round(n, objective, gpu):
    c, d = regular(n)
    P = 300
    X, S, T = logistic_problem(n, P)
    got_x, got_s = run_csr(X, S, T, c, d, gpu, objective=objective)
    XT, ST, TT = (pm(A, gpu) for A in (X, S, T))
    XO, SO = torch.zeros_like(XT), torch.zeros_like(XT)
    ops.gt_csr_pm(XT, ST, XO, SO, *csr_dev(c, gpu), TT, self_weight=torch.as_tensor(d, device=gpu),
                  objective=objective, lr=0.1)
    torch.cuda.synchronize()
    assert bits_equal(got_x, am(XO, n))
    assert bits_equal(got_s, am(SO, n))


@pytest.mark.parametrize("self_w", [False, True], ids=["no self weights", "self weights"])
def test_logistic_vs_device_composition_beyond_the_cap(self_w, gpu):
    """4100 x 132, where neither sibling runs: gt_cases.logistic_round with ax,
    as from ops.mix_csr."""
    n, P = 4100, 132
    c, d = regular(n)
    d = d if self_w else None
    X, S, T = logistic_problem(n, P)
    got_x, got_s = run_csr(X, S, T, c, d, gpu, objective="logistic")
    rp, col, val = csr_dev(c, gpu)

    def mix(A):
        Y = torch.empty(n, P, device=gpu)
        ops.mix_csr(torch.as_tensor(A, device=gpu), Y, rp, col, val)
        return Y.cpu().numpy()
    want_x, want_s = gt_cases.logistic_round(mix, X, S, T, d, gpu)
    assert bits_equal(got_x, want_x)
    assert bits_equal(got_s, want_s)


# ---------------------------------------------------------------------------
# MixingPlan.apply_gt
# ---------------------------------------------------------------------------
def _bank5(n, P, gpu, seed=3):
    g = torch.Generator(device=gpu).manual_seed(seed)
    ld = (P + 3) // 4 * 4
    X, S, T = (torch.randn(n, ld, generator=g, device=gpu)[:, :P] for _ in range(3))
    return X, S, T, torch.zeros(n, ld, device=gpu)[:, :P], torch.zeros(n, ld, device=gpu)[:, :P]


@pytest.mark.parametrize("objective", ["least_squares", "logistic"])
def test_apply_gt_ring_plan_and_csr_plan_of_one_w_agree(objective, gpu):
    n, P = 64, 1031
    torch.manual_seed(2028)
    c = G.communication_csr("circle", "stochastic", n)[0]
    ring, csr = G.MixingPlan(c, gpu), G.MixingPlan(c, gpu, allow_ring=False)
    assert ring.kind == "ring" and csr.kind == "csr"
    X, S, T, XO, SO = _bank5(n, P, gpu)
    XO2, SO2 = torch.zeros_like(XO), torch.zeros_like(SO)
    d = torch.linspace(0.05, 0.45, n, device=gpu)
    out = ring.apply_gt(X, S, XO, SO, T, self_weight=d, objective=objective, lr=0.1)
    assert out[0] is XO and out[1] is SO
    csr.apply_gt(X, S, XO2, SO2, T, self_weight=d, objective=objective, lr=0.1)
    torch.cuda.synchronize()
    assert XO.abs().sum() > 0 and same_bits(XO, XO2) and same_bits(SO, SO2)


def test_apply_gt_with_a_slab_pack_runs_gt_csr_and_dense_raises(gpu, monkeypatch):
    n, P = 100, 300
    c, d = regular(n)
    plan = G.MixingPlan(c, gpu, slab=True)
    assert plan.kind == "csr" and plan.ent is not None
    X, S, T, XO, SO = _bank5(n, P, gpu)
    seen = []
    real = ops.gt_csr
    monkeypatch.setattr(ops, "gt_csr", lambda *a, **k: seen.append("gt_csr") or real(*a, **k))
    monkeypatch.setattr(ops, "mix_csr_slab", lambda *a, **k: seen.append("slab"))
    dw = torch.as_tensor(d, device=gpu)
    plan.apply_gt(X, S, XO, SO, T, self_weight=dw, lr=0.1)
    torch.cuda.synchronize()
    assert seen == ["gt_csr"]
    want_x, want_s = gt_cases.gt_round(X.cpu().numpy(), S.cpu().numpy(), T.cpu().numpy(), c, d, 0.1)
    assert bits_equal(XO.cpu().numpy(), want_x) and bits_equal(SO.cpu().numpy(), want_s)
    dense = G.MixingPlan(c, gpu, dense=True)
    with pytest.raises(NotImplementedError, match="use a ring/CSR plan"):
        dense.apply_gt(X, S, XO, SO, T)


# ---------------------------------------------------------------------------
# ops.gt_csr's rules that only device tensors reach, and the accepted call
# ---------------------------------------------------------------------------
@pytest.fixture
def rec(monkeypatch):
    return gt_cases.recorder(monkeypatch)


def _args(dev):
    """gt_cases.host_args with a W that is square: the perfect matching 0 - 1, 2 - 3."""
    return dict(gt_cases.host_args("gt_csr", dev), rowptr=torch.tensor([0, 1, 2, 3, 4], dtype=I32, device=dev),
                col=torch.tensor([1, 0, 3, 2], dtype=I32, device=dev))


def _call(t, **kw):
    return gt_cases.host_call("gt_csr", t, **kw)


def test_a_non_square_w_is_refused(gpu, rec):
    t = _args(gpu)
    t["col"][2] = 4  # in place: the square-W check keeps its answers per (buffers, versions)
    with pytest.raises(ValueError, match="needs a square W"):
        _call(t)
    assert rec.calls == []


@pytest.mark.parametrize("name", ["X", "S", "XO", "SO", "target"])
def test_short_matrices_are_refused(name, gpu, rec):
    t = _args(gpu)
    t[name] = mat(gpu, 3, 10, 12)
    with pytest.raises(ValueError, match=f"{name}: expected >= 4 rows on cuda"):
        _call(t)
    t = _args(gpu)
    t[name] = mat(gpu, 4, 9, 12)
    with pytest.raises(ValueError, match=f"{name}: has 9 columns < P=10"):
        _call(t, P=10)
    t = _args(gpu)
    t[name] = mat(torch.device("cpu"), 4, 10, 12)
    with pytest.raises(ops.DolNativeError, match="cpu"):
        _call(t)
    assert rec.calls == []


def test_the_accepted_call_reaches_the_library_with_these_arguments(gpu, rec):
    t = _args(gpu)
    t["self_weight"] = vec(gpu, 4)
    out = _call(t, self_weight=t["self_weight"], objective="logistic", lr=0.5)
    assert out[0] is t["XO"] and out[1] is t["SO"]
    assert named(rec.calls, t, gpu) == [
        ("dol_gt_csr_f32", "X+0", 12, "S+0", 12, "XO+0", 12, "SO+0", 12, 4, 10, "rowptr+0", "col+0", "val+0",
         "self_weight+0", "target+0", 12, 1, 0.5, "stream")]
    rec.calls.clear()
    _call(t, P=8)
    assert named(rec.calls, t, gpu) == [
        ("dol_gt_csr_f32", "X+0", 12, "S+0", 12, "XO+0", 12, "SO+0", 12, 4, 8, "rowptr+0", "col+0", "val+0", None,
         "target+0", 12, 0, 0.01, "stream")]


# ---------------------------------------------------------------------------
# SeparableGTCSR
# ---------------------------------------------------------------------------
def gt_problem(gpu, P, n=16, objective="least_squares", lr=0.1, seed=7):
    W, d = G.metropolis_weights(G.random_regular_csr(n, 4, seed=5))
    plan = G.MixingPlan(W, gpu)
    assert plan.kind == "csr"
    return SeparableGTCSR(plan, P, objective=objective, lr=lr, self_weight=d, seed=seed), W, d


def test_problem_reaches_the_optimum_that_dgd_misses(gpu):
    """Random 4-regular, 16 agents x 4096, Metropolis weights, lr 0.1, least
    squares (the setup and bound of tests/test_gt_pm_gpu.py): after 200 rounds
    every agent is within 1e-5 of mean_i t_i (a float32 replay of
    gt_cases.gt_round on this graph at P = 64 gives 2.8e-7); SeparableDGD on
    W + diag(d) (the diagonal as a CSR entry), same lr and seed and so the same
    problem, stays above 1e-5 at its biased fixed point."""
    prob, W, d = gt_problem(gpu, 4096)
    assert same_bits(prob.tracker(), ops.separable_grad(prob.params(), prob.targets()))
    dgd = SeparableDGD(G.MixingPlan(gt_cases.with_diagonal(W, d), gpu), 4096, objective="least_squares", lr=0.1,
                       seed=7)
    assert same_bits(dgd.targets(), prob.targets()) and same_bits(dgd.params(), prob.params())  # the same problem
    opt = prob.targets().double().mean(0, keepdim=True)
    for _ in range(200):
        prob.round()
        dgd.round()
    torch.cuda.synchronize()
    x = prob.params().double()
    err = float((x - opt).abs().max())
    err_dgd = float((dgd.params().double() - opt).abs().max())
    print(f"max |x - mean t| after 200 rounds: gradient tracking {err:.3g} (consensus error "
          f"{prob.consensus_error():.3g}), DGD {err_dgd:.3g}")
    assert prob.rounds == 200
    torch.testing.assert_close(x, opt.expand_as(x), rtol=0, atol=1e-5)
    assert prob.distance_to_optimum() == err and err <= 1e-5
    assert err_dgd > 1e-5


@pytest.mark.parametrize("objective", ["least_squares", "logistic"])
def test_problem_rounds_equal_the_parameter_major_problem(objective, gpu):
    """After 5 rounds params() and tracker() have the bits of SeparableGTPM on
    the same problem (from_agent_major works on SeparableGTCSR unchanged)."""
    prob, _, _ = gt_problem(gpu, 513, n=100, objective=objective)
    twin = SeparableGTPM.from_agent_major(prob)
    for _ in range(5):
        prob.round()
        twin.round()
    torch.cuda.synchronize()
    assert prob.rounds == twin.rounds == 5
    assert same_bits(prob.params().contiguous(), twin.params())
    assert same_bits(prob.tracker().contiguous(), twin.tracker())


@pytest.mark.parametrize("objective", ["least_squares", "logistic"])
def test_problem_on_a_ring_plan_equals_the_ring_problem(objective, gpu):
    torch.manual_seed(2028)
    pattern = G.communication_csr("circle", "stochastic", 9)[0]
    w_off, d = G.metropolis_weights(pattern)
    probs = [cls(G.MixingPlan(w_off, gpu), 1031, objective=objective, lr=0.1, self_weight=d, seed=7)
             for cls in (SeparableGTCSR, SeparableGT)]
    assert probs[0].plan.kind == "ring"
    assert same_bits(probs[0].params(), probs[1].params()) and same_bits(probs[0].targets(), probs[1].targets())
    for _ in range(5):
        for p in probs:
            p.round()
    torch.cuda.synchronize()
    assert same_bits(probs[0].params(), probs[1].params()) and same_bits(probs[0].tracker(), probs[1].tracker())


@pytest.mark.parametrize("objective", ["least_squares", "logistic"])
def test_tracking_invariant(objective, gpu):
    """W is doubly stochastic, so after a round mean_i s_i = mean_i g(x_i)
    (the tolerances of tests/test_gt_pm_gpu.py::test_tracking_invariant)."""
    prob, _, _ = gt_problem(gpu, 1000, objective=objective)
    prob.round()
    g = ops.separable_grad(prob.params(), prob.targets(), None, objective)
    torch.testing.assert_close(prob.tracker().double().mean(0), g.double().mean(0), rtol=1e-4, atol=1e-5)


# ---------------------------------------------------------------------------
# ColumnSharded.gt_step
# ---------------------------------------------------------------------------
def test_column_sharded_gt_step_at_world_1(gpu):
    """One process owns every column: gt_step gives the bits of ops.gt_csr on
    the full matrices, swaps x / y and returns the tracker pair swapped."""
    n, P = 100, 1031
    c, d = regular(n)
    plan = G.MixingPlan(c, gpu)
    sh = parallel.ColumnSharded(plan, P, gpu)
    assert (sh.c0, sh.c1) == (0, P)
    X, S, T, XO, SO = _bank5(n, P, gpu)
    dw = torch.as_tensor(d, device=gpu)
    ops.gt_csr(X, S, XO, SO, *csr_dev(c, gpu), T, self_weight=dw, objective="logistic", lr=0.1)
    sh.x[:, :P] = X
    s, s_out, t = (torch.zeros_like(sh.x) for _ in range(3))
    s[:, :P], t[:, :P] = S, T
    x_before, y_before = sh.x, sh.y
    got = sh.gt_step(s, s_out, t, self_weight=dw, objective="logistic", lr=0.1)
    torch.cuda.synchronize()
    assert got[0] is s_out and got[1] is s and sh.x is y_before and sh.y is x_before
    assert same_bits(sh.x[:, :P], XO) and same_bits(got[0][:, :P], SO)
    assert same_bits(sh.gather(0), XO.contiguous()) and same_bits(sh.gather(0, src=got[0]), SO.contiguous())
