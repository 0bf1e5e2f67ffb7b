"""The EXTRA round on the agent-major bank with any sparse W
(dol_extra_csr_f32, ops.extra_csr, MixingPlan.apply_extra, SeparableEXTRA,
ColumnSharded.extra_step).

Least squares is bit-exact against tests/extra_cases.py::extra_round, the host
restatement built from the golden-pinned oracle (every operation has one
rounding on both sides), on random 4-regular graphs with their own unequal
values (equal weights would hide an ordering mistake) and a nonzero correction
(a zero one would hide it altogether).  The round runs csr.hip's mixing kernels
with the ExtraEpi epilogue; the shapes name their roles in that geometry (16
rows per block; 32-f4 = 512-B XCD-pinned tiles from 512 rows; 256-thread 4 KiB
tiles below that and for the columns the pinned tiles leave over; scalar
columns for P % 4 and for unaligned rows):
  n  5 fewer rows than a block, 16 one block, 17 / 33 ragged blocks on the
     small-n kernel; 512 / 513 / 527 the pinned kernel, whole and ragged blocks;
  P  1 and 7 scalar tail only; 128 exactly one pinned tile; 131 one tile + a
     3-float tail; 300 two tiles + 11 left-over f4s on the 4 KiB-tile kernel;
     1031 eight tiles (one per XCD) + one f4 + a 3-float tail.
Irregular degrees (0, 1, 2, 3, 4, 5 and >= 9 in one 16-row block) reach the
4-at-a-time loop, its remainder loop and the branch that leaves the degree-4
fast path.  Odd ld, ld = P + 8, a base pointer off by one float, and a corr
whose ld differs from X's; non-finite and signed-zero inputs.  Logistic is
compared with a device composition (ops.mix_csr, ops.separable_grad, two torch
subtractions; the host has no expf that matches the device's bit for bit).
Buffers: NaN in the inputs' padding columns, 7.0 in the padding columns of Y
and corr and in a guard row before and after each; the padding must survive
and X and the targets keep their bits.

SeparableEXTRA: its rounds are the restatement's, and on the 16-agent random
4-regular graph with Metropolis weights, lr 0.1, 200 rounds end within 1e-5 of
mean_i t_i (tests/test_extra_host.py's bound; the float32 restatement gives
2.0e-6 at P = 8 from a zero start) where SeparableDGD on the same W, lr and
seed stays more than 0.05 away.  Measured on an MI355X, 16 x 4096 from the
seeded start: 8.2e-6, which is the floor |sum_i c_i| / (n lr) = 8.5e-6 at its
worst coordinate of 4096; DGD 0.65."""
import functools

import numpy as np
import pytest
import torch

import extra_cases as E
import gt_cases
import gt_push_cases
from gt_cases import add_self, csr_dev, logistic_problem, padded, problem, regular, same_bits, sgd_step
from oracle import bits_equal
from dolhip import graph as G
from dolhip import ops, parallel
from dolhip.synthetic import SeparableDGD, SeparableEXTRA, SeparableGTCSR

pytestmark = pytest.mark.gpu

F32 = np.float32


def run_csr(X, C, T, c, ws, gpu, objective="least_squares", lr=0.1, ld=None, off=0, ldc=None):
    """One round through ops.extra_csr on host X, C, T [n, P]; returns host (X',
    C').  off = 1: every matrix is the view M[:, 1:] of its buffer (a base
    pointer off by one float); ldc: corr's own row stride.  The padding columns
    and guard rows of Y and corr must still hold 7.0 and X and T must be
    untouched."""
    n, P = X.shape
    ld = (P + off + 3) // 4 * 4 if ld is None else ld
    ldc = ld if ldc is None else ldc
    Xd, Td = (padded(A, ld, gpu, off=off) for A in (X, T))
    keep = [t.clone() for t in (Xd, Td)]
    YG, CG = torch.full((n + 2, ld), 7.0, device=gpu), torch.full((n + 2, ldc), 7.0, device=gpu)
    Y, Cd = YG[1:n + 1, off:], CG[1:n + 1, off:]
    Cd[:, :P] = torch.as_tensor(C, device=gpu)
    wsd = None if ws is None else torch.as_tensor(ws, device=gpu)
    out = ops.extra_csr(Xd[:, off:], Y, *csr_dev(c, gpu), Td[:, off:], Cd, self_weight=wsd, objective=objective, lr=lr,
                        P=P)
    assert out is Y
    torch.cuda.synchronize()
    for G_ in (YG, CG):
        assert (G_[0] == 7.0).all() and (G_[n + 1] == 7.0).all(), "wrote into a guard row"
        assert (G_[:, off + P:] == 7.0).all() and (G_[:, :off] == 7.0).all(), "wrote outside columns [0, P)"
    for t, k in zip((Xd, Td), keep):
        assert same_bits(t, k), "an input changed"
    return Y[:, :P].cpu().numpy(), Cd[:, :P].cpu().numpy()


@functools.lru_cache(maxsize=None)
def ls_case(n, P, self_w):
    c, d = regular(n)
    d = d if self_w else None
    X, C, T = problem(n, P, 7 * n + P)
    return X, C, T, c, d, E.extra_round(X, C, T, c, d, 0.1)


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
    X, C, T, c, d, (want_x, want_c) = ls_case(n, P, self_w)
    got_x, got_c = run_csr(X, C, T, c, d, gpu)
    assert bits_equal(got_x, want_x)
    assert bits_equal(got_c, want_c)


# ---------------------------------------------------------------------------
# irregular degrees
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [37, 520], ids=["n=37 small-n kernel", "n=520 pinned kernel"])
@pytest.mark.parametrize("P", [1031, 7])
def test_irregular_degrees(n, P, gpu):
    c = gt_push_cases.irregular(n)
    deg = np.diff(c.rowptr)
    assert {0, 1, 2, 3, 4, 5} <= set(deg.tolist()) and deg.max() >= 9
    assert 4 in deg[:16] and len(set(deg[:16].tolist())) >= 6 and (deg[n - 16:] == 4).any()
    d = np.linspace(0.05, 0.45, n).astype(F32)
    X, C, T = problem(n, P, n + P)
    want_x, want_c = E.extra_round(X, C, T, c, d, 0.1)
    got_x, got_c = run_csr(X, C, T, c, d, gpu)
    assert bits_equal(got_x, want_x) and bits_equal(got_c, want_c)


# ---------------------------------------------------------------------------
# strides and alignment
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [33, 520])
@pytest.mark.parametrize("ld", [1033, 1039], ids=["odd ld", "ld = P + 8"])
def test_odd_row_strides(n, ld, gpu):
    """An odd ld leaves no row but the first 16-B aligned: every column goes
    down the scalar kernel.  ld = P + 8 = 1039 is odd as well; the aligned
    form of 'eight more than P' is the next test."""
    X, C, T, c, d, (want_x, want_c) = ls_case(n, 1031, True)
    got_x, got_c = run_csr(X, C, T, c, d, gpu, ld=ld)
    assert bits_equal(got_x, want_x) and bits_equal(got_c, want_c)


@pytest.mark.parametrize("n", [33, 520])
def test_padded_aligned_rows(n, gpu):
    """ld = P + 8 with 16-B aligned rows: the f4 body on rows with a gap between them."""
    X, C, T, c, d, (want_x, want_c) = ls_case(n, 1032, True)
    got_x, got_c = run_csr(X, C, T, c, d, gpu, ld=1040)
    assert bits_equal(got_x, want_x) and bits_equal(got_c, want_c)


@pytest.mark.parametrize("n", [33, 520])
def test_base_pointer_off_by_one_float(n, gpu):
    """M[:, 1:] of 16-B aligned rows: unaligned bases, every column scalar."""
    X, C, T, c, d, (want_x, want_c) = ls_case(n, 1031, True)
    got_x, got_c = run_csr(X, C, T, c, d, gpu, off=1)
    assert bits_equal(got_x, want_x) and bits_equal(got_c, want_c)


@pytest.mark.parametrize("n", [33, 520])
@pytest.mark.parametrize("ldc", [1048, 1037], ids=["corr ld = 1048 (f4 columns)", "corr ld = 1037 (scalar columns)"])
def test_corr_with_its_own_row_stride(n, ldc, gpu):
    """X, Y and target at ld = 1032; corr at another stride: aligned (the f4
    kernels with two strides) and odd (corr alone sends every column down the
    scalar kernel)."""
    X, C, T, c, d, (want_x, want_c) = ls_case(n, 1031, True)
    got_x, got_c = run_csr(X, C, T, c, d, gpu, ldc=ldc)
    assert bits_equal(got_x, want_x) and bits_equal(got_c, want_c)


# ---------------------------------------------------------------------------
# non-finite and signed-zero inputs
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("self_w", [False, True], ids=["no self weights", "self weights"])
@pytest.mark.parametrize("P", [1031, 7])
@pytest.mark.parametrize("n", [33, 520])
def test_nonfinite_and_signed_zero_inputs(n, P, self_w, gpu):
    """NaN, +-Inf, -0 and denormals in X, C and T come out like the host's, NaN
    for NaN.  Column 0 holds -0 in every row of X, C and T."""
    c, d = regular(n)
    d = d if self_w else None
    X, C, T = problem(n, P, 11)
    for A, k in ((X, 1), (C, 2), (T, 3)):
        A[0, k], A[2, k], A[4, k], A[6, k], A[8, k] = np.nan, np.inf, -np.inf, -0.0, 1e-40
        A[1, 4], A[5, 5] = F32(-1e-42), F32(0.0)
    X[:, 0], C[:, 0], T[:, 0] = -0.0, -0.0, -0.0
    got_x, got_c = run_csr(X, C, T, c, d, gpu)
    want_x, want_c = E.extra_round(X, C, T, c, d, 0.1)
    assert np.isnan(want_x).any() and np.isinf(want_x).any() and np.isnan(want_c).any()
    assert np.array_equal(np.isnan(got_x), np.isnan(want_x)) and np.array_equal(np.isnan(got_c), np.isnan(want_c))
    assert bits_equal(got_x, want_x) and bits_equal(got_c, want_c)


# ---------------------------------------------------------------------------
# logistic against a device composition
# ---------------------------------------------------------------------------
def logistic_round(mix, X, C, T, d, gpu, lr=0.1):
    """(x', c') of the logistic round as a device composition: mix(A) the
    layout's own device mix of host A [n, P]; the self-weight term and the two
    fmas on the host (one rounding each, exact); g(x, t) from
    ops.separable_grad; r and x' from two separate fp32 torch subtractions."""
    ax = add_self(mix(X), d, X)
    y = sgd_step(ax, gt_cases.device_grad(gpu, "logistic")(X, T), lr)
    yd, cd, xd, axd = (torch.as_tensor(np.ascontiguousarray(a, F32), device=gpu) for a in (y, C, X, ax))
    return torch.sub(yd, cd).cpu().numpy(), sgd_step(C, torch.sub(xd, axd).cpu().numpy(), -0.5)


@pytest.mark.parametrize("self_w", [False, True], ids=["no self weights", "self weights"])
@pytest.mark.parametrize("n,P", [(33, 131), (520, 1031)], ids=["small-n kernel", "pinned kernel"])
def test_logistic_vs_device_composition(n, P, self_w, gpu):
    c, d = regular(n)
    d = d if self_w else None
    X, C, T = logistic_problem(n, P)
    got_x, got_c = run_csr(X, C, T, c, d, gpu, objective="logistic")
    rp, col, val = csr_dev(c, gpu)

    def mix(A):
        Y = torch.empty(n, P, device=gpu)
        ops.mix_csr(torch.as_tensor(A, device=gpu), Y, rp, col, val)
        return Y.cpu().numpy()
    want_x, want_c = logistic_round(mix, X, C, T, d, gpu)
    assert bits_equal(got_x, want_x)
    assert bits_equal(got_c, want_c)


# ---------------------------------------------------------------------------
# MixingPlan.apply_extra with a slab pack
# ---------------------------------------------------------------------------
def _bank4(n, P, gpu, seed=3):
    """X, target, corr (standard normal) and a zeroed Y, rows of round_up(P, 4) floats."""
    g = torch.Generator(device=gpu).manual_seed(seed)
    ld = (P + 3) // 4 * 4
    X, T, C = (torch.randn(n, ld, generator=g, device=gpu)[:, :P] for _ in range(3))
    return X, torch.zeros(n, ld, device=gpu)[:, :P], T, C


def test_apply_extra_with_a_slab_pack_runs_extra_csr(gpu, monkeypatch):
    n, P = 100, 300
    c, d = regular(n)
    plan = G.MixingPlan(c, gpu, slab=True)
    assert plan.kind == "csr" and plan.ent is not None
    X, Y, T, C = _bank4(n, P, gpu)
    want_x, want_c = E.extra_round(X.cpu().numpy(), C.cpu().numpy(), T.cpu().numpy(), c, d, 0.1)
    monkeypatch.setattr(ops, "mix_csr_slab", lambda *a, **k: pytest.fail("the slab kernel has no epilogue"))
    assert plan.apply_extra(X, Y, T, C, self_weight=torch.as_tensor(d, device=gpu), lr=0.1) is Y
    torch.cuda.synchronize()
    assert bits_equal(Y.cpu().numpy(), want_x) and bits_equal(C.cpu().numpy(), want_c)


# ---------------------------------------------------------------------------
# SeparableEXTRA
# ---------------------------------------------------------------------------
def extra_problem(gpu, P, n=16, objective="least_squares", lr=0.1, seed=7):
    W, d = G.metropolis_weights(G.random_regular_csr(n, 4, seed=5))
    plan = G.MixingPlan(W, gpu)
    assert plan.kind == "csr"
    return SeparableEXTRA(plan, P, objective=objective, lr=lr, self_weight=d, seed=seed), W, d


def test_problem_is_the_gradient_tracking_problem_and_its_rounds_are_the_restatements(gpu):
    prob, W, d = extra_problem(gpu, 513, n=100)
    twin = SeparableGTCSR(prob.plan, 513, lr=0.1, self_weight=d, seed=7)
    assert same_bits(prob.params(), twin.params()) and same_bits(prob.targets(), twin.targets())
    assert not prob.correction().any()
    X, C, T = (t.cpu().numpy() for t in (prob.params(), prob.correction(), prob.targets()))
    for _ in range(5):
        prob.round()
        X, C = E.extra_round(X, C, T, W, d, 0.1)
    torch.cuda.synchronize()
    assert prob.rounds == 5
    assert bits_equal(prob.params().cpu().numpy(), X) and bits_equal(prob.correction().cpu().numpy(), C)
    assert bits_equal(prob.targets().cpu().numpy(), T)


def test_problem_reaches_the_optimum_that_dgd_misses(gpu):
    """Random 4-regular, 16 agents x 4096, Metropolis weights, lr 0.1, least
    squares: after 200 rounds every agent is within 1e-5 of mean_i t_i;
    SeparableDGD on W + diag(d) (the diagonal as a CSR entry), same lr and seed
    and so the same problem, stays more than 0.05 away at its biased fixed
    point."""
    prob, W, d = extra_problem(gpu, 4096)
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
    floor = float(prob.correction().double().sum(0).abs().max()) / (16 * 0.1)
    print(f"max |x - mean t| after 200 rounds: EXTRA {err:.3g} (consensus error {prob.consensus_error():.3g}, "
          f"|sum c| / (n lr) {floor:.3g}), DGD {err_dgd:.3g}")
    assert prob.rounds == 200
    assert prob.distance_to_optimum() == err and err <= 1e-5
    assert err_dgd > 0.05


# ---------------------------------------------------------------------------
# ColumnSharded.extra_step
# ---------------------------------------------------------------------------
def test_column_sharded_extra_step_at_world_1(gpu):
    """One process owns every column: extra_step gives the bits of ops.extra_csr
    on the full matrices, updates corr in place and swaps x / y."""
    n, P = 100, 1031
    c, d = regular(n)
    plan = G.MixingPlan(c, gpu)
    sh = parallel.ColumnSharded(plan, P, gpu)
    assert (sh.c0, sh.c1) == (0, P)
    X, Y, T, C = _bank4(n, P, gpu)
    dw = torch.as_tensor(d, device=gpu)
    t, corr = (torch.zeros_like(sh.x) for _ in range(2))
    sh.x[:, :P], t[:, :P], corr[:, :P] = X, T, C
    ops.extra_csr(X, Y, *csr_dev(c, gpu), T, C, self_weight=dw, objective="logistic", lr=0.1)
    x_before, y_before = sh.x, sh.y
    sh.extra_step(t, corr, self_weight=dw, objective="logistic", lr=0.1)
    torch.cuda.synchronize()
    assert sh.x is y_before and sh.y is x_before
    assert Y.abs().sum() > 0 and same_bits(sh.x[:, :P], Y) and same_bits(corr[:, :P], C)
    assert same_bits(sh.gather(0), Y.contiguous()) and same_bits(sh.gather(0, src=corr), C.contiguous())
