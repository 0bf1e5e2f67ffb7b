"""The push-sum gradient-tracking round on the agent-major bank
(dol_gt_push_csr_f32, ops.gt_push_csr, MixingPlan.apply_gt_push,
SeparableGTPush).

Least squares is bit-exact against tests/gt_push_cases.py::gt_push_round, the
host restatement built from the golden-pinned oracle and single numpy float32
operations (the two divisions among them: correctly rounded on both sides).
Every bit test runs with an arbitrary positive v (linspace(0.5, 2, n)), CSR
values that are not stochastic in any sense, and NaN in the inputs' padding
columns.  The shapes play the roles they play in tests/test_gt_csr_gpu.py:
both rounds run the kernels of csrc/gt_csr.hip (16 rows per block; 512-B
XCD-pinned tiles from 512 rows; 4 KiB tiles below that and for left-over
columns; scalar columns for P % 4 and unaligned rows):
  n  5 under a block, 17 ragged on the small-n kernel, 512 / 527 the pinned
     kernel, whole and ragged blocks;
  P  1 and 7 scalar tail only, 131 one pinned tile + a 3-float tail, 300 two
     tiles + 11 left-over f4s, 1031 eight tiles + one f4 + a 3-float tail.
Irregular degrees (0 ... 9+) leave the degree-4 fast path; odd ld, a base
pointer off by one float and ld = P + 8; rows past element 2^31 on both
kernels; non-finite, signed-zero and denormal inputs with a zero and a negative
v_i.  Logistic against a device composition; ops.gt_csr's bits at v = 1 on
weights whose av is exactly 1.  Buffers: 7.0 in the outputs' padding columns
and in guard rows / guard elements around UO, SO and v_out; the padding must
survive and the four inputs keep their bits."""
import functools

import numpy as np
import pytest
import torch

import gt_cases
import gt_push_cases
from gt_cases import csr_dev, logistic_problem, padded, problem, regular, same_bits
from gt_push_cases import gt_push_round
from oracle import bits_equal
from dolhip import graph as G
from dolhip import ops
from dolhip.synthetic import SeparableGTCSR, SeparableGTPush

pytestmark = pytest.mark.gpu

F32 = np.float32


def pos_v(n):
    return np.linspace(0.5, 2.0, n).astype(F32)


def run_push(U, S, T, v, c, ws, gpu, objective="least_squares", lr=0.1, ld=None, off=0):
    """One round through ops.gt_push_csr on host U, S, T [n, P] and v [n];
    returns host (U', S', v').  off = 1: every matrix is the view M[:, 1:] of
    its buffer.  The outputs' padding columns, guard rows and v_out's guard
    elements must still hold 7.0 and the four inputs must be untouched."""
    n, P = U.shape
    ld = (P + off + 3) // 4 * 4 if ld is None else ld
    Ud, Sd, Td = (padded(A, ld, gpu, off=off) for A in (U, S, T))
    vd = torch.as_tensor(v, device=gpu)
    keep = [t.clone() for t in (Ud, Sd, Td, vd)]
    UG, SG = (torch.full((n + 2, ld), 7.0, device=gpu) for _ in range(2))
    VG = torch.full((n + 2,), 7.0, device=gpu)
    UO, SO, VO = UG[1:n + 1, off:], SG[1:n + 1, off:], VG[1:n + 1]
    wsd = None if ws is None else torch.as_tensor(ws, device=gpu)
    out = ops.gt_push_csr(Ud[:, off:], Sd[:, off:], UO, SO, *csr_dev(c, gpu), Td[:, off:], vd, VO, self_weight=wsd,
                          objective=objective, lr=lr, P=P)
    assert out[0] is UO and out[1] is SO and out[2] is VO
    torch.cuda.synchronize()
    for G_ in (UG, SG):
        assert (G_[0] == 7.0).all() and (G_[n + 1] == 7.0).all(), "wrote into a guard row"
        assert (G_[:, off + P:] == 7.0).all() and (G_[:, :off] == 7.0).all(), "wrote outside columns [0, P)"
    assert VG[0] == 7.0 and VG[n + 1] == 7.0, "wrote outside v_out"
    for t, k in zip((Ud, Sd, Td, vd), keep):
        assert same_bits(t, k), "an input changed"
    return UO[:, :P].cpu().numpy(), SO[:, :P].cpu().numpy(), VO.cpu().numpy()


def all_bits_equal(got, want):
    return all(bits_equal(g, w) for g, w in zip(got, want))


@functools.lru_cache(maxsize=None)
def ls_case(n, P, self_w):
    c, d = regular(n)
    d = d if self_w else None
    U, S, T = problem(n, P, 7 * n + P)
    v = pos_v(n)
    return U, S, T, v, c, d, gt_push_round(U, S, T, v, c, d, 0.1)


# ---------------------------------------------------------------------------
# least squares against the host restatement
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("self_w", [False, True], ids=["no self weights", "self weights"])
@pytest.mark.parametrize("P", [1, 7, 131, 300, 1031],
                         ids=["P=1 tail only", "P=7 tail only", "P=131 tile + 3-float tail", "P=300 two tiles + 11 f4",
                              "P=1031 eight tiles + f4 + tail"])
@pytest.mark.parametrize("n", [5, 17, 512, 527],
                         ids=["n=5 under a block", "n=17 ragged", "n=512 pinned", "n=527 pinned ragged"])
def test_least_squares_vs_host_restatement(n, P, self_w, gpu):
    U, S, T, v, c, d, want = ls_case(n, P, self_w)
    assert (np.diff(c.rowptr) == 4).all()  # the degree-4 fast path
    assert all_bits_equal(run_push(U, S, T, v, c, d, gpu), want)


@pytest.mark.parametrize("n", [37, 520], ids=["n=37 small-n kernel", "n=520 pinned kernel"])
@pytest.mark.parametrize("P", [1031, 7])
def test_irregular_degrees(n, P, gpu):
    """Degrees 0, 1, 2, 3, 4, 5 and >= 9 in one 16-row block; every row has a
    self weight, so the zero-degree row's av is not 0."""
    c = gt_push_cases.irregular(n)
    deg = np.diff(c.rowptr)
    assert {0, 1, 2, 3, 4, 5} <= set(deg.tolist()) and deg.max() >= 9
    assert 4 in deg[:16] and len(set(deg[:16].tolist())) >= 6 and (deg[n - 16:] == 4).any()
    d = np.linspace(0.05, 0.45, n).astype(F32)
    U, S, T = problem(n, P, n + P)
    want = gt_push_round(U, S, T, pos_v(n), c, d, 0.1)
    assert (want[2] != 0).all()
    assert all_bits_equal(run_push(U, S, T, pos_v(n), c, d, gpu), want)


# ---------------------------------------------------------------------------
# strides
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [33, 520])
def test_odd_row_stride(n, gpu):
    """ld = 1033 leaves no row but the first 16-B aligned: every column scalar."""
    U, S, T, v, c, d, want = ls_case(n, 1031, True)
    assert all_bits_equal(run_push(U, S, T, v, c, d, gpu, ld=1033), want)


@pytest.mark.parametrize("n", [33, 520])
def test_base_pointer_off_by_one_float(n, gpu):
    """M[:, 1:] of 16-B aligned rows: unaligned bases, every column scalar."""
    U, S, T, v, c, d, want = ls_case(n, 1031, True)
    assert all_bits_equal(run_push(U, S, T, v, c, d, gpu, off=1), want)


@pytest.mark.parametrize("n", [33, 520])
def test_padded_aligned_rows(n, gpu):
    """ld = P + 8 with 16-B aligned rows: the f4 body on rows with a gap between them."""
    U, S, T, v, c, d, want = ls_case(n, 1032, True)
    assert all_bits_equal(run_push(U, S, T, v, c, d, gpu, ld=1040), want)


# ---------------------------------------------------------------------------
# rows past element 2^31
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n,ld", [(5, (1 << 29) + 64), (520, (1 << 22) + 64)],
                         ids=["small-n kernel, 10.7 GB", "pinned kernel, 8.7 GB"])
def test_rows_past_element_2_pow_31(n, ld, gpu):
    """Built as tests/test_gt_csr_gpu.py::test_rows_past_element_2_pow_31: the
    five matrices are disjoint column ranges of ONE allocation (never
    initialised beyond them); the last row starts past element 2^31."""
    P = 1031
    assert (n - 1) * ld >= 1 << 31
    c, d = regular(n)
    U, S, T = problem(n, P, n)
    v = pos_v(n)
    want = gt_push_round(U, S, T, v, c, d, 0.1)
    big = torch.empty(n * ld, dtype=torch.float32, device=gpu).view(n, ld)
    Ud, Sd, Td, UO, SO = (big[:, k * 2048:k * 2048 + P] for k in range(5))
    for dst, src in ((Ud, U), (Sd, S), (Td, T)):
        dst.copy_(torch.as_tensor(src, device=gpu))
    big[:, 3 * 2048:5 * 2048] = 7.0
    VO = torch.zeros(n, device=gpu)
    ops.gt_push_csr(Ud, Sd, UO, SO, *csr_dev(c, gpu), Td, torch.as_tensor(v, device=gpu), VO,
                    self_weight=torch.as_tensor(d, device=gpu), lr=0.1)
    torch.cuda.synchronize()
    assert all_bits_equal((UO.cpu().numpy(), SO.cpu().numpy(), VO.cpu().numpy()), want)
    assert (big[:, 3 * 2048 + P:4 * 2048] == 7.0).all() and (big[:, 4 * 2048 + P:5 * 2048] == 7.0).all()
    del Ud, Sd, Td, UO, SO, big
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------
# non-finite, signed-zero and denormal inputs; a zero and a negative v_i
# ---------------------------------------------------------------------------
def same_bits_or_both_nan(got, want):
    """NaN wherever the host has NaN (the payload and sign of a NaN are the
    hardware's: x86's 0 / 0 is not the GPU's), every other element bit-equal."""
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and \
        np.array_equal(got.view(np.uint32)[~nan], np.ascontiguousarray(want).view(np.uint32)[~nan])


@pytest.mark.parametrize("self_w", [False, True], ids=["no self weights", "self weights"])
@pytest.mark.parametrize("P", [1031, 7])
@pytest.mark.parametrize("n", [33, 520])
def test_nonfinite_inputs_and_zero_or_negative_weights(n, P, self_w, gpu):
    c, d = regular(n)
    d = d if self_w else None
    U, S, T = problem(n, P, 11)
    for A, k in ((U, 1), (S, 2), (T, 3)):
        A[0, k], A[2, k], A[4, k], A[6, k], A[8, k] = np.nan, np.inf, -np.inf, -0.0, 1e-40
        A[1, 4], A[5, 5] = F32(-1e-42), F32(0.0)
    U[:, 0], S[:, 0] = -0.0, 0.0
    v = pos_v(n)
    v[3], v[9] = 0.0, -1.25  # z = u / 0 and a negative weight: IEEE, not validated
    want = gt_push_round(U, S, T, v, c, d, 0.1)
    assert np.isnan(want[0]).any() and np.isinf(want[0]).any() and np.isnan(want[1]).any()
    assert np.isinf(want[1][3]).any() or np.isnan(want[1][3]).any()  # the zero weight shows in row 3's tracker
    got = run_push(U, S, T, v, c, d, gpu)
    for g, w in zip(got, want):
        assert same_bits_or_both_nan(g, w)
    assert (got[0][:, 0].view(np.uint32) == 0).all(), "-0 inputs must mix to +0"


# ---------------------------------------------------------------------------
# logistic against a device composition
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("self_w", [False, True], ids=["no self weights", "self weights"])
@pytest.mark.parametrize("P", [1031, 7])
@pytest.mark.parametrize("n", [33, 520])
def test_logistic_vs_device_composition(n, P, self_w, gpu):
    """In the style of gt_cases.logistic_round: au, as, av from ops.mix_csr; the
    self-weight terms, u' and the two divisions on the host (one rounding
    each); g(z') and g(z) from ops.separable_grad; s' from two separate fp32
    torch ops."""
    c, d = regular(n)
    d = d if self_w else None
    U, S, T = logistic_problem(n, P)
    v = pos_v(n)
    rp, col, val = csr_dev(c, gpu)

    def mix(A):
        Y = torch.empty(A.shape, device=gpu)
        ops.mix_csr(torch.as_tensor(np.ascontiguousarray(A), device=gpu), Y, rp, col, val)
        return Y.cpu().numpy()
    vc = np.ascontiguousarray(v[:, None])
    au, as_, av = (gt_cases.add_self(mix(A), d, A) for A in (U, S, vc))
    want_u = gt_cases.sgd_step(au, S, 0.1)
    z, zn = (U / vc).astype(F32), (want_u / av).astype(F32)
    grad = gt_cases.device_grad(gpu, "logistic")
    g1, g0, asd = (torch.as_tensor(a, device=gpu) for a in (grad(zn, T), grad(z, T), as_))
    want_s = torch.sub(torch.add(asd, g1), g0).cpu().numpy()
    got = run_push(U, S, T, v, c, d, gpu, objective="logistic")
    assert all_bits_equal(got, (want_u, want_s, av[:, 0]))


# ---------------------------------------------------------------------------
# ops.gt_csr's bits at v = 1
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("objective", ["least_squares", "logistic"])
@pytest.mark.parametrize("n", [33, 520])
def test_same_bits_as_gt_csr_when_every_weight_is_one(n, objective, gpu):
    """A 4-regular pattern with every value 0.25 and no self weights: the host's
    av is ((0.25 + 0.25) + 0.25) + 0.25 = 1 exactly, u / 1 = u, and the round is
    ops.gt_csr's."""
    P = 1031
    pat = regular(n)[0]
    c = G.CSR(n, n, pat.rowptr, pat.col, np.full(pat.col.size, 0.25, F32))
    U, S, T = logistic_problem(n, P)
    ones = np.ones(n, F32)
    assert (gt_push_round(U, S, T, ones, c, None, 0.1)[2] == 1.0).all()
    got_u, got_s, got_v = run_push(U, S, T, ones, c, None, gpu, objective=objective)
    assert (got_v == 1.0).all()
    Xd, Sd, Td = (padded(A, 1032, gpu) for A in (U, S, T))
    XO, SO = torch.zeros(n, 1032, device=gpu), torch.zeros(n, 1032, device=gpu)
    ops.gt_csr(Xd, Sd, XO, SO, *csr_dev(c, gpu), Td, objective=objective, lr=0.1, P=P)
    torch.cuda.synchronize()
    assert bits_equal(got_u, XO[:, :P].cpu().numpy()) and bits_equal(got_s, SO[:, :P].cpu().numpy())


# ---------------------------------------------------------------------------
# SeparableGTPush
# ---------------------------------------------------------------------------
def _converges_where_gt_csr_is_biased(c, d, lr, rounds, gpu):
    plan = G.MixingPlan(c, gpu, allow_ring=False)
    assert plan.kind == "csr"
    push = SeparableGTPush(plan, 4096, objective="least_squares", lr=lr, self_weight=d, seed=7)
    plain = SeparableGTCSR(plan, 4096, objective="least_squares", lr=lr, self_weight=d, seed=7)
    assert same_bits(push.targets(), plain.targets()) and same_bits(push.params(), plain.params())  # the same problem
    assert same_bits(push.tracker(), ops.separable_grad(push.params(), push.targets()))
    assert (push.weights() == 1).all()
    opt = push.targets().double().mean(0, keepdim=True)
    for _ in range(rounds):
        push.round()
        plain.round()
    torch.cuda.synchronize()
    z = push.params().double()
    err = float((z - opt).abs().max())
    err_plain = float((plain.params().double() - opt).abs().max())
    print(f"max |z - mean t| after {rounds} rounds: push-sum {err:.3g} (consensus error {push.consensus_error():.3g}, "
          f"sum v {float(push.weights().double().sum()):.7f}), gt_csr on the same weights {err_plain:.3g}")
    assert push.rounds == rounds
    assert abs(float(push.weights().double().sum()) - plan.n_rows) <= 1e-5 * plan.n_rows
    assert push.distance_to_optimum() == err and err <= 1e-5
    assert err_plain > 0.05


def test_problem_reaches_the_optimum_on_a_digraph_where_gt_csr_is_biased(gpu):
    """digraph(9) with out-degree weights, 9 agents x 4096, lr 0.1, 200 rounds
    (the host tier's setting and bounds, tests/test_gt_push_host.py)."""
    c, d = G.push_sum_weights(gt_push_cases.digraph(9))
    _converges_where_gt_csr_is_biased(c, d, 0.1, 200, gpu)


def test_problem_reaches_the_optimum_on_the_reference_w_transposed(gpu):
    """The reference's 9-agent stochastic circle W as C = 1/2 (I + W^T), lr 0.05, 400 rounds."""
    c, d = gt_push_cases.reference_ring_weights(9)
    _converges_where_gt_csr_is_biased(c, d, 0.05, 400, gpu)


@pytest.mark.parametrize("objective", ["least_squares", "logistic"])
def test_problem_rounds_equal_the_op(objective, gpu):
    """Three rounds of SeparableGTPush have the bits of three ops.gt_push_csr
    calls on copies of its start state."""
    c, d = G.push_sum_weights(gt_push_cases.digraph(33))
    plan = G.MixingPlan(c, gpu)
    prob = SeparableGTPush(plan, 1031, objective=objective, lr=0.1, self_weight=d, seed=5)
    U, S, T = (t.clone() for t in (prob.bank.buffer("u"), prob.bank.buffer("s"), prob.bank.buffer("target")))
    UO, SO = torch.zeros_like(U), torch.zeros_like(S)
    v, vo = torch.ones(33, device=gpu), torch.zeros(33, device=gpu)
    for _ in range(3):
        prob.round()
        ops.gt_push_csr(U, S, UO, SO, plan.rowptr, plan.col, plan.val, T, v, vo, self_weight=prob.self_weight,
                        objective=objective, lr=0.1, P=1031)
        U, UO, S, SO, v, vo = UO, U, SO, S, vo, v
    torch.cuda.synchronize()
    assert same_bits(prob.bank.rows("u"), U[:, :1031]) and same_bits(prob.tracker(), S[:, :1031])
    assert same_bits(prob.weights(), v) and not (v == 1).all()
    assert same_bits(prob.params(), U[:, :1031] / v[:, None])


# ---------------------------------------------------------------------------
# MixingPlan.apply_gt_push
# ---------------------------------------------------------------------------
def test_apply_gt_push_gives_the_ops_bits_and_refuses_ring_and_dense_plans(gpu):
    n, P = 64, 1031
    c, d = gt_push_cases.reference_ring_weights(n)
    ring, csr = G.MixingPlan(c, gpu), G.MixingPlan(c, gpu, allow_ring=False)
    assert ring.kind == "ring" and csr.kind == "csr"
    g = torch.Generator(device=gpu).manual_seed(3)
    U, S, T = (torch.randn(n, 1032, generator=g, device=gpu)[:, :P] for _ in range(3))
    UO, SO, UO2, SO2 = (torch.zeros(n, 1032, device=gpu)[:, :P] for _ in range(4))
    v = torch.linspace(0.5, 2.0, n, device=gpu)
    vo, vo2 = torch.zeros(n, device=gpu), torch.zeros(n, device=gpu)
    dw = torch.as_tensor(d, device=gpu)
    out = csr.apply_gt_push(U, S, UO, SO, T, v, vo, self_weight=dw, objective="logistic", lr=0.1)
    assert out[0] is UO and out[1] is SO and out[2] is vo
    ops.gt_push_csr(U, S, UO2, SO2, *csr_dev(c, gpu), T, v, vo2, self_weight=dw, objective="logistic", lr=0.1)
    torch.cuda.synchronize()
    assert UO.abs().sum() > 0 and same_bits(UO, UO2) and same_bits(SO, SO2) and same_bits(vo, vo2)
    with pytest.raises(NotImplementedError, match="allow_ring=False"):
        ring.apply_gt_push(U, S, UO, SO, T, v, vo)
    with pytest.raises(NotImplementedError, match="use a CSR plan"):
        G.MixingPlan(c, gpu, dense=True).apply_gt_push(U, S, UO, SO, T, v, vo)
