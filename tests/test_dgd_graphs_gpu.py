"""The fused DGD round (dol_dgd_ring_f32, dol_dgd_ring_edges_f32,
dol_dgd_csr_f32, dol_dgd_csr_pm_f32) and the parameter-major mix
(dol_mix_csr_pm_f32) off the easy case: irregular graphs (row degrees 0, 1, 2,
3, 4, 5, 8, 15, 16 and 40 in one graph, dgd_cases.irregular_csr), rectangular
blocks (x_rows != n_rows), non-finite and signed-zero inputs, and a logistic
objective whose expf overflows, underflows and meets +/-Inf.

Reference: oracle.mix_csr / oracle.mix_ring, then oracle.dgd_local.  Least
squares is bit-exact (bits_equal: any two NaNs are equal).  Logistic is held to
LOGISTIC_TOL (rtol 2e-6, atol 1e-6; tests/test_dgd_ref_host.py holds the oracle
itself to it against fp64 torch.optim.SGD, at N(0, 1) and at N(0, 1) x 12), and
is bit-identical between the two CSR kernels, which share the device expf.
Every output buffer has a sentinel in its padding columns and, past n_rows, in
whole rows (agent-major) / agent columns (parameter-major); all must come back
untouched.

Which test reaches which kernel template and geometry class (classes as named
by dgd_cases.pm_classes; tests/test_dgd_ref_host.py checks that the shape lists
reach every class the launch code can produce):

test_dgd_csr_irregular[<objective>-<mode>-<shape>], DgdEpi<OBJ, MODE> of each:
  40x4099      csr_mix_kernel<f4, 16> on 1024 f4 columns (one 4 KiB tile, rows of
               every degree in each 16-row group) + csr_mix_kernel<float, 16> on 3
  523x150      csr_xcd_kernel<32, 2> on 32 f4 columns: threads whose two rows are
               (4, 4), (4, other), (other, 4), (other, other), a ragged last row
               block (523 % 16 = 11, clamped to the empty last row);
               csr_mix_kernel<f4> on the 5 f4 columns left; <float> on 2
  523x259      ld = P odd: csr_mix_kernel<float, 16> on every column
  700to523x150 the 523 x 150 launches on X of 700 rows, columns up to 699
test_mix_csr_irregular_nonfinite[<shape>]: the same four launches with NoEpi
test_pm_dgd_irregular_least_squares[<x_rows>to<n_rows>-<P>-<mode>],
test_pm_dgd_irregular_logistic[<x_rows>to<n_rows>-<P>] (mode 2):
  csr_pm_kernel<1024, 16384, 2, 1, OBJ, 0 / 1> (64 KiB stages) and
  csr_pm_kernel<1024, 20480, 2, 1, OBJ, 2> (80 KiB stages); long rows (d > 4)
  through mix_quad's global-memory tail in each; per shape, modes 0 / 1 | mode 2:
  5to5        sr < gr, spt 1 | same                 (one ragged quad)
  100to100    sr = gr, spt 1 | same
  257to257    sr = 2 gr, spt 2 | same               (ragged last quad, xw 512)
  1025to1025  sr = 3 gr, spt 3 | same               (ragged last quad)
  3000to3000  sr = 2 gr = 2, spt 2 | same
  4096to4096  sr = 2, spt 2 | sr = 1, spt 1         (the largest fused launch)
  64to1000    sr = 3 gr, spt 3 | sr = 2 gr, spt 2   (nw = 1000 > xw = 256)
  4096to100   sr = 3 < gr = 32, spt 1 | sr = 4      (xw = 4096 > nw = 100)
  100to4096   sr = 3 gr = 3, spt 3 | sr = 2, spt 2  (nw = 4096 > xw = 256)
  4096to9     sr = 3 < gr = 256 | sr = 4            (three quads, the last ragged)
  200to1026   sr capped at 4 gr = 8, spt 4 | same   (ragged last quad)
test_pm_mix_irregular[<x_rows>to<n_rows>-<P>]:
  5000to5000, 8192to8192, 8190to8190  csr_pm_kernel<1024, 8192, 5, 2>: big by nq and
              by xw, long rows in second-slot quads, 8190: ragged last quad there
  5000to50    big by xw, every second-slot quad dropped
  50to5000    big by nq, xw = 256
  4096to9     csr_pm_kernel<1024, 16384, 2, 1>: sr < gr, spt 1
  100to4096   sr capped at 4 gr = 4, spt 4
  100to100    sr = 2 gr, spt 2
  1100to516   sr = 3 gr, spt 3
test_nonfinite_least_squares[<mode>-<kernel>], test_saturated_logistic[<mode>-<kernel>]:
  ring        ring_mix_dma_kernel<4, DgdEpi, true, false> on 256 f4 columns +
              ring_mix_kernel<float, DgdEpi> on 3, wrap-around, 7 rows (4 + 3)
  edges       ring_edges_kernel<f4 / float, DgdEpi>, n = 2 (both halos)
  csr         the 40x4099 launches above
  csr_xcd     the 523x150 launches above (saturated logistic only)
  csr_pm      csr_pm_kernel<.., OBJ, MODE> at 100to100, P = 7

Saturated logistic, measured on an MI355X: LOGISTIC_TOL holds at N(0, 1) x 12 on
every kernel; the largest error was 0.12 of it (csr, momentum continuing)."""
import functools

import numpy as np
import pytest
import torch

import oracle
from oracle import bits_equal
import dgd_cases as D
from dgd_cases import LOGISTIC_TOL
from dolhip import ops

pytestmark = pytest.mark.gpu

MODES = [(0.0, False), (0.9, True), (0.9, False)]  # DgdEpi<., 0>, <., 1>, <., 2>
MODE_IDS = ["mode0", "mode1", "mode2"]
LR = 0.05
SENT_Y, SENT_M = 7.0, -3.0


def r4(n):
    return (n + 3) // 4 * 4


def csr_dev(c, gpu, val=None):
    """The CSR triple on the device (copies: irregular_csr's arrays are read-only)."""
    return (torch.tensor(np.array(c.rowptr, np.int32), device=gpu), torch.tensor(np.array(c.col, np.int32), device=gpu),
            torch.tensor(np.array(c.val if val is None else val, np.float32), device=gpu))


def rows(a, n_rows, ld, gpu, fill):
    """Device matrix [n_rows, ld] of `fill` holding a in its top left corner."""
    t = torch.full((n_rows, ld), fill, dtype=torch.float32, device=gpu)
    t[:a.shape[0], :a.shape[1]] = torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    return t


def corner(t, n, P, sentinel):
    """t[:n, :P] on the host, after checking that the rest of t still holds the sentinel."""
    a = t.cpu().numpy()
    assert (a[:n, P:] == sentinel).all(), "padding columns written"
    assert (a[n:] == sentinel).all(), "rows past n_rows written"
    return np.ascontiguousarray(a[:n, :P])


def check(got, want, objective, what):
    if objective == "least_squares":
        assert bits_equal(got, want), what
    else:
        np.testing.assert_allclose(got, want, err_msg=what, **LOGISTIC_TOL)


def want_csr(c, X, T, M, objective, steps, momentum, first, val=None):
    mixed = oracle.mix_csr(X, c.rowptr, c.col, c.val if val is None else val)
    return oracle.dgd_local(mixed, T, M if momentum else None, objective, steps, LR, momentum, first)


# ----------------------------------------------------------------------------
# launchers: each returns (Y [n, P], momentum [n, P] or None) on the host
# ----------------------------------------------------------------------------
def run_csr(c, X, T, M, ld, gpu, objective, steps, momentum, first, val=None):
    """dol_dgd_csr_f32: X [x_rows, ld]; Y, the targets and the momentum have 5
    rows more than the graph, which (like columns P .. ld) hold sentinels."""
    n, P = c.n_rows, X.shape[1]
    rp, col, vd = csr_dev(c, gpu, val)
    Xd = rows(X, X.shape[0], ld, gpu, float("nan"))
    Td = rows(T, n + 5, ld, gpu, float("nan"))
    Md = rows(M, n + 5, ld, gpu, SENT_M) if momentum else None
    Yd = torch.full((n + 5, ld), SENT_Y, device=gpu)
    ops.dgd_csr(Xd, Yd, rp, col, vd, Td, Md, objective=objective, steps=steps, lr=LR, momentum=momentum,
                first_step=first, P=P)
    torch.cuda.synchronize()
    return corner(Yd, n, P, SENT_Y), corner(Md, n, P, SENT_M) if momentum else None


def run_pm(c, X, T, M, gpu, objective, steps, momentum, first, val=None):
    """dol_dgd_csr_pm_f32 on the transposed matrices: XT [P, r4(x_rows) (+ 4 or
    8)], YT / TT / MT [P, r4(n) + 8]; agent columns n .. hold sentinels."""
    n, (x_rows, P) = c.n_rows, X.shape
    rp, col, vd = csr_dev(c, gpu, val)
    XT = rows(X.T, P, r4(x_rows) + 4 * (x_rows % 3), gpu, float("nan"))
    TT = rows(T.T, P, r4(n) + 8, gpu, float("nan"))
    MT = rows(M.T, P, r4(n) + 8, gpu, SENT_M) if momentum else None
    YT = torch.full((P, r4(n) + 8), SENT_Y, device=gpu)
    ops.dgd_csr_pm(XT, YT, rp, col, vd, TT, MT, objective=objective, steps=steps, lr=LR, momentum=momentum,
                   first_step=first, x_agents=x_rows)
    torch.cuda.synchronize()
    y = corner(YT, P, n, SENT_Y).T
    return np.ascontiguousarray(y), np.ascontiguousarray(corner(MT, P, n, SENT_M).T) if momentum else None


def run_ring(X, T, M, wp, wn, gpu, objective, steps, momentum, first, halos=None):
    """dol_dgd_ring_f32 (wrap-around), or with halos = (prev, next) the two
    boundary rows through dol_dgd_ring_edges_f32; rows of ld = r4(P)."""
    n, P = X.shape
    ld = r4(P)
    Xd, Td = rows(X, n, ld, gpu, float("nan")), rows(T, n + 2, ld, gpu, float("nan"))
    Md = rows(M, n + 2, ld, gpu, SENT_M) if momentum else None
    Yd = torch.full((n + 2, ld), SENT_Y, device=gpu)
    wpd, wnd = (torch.from_numpy(w).to(gpu) for w in (wp, wn))
    kw = dict(mom=Md, objective=objective, steps=steps, lr=LR, momentum=momentum, first_step=first, P=P, n_rows=n)
    if halos is None:
        ops.dgd_ring(Xd, Yd, wpd, wnd, Td, **kw)
    else:
        hp, hn = (torch.from_numpy(np.concatenate([h, np.full(ld - P, np.nan, np.float32)])).to(gpu) for h in halos)
        ops.dgd_ring_edges(Xd, Yd, wpd, wnd, Td, hp, hn, **kw)
    torch.cuda.synchronize()
    return corner(Yd, n, P, SENT_Y), corner(Md, n, P, SENT_M) if momentum else None


# ----------------------------------------------------------------------------
# 1. the agent-major round on irregular graphs
# ----------------------------------------------------------------------------
# id: (x_rows, n_rows, P, ld)
CSR_SHAPES = {"40x4099": (40, 40, 4099, 4100), "523x150": (523, 523, 150, 152), "523x259": (523, 523, 259, 259),
              "700to523x150": (700, 523, 150, 152)}


@functools.lru_cache(maxsize=None)
def _csr_case(shape):
    x_rows, n, P, _ = CSR_SHAPES[shape]
    seed = x_rows + n + P
    return (D.irregular_csr(n, x_rows, seed), D.normal(x_rows, P, seed + 1), D.normal(n, P, seed + 2),
            D.normal(n, P, seed + 3))


@pytest.mark.parametrize("shape", list(CSR_SHAPES))
@pytest.mark.parametrize("momentum,first", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("objective", ["least_squares", "logistic"])
def test_dgd_csr_irregular(objective, momentum, first, shape, gpu):
    c, X, T, M = _csr_case(shape)
    got_y, got_m = run_csr(c, X, T, M, CSR_SHAPES[shape][3], gpu, objective, 2, momentum, first)
    want_y, want_m = want_csr(c, X, T, M, objective, 2, momentum, first)
    check(got_y, want_y, objective, "Y")
    if momentum:
        check(got_m, want_m, objective, "momentum")


@pytest.mark.parametrize("shape", list(CSR_SHAPES))
def test_mix_csr_irregular_nonfinite(shape, gpu):
    """The same launches without an epilogue (dol_mix_csr_f32, NoEpi), X non-finite."""
    x_rows, n, P, ld = CSR_SHAPES[shape]
    c = _csr_case(shape)[0]
    X = D.special(x_rows, P, x_rows + P)
    Yd = torch.full((n + 5, ld), SENT_Y, device=gpu)
    ops.mix_csr(rows(X, x_rows, ld, gpu, float("nan")), Yd, *csr_dev(c, gpu), P=P)
    torch.cuda.synchronize()
    assert bits_equal(corner(Yd, n, P, SENT_Y), oracle.mix_csr(X, c.rowptr, c.col, c.val))


# ----------------------------------------------------------------------------
# 2. the parameter-major round on irregular graphs
# ----------------------------------------------------------------------------
def _pm_id(s):
    return f"{s[0]}to{s[1]}"


@functools.lru_cache(maxsize=4)
def _pm_case(x_rows, n, P):
    seed = 3 * x_rows + 5 * n + P
    return (D.irregular_csr(n, x_rows, x_rows + n), D.normal(x_rows, P, seed + 1), D.normal(n, P, seed + 2),
            D.normal(n, P, seed + 3))


@pytest.mark.parametrize("momentum,first", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("P", D.PM_P)
@pytest.mark.parametrize("shape", D.PM_DGD_SHAPES, ids=_pm_id)
def test_pm_dgd_irregular_least_squares(shape, P, momentum, first, gpu):
    c, X, T, M = _pm_case(*shape, P)
    got_y, got_m = run_pm(c, X, T, M, gpu, "least_squares", 3, momentum, first)
    want_y, want_m = want_csr(c, X, T, M, "least_squares", 3, momentum, first)
    assert bits_equal(got_y, want_y)
    if momentum:
        assert bits_equal(got_m, want_m)


@pytest.mark.parametrize("P", D.PM_P)
@pytest.mark.parametrize("shape", D.PM_DGD_SHAPES, ids=_pm_id)
def test_pm_dgd_irregular_logistic(shape, P, gpu):
    """Momentum continuing (mode 2, the 80 KiB stages): the same bits as the
    agent-major kernel on the same inputs, and the oracle's values."""
    c, X, T, M = _pm_case(*shape, P)
    got_y, got_m = run_pm(c, X, T, M, gpu, "logistic", 3, 0.9, False)
    am_y, am_m = run_csr(c, X, T, M, r4(P), gpu, "logistic", 3, 0.9, False)
    assert bits_equal(got_y, am_y) and bits_equal(got_m, am_m)
    want_y, want_m = want_csr(c, X, T, M, "logistic", 3, 0.9, False)
    check(got_y, want_y, "logistic", "Y")
    check(got_m, want_m, "logistic", "momentum")


def test_pm_dgd_irregular_argument_errors(gpu):
    """More agents than a fused stage holds, on either side, and a momentum
    whose p-rows are shorter than round_up(n_rows, 4): DOL_EINVAL (-1), no launch."""
    c = D.irregular_csr(16, 5000, 1)
    Z = torch.zeros(3, 5000, device=gpu)
    with pytest.raises(ops.DolNativeError, match="returned -1: .*at most 4096"):
        ops.dgd_csr_pm(Z, torch.zeros(3, 16, device=gpu), *csr_dev(c, gpu), torch.zeros(3, 16, device=gpu),
                       x_agents=5000)
    c = D.irregular_csr(4100, 64, 1)
    Z = torch.zeros(3, 4100, device=gpu)
    with pytest.raises(ops.DolNativeError, match="returned -1: .*at most 4096"):
        ops.dgd_csr_pm(torch.zeros(3, 64, device=gpu), Z, *csr_dev(c, gpu), Z.clone(), x_agents=64)
    c = D.irregular_csr(17, 17, 1)
    Z = torch.zeros(3, 20, device=gpu)
    short = torch.as_strided(torch.zeros(3 * 20, device=gpu), (3, 17), (16, 1))  # ldm = 16 < 20
    with pytest.raises(ops.DolNativeError, match="returned -1: .*ldt / ldm"):
        ops.dgd_csr_pm(Z, Z.clone(), *csr_dev(c, gpu), Z.clone(), short, momentum=0.9)


# ----------------------------------------------------------------------------
# 3. the plain parameter-major mix on irregular graphs, non-finite X
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("P", D.PM_P)
@pytest.mark.parametrize("shape", D.PM_MIX_SHAPES, ids=_pm_id)
def test_pm_mix_irregular(shape, P, gpu):
    x_rows, n = shape
    c = D.irregular_csr(n, x_rows, x_rows + n)
    X = D.special(x_rows, P, x_rows + P)
    XT = rows(X.T, P, r4(x_rows) + 4 * (x_rows % 3), gpu, float("nan"))
    YT = torch.full((P, r4(n) + 8), SENT_Y, device=gpu)
    ops.mix_csr_pm(XT, YT, *csr_dev(c, gpu), x_agents=x_rows)
    torch.cuda.synchronize()
    assert bits_equal(corner(YT, P, n, SENT_Y).T, oracle.mix_csr(X, c.rowptr, c.col, c.val))


# ----------------------------------------------------------------------------
# 4 / 5. non-finite values and a saturated logistic through every epilogue
# ----------------------------------------------------------------------------
KERNELS = ["ring", "edges", "csr", "csr_pm"]
RING_N, EDGES_N, RING_P = 7, 2, 1027


def _ring_weights(n):
    rng = np.random.default_rng(n)
    return rng.random(n).astype(np.float32), rng.random(n).astype(np.float32)


def _graph(kernel):
    """(CSR or None, x_rows, n_rows, P, ld) of a kernel's case."""
    if kernel == "ring":
        return None, RING_N, RING_N, RING_P, r4(RING_P)
    if kernel == "edges":
        return None, EDGES_N, EDGES_N, RING_P, r4(RING_P)
    if kernel == "csr":
        return D.irregular_csr(40, 40, 4179), 40, 40, 4099, 4100
    if kernel == "csr_xcd":
        return D.irregular_csr(523, 523, 1196), 523, 523, 150, 152
    return D.irregular_csr(100, 100, 200), 100, 100, 7, None


def _run(kernel, c, X, T, M, w, halos, gpu, objective, steps, momentum, first, val=None):
    """(got Y, got momentum, want Y, want momentum, the oracle's mix, checked rows)."""
    n = T.shape[0]
    if kernel in ("ring", "edges"):
        wp, wn = w
        h = halos if kernel == "edges" else None
        got = run_ring(X, T, M, wp, wn, gpu, objective, steps, momentum, first, halos=h)
        mixed = oracle.mix_ring(X, wp, wn, *(h or ()))
        keep = [0, n - 1] if kernel == "edges" else list(range(n))
    else:
        if kernel == "csr_pm":
            got = run_pm(c, X, T, M, gpu, objective, steps, momentum, first, val=val)
        else:
            got = run_csr(c, X, T, M, _graph(kernel)[4], gpu, objective, steps, momentum, first, val=val)
        mixed = oracle.mix_csr(X, c.rowptr, c.col, c.val if val is None else val)
        keep = list(range(n))
    want = oracle.dgd_local(mixed, T, M if momentum else None, objective, steps, LR, momentum, first)
    return got[0], got[1], want[0], want[1], mixed, keep


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("momentum,first", MODES, ids=MODE_IDS)
def test_nonfinite_least_squares(momentum, first, kernel, gpu):
    """X, the targets, the momentum (and the halos) hold NaN, +/-Inf, -0.0, 3e38
    and subnormals: every bit of Y and of the momentum is the oracle's."""
    c, x_rows, n, P, _ = _graph(kernel)
    seed = 11 * n + P
    X, T, M = D.special(x_rows, P, seed), D.special(n, P, seed + 1), D.special(n, P, seed + 2)
    halos = tuple(D.special(1, P, seed + 3 + i)[0] for i in range(2))
    got_y, got_m, want_y, want_m, _, keep = _run(kernel, c, X, T, M, _ring_weights(n), halos, gpu, "least_squares",
                                                  2, momentum, first)
    assert np.isnan(want_y).any() and np.isinf(X).any() and np.isinf(T).any()  # (two steps turn an Inf into NaN)
    assert bits_equal(got_y[keep], want_y[keep])
    if momentum:
        assert bits_equal(got_m[keep], want_m[keep])


def _plant_saturation(kernel, c, X, T, w, halos):
    """Make the MIXED value of nine entries the saturation points (the local
    steps see the mixed row): on the ring, row 0 takes its previous row (or
    halo) with weight 1 and a zero next row in the first nine columns; on a
    graph, rows of degree 1 take their one neighbour with weight 1, the points
    laid along the columns (P >= 9: one row).  Writes X, T, the weights and the
    halo in place; returns (the CSR weights or None, the planted (rows, columns))."""
    k = len(D.SAT_X)
    if c is None:
        n = X.shape[0]
        w[0][0] = 1.0
        src = halos[0] if kernel == "edges" else X[n - 1]
        src[:k] = D.SAT_X
        X[1, :k] = 0.0
        T[0, :k] = D.SAT_T
        return None, (np.zeros(k, np.int64), np.arange(k))
    P = X.shape[1]
    val = c.val.copy()
    deg1 = np.flatnonzero(np.diff(c.rowptr) == 1)
    rr, pp = deg1[np.arange(k) // P], np.arange(k) % P
    e = c.rowptr[rr]
    assert len({(j, p) for j, p in zip(c.col[e], pp)}) == k, "two points share a source"
    val[e] = 1.0
    X[c.col[e], pp] = D.SAT_X
    T[rr, pp] = D.SAT_T
    return val, (rr, pp)


@pytest.mark.parametrize("kernel", KERNELS + ["csr_xcd"])
@pytest.mark.parametrize("momentum,first", [MODES[0], MODES[2]], ids=["mode0", "mode2"])
def test_saturated_logistic(momentum, first, kernel, gpu):
    """x, t (and the momentum) N(0, 1) x 12, 3 steps: a third of the entries
    have |t x| > 88 (expf overflows to +Inf, g = -0, or underflows, g = -t).
    Everything stays finite and within LOGISTIC_TOL of the oracle.  Nine mixed
    entries are the saturation points of tests/test_dgd_ref_host.py (t x =
    +/-100, +/-1e60, 0, 88.7 and 88.8 around expf's overflow): where the
    oracle's x comes back as the mixed value or as zero, the bits are equal."""
    c, x_rows, n, P, _ = _graph(kernel)
    seed = 13 * n + P
    X, T, M = (D.normal(r, P, seed + i, 12.0) for i, r in enumerate((x_rows, n, n)))
    w = _ring_weights(n)
    halos = tuple(D.normal(1, P, seed + 3 + i, 12.0)[0] for i in range(2))
    val, at = _plant_saturation(kernel, c, X, T, w, halos)
    got_y, got_m, want_y, want_m, mixed, keep = _run(kernel, c, X, T, M, w, halos, gpu, "logistic", 3, momentum,
                                                      first, val=val)
    assert np.array_equal(mixed[at], D.SAT_X), "the planted points did not survive the mix"
    assert np.mean(np.abs(mixed.astype(np.float64) * T) > 88) > 0.2
    err = np.abs(got_y[keep] - want_y[keep]) / (LOGISTIC_TOL["atol"] + LOGISTIC_TOL["rtol"] * np.abs(want_y[keep]))
    print(f"{kernel}: x uses {err.max():.3f} of LOGISTIC_TOL")
    assert np.isfinite(got_y[keep]).all() and (got_m is None or np.isfinite(got_m[keep]).all())
    check(got_y[keep], want_y[keep], "logistic", "Y")
    if momentum:
        check(got_m[keep], want_m[keep], "logistic", "momentum")
    same = (want_y[at] == 0) | (want_y[at].view(np.uint32) == mixed[at].view(np.uint32))
    assert same.any() and bits_equal(got_y[at][same], want_y[at][same])
