"""The checker of the fused DGD round's logistic step, checked itself, on the
CPU (the GPU side is tests/test_dgd_graphs_gpu.py):

1. oracle.dgd_local("logistic") agrees with the reference's own local update
   (DIST/clients.py:43-49: torch.optim.SGD(lr, momentum)) taken in fp64 on
   softplus(-t x).sum(), for 1 and 3 steps, the three momentum modes and two
   input scales on a (6, 4001) matrix: N(0, 1), and N(0, 1) x 12 on x and t,
   where 35 % of the entries have |t x| > 88 (expf overflows) and everything
   stays finite.
     x: LOGISTIC_TOL (rtol 2e-6, atol 1e-6).  Measured: no violation; largest
        absolute error 3.5e-7 at scale 1, 5.5e-6 at scale 12 (|x| in the tens).
     momentum: |error| <= MOM_RTOL * max(|M'|, |t|) per entry.  Measured on
        these seeded inputs: largest error 1.0e-6 at scale 1 and 3.7e-5 at
        scale 12 after 3 steps; relative to max(|M'|, |t|) the largest ratio is
        5.7e-7 (scale 12, 3 steps, first-step mode).  MOM_RTOL = 2.3e-6 is 4 x
        that measured value.
2. a numpy fp32 restatement of the step stays inside those tolerances, and each
   of five deliberate errors (exp(-t x) for exp(t x); +t for -t; the buffer not
   reset on a first step; dampening; x updated before the buffer) leaves them
   by at least ten times on every case it applies to;
3. the logistic formula of SeparableDGD.loss has the oracle's g as its gradient;
4. the nine saturation points give the exact known values;
5. the parameter-major shapes of the GPU tests reach every class of launch
   geometry mix_csr_pm_impl can produce."""
import functools

import numpy as np
import pytest
import torch

import oracle
import dgd_cases as D
from dgd_cases import LOGISTIC_TOL

MOM_RTOL = 2.3e-6   # 4 x 5.7e-7, the oracle's measured momentum error relative to max(|M'|, |t|)
MARGIN = 10.0
LR, MU = 0.05, 0.9
MODES = [(0.0, False), (MU, True), (MU, False)]
SCALES = [1.0, 12.0]
SHAPE = (6, 4001)


@functools.lru_cache(maxsize=None)
def _inputs(scale):
    return tuple(D.normal(*SHAPE, seed, scale) for seed in (101, 102, 103))


@functools.lru_cache(maxsize=None)
def _ref(scale, steps, momentum, first):
    Y, T, M = _inputs(scale)
    return D.dgd_local_fp64(Y, T, M, steps, LR, momentum, first)


def _ratios(got, want, T):
    """(x, momentum) errors as fractions of their tolerances (momentum 0.0 when there is none)."""
    (gy, gm), (wy, wm) = got, want
    rx = float(np.max(np.abs(gy - wy) / (LOGISTIC_TOL["atol"] + LOGISTIC_TOL["rtol"] * np.abs(wy))))
    rm = 0.0
    if wm is not None:
        rm = float(np.max(np.abs(gm - wm) / (MOM_RTOL * np.maximum(np.abs(wm), np.abs(T)))))
    return rx, rm


def test_scale_12_saturates_a_third_of_the_entries():
    Y, T, _ = _inputs(12.0)
    assert 0.3 < np.mean(np.abs(Y.astype(np.float64) * T) > 88) < 0.4


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("momentum,first", MODES)
@pytest.mark.parametrize("steps", [1, 3])
def test_logistic_oracle_matches_fp64_sgd(steps, momentum, first, scale):
    Y, T, M = _inputs(scale)
    got = oracle.dgd_local(Y, T, M if momentum else None, "logistic", steps, LR, momentum, first)
    want = _ref(scale, steps, momentum, first)
    assert np.isfinite(got[0]).all() and (not momentum or np.isfinite(got[1]).all())
    rx, rm = _ratios(got, want, T)
    print(f"x uses {rx:.3f} of LOGISTIC_TOL, momentum {rm:.3f} of MOM_RTOL")
    np.testing.assert_allclose(got[0], want[0], **LOGISTIC_TOL)
    assert rx <= 1.0 and rm <= 1.0, f"x uses {rx:.3f} of its tolerance, the momentum {rm:.3f}"


MUTATIONS = ("exp_sign", "t_sign", "no_reset", "dampening", "x_before_buffer")


def mutation_applies(mut, steps, momentum, first):
    if mut in ("exp_sign", "t_sign"):
        return True
    if not momentum:
        return False
    if mut == "no_reset":
        return first
    if mut == "dampening":  # torch applies it from the second buffer update on
        return steps > 1 or not first
    return True


def step_f32(Y, T, M, steps, lr, momentum, first, mutate=None):
    """oracle_dgd_local_f32's logistic step in numpy fp32 (fp64 products rounded
    once where the C has one rounding), with one deliberate error."""
    if mutate is not None and mutate not in MUTATIONS:
        raise ValueError(f"unknown mutation {mutate}")
    f32, f64 = np.float32, np.float64
    x, t = Y.astype(f32), T.astype(f32)
    b = M.astype(f32) if momentum else None
    lr, mom = f32(lr), f32(momentum)
    with np.errstate(over="ignore", under="ignore"):
        for s in range(steps):
            z = t * x
            num = t if mutate == "t_sign" else -t
            g = num / (f32(1) + np.exp(-z if mutate == "exp_sign" else z, dtype=f32))
            d = g
            if momentum:
                old = b
                if first and s == 0 and mutate != "no_reset":
                    b = g
                else:
                    b = b * mom + (g * (f32(1) - mom) if mutate == "dampening" else g)
                d = old if mutate == "x_before_buffer" else b
            x = (x.astype(f64) - lr.astype(f64) * d.astype(f64)).astype(f32)
    return x, b


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("momentum,first", MODES)
@pytest.mark.parametrize("steps", [1, 3])
def test_restatement_inside_and_every_mutant_10x_outside(steps, momentum, first, scale):
    Y, T, M = _inputs(scale)
    want = _ref(scale, steps, momentum, first)
    assert max(_ratios(step_f32(Y, T, M, steps, LR, momentum, first), want, T)) <= 1.0
    for mut in MUTATIONS:
        if not mutation_applies(mut, steps, momentum, first):
            continue
        worst = max(_ratios(step_f32(Y, T, M, steps, LR, momentum, first, mutate=mut), want, T))
        assert worst >= MARGIN, f"{mut}: moves the checked outputs by only {worst:.2f} x the tolerance"


def test_every_mutation_applies_somewhere_and_unknown_ones_are_refused():
    cases = [(s, m, f) for s in (1, 3) for m, f in MODES]
    for mut in MUTATIONS:
        assert any(mutation_applies(mut, *c) for c in cases), mut
    with pytest.raises(ValueError, match="unknown mutation"):
        step_f32(*_inputs(1.0), 1, LR, 0.0, False, mutate="nope")


@pytest.mark.parametrize("scale", SCALES)
def test_loss_formula_has_the_oracles_gradient(scale):
    """SeparableDGD.loss (dolhip/synthetic.py) returns, for the logistic
    objective, softplus(-t * x).sum(1) per agent: restated here (the class
    needs a device).  Its fp64 autograd gradient is the oracle's g, read off
    the momentum buffer after one first momentum step (buf = g)."""
    x, t = (D.normal(3, 257, seed, scale) for seed in (7, 8))
    xd = torch.tensor(x.astype(np.float64), requires_grad=True)
    td = torch.tensor(t.astype(np.float64))
    torch.nn.functional.softplus(-td * xd).sum(1).sum().backward()
    _, g = oracle.dgd_local(x, t, np.zeros_like(x), "logistic", 1, LR, MU, True)
    want = xd.grad.numpy()
    assert np.all(np.abs(g - want) <= MOM_RTOL * np.maximum(np.abs(want), np.abs(t)))


def test_saturation_points_exact():
    got, _ = oracle.dgd_local(D.SAT_X[None], D.SAT_T[None], None, "logistic", 1, D.SAT_LR, 0.0, False)
    assert not np.isnan(got).any()
    assert np.array_equal(got[0], D.SAT_WANT), got[0]
    assert not np.signbit(got[0][5:7]).any()  # x = +/-0 both move to +0.15
    unchanged = [0, 2, 3, 7, 8]               # g = -0, or below half an ulp of x
    assert oracle.bits_equal(got[0][unchanged], D.SAT_X[unchanged])
    want64, _ = D.dgd_local_fp64(D.SAT_X[None], D.SAT_T[None], None, 1, D.SAT_LR, 0.0, False)
    np.testing.assert_allclose(got, want64, **LOGISTIC_TOL)


# ----------------------------------------------------------------------------
# the parameter-major launch geometry
# ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _reachable(ne):
    """Every class mix_csr_pm_impl can produce for ne staged operands, by
    walking all image widths xw and quad counts nq it accepts."""
    lim = D.PM_MAX if ne == 0 else D.PM_DGD_MAX
    out = set()
    for xw in range(256, lim + 1, 256):
        for nq in range(1, lim // 4 + 1):
            out |= D.pm_classes(xw, 4 * nq, ne)
    return out


def test_pm_geometry_restates_known_launches():
    """Geometries stated in csrc/pmajor.hip's comments: 1024 agents run 64 KiB
    stages of 16 p-rows (80 KiB with the momentum read), four quads' p-rows
    side by side; beyond 4096 agents one p-row per 32 KiB stage, two quads
    per thread."""
    g = D.pm_geometry(1024, 1024, 0)
    assert (g["xw"], g["nq"], g["SF"], g["sr"], g["gr"], g["spt"], g["big"]) == (1024, 256, 16384, 16, 4, 4, False)
    g = D.pm_geometry(1024, 1024, 2)
    assert (g["SF"], g["sr"], g["spt"]) == (20480, 4, 1)
    g = D.pm_geometry(8192, 8192, 0)
    assert (g["big"], g["SF"], g["sr"], g["spt"]) == (True, 8192, 1, 2)
    assert not D.pm_geometry(4096, 4096, 2)["big"] and D.pm_geometry(4097, 9, 0)["big"]
    assert D.pm_geometry(9, 4097, 0)["big"]


@pytest.mark.parametrize("ne,shapes", [(0, "PM_MIX_SHAPES"), (1, "PM_DGD_SHAPES"), (2, "PM_DGD_SHAPES")])
def test_gpu_shapes_reach_every_geometry_class(ne, shapes):
    """ne = 0: csr_pm_kernel<.., 1> / <.., 2> of the plain mix; 1: the fused
    round without a momentum read (64 KiB stages); 2: with it (80 KiB)."""
    want = _reachable(ne)
    named = {"sr < gr", "sr capped at 4 gr", "sr a multiple of gr below the cap", "spt 1", "spt 2", "spt 4"}
    named |= {"big by nq", "big by xw", "SF 16384"} if ne == 0 else {"SF 20480" if ne == 2 else "SF 16384"}
    assert named <= want, f"the launch code no longer produces {sorted(named - want)}"
    have = set()
    for s in getattr(D, shapes):
        g = D.pm_geometry(*s, ne)
        assert g["sr"] >= 1 and (ne == 0 or not g["big"]), s
        have |= D.pm_classes(*s, ne)
    assert have == want, f"ne = {ne}: no shape of {shapes} reaches {sorted(want - have)}"


def test_pm_shapes_cover_the_row_cases():
    """Besides the geometry: x_rows != n_rows both ways, a ragged last quad in
    either slot, an empty second slot, and long rows in a second-slot quad."""
    dgd, mix = D.PM_DGD_SHAPES, D.PM_MIX_SHAPES
    assert any(x < n for x, n in dgd) and any(x > n for x, n in dgd)
    assert any(n % 4 for _, n in dgd) and any(n % 4 == 0 for _, n in dgd)
    assert any(n > 4 * D.K_T1 and n % 4 for _, n in mix), "ragged last quad in the second slot"
    assert any(x > 4096 and n <= 4 * D.K_T1 for x, n in mix), "big by xw with every second-slot quad dropped"
    for x, n in mix:
        if n > 4 * D.K_T1:
            assert D.row_degrees(n, x)[4 * D.K_T1:].max() > 4, "no long row in the second slot"
