"""The SCAFFOLD least-squares round, CPU tier.

* The host restatement (tests/scaffold_cases.py: numpy float32 terms around
  the golden-pinned oracle.prox_admm_sgd and oracle.ordered_sum) against an
  independent per-element loop that rounds every operation itself and takes
  the fma exactly (rational arithmetic, rounded once).
* What the control variates are for: under client sampling (frac = 0.25)
  SeparableScaffold reaches mean_k t_k where SeparableFedAvg keeps moving, and
  the server's c stays the mean of the clients' c_k.
* The surface (ops.scaffold_ls_round, the SIGNATURES row, FED_ALGORITHMS
  untouched) and the argument rules of the op and of the entry point, without
  a launch.  The op's rules that can only be reached with device tensors
  (duplicate agents, outputs aliasing rows, theta_out = theta accepted) are
  checked, also without a launch, in tests/test_scaffold_gpu.py."""
from fractions import Fraction

import numpy as np
import pytest
import torch

from dolhip import _native, ops
from dolhip.synthetic import SeparableFedAvg, SeparableScaffold
from oracle import bits_equal
from scaffold_cases import cpu_scaffold_round, inv_steps_lr, scaffold_ls_round_ref
from test_admm_ls_host import cpu_ordered_sum
from test_fed_ls_host import cpu_fed_ls_round
from test_ops_args_gpu import Recorder

f32 = np.float32


# ---------------------------------------------------------------------------
# the restatement against an independent loop
# ---------------------------------------------------------------------------
def _round_f32(r):
    """The float32 nearest the rational r (ties to even); r != 0."""
    f = f32(float(r))  # within an ulp: the double is correctly rounded, then rounded again
    if not np.isfinite(f):
        return f
    cands = [f, np.nextafter(f, f32(np.inf)), np.nextafter(f, f32(-np.inf))]
    cands = [x for x in cands if np.isfinite(x)]
    best = min(abs(Fraction(float(x)) - r) for x in cands)
    near = [x for x in cands if abs(Fraction(float(x)) - r) == best]
    if len(near) > 1:
        near = [x for x in near if (x.view(np.uint32) & 1) == 0]
    return near[0]


def fma32(a, b, c):
    """fl(a * b + c) with one rounding."""
    a, b, c = f32(a), f32(b), f32(c)
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        with np.errstate(invalid="ignore"):
            return f32(np.float64(a) * np.float64(b) + np.float64(c))  # Inf / NaN: no rounding involved
    r = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    if r != 0:
        return _round_f32(r)
    if a == 0 or b == 0:  # a zero product keeps its sign: (-0) + (-0) = -0, every other sum of zeros is +0
        neg_prod = bool(np.signbit(a)) != bool(np.signbit(b))
        return f32(-0.0) if (neg_prod and c == 0 and np.signbit(c)) else f32(0.0)
    return f32(0.0)  # exact cancellation


def loop_round(w, buf, ci, T, theta, c, agents, first, lr, mom, steps, global_lr, scale_w, n_total):
    """The issue's arithmetic, one element and one rounding at a time."""
    w, buf, ci = w.copy(), buf.copy(), ci.copy()
    P = theta.size
    theta_out, c_out = np.empty(P, f32), np.empty(P, f32)
    inv = f32(1.0 / (steps * lr))
    nlr, mu = f32(-f32(lr)), f32(mom)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(P):
            acc_w = acc_c = None
            for k, a in enumerate(agents):
                x, b = theta[j], buf[a, j]
                for s in range(steps):
                    g = f32(x - T[a, j])
                    gp = f32(f32(g + c[j]) - ci[a, j])
                    d = gp
                    if mom != 0:
                        b = gp if (first[k] and s == 0) else f32(f32(b * mu) + gp)
                        d = b
                    x = fma32(nlr, d, x)
                dl = f32(x - theta[j])
                cn = f32(f32(ci[a, j] - c[j]) - f32(dl * inv))
                dc = f32(cn - ci[a, j])
                w[a, j], ci[a, j], buf[a, j] = x, cn, b
                acc_w = dl if k == 0 else f32(acc_w + dl)
                acc_c = dc if k == 0 else f32(acc_c + dc)
            theta_out[j] = f32(theta[j] + f32(f32(global_lr) * f32(acc_w / f32(scale_w))))
            c_out[j] = f32(c[j] + f32(acc_c / f32(n_total)))
    return w, buf, ci, theta_out, c_out


@pytest.mark.parametrize("mom,steps", [(0.5, 3), (0.0, 1), (0.9, 2)])
def test_restatement_matches_an_independent_loop(mom, steps):
    """3 agents x 5 columns: theta = -0 with t = +0 (column 0, all control
    variates zero there: the sign of the zero survives), an Inf target, a
    denormal target; two of the three agents sampled, one on its first step."""
    rng = np.random.default_rng(11)
    n, P = 3, 5
    T = rng.standard_normal((n, P)).astype(f32)
    B = rng.standard_normal((n, P)).astype(f32)
    CI = (0.3 * rng.standard_normal((n, P))).astype(f32)
    th = rng.standard_normal(P).astype(f32)
    c = (0.3 * rng.standard_normal(P)).astype(f32)
    th[0], T[:, 0], CI[:, 0], c[0] = -0.0, 0.0, 0.0, 0.0
    T[2, 1], T[0, 2] = np.inf, 1e-40
    agents, first = np.array([2, 0]), np.array([1, 0])
    w0 = np.full((n, P), 7.0, f32)
    lr, glr, scale_w, n_total = 0.05, 0.5, 2.0, 3
    got = scaffold_ls_round_ref(w0, B, CI, T, th, c, agents, first, lr, mom, steps, glr, scale_w, n_total)
    want = loop_round(w0, B, CI, T, th, c, agents, first, lr, mom, steps, glr, scale_w, n_total)
    assert bits_equal(got[0], want[0])
    if mom:
        assert bits_equal(got[1], want[1])
    else:
        assert got[1] is None
    for g, x in zip(got[2:5], want[2:]):
        assert bits_equal(g, x)
    assert bits_equal(got[0][1], w0[1]) and bits_equal(got[2][1], CI[1])  # the row not sampled
    assert not np.isfinite(got[3][1]) and np.isfinite(got[3][[0, 2, 3, 4]]).all()  # the Inf target's column only
    if steps == 1 and mom == 0.0:  # theta -0, t +0: g = -0, g' = +0 (two additions), w = fma(-lr, +0, -0) = -0
        assert got[0][0, 0] == 0 and np.signbit(got[0][0, 0])
    assert inv_steps_lr(steps, lr) == f32(1.0 / (steps * lr))


def test_fma32_is_one_rounding():
    a, b = f32(1 + 2 ** -12), f32(1 + 2 ** -12)  # a*b = 1 + 2^-11 + 2^-24: the product alone would round the tail away
    assert fma32(a, b, f32(-1.0)) == f32(2 ** -11 + 2 ** -24)
    assert f32(f32(a * b) - f32(1.0)) != fma32(a, b, f32(-1.0))
    assert np.signbit(fma32(f32(-0.05), f32(0.0), f32(-0.0))) and not np.signbit(fma32(f32(0.05), f32(0.0), f32(-0.0)))


# ---------------------------------------------------------------------------
# client sampling: SCAFFOLD settles at the optimum, FedAvg does not
# ---------------------------------------------------------------------------
SAMPLING_KW = dict(lr=0.1, local_steps=10, frac=0.25, seed=2028, device="cpu")


@pytest.mark.parametrize("mom", [0.0, 0.5])
def test_sampling_run_reaches_the_optimum_where_fedavg_does_not(mom):
    """64 x 200, 16 of 64 clients a round, 10 local steps, lr 0.1.  SCAFFOLD:
    max |theta - mean t| <= 1e-5 after 150 rounds (and up to round 200), and c
    is the mean of all 64 c_k to 1e-5.  FedAvg on the same problem (same
    targets, theta_0 and sampling stream): >= 0.1 over rounds 150-200."""
    s = SeparableScaffold(64, 200, momentum=mom, round_fn=cpu_scaffold_round, **SAMPLING_KW)
    a = SeparableFedAvg(64, 200, momentum=mom, round_fn=cpu_fed_ls_round("fedavg"), ordered_sum=cpu_ordered_sum,
                        **SAMPLING_KW)
    assert bits_equal(s.target[:, :200].numpy(), a.target[:, :200].numpy())
    assert bits_equal(s.theta[:200].numpy(), a.theta[:200].numpy())
    opt = s.optimum()

    def err(p):
        return float((p.theta[:200].double() - opt).abs().max())
    worst_s, best_a, worst_c = 0.0, np.inf, 0.0
    for r in range(200):
        s.round()
        a.round()
        if r + 1 >= 150:
            worst_s, best_a = max(worst_s, err(s)), min(best_a, err(a))
            worst_c = max(worst_c, float((s.c[:200].double() - s.ci[:, :200].double().mean(0)).abs().max()))
    print(f"momentum {mom}: rounds 150-200 scaffold max err {worst_s:.3e}, fedavg min err {best_a:.3e}, "
          f"|c - mean c_k| {worst_c:.3e}")
    assert worst_s <= 1e-5
    assert best_a >= 0.1
    assert worst_c <= 1e-5
    assert s.mom_started.sum() == (64 if mom else 0) and s.rounds == 200  # every client was sampled in 200 rounds
    h = s.history
    assert [sorted(e) for e in h] == [["dual_sq", "primal_resid_sq", "round"]] * 200
    assert h[-1]["primal_resid_sq"] > 0 and h[-1]["dual_sq"] > 0


def test_problem_class_seeding_and_order():
    from dolhip.synthetic import SeparableADMM
    s = SeparableScaffold(11, 70, momentum=0.5, local_steps=2, frac=0.5, seed=5, device="cpu",
                          round_fn=cpu_scaffold_round)
    a = SeparableADMM(11, 70, frac=0.5, seed=5, device="cpu", round_fn=cpu_fed_ls_round("fedavg"),
                      ordered_sum=cpu_ordered_sum, algorithm="fedavg")
    assert bits_equal(s.target[:, :70].numpy(), a.target[:, :70].numpy())
    assert bits_equal(s.theta[:70].numpy(), a.theta[:70].numpy())
    assert not s.ci.any() and not s.c.any() and s.m == 5
    assert list(s.sample()) == list(a.sample())  # the same np.random.choice stream
    s.round(order=[3, 9])
    assert s.mom_started.nonzero()[0].tolist() == [3, 9]
    assert not s.w[[0, 1, 2, 4]].any() and s.w[3].any() and s.ci[9].any()
    with pytest.raises(ValueError, match="distinct agent ids"):
        s.round(order=[3, 3])
    assert not isinstance(s, SeparableADMM)
    import dolhip
    assert dolhip.SeparableScaffold is SeparableScaffold


# ---------------------------------------------------------------------------
# the surface and the argument rules, without a launch
# ---------------------------------------------------------------------------
def test_surface():
    assert callable(ops.scaffold_ls_round) and "scaffold_ls_round" not in ops.__all__
    assert ops.FED_ALGORITHMS == {"fedavg": 0, "fedprox": 1, "fedadmm": 2}
    assert len(_native.SIGNATURES["dol_scaffold_ls_round_f32"]) == 26
    assert hasattr(_native.lib(), "dol_scaffold_ls_round_f32")


@pytest.fixture
def rec(monkeypatch):
    r = Recorder()
    monkeypatch.setattr(ops._native, "call", r)
    return r


def test_op_rules_reachable_on_the_host(rec):
    w, th = torch.zeros(4, 8), torch.zeros(8)
    with pytest.raises(ops.DolNativeError, match="cpu"):  # no CPU path
        ops.scaffold_ls_round(w, w.clone(), w.clone(), th, th.clone())
    with pytest.raises(ValueError, match="local_steps must be >= 1"):
        ops.scaffold_ls_round(w, w.clone(), w.clone(), th, th.clone(), local_steps=0)
    with pytest.raises(ValueError, match="lr must be > 0"):
        ops.scaffold_ls_round(w, w.clone(), w.clone(), th, th.clone(), lr=0.0)
    assert rec.calls == []


def test_entry_point_checks_arguments_without_launch():
    L = _native.lib()
    fake = 1 << 20  # never dereferenced: every call below fails its argument check first
    W, B, CI, T, TH, C, OUT, COUT = (fake + (i << 16) for i in range(8))

    def call(w=W, buf=B, ci=CI, t=T, th=TH, c=C, m=2, P=8, mom=0.5, steps=1, out=OUT, sw=2.0, cout=COUT, sc=4.0,
             ld=8, resid=None, work=None):
        return L.dol_scaffold_ls_round_f32(w, ld, buf, ld, ci, ld, t, ld, th, c, None, None, m, P, 0.1, mom, steps,
                                           10.0, 1.0, out, sw, cout, sc, resid, work, None)

    def refused(text, **kw):
        assert call(**kw) == -1 and text in L.dol_last_error(), (kw, L.dol_last_error())
    refused(b"m must be >= 1", m=0)
    refused(b"negative size", P=-1)
    refused(b"local_steps must be >= 1", steps=0)
    refused(b"scale_w and scale_c must be > 0", sw=0.0)
    refused(b"scale_w and scale_c must be > 0", sc=-1.0)
    refused(b"scale_w and scale_c must be > 0", sc=float("nan"))
    for name in ("w", "ci", "t", "th", "c", "out", "cout", "buf"):
        refused(b"null pointer", **{name: None})
    assert call(buf=None, mom=0.0, ld=4) == -1 and b"ld < P" in L.dol_last_error()  # no momentum: buf not needed
    for rows in (W, CI, T, B):
        refused(b"theta_out aliases the rows", out=rows)
        refused(b"c_out aliases the rows", cout=rows)
    refused(b"theta_out and c_out alias", cout=OUT)
    refused(b"resid_total needs a workspace", resid=fake)
    refused(b"ld < P", ld=7)
    refused(b"P >= 2^29", P=(1 << 29) - 15, ld=1 << 29)
    refused(b"size above 2^40", P=(1 << 40) + 1)
    # theta_out = theta and c_out = c pass the aliasing rule (the next check refuses this call)
    refused(b"ld < P", out=TH, cout=C, ld=7)
    assert call(P=0) == 0  # an empty problem: nothing to do (resid_total NULL: nothing to zero)
    assert call(P=0, ld=0, w=None, buf=None, ci=None, t=None, th=None, c=None, out=None, cout=None) == 0  # nor pointers
