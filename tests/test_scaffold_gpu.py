"""The one-pass SCAFFOLD least-squares round on the GPU
(dol_scaffold_ls_round_f32, ops.scaffold_ls_round, SeparableScaffold).

Everything is bit for bit the host restatement of tests/scaffold_cases.py
(which tests/test_scaffold_host.py holds to an independent loop); resid_total
is within rtol 1e-12 of it (another fp64 summation order).

* test_fed_ls_gpu.py's grid: the f4 path, the scalar path (rows off 16-byte
  alignment), the tail, full and partial prefetch groups, 256-lane strips;
  nonzero c and c_k, mixed first-step flags, NaN padding, rows not sampled.
* One case on 1024-lane strips (the smallest that takes that branch).
* theta_out = theta and c_out = c; global_lr and scale_w.
* SeparableScaffold on the GPU against its CPU replay; graph capture.
* The op's argument rules that need device tensors, without a launch."""
import numpy as np
import pytest
import torch

from dolhip import ops
from dolhip.synthetic import SeparableScaffold
from oracle import bits_equal
from scaffold_cases import FIRST, LR, N, ORDER, cpu_scaffold_round, inputs, scaffold_ls_round_ref
from test_ops_args_gpu import Recorder

pytestmark = pytest.mark.gpu

GRID = [(4096, 0), (1031, 0), (1031, 1), (3, 0), (5000, 3), (70001, 0)]
MOM_STEPS = [(0.5, 3), (0.0, 1), (0.9, 2)]
SCALES = [(1.0, None), (0.5, 1.0)]  # (global_lr, scale_w)
W0 = 7.0  # what the w rows hold before the round (w is only written, and only for the sampled rows)


def _mat(a, ld, gpu):
    """a in a NaN-filled [rows, ld] matrix (ld - P columns of padding)."""
    t = torch.full((a.shape[0], ld), float("nan"), device=gpu)
    t[:, :a.shape[1]] = torch.as_tensor(a, device=gpu)
    return t


def _check_state(got, want, P, mom):
    """got: the device (w, ci, buf); want: the restatement's.  The sampled rows
    carry the round, every other row its input bits (the restatement copies
    them through), and the padding stays NaN."""
    for name, g, x in zip(("w", "ci", "buf"), got, want):
        if name == "buf" and not mom:
            continue
        gn = g.cpu().numpy()
        assert bits_equal(gn[:, :P], x), name
        assert np.isnan(gn[:, P:]).all(), name


@pytest.mark.parametrize("P,extra", GRID)
@pytest.mark.parametrize("mom,steps", MOM_STEPS)
@pytest.mark.parametrize("m", [5, 1, 6, 9])
def test_scaffold_round_vs_restatement(P, extra, mom, steps, m, gpu):
    """Groups of three agents in flight: m = 6 / 9 end on a full group, 5 / 1
    on a partial one."""
    T, B, CI, th, c = inputs(P, P + 7 * steps + m)
    order, first = ORDER[:m], FIRST[:m]
    w_in = np.full((N, P), W0, np.float32)
    for global_lr, scale_w in SCALES:
        want = scaffold_ls_round_ref(w_in, B if mom else None, CI, T, th, c, order, first, LR, mom, steps, global_lr,
                                     scale_w, N)
        w, b, ci, t = (_mat(a, P + extra, gpu) for a in (w_in, B, CI, T))
        theta, cg = torch.as_tensor(th, device=gpu), torch.as_tensor(c, device=gpu)
        tot = torch.full((2,), float("nan"), dtype=torch.float64, device=gpu)
        th1, c1 = ops.scaffold_ls_round(w, ci, t, theta, cg, agents=torch.as_tensor(order, device=gpu),
                                        first=torch.as_tensor(first, device=gpu), buf=b if mom else None, lr=LR,
                                        momentum=mom, local_steps=steps, global_lr=global_lr, scale_w=scale_w,
                                        resid_total=tot, P=P)
        torch.cuda.synchronize()
        _check_state((w, ci, b), (want[0], want[2], want[1]), P, mom)
        assert bits_equal(th1.cpu().numpy(), want[3])
        assert bits_equal(c1.cpu().numpy(), want[4])
        assert bits_equal(theta.cpu().numpy(), th) and bits_equal(cg.cpu().numpy(), c)  # out of place: inputs kept
        np.testing.assert_allclose(tot.cpu().numpy(), want[5], rtol=1e-12)


def test_1024_lane_strips(gpu):
    """P = 4 * 1024 * CUs + 4: the first width whose f4 columns fill one
    1024-lane strip per CU, plus one strip that is all dead lanes but one."""
    n_cu = torch.cuda.get_device_properties(gpu).multi_processor_count
    P, n, m, steps, mom = 4 * 1024 * n_cu + 4, 4, 4, 2, 0.5
    T, B, CI, th, c = inputs(P, 5, n=n)
    order, first = np.array([2, 0, 3, 1], np.int32), np.array([0, 1, 0, 0], np.int32)
    w_in = np.full((n, P), W0, np.float32)
    want = scaffold_ls_round_ref(w_in, B, CI, T, th, c, order, first, LR, mom, steps)
    w, b, ci, t = (_mat(a, P, gpu) for a in (w_in, B, CI, T))
    tot = torch.full((2,), float("nan"), dtype=torch.float64, device=gpu)
    th1, c1 = ops.scaffold_ls_round(w, ci, t, torch.as_tensor(th, device=gpu), torch.as_tensor(c, device=gpu),
                                    agents=torch.as_tensor(order, device=gpu), first=torch.as_tensor(first, device=gpu),
                                    buf=b, lr=LR, momentum=mom, local_steps=steps, resid_total=tot, P=P)
    torch.cuda.synchronize()
    _check_state((w, ci, b), (want[0], want[2], want[1]), P, mom)
    assert bits_equal(th1.cpu().numpy(), want[3]) and bits_equal(c1.cpu().numpy(), want[4])
    np.testing.assert_allclose(tot.cpu().numpy(), want[5], rtol=1e-12)


@pytest.mark.parametrize("P", [2051, 4096])
def test_in_place_outputs(P, gpu):
    """theta_out = theta and c_out = c: the out-of-place bits."""
    T, B, CI, th, c = inputs(P, 3)
    agents = torch.as_tensor(ORDER[:5], device=gpu)
    kw = dict(agents=agents, lr=LR, momentum=0.5, local_steps=2, global_lr=0.5, P=P)

    def state():
        return [torch.as_tensor(a, device=gpu) for a in (np.zeros((N, P), np.float32), CI, T, B, th, c)]
    w1, ci1, t1, b1, th1, c1 = state()
    ref = ops.scaffold_ls_round(w1, ci1, t1, th1, c1, buf=b1, **kw)
    w2, ci2, t2, b2, th2, c2 = state()
    out = ops.scaffold_ls_round(w2, ci2, t2, th2, c2, buf=b2, theta_out=th2, c_out=c2, **kw)
    torch.cuda.synchronize()
    assert out[0] is th2 and out[1] is c2
    for x, y in ((th2, ref[0]), (c2, ref[1]), (w2, w1), (ci2, ci1), (b2, b1)):
        assert bits_equal(x.cpu().numpy(), y.cpu().numpy())
    assert not bits_equal(th2.cpu().numpy(), th)


def test_problem_class_matches_its_cpu_replay(gpu):
    kw = dict(lr=0.1, momentum=0.5, local_steps=3, frac=0.5, global_lr=1.0, seed=9)
    a = SeparableScaffold(11, 70, device=gpu, **kw)
    b = SeparableScaffold(11, 70, device="cpu", round_fn=cpu_scaffold_round, **kw)
    b.target[:, :70] = a.target[:, :70].cpu()  # one problem on both devices (the generators differ)
    b.theta[:70] = a.theta[:70].cpu()
    for _ in range(5):
        a.round()
        b.round()
    torch.cuda.synchronize()
    for x, y in ((a.theta[:70], b.theta[:70]), (a.c[:70], b.c[:70]), (a.w[:, :70], b.w[:, :70]),
                 (a.ci[:, :70], b.ci[:, :70]), (a.mom[:, :70], b.mom[:, :70])):
        assert bits_equal(x.cpu().numpy(), y.numpy())
    assert (a.mom_started == b.mom_started).all() and a.mom_started.any()
    assert len(a.history) == 5
    for ha, hb in zip(a.history, b.history):
        assert ha["round"] == hb["round"]
        np.testing.assert_allclose([ha["primal_resid_sq"], ha["dual_sq"]], [hb["primal_resid_sq"], hb["dual_sq"]],
                                   rtol=1e-12)


def test_round_captures_into_a_graph(gpu):
    """One in-place round (theta_out = theta, c_out = c) run once eagerly,
    then captured with torch.cuda.graph as one linear chain (the host check of
    the ids is not made while capturing) and replayed twice: the state after
    three eager rounds."""
    P, m = 5003, 5
    T, B, CI, th, c = inputs(P, 12)
    agents = torch.as_tensor(ORDER[:m], device=gpu)
    first = torch.as_tensor([0, 1, 0, 0, 1], dtype=torch.int32, device=gpu)
    t = torch.as_tensor(T, device=gpu)

    def state():
        return [torch.as_tensor(a, device=gpu) for a in (np.zeros((N, P), np.float32), CI, B, th, c)] + \
            [torch.zeros(2, dtype=torch.float64, device=gpu)]

    def call(w, ci, b, theta, cg, tot):
        ops.scaffold_ls_round(w, ci, t, theta, cg, agents=agents, first=first, buf=b, lr=LR, momentum=0.5,
                              local_steps=3, theta_out=theta, c_out=cg, resid_total=tot, P=P)
    eager = state()
    for _ in range(3):
        call(*eager)
    got = state()
    call(*got)  # round 1, eager; also sizes the shared workspace before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call(*got)
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    for x, y in zip(got[:5], eager[:5]):
        assert bits_equal(x.cpu().numpy(), y.cpu().numpy())
    assert np.array_equal(got[5].cpu().numpy(), eager[5].cpu().numpy())


@pytest.fixture
def rec(monkeypatch):
    r = Recorder()
    monkeypatch.setattr(ops._native, "call", r)
    return r


def test_op_rules_on_device_tensors_without_a_launch(rec, gpu):
    w, th, c = torch.zeros(4, 8, device=gpu), torch.zeros(8, device=gpu), torch.zeros(8, device=gpu)
    ci, t, b = w.clone(), w.clone(), w.clone()
    with pytest.raises(ValueError, match="agents must be distinct"):
        ops.scaffold_ls_round(w, ci, t, th, c, agents=torch.as_tensor([1, 1], dtype=torch.int32, device=gpu))
    with pytest.raises(ValueError, match="agents must be distinct"):
        ops.scaffold_ls_round(w, ci, t, th, c, agents=torch.as_tensor([4], dtype=torch.int32, device=gpu))
    for rows in (w, ci, t, b):
        with pytest.raises(ValueError, match="theta_out aliases the rows"):
            ops.scaffold_ls_round(w, ci, t, th, c, buf=b, momentum=0.5, theta_out=rows[0])
        with pytest.raises(ValueError, match="c_out aliases the rows"):
            ops.scaffold_ls_round(w, ci, t, th, c, buf=b, momentum=0.5, c_out=rows[0])
    with pytest.raises(ValueError, match="theta_out and c_out alias"):
        ops.scaffold_ls_round(w, ci, t, th, c, theta_out=th, c_out=th)
    with pytest.raises(ValueError, match="local_steps must be >= 1"):
        ops.scaffold_ls_round(w, ci, t, th, c, local_steps=0)
    with pytest.raises(ValueError, match="expected a contiguous float32 vector"):
        ops.scaffold_ls_round(w, ci, t, th, c[:7])
    assert rec.calls == []
    out = ops.scaffold_ls_round(w, ci, t, th, c, lr=0.1, local_steps=10, theta_out=th, c_out=c, n_total=64)
    assert out[0] is th and out[1] is c
    (name, args), = rec.calls
    assert name == "dol_scaffold_ls_round_f32" and len(args) == 26
    assert args[8] == args[19] == th.data_ptr() and args[9] == args[21] == c.data_ptr()
    assert args[2] is None and args[3] == 0  # no momentum: no buf
    assert args[12:14] == (4, 8) and args[16] == 10 and args[17] == 1.0 / (10 * 0.1)
    assert args[20] == 4.0 and args[22] == 64.0  # scale_w = m, scale_c = n_total
    assert args[23] is None and args[24] is None
