"""The fused MLP step's dispatch matrix (csrc/mlp_step.hip) against the fp64
reference of the whole step (oracle/mlp_ref.py): every update template
(plain / prox / ADMM x SGD / first momentum step / momentum x grad written or
not) at the shapes where mlp_fwd_kernel and mlp_dw1_kernel take another branch,
the ABI edges of dol_mlp_step_f32 (strided X, strided labels, no loss,
rows= slices), and the launch geometry at and above the forward's stagger
threshold (4 n_cu agents), where config 5 runs.

Tolerances: oracle/mlp_ref.py (LOSS_TOL, TOL), stated there once;
tests/test_mlp_ref_host.py shows on the CPU that fp32 stays inside them on
these inputs and that each deliberate error leaves them tenfold.

Which test reaches which path of mlp_step.hip:
  launch above 16 agents, a.stagger, dW1's reversed XCD groups with a ragged
    last one            test_small_rows_every_agent_above_the_stagger_threshold,
                        test_config5_launch_..., test_step_matrix_matches_fp64[13-7-20-32-5 / 17-1-32-32-1]
  KS = 32 with UPD >= 1 test_step_matrix_matches_fp64[3-33-100-96-17 / 2-64-36-64-3 / 2-64-40-256-32]
  TH / AL x mode 0 / 1 / 2 x write_grad
                        test_step_matrix_matches_fp64[*-prox-* / *-admm-*]
  w2_in_regs == false under an update
                        test_step_matrix_matches_fp64[2-64-40-256-32 / 2-8-4-224-10]
  kThreads % h != 0     test_step_matrix_matches_fp64[3-33-100-96-17 / 2-8-4-224-*]
  B h > 16 kThreads     test_step_matrix_matches_fp64[2-64-40-256-32]
  mode 1 ignores mom    test_step_matrix_matches_fp64[*-0.5-*] (mom starts as NaN)
  DOL_MLP_FWD_STAGGER "0" / mode 2
                        test_small_rows_every_agent_above_the_stagger_threshold
  DOL_MLP_F1_KEEP=0, DOL_MLP_DW1_REVERSE=0
                        test_mlp_gpu.py::test_step_paths_bit_identical,
                        pinned by test_mlp_gpu.py::test_base_step_child_matches_fp64
  ldx_row > d, padded agent stride / ldy_agent > B / loss = NULL / rows=
                        test_padded_x_rows_and_agent_stride, test_labels_as_a_column_view,
                        test_step_without_a_loss_buffer, test_rows_slice_steps_only_its_agents,
                        the two launch-geometry tests (slices of 8 of >= 1024 agents)"""
import functools

import pytest
import torch

from dolhip import ops
from dolhip.bank import AgentBank
from dolhip.mlp import BatchedMLP, mlp_layout
from oracle import mlp_ref as R

pytestmark = pytest.mark.gpu

PAD = 12345.0    # row padding [:, P:] of every bank buffer
KEEP = -777.25   # buffers the step must not write


@functools.lru_cache(maxsize=None)
def _inputs(shape):
    return R.make_inputs(*shape)


@functools.lru_cache(maxsize=None)
def _ref(shape, kind, momentum):
    return R.run_steps(_inputs(shape), *shape[2:], kind, momentum)


def _bank(shape, gpu, inp, kind="admm", mom_fill=float("nan"), grad_fill=KEEP):
    """A bank holding inp.W (and inp.alpha), every buffer's padding = PAD, the
    momentum rows = mom_fill (NaN: a first step must not read them)."""
    n, _, d, h, c = shape
    bank = AgentBank(n, mlp_layout(d, h, c), gpu)
    P = bank.P
    for name, rows in (("x", inp.W), ("mom", None), ("grad", None), ("alpha", inp.alpha)):
        t = bank.buffer(name)
        t.fill_(PAD)
        if rows is not None:
            t[:, :P] = rows.to(gpu)
    bank.rows("mom").fill_(mom_fill)
    bank.rows("grad").fill_(grad_fill)
    if kind != "admm":
        bank.rows("alpha").fill_(KEEP)
    return bank, BatchedMLP(bank, d, h, c)


def _check_padding(bank):
    for name in ("x", "mom", "grad", "alpha"):
        assert torch.all(bank.buffer(name)[:, bank.P:] == PAD), name


def _close(got, want, tol, what):
    torch.testing.assert_close(got.double().cpu(), want, msg=lambda m: f"{what}: {m}", **tol)


@pytest.mark.parametrize("kind,momentum,write_grad", R.MATRIX_VARIANTS)
@pytest.mark.parametrize("shape", R.MATRIX_SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_step_matrix_matches_fp64(shape, kind, momentum, write_grad, gpu):
    """Two consecutive steps (first_step, then not) of every agent against
    mlp_step_ref: loss, grad (when written), mom, x after each.  mom starts as
    NaN (a first momentum step that read it would show), grad keeps a
    sentinel when it is not written, theta / alpha / X / y are read-only and
    the row padding of every buffer is untouched."""
    n, B, d, h, c = shape
    inp = _inputs(shape)
    ref = _ref(shape, kind, momentum)
    bank, mlp = _bank(shape, gpu, inp, kind)
    theta = inp.theta.to(gpu) if kind != "plain" else None
    alpha0 = bank.buffer("alpha").clone()
    for s in range(2):
        X, y = inp.X[s].to(gpu), inp.y[s].to(gpu)
        loss = mlp.step(X, y, lr=R.LR, momentum=momentum, first_step=(s == 0), theta=theta,
                        rho=R.RHO if theta is not None else 0.0, admm=(kind == "admm"), write_grad=write_grad)
        torch.cuda.synchronize()
        rl, rg, rb, rw = ref[s]
        _close(loss, rl, R.LOSS_TOL, f"loss, step {s}")
        _close(bank.rows(), rw, R.TOL, f"x, step {s}")
        if write_grad:
            _close(bank.rows("grad"), rg, R.TOL, f"grad, step {s}")
        else:
            assert torch.all(bank.rows("grad") == KEEP), "grad written without write_grad"
        if momentum:
            _close(bank.rows("mom"), rb, R.TOL, f"mom, step {s}")
        else:
            assert torch.all(torch.isnan(bank.rows("mom"))), "mom written without momentum"
        assert torch.equal(X.cpu(), inp.X[s]) and torch.equal(y.cpu(), inp.y[s])
        assert torch.equal(bank.buffer("alpha"), alpha0)
        if theta is not None:
            assert torch.equal(theta.cpu(), inp.theta)
        _check_padding(bank)


# ---------------------------------------------------------------- ABI edges of dol_mlp_step_f32
def _edge_call(gpu, X=None, y=None, loss="new"):
    """One ADMM momentum step (not the first) at EDGE_SHAPE through ops.mlp_step,
    from inp.mom; returns (bank, loss)."""
    shape = R.EDGE_SHAPE
    n, B, d, h, c = shape
    inp = _inputs(shape)
    bank, _ = _bank(shape, gpu, inp, "admm")
    bank.rows("mom").copy_(inp.mom.to(gpu))
    if loss == "new":
        loss = torch.full((n,), KEEP, device=gpu)
    ops.mlp_step(bank.buffer("x"), inp.X[0].to(gpu) if X is None else X, inp.y[0].to(gpu) if y is None else y,
                 d, h, c, grad=bank.buffer("grad"), mom=bank.buffer("mom"), theta=inp.theta.to(gpu),
                 alpha=bank.buffer("alpha"), loss=loss, lr=R.LR, momentum=R.MU, rho=R.RHO, first_step=False,
                 update=True)
    torch.cuda.synchronize()
    _check_padding(bank)
    return bank, loss


@pytest.fixture(scope="module")
def edge_plain(gpu):
    """The contiguous call, checked against fp64 once; the edge calls below
    must reproduce its bits."""
    shape = R.EDGE_SHAPE
    inp = _inputs(shape)
    bank, loss = _edge_call(gpu)
    rl, rg, rb, rw = R.mlp_step_ref(inp.W, inp.X[0], inp.y[0], *shape[2:], theta=inp.theta, alpha=inp.alpha,
                                    mom=inp.mom, lr=R.LR, momentum=R.MU, rho=R.RHO, first_step=False, update=True)
    _close(loss, rl, R.LOSS_TOL, "loss")
    for name, want in (("x", rw), ("grad", rg), ("mom", rb)):
        _close(bank.rows(name), want, R.TOL, name)
    return {k: bank.rows(k).clone() for k in ("x", "grad", "mom")}, loss.clone()


def _same_bits(bank, loss, edge_plain):
    rows, l0 = edge_plain
    for k, t in rows.items():
        assert torch.equal(bank.rows(k), t), k
    if loss is not None:
        assert torch.equal(loss, l0)


def test_padded_x_rows_and_agent_stride(gpu, edge_plain):
    """X as a view with stride(1) = d + 12 and stride(0) = B (d + 12) + 8; the
    gaps hold NaN, so a read past a row's d floats shows."""
    n, B, d, h, c = R.EDGE_SHAPE
    lds, lda = d + 12, B * (d + 12) + 8
    base = torch.full((n * lda,), float("nan"), device=gpu)
    X = base.as_strided((n, B, d), (lda, lds, 1))
    X.copy_(_inputs(R.EDGE_SHAPE).X[0].to(gpu))
    before = base.clone()
    bank, loss = _edge_call(gpu, X=X)
    _same_bits(bank, loss, edge_plain)
    assert torch.equal(torch.nan_to_num(base, nan=PAD), torch.nan_to_num(before, nan=PAD))


def test_labels_as_a_column_view(gpu, edge_plain):
    """y as columns [1, B + 1) of an [n, B + 3] tensor whose other columns hold
    an invalid label (a read of them gives a NaN loss)."""
    n, B, d, h, c = R.EDGE_SHAPE
    Y = torch.full((n, B + 3), c + 7, dtype=torch.int64, device=gpu)
    y = Y[:, 1:B + 1]
    y.copy_(_inputs(R.EDGE_SHAPE).y[0].to(gpu))
    assert y.stride(0) == B + 3
    bank, loss = _edge_call(gpu, y=y)
    _same_bits(bank, loss, edge_plain)


def test_step_without_a_loss_buffer(gpu, edge_plain):
    bank, loss = _edge_call(gpu, loss=None)
    assert loss is None
    _same_bits(bank, None, edge_plain)


def test_rows_slice_steps_only_its_agents(gpu):
    """BatchedMLP.step(rows=slice(2, 4)): the other agents' rows of x, mom and
    loss stay bit-unchanged; the stepped rows equal the full launch's."""
    shape = R.EDGE_SHAPE
    n = shape[0]
    inp = _inputs(shape)
    out = []
    for rows in (None, slice(2, 4)):
        bank, mlp = _bank(shape, gpu, inp, "admm", mom_fill=KEEP)
        loss = torch.full((n,), KEEP, device=gpu)
        got = mlp.step(inp.X[0].to(gpu), inp.y[0].to(gpu), lr=R.LR, momentum=R.MU, first_step=True,
                       theta=inp.theta.to(gpu), rho=R.RHO, admm=True, rows=rows, loss=loss)
        torch.cuda.synchronize()
        assert got is loss
        _check_padding(bank)
        out.append((bank.rows().clone(), bank.rows("mom").clone(), loss))
    (xf, mf, lf), (xs, ms, ls) = out
    for full, part in ((xf, xs), (mf, ms), (lf, ls)):
        assert torch.equal(part[2:4], full[2:4])
    others = [0, 1, 4]
    assert torch.equal(xs[others], inp.W.to(gpu)[others])
    assert torch.all(ms[others] == KEEP) and torch.all(ls[others] == KEEP)
    assert not torch.equal(xf[others], xs[others])  # the full launch did step them


# ---------------------------------------------------------------- launch geometry at >= 4 n_cu agents
def _n_cu(gpu):
    return torch.cuda.get_device_properties(gpu).multi_processor_count


def _run_bank(mlp, bank, W, Xs, ys, momentum, lr, chunk=None):
    """Two steps from W (momentum rows NaN first) in one launch per step, or in
    rows= slices of `chunk` agents; returns clones of (x, mom, losses)."""
    bank.rows().copy_(W)
    bank.rows("mom").fill_(float("nan"))
    n, losses = bank.n, []
    for s, (X, y) in enumerate(zip(Xs, ys)):
        loss = torch.full((n,), KEEP, device=W.device)
        if chunk is None:
            mlp.step(X, y, lr=lr, momentum=momentum, first_step=(s == 0), loss=loss)
        else:
            for a in range(0, n, chunk):
                mlp.step(X, y, lr=lr, momentum=momentum, first_step=(s == 0), rows=slice(a, a + chunk), loss=loss)
        losses.append(loss)
    torch.cuda.synchronize()
    return bank.rows().clone(), bank.rows("mom").clone(), torch.stack(losses)


def test_small_rows_every_agent_above_the_stagger_threshold(gpu, monkeypatch):
    """n = 4 n_cu + 3 agents (the forward staggers, dW1 walks ragged XCD groups
    last to first): (a) every agent against fp64; (b) one launch = slices of 8
    agents, bit for bit; (c) the same bits with the stagger off and in mode 2."""
    monkeypatch.delenv("DOL_MLP_FWD_STAGGER", raising=False)
    n_cu = _n_cu(gpu)
    n = 4 * n_cu + 3
    assert n >= 4 * n_cu
    shape = (n,) + R.SMALL_ROWS
    B, d, h, c = R.SMALL_ROWS
    inp = R.make_inputs(*shape)
    ref = R.run_steps(inp, d, h, c, "plain", R.MU)
    bank = AgentBank(n, mlp_layout(d, h, c), gpu)
    mlp = BatchedMLP(bank, d, h, c)
    W, Xs, ys = inp.W.to(gpu), [x.to(gpu) for x in inp.X], [y.to(gpu) for y in inp.y]
    x1, m1, l1 = _run_bank(mlp, bank, W, Xs, ys, R.MU, R.LR)
    _close(x1, ref[1][3], R.TOL, "x")
    _close(m1, ref[1][2], R.TOL, "mom")
    for s in range(2):
        _close(l1[s], ref[s][0], R.LOSS_TOL, f"loss, step {s}")
    x2, m2, l2 = _run_bank(mlp, bank, W, Xs, ys, R.MU, R.LR, chunk=8)
    assert torch.equal(x1, x2) and torch.equal(m1, m2) and torch.equal(l1, l2), "one launch vs slices of 8"
    for mode in ("0", "6,2"):
        monkeypatch.setenv("DOL_MLP_FWD_STAGGER", mode)
        x3, m3, l3 = _run_bank(mlp, bank, W, Xs, ys, R.MU, R.LR)
        assert torch.equal(x1, x3) and torch.equal(m1, m3) and torch.equal(l1, l3), f"DOL_MLP_FWD_STAGGER={mode}"


def test_config5_launch_bit_identical_to_slices_and_sampled_against_fp64(gpu, monkeypatch):
    """Config 5's own launch (>= 1024 agents of 784-128-10, B = 32, momentum
    0.5, default environment), two steps: (a) the whole bank (x, mom, loss) is
    bit-identical to the same bank stepped in 8-agent slices; (b) sampled
    agents -- around the stagger's block range [n_cu, 2 n_cu), the first and
    last agent of the first and last XCD group, n - 1 -- against fp64."""
    monkeypatch.delenv("DOL_MLP_FWD_STAGGER", raising=False)
    n_cu = _n_cu(gpu)
    n = max(1024, 4 * n_cu)
    assert n >= 4 * n_cu
    B, d, h, c = 32, 784, 128, 10
    inp = R.make_inputs(n, B, d, h, c, device=gpu)
    bank = AgentBank(n, mlp_layout(d, h, c), gpu)
    mlp = BatchedMLP(bank, d, h, c)
    x1, m1, l1 = _run_bank(mlp, bank, inp.W, inp.X, inp.y, R.MU, R.LR)
    x2, m2, l2 = _run_bank(mlp, bank, inp.W, inp.X, inp.y, R.MU, R.LR, chunk=8)
    assert torch.equal(x1, x2) and torch.equal(m1, m2) and torch.equal(l1, l2), "one launch vs slices of 8"
    last_group = 8 * ((n - 1) // 8)
    sample = sorted({0, 7, last_group, n - 1, n_cu - 1, n_cu, n_cu + 1, 2 * n_cu - 1, 2 * n_cu, 2 * n_cu + 1,
                     3 * n_cu, 4 * n_cu - 1, 8, n // 2 - 1, n // 2, n // 3, n - 9, n - 8,
                     n // 7, n // 5, 3 * n // 5 + 1, 7 * n // 8 + 5})
    assert len(sample) >= 16
    idx = torch.tensor(sample, device=gpu)
    host = R.MlpInputs(inp.W[idx].cpu(), inp.theta.cpu(), inp.alpha[idx].cpu(), inp.mom[idx].cpu(),
                       [x[idx].cpu() for x in inp.X], [y[idx].cpu() for y in inp.y])
    ref = R.run_steps(host, d, h, c, "plain", R.MU)
    _close(x1[idx], ref[1][3], R.TOL, "x")
    _close(m1[idx], ref[1][2], R.TOL, "mom")
    for s in range(2):
        _close(l1[s][idx], ref[s][0], R.LOSS_TOL, f"loss, step {s}")
