"""Fused per-agent MLP local step (dol_mlp_step_f32, csrc/mlp_step.hip) vs one
nn.Module per agent — the reference's per-agent loop structure
(DIST/clients.py:34-59; prox/ADMM terms DEC/clients.py:101-139).

The reference checks are torch fp64 on the CPU.  The kernel's GEMMs are fp32
fma chains over K = d (forward) and K = B (dW1), so its results carry fp32
rounding of ~K ulps on dot products of O(1) terms.  Tolerance, stated once:
loss rtol 1e-5 / atol 1e-6, gradients and parameters rtol 1e-4 / atol 1e-5
(the observed max deviation is ~1e-6 at 784-128-10)."""
import numpy as np
import pytest
import torch

from dolhip import ops
from dolhip.bank import AgentBank
from dolhip.mlp import BatchedMLP, mlp_layout
from oracle.mlp_ref import LOSS_TOL, TOL  # the statement above as numbers, shared with test_mlp_matrix_gpu.py

pytestmark = pytest.mark.gpu

SHAPES = [(3, 7, 20, 32, 5), (8, 32, 784, 128, 10), (5, 64, 36, 64, 3), (2, 1, 4, 256, 32), (4, 33, 100, 96, 17),
          (6, 32, 12, 160, 2)]


def _modules(n, d, h, c, seed):
    torch.manual_seed(seed)
    return [torch.nn.Sequential(torch.nn.Linear(d, h), torch.nn.ReLU(), torch.nn.Linear(h, c)) for _ in range(n)]


def _flat(m, grad=False):
    return torch.cat([(p.grad if grad else p.detach()).reshape(-1) for p in m.parameters()])


def _setup(n, B, d, h, c, gpu, seed=0):
    bank = AgentBank(n, mlp_layout(d, h, c), gpu)
    mlp = BatchedMLP(bank, d, h, c)
    mods = _modules(n, d, h, c, seed)
    for i, m in enumerate(mods):
        bank.load_module(i, m)
    g = torch.Generator().manual_seed(seed + 1)
    X = torch.randn(n, B, d, generator=g)
    y = torch.randint(0, c, (n, B), generator=g)
    return bank, mlp, mods, X, y


def _ref_grad(m, X, y):
    m64 = [p.detach().double().clone().requires_grad_(True) for p in m.parameters()]
    W1, b1, W2, b2 = m64
    z = torch.relu(X.double() @ W1.T + b1) @ W2.T + b2
    loss = torch.nn.functional.cross_entropy(z, y)
    loss.backward()
    return loss.detach(), torch.cat([p.grad.reshape(-1) for p in m64])


@pytest.mark.parametrize("n,B,d,h,c", SHAPES)
def test_fused_forward_backward_matches_per_agent_modules(n, B, d, h, c, gpu):
    bank, mlp, mods, X, y = _setup(n, B, d, h, c, gpu)
    loss = mlp.forward_backward(X.to(gpu), y.to(gpu))
    torch.cuda.synchronize()
    for i, m in enumerate(mods):
        li, gi = _ref_grad(m, X[i], y[i])
        torch.testing.assert_close(loss[i].double().cpu(), li, **LOSS_TOL)
        torch.testing.assert_close(bank.rows("grad")[i].double().cpu(), gi, **TOL)


def test_fused_matches_bmm_formulation(gpu):
    n, B, d, h, c = 16, 32, 784, 128, 10
    bank, mlp, _, X, y = _setup(n, B, d, h, c, gpu, seed=3)
    Xd, yd = X.to(gpu), y.to(gpu)
    l1 = mlp.forward_backward(Xd, yd)
    g1 = bank.rows("grad").clone()
    l2 = mlp.forward_backward_torch(Xd, yd)
    torch.testing.assert_close(l1, l2, **LOSS_TOL)
    torch.testing.assert_close(g1, bank.rows("grad"), **TOL)


@pytest.mark.parametrize("momentum", [0.0, 0.5])
def test_fused_sgd_steps_match_torch_sgd(momentum, gpu):
    n, B, d, h, c = 4, 16, 40, 64, 6
    bank, mlp, mods, _, _ = _setup(n, B, d, h, c, gpu, seed=1)
    mods = [m.double() for m in mods]
    opts = [torch.optim.SGD(m.parameters(), lr=0.1, momentum=momentum) for m in mods]
    g = torch.Generator().manual_seed(11)
    for step in range(3):
        X = torch.randn(n, B, d, generator=g)
        y = torch.randint(0, c, (n, B), generator=g)
        loss = mlp.step(X.to(gpu), y.to(gpu), lr=0.1, momentum=momentum, first_step=(step == 0))
        for i, (m, o) in enumerate(zip(mods, opts)):
            o.zero_grad()
            li = torch.nn.functional.cross_entropy(m(X[i].double()), y[i])
            li.backward()
            o.step()
            torch.testing.assert_close(loss[i].double().cpu(), li.detach(), **LOSS_TOL)
    for i, m in enumerate(mods):
        torch.testing.assert_close(bank.rows()[i].double().cpu(), _flat(m), **TOL)


@pytest.mark.parametrize("admm", [False, True])
def test_fused_prox_admm_step(admm, gpu):
    """FedProx (g += rho (w - theta)) / FedADMM (g += alpha + rho (w - theta)) then
    SGD with momentum, DEC/clients.py:101-115 / :125-139; g' written back to grad."""
    n, B, d, h, c = 3, 32, 64, 32, 4
    rho, lr, mu = 0.1, 0.05, 0.5
    bank, mlp, mods, X, y = _setup(n, B, d, h, c, gpu, seed=5)
    P = bank.P
    gen = torch.Generator().manual_seed(9)
    theta = torch.randn(P, generator=gen)
    alpha = torch.randn(n, P, generator=gen) if admm else torch.zeros(n, P)
    mom0 = torch.randn(n, P, generator=gen)
    bank.buffer("mom", zero=True)[:, :P] = mom0.to(gpu)
    if admm:
        bank.buffer("alpha", zero=True)[:, :P] = alpha.to(gpu)
    w0 = bank.rows().double().cpu().clone()
    mlp.step(X.to(gpu), y.to(gpu), lr=lr, momentum=mu, first_step=False, theta=theta.to(gpu), rho=rho, admm=admm,
             write_grad=True)
    torch.cuda.synchronize()
    for i, m in enumerate(mods):
        _, g = _ref_grad(m, X[i], y[i])
        t = rho * (w0[i] - theta.double())
        if admm:
            t = alpha[i].double() + t
        g2 = g + t
        buf = mom0[i].double() * mu + g2
        torch.testing.assert_close(bank.rows("grad")[i].double().cpu(), g2, **TOL)
        torch.testing.assert_close(bank.rows("mom")[i].double().cpu(), buf, **TOL)
        torch.testing.assert_close(bank.rows()[i].double().cpu(), w0[i] - lr * buf, **TOL)


def test_fused_step_leaves_padding_and_neighbours_untouched(gpu):
    """Only the P parameter floats of each row are written; the row padding and
    the X / label inputs are not."""
    n, B, d, h, c = 5, 8, 28, 32, 3
    bank, mlp, _, X, y = _setup(n, B, d, h, c, gpu, seed=7)
    x = bank.buffer("x")
    x[:, bank.P:] = 12345.0
    Xd, yd = X.to(gpu), y.to(gpu)
    mlp.step(Xd, yd, lr=0.1, momentum=0.0, first_step=True)
    torch.cuda.synchronize()
    assert torch.all(x[:, bank.P:] == 12345.0)
    assert torch.equal(Xd.cpu(), X) and torch.equal(yd.cpu(), y)


def test_out_of_range_label_gives_nan_loss(gpu):
    n, B, d, h, c = 2, 4, 8, 32, 3
    bank, mlp, _, X, y = _setup(n, B, d, h, c, gpu)
    y[1, 2] = c  # invalid for agent 1 only
    loss = mlp.forward_backward(X.to(gpu), y.to(gpu)).cpu()
    assert torch.isfinite(loss[0]) and torch.isnan(loss[1])


def test_rejects_unsupported_shapes(gpu):
    bank = AgentBank(2, mlp_layout(8, 48, 3), gpu)
    X = torch.zeros(2, 4, 8, device=gpu)
    y = torch.zeros(2, 4, dtype=torch.int64, device=gpu)
    with pytest.raises(ops.DolNativeError, match="multiple of 32"):
        ops.mlp_step(bank.buffer("x"), X, y, 8, 48, 3, grad=bank.buffer("grad"), update=False)


_FUSED_CHILD = r"""
import sys, torch
sys.path[:0] = sys.argv[1:3]
from dolhip.bank import AgentBank
from dolhip.mlp import BatchedMLP, mlp_layout
from oracle import mlp_ref as R
out = {}
for (n, B, d, h, c) in [(8, 32, 784, 128, 10), (3, 7, 100, 128, 5), (2, 32, 128, 128, 10), (5, 20, 800, 128, 3),
                        (4, 33, 100, 96, 17), (13, 7, 100, 128, 5), (3, 64, 36, 64, 3), (2, 8, 4, 224, 10)]:
    inp = R.child_inputs(n, B, d, h, c)
    for kind in R.KINDS:
        for mom in (0.0, 0.5):
            bank = AgentBank(n, mlp_layout(d, h, c), "cuda:0")
            bank.rows().copy_(inp.W)
            if mom:
                bank.rows("mom").copy_(inp.mom)  # the first step ignores it
            if kind == "admm":
                bank.rows("alpha").copy_(inp.alpha)
            theta = inp.theta.cuda() if kind != "plain" else None
            mlp = BatchedMLP(bank, d, h, c)
            for step in range(R.CHILD_STEPS):
                loss = mlp.step(inp.X[step].cuda(), inp.y[step].cuda(), lr=R.CHILD_LR, momentum=mom,
                                first_step=(step == 0), theta=theta, rho=R.RHO if theta is not None else 0.0,
                                admm=(kind == "admm"), write_grad=(step == R.CHILD_STEPS - 1))
            torch.cuda.synchronize()
            k = f"{n},{B},{d},{h},{c},{mom}" + ("" if kind == "plain" else "," + kind)
            out[k + ",x"] = bank.rows().cpu().clone()
            out[k + ",grad"] = bank.rows("grad").cpu().clone()
            out[k + ",loss"] = loss.cpu().clone()
            if mom:
                out[k + ",mom"] = bank.rows("mom").cpu().clone()
torch.save(out, sys.argv[3])
print("ok")
"""


_STEP_PATHS = {  # env of each alternative launch path (read once per process: run in children)
    "base": dict(DOL_MLP_DW1_REVERSE="1", DOL_MLP_F1_KEEP="1"),
    "dw1reverse0": dict(DOL_MLP_DW1_REVERSE="0"),
    "f1keep0": dict(DOL_MLP_F1_KEEP="0"),
}


def _run_step_child(root, tmp_path, name):
    import os
    import subprocess
    import sys
    f = str(tmp_path / f"{name}.pt")
    env = dict(os.environ, **_STEP_PATHS["base"])  # the base environment, overlaid with the path's own settings
    env.update(_STEP_PATHS[name])
    r = subprocess.run([sys.executable, "-c", _FUSED_CHILD, root,
                        os.path.join(root, "distributed-optimization-and-learning_amd"), f],
                       env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-2000:]
    return torch.load(f, weights_only=True)


def _repo_root():
    import os
    return os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def step_child(gpu, tmp_path_factory):
    """step_child(name): the result of path `name`'s child.  The default
    path's child runs once for every comparison below."""
    tmp, kept = tmp_path_factory.mktemp("mlp_step_paths"), {}

    def run(name):
        if name in kept:
            return kept[name]
        r = _run_step_child(_repo_root(), tmp, name)
        if name == "base":
            kept[name] = r
        return r
    return run


def test_base_step_child_matches_fp64(step_child):
    """The bit-identical family hangs on a checked member: the base child's
    plain, prox and ADMM results at (13, 7, 100, 128, 5) -- two XCD groups, the
    last one ragged -- against the fp64 reference of the whole step."""
    from oracle import mlp_ref as R
    shape = R.CHILD_PIN_SHAPE
    inp = R.child_inputs(*shape)
    got = step_child("base")
    for kind in R.KINDS:
        for mom in (0.0, 0.5):
            loss, g, buf, w = R.run_steps(inp, *shape[2:], kind, mom, lr=R.CHILD_LR, steps=R.CHILD_STEPS)[-1]
            k = ",".join(map(str, shape)) + f",{mom}" + ("" if kind == "plain" else "," + kind)
            torch.testing.assert_close(got[k + ",loss"].double(), loss, **LOSS_TOL)
            torch.testing.assert_close(got[k + ",x"].double(), w, **TOL)
            torch.testing.assert_close(got[k + ",grad"].double(), g, **TOL)
            if mom:
                torch.testing.assert_close(got[k + ",mom"].double(), buf, **TOL)


@pytest.mark.parametrize("path", [p for p in _STEP_PATHS if p != "base"])
def test_step_paths_bit_identical(path, step_child):
    """Each runtime switch of the step's launch gives the same parameters,
    momentum, gradients and losses as the default, bit for bit: F1's
    nontemporal staging (DOL_MLP_F1_KEEP=0) and dW1 walking the agents first
    to last (DOL_MLP_DW1_REVERSE=0).  Cases: d with and without a partial last
    chunk, B < 32, B > 32 (KS = 32), two XCD groups with a ragged last one,
    c h > 2048 (W2 staged from memory), plain / prox / ADMM with plain and
    momentum SGD, first steps and write_grad."""
    base = step_child("base")
    alt = step_child(path)
    assert base.keys() == alt.keys()
    for k, t in base.items():
        assert torch.equal(t, alt[k]), f"{k}: max |difference| {float((t - alt[k]).abs().max()):.3g}"
