"""The fp64 reference of the fused MLP step (oracle/mlp_ref.py), checked on
the CPU for every shape x variant the GPU tests use (tests/test_mlp_matrix_gpu.py,
the bit-identity children's pinned member in tests/test_mlp_gpu.py), with the
same input generator:

1. it agrees with one fp64 nn.Sequential per agent driven the reference's way
   (autograd backward, p.grad += alpha + rho (p - theta) as DEC/clients.py:101-139,
   torch.optim.SGD with momentum) over three steps, to fp64 round-off;
2. run in fp32 it stays inside the step's stated tolerances, so a correct fp32
   kernel passes on these inputs;
3. every applicable deliberate error moves some checked output by at least
   ten times the tolerance, so a wrong kernel fails on them.

Checked outputs are the ones the GPU test compares: the loss, x and (with
momentum) mom after every step, grad where it is written."""
import functools

import pytest
import torch

from oracle import mlp_ref as R

# fp64 round-off: rtol 1e-12; the absolute floor is for sums that cancel
# (K <= 784 terms of magnitude <= ~1 at 1.1e-16 each)
FP64_TOL = dict(rtol=1e-12, atol=1e-13)
MARGIN = 10.0

# (id, (n, B, d, h, c), kind, momentum, write_grad, generator, lr, steps, checked steps)
CASES = []
for _s in R.MATRIX_SHAPES:
    for _k, _m, _wg in R.MATRIX_VARIANTS:
        CASES.append((_s, _k, _m, _wg, "make", R.LR, 2, (0, 1)))
CASES.append((R.EDGE_SHAPE, "admm", R.MU, True, "make", R.LR, 2, (0, 1)))
CASES.append(((1027,) + R.SMALL_ROWS, "plain", R.MU, False, "make", R.LR, 2, (0, 1)))
for _k in R.KINDS:
    for _m in (0.0, R.MU):  # the children write grad and are compared on their last step only
        CASES.append((R.CHILD_PIN_SHAPE, _k, _m, True, "child", R.CHILD_LR, R.CHILD_STEPS, (R.CHILD_STEPS - 1,)))
IDS = ["-".join(map(str, s)) + f"-{k}-mom{m}-wg{int(wg)}-{gen}" for s, k, m, wg, gen, *_ in CASES]


@functools.lru_cache(maxsize=None)
def _inputs(shape, gen, steps):
    return R.child_inputs(*shape) if gen == "child" else R.make_inputs(*shape, steps=steps)


@functools.lru_cache(maxsize=None)
def _ref(shape, kind, momentum, gen, lr, steps):
    return R.run_steps(_inputs(shape, gen, steps), *shape[2:], kind, momentum, lr=lr, steps=steps)


def _worst(got, want, momentum, write_grad, checked):
    """The largest tolerance ratio over the outputs the GPU test compares."""
    w = 0.0
    for s in checked:
        (l1, g1, b1, w1), (l0, g0, b0, w0) = got[s], want[s]
        w = max(w, R.tol_ratio(l1, l0, **R.LOSS_TOL), R.tol_ratio(w1, w0, **R.TOL))
        if write_grad:
            w = max(w, R.tol_ratio(g1, g0, **R.TOL))
        if momentum:
            w = max(w, R.tol_ratio(b1, b0, **R.TOL))
    return w


@pytest.mark.parametrize("shape,kind,momentum,gen,lr",
                         sorted({(s, k, m, gen, lr) for s, k, m, _, gen, lr, _, _ in CASES}, key=str))
def test_ref_matches_per_agent_modules_fp64(shape, kind, momentum, gen, lr):
    n, B, d, h, c = shape
    inp = _inputs(shape, gen, 3) if gen == "child" else R.make_inputs(*shape, steps=3)
    ref = R.run_steps(inp, d, h, c, kind, momentum, lr=lr, steps=3)
    o1, o2, o3 = h * d, h * d + h, h * d + h + c * h
    split = lambda v: (v[:o1].view(h, d), v[o1:o2], v[o2:o3].view(c, h), v[o3:])  # noqa: E731
    agents = range(n) if n <= 32 else sorted({*range(0, n, 64), 1, 7, 8, n - 2, n - 1})
    for i in agents:
        m = torch.nn.Sequential(torch.nn.Linear(d, h), torch.nn.ReLU(), torch.nn.Linear(h, c)).double()
        with torch.no_grad():
            for p, v in zip(m.parameters(), split(inp.W[i].double())):
                p.copy_(v)
        opt = torch.optim.SGD(m.parameters(), lr=lr, momentum=momentum)
        theta, alpha = split(inp.theta.double()), split(inp.alpha[i].double())
        for s in range(3):
            m.zero_grad()
            opt.zero_grad()
            loss = torch.nn.functional.cross_entropy(m(inp.X[s][i].double()), inp.y[s][i])
            loss.backward()
            pre = [p.detach().clone() for p in m.parameters()]
            for j, p in enumerate(m.parameters()):
                if kind == "prox":
                    p.grad = p.grad + R.RHO * (pre[j] - theta[j])
                elif kind == "admm":
                    p.grad = p.grad + (alpha[j] + R.RHO * (pre[j] - theta[j]))
            g = torch.cat([p.grad.reshape(-1) for p in m.parameters()])
            opt.step()
            rl, rg, rb, rw = ref[s]
            torch.testing.assert_close(rl[i], loss.detach(), **FP64_TOL)
            torch.testing.assert_close(rg[i], g, **FP64_TOL)
            torch.testing.assert_close(rw[i], torch.cat([p.detach().reshape(-1) for p in m.parameters()]), **FP64_TOL)
            if momentum:
                buf = torch.cat([opt.state[p]["momentum_buffer"].reshape(-1) for p in m.parameters()])
                torch.testing.assert_close(rb[i], buf, **FP64_TOL)


@pytest.mark.parametrize("shape,kind,momentum,write_grad,gen,lr,steps,checked", CASES, ids=IDS)
def test_fp32_on_cpu_stays_inside_the_tolerances(shape, kind, momentum, write_grad, gen, lr, steps, checked):
    got = R.run_steps(_inputs(shape, gen, steps), *shape[2:], kind, momentum, lr=lr, steps=steps, dtype=torch.float32)
    worst = _worst(got, _ref(shape, kind, momentum, gen, lr, steps), momentum, write_grad, checked)
    assert worst <= 1.0, f"fp32 uses {worst:.3f} of the tolerance"


@pytest.mark.parametrize("shape,kind,momentum,write_grad,gen,lr,steps,checked", CASES, ids=IDS)
def test_every_mutation_leaves_the_tolerances_by_10x(shape, kind, momentum, write_grad, gen, lr, steps, checked):
    want = _ref(shape, kind, momentum, gen, lr, steps)
    inp = _inputs(shape, gen, steps)
    for mut in R.MUTATIONS:
        if not R.mutation_applies(mut, shape[4], kind, momentum):
            continue
        got = R.run_steps(inp, *shape[2:], kind, momentum, lr=lr, steps=steps, mutate=mut)
        worst = _worst(got, want, momentum, write_grad, checked)
        assert worst >= MARGIN, f"{mut}: moves the checked outputs by only {worst:.2f} x the tolerance"


def test_mutations_are_rejected_by_name_and_update_false_returns_raw_gradients():
    shape = R.EDGE_SHAPE
    inp = R.make_inputs(*shape)
    with pytest.raises(ValueError, match="unknown mutation"):
        R.mlp_step_ref(inp.W, inp.X[0], inp.y[0], *shape[2:], mutate="nope")
    _, g, _, W = R.mlp_step_ref(inp.W, inp.X[0], inp.y[0], *shape[2:], theta=inp.theta, rho=R.RHO, update=False)
    _, g0, _, _ = R.mlp_step_ref(inp.W, inp.X[0], inp.y[0], *shape[2:], lr=R.LR, update=True)
    assert torch.equal(g, g0) and torch.equal(W, inp.W.double())
