"""fp64 reference of the fused per-agent MLP local step — TEST INFRASTRUCTURE.

One local iteration of N independent nn.Sequential(Linear(d, h), ReLU(),
Linear(h, c)) agents (DIST/clients.py:34-59) with the FedProx / FedADMM
gradient terms (DEC/clients.py:101-139) and torch.optim.SGD's momentum, in
plain torch on the CPU, vectorised over the agents with bmm.  Term order as in
dolhip/mlp.py and csrc/mlp_step.hip:

  g'  = g + (alpha + rho (w - theta))      (prox: without alpha; plain: g' = g)
  buf = g'                                 momentum == 0, or the first momentum step
  buf = mom * mu + g'                      later momentum steps
  w  -= lr * buf

The tolerances of the fused step and the input generator of its tests are
stated here, once; tests/test_mlp_ref_host.py shows on the CPU that a correct
fp32 implementation stays inside them on these inputs and that every
deliberate error (`mutate=`) leaves them by a factor of ten or more.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch

# The kernel's GEMMs are fp32 fma chains over K = d (forward) and K = B (dW1):
# ~K ulps on dot products of O(1) terms.
LOSS_TOL = dict(rtol=1e-5, atol=1e-6)
TOL = dict(rtol=1e-4, atol=1e-5)  # gradients, momentum, parameters

MUTATIONS = ("f1_drop_col", "f2_drop_hidden", "dh_drop_class", "dw1_drop_sample", "db1_drop_sample",
             "omit_rho", "omit_alpha", "mode1_old_mom", "mode2_no_mom")

KINDS = ("plain", "prox", "admm")
RHO, LR, MU = 0.1, 0.05, 0.5


def mutation_applies(name: str, c: int, kind: str, momentum: float) -> bool:
    """A mutation is inapplicable where it has nothing to change: with one
    class softmax is 1 and dZ2 = p - onehot is exactly zero, so the loss
    gradient vanishes identically and no GEMM error can show; the prox / dual
    / momentum terms need the variant that has them."""
    if name in ("f1_drop_col", "f2_drop_hidden", "dh_drop_class", "dw1_drop_sample", "db1_drop_sample"):
        return c > 1
    if name == "omit_rho":
        return kind != "plain"
    if name == "omit_alpha":
        return kind == "admm"
    if name == "mode1_old_mom":
        return momentum != 0.0
    if name == "mode2_no_mom":  # the carried momentum is g' of the step before: zero for plain SGD at c = 1
        return momentum != 0.0 and (c > 1 or kind != "plain")
    raise ValueError(name)


class MlpInputs(NamedTuple):
    W: torch.Tensor       # [n, P]
    theta: torch.Tensor   # [P]
    alpha: torch.Tensor   # [n, P]
    mom: torch.Tensor     # [n, P]
    X: list               # steps x [n, B, d]
    y: list               # steps x [n, B] int64


def mlp_P(d: int, h: int, c: int) -> int:
    return h * d + h + c * h + c


# Seeds other than 0, per shape.  (2, 64, 36, 64, 3): with seed 0 the last sample's dZ1 is
# small in both agents and dropping it from db1 moves x by only 8.6 x the tolerance
# when neither grad nor mom is written (tests/test_mlp_ref_host.py asks for 10 x).
SEEDS = {(2, 64, 36, 64, 3): 1}


def make_inputs(n: int, B: int, d: int, h: int, c: int, steps: int = 2, seed: Optional[int] = None,
                device="cpu") -> MlpInputs:
    """W, theta, alpha, mom ~ 0.05 randn, X ~ randn, labels uniform; fp32, from
    one seeded generator on `device` (the values are what the kernel reads; the
    reference converts them to fp64)."""
    if seed is None:
        seed = SEEDS.get((n, B, d, h, c), 0)
    g =torch.Generator(device=device).manual_seed(1000003 * seed + 7919 * n + 131 * B + 17 * d + 3 * h + c)
    P = mlp_P(d, h, c)
    r = lambda *s: torch.randn(*s, generator=g, device=device)  # noqa: E731
    W, theta, alpha, mom = 0.05 * r(n, P), 0.05 * r(P), 0.05 * r(n, P), 0.05 * r(n, P)
    X, y = [], []
    for _ in range(steps):  # step by step: a longer run starts with the shorter one's inputs
        X.append(r(n, B, d))
        y.append(torch.randint(0, c, (n, B), generator=g, device=device))
    return MlpInputs(W, theta, alpha, mom, X, y)


def mlp_step_ref(W, X, y, d: int, h: int, c: int, *, theta=None, alpha=None, mom=None, lr: float = 0.0,
                 momentum: float = 0.0, rho: float = 0.0, first_step: bool = False, update: bool = True,
                 mutate: Optional[str] = None, dtype=torch.float64):
    """(loss [n], g [n, P], buf [n, P], W_new [n, P]) of one step from W [n, P],
    X [n, B, d], y [n, B].  g is what the kernel's grad rows hold: g' under an
    update, the raw loss gradient with update=False (buf, W_new are then g, W).
    `mutate` names one deliberate error (MUTATIONS); `dtype` runs the same
    formulas in another precision."""
    if mutate is not None and mutate not in MUTATIONS:
        raise ValueError(f"unknown mutation {mutate!r}")
    W, X = W.to(dtype), X.to(dtype)
    n, B = X.shape[0], X.shape[1]
    o1, o2, o3, P = h * d, h * d + h, h * d + h + c * h, mlp_P(d, h, c)
    if W.shape != (n, P) or X.shape[2] != d or y.shape != (n, B):
        raise ValueError("W [n, P], X [n, B, d], y [n, B] expected")
    W1, b1, W2, b2 = W[:, :o1].reshape(n, h, d), W[:, o1:o2], W[:, o2:o3].reshape(n, c, h), W[:, o3:]
    kd = d - 1 if mutate == "f1_drop_col" else d
    kh = h - 1 if mutate == "f2_drop_hidden" else h
    kc = c - 1 if mutate == "dh_drop_class" else c
    kw = B - 1 if mutate == "dw1_drop_sample" else B
    kb = B - 1 if mutate == "db1_drop_sample" else B
    Z1 = torch.baddbmm(b1.unsqueeze(1), X[:, :, :kd], W1[:, :, :kd].transpose(1, 2))     # [n, B, h]
    H = torch.relu(Z1)
    Z2 = torch.baddbmm(b2.unsqueeze(1), H[:, :, :kh], W2[:, :, :kh].transpose(1, 2))      # [n, B, c]
    logp = torch.log_softmax(Z2, dim=2)
    yy = y.unsqueeze(2)
    loss = -logp.gather(2, yy).squeeze(2).mean(1)
    dZ2 = torch.exp(logp)
    dZ2.scatter_add_(2, yy, torch.full_like(logp[..., :1], -1.0))
    dZ2 = dZ2 / B
    gW2 = torch.bmm(dZ2.transpose(1, 2), H)                                                # [n, c, h]
    gb2 = dZ2.sum(1)
    dH = torch.bmm(dZ2[:, :, :kc], W2[:, :kc, :])                                          # [n, B, h]
    dZ1 = dH * (Z1 > 0)
    gW1 = torch.bmm(dZ1[:, :kw].transpose(1, 2), X[:, :kw])                                # [n, h, d]
    gb1 = dZ1[:, :kb].sum(1)
    g = torch.cat([gW1.reshape(n, -1), gb1, gW2.reshape(n, -1), gb2], dim=1)
    if not update:
        return loss, g, g, W
    if theta is not None:
        t = torch.zeros_like(W) if mutate == "omit_rho" else rho * (W - theta.to(dtype))
        if alpha is not None and mutate != "omit_alpha":
            t = alpha.to(dtype) + t
        g = g + t
    elif alpha is not None:
        raise ValueError("alpha needs theta")
    if momentum == 0.0:
        buf = g
    elif first_step:
        buf = mom.to(dtype) * momentum + g if mutate == "mode1_old_mom" else g
    else:
        buf = g if mutate == "mode2_no_mom" else mom.to(dtype) * momentum + g
    return loss, g, buf, W - lr * buf


def run_steps(inp: MlpInputs, d: int, h: int, c: int, kind: str, momentum: float, *, steps: Optional[int] = None,
              lr: float = LR, rho: float = RHO, mutate: Optional[str] = None, dtype=torch.float64):
    """Consecutive steps (the first with first_step=True, starting from
    inp.mom, which a correct step ignores), each from the state the step
    before left; a list of (loss, g', buf, W) per step."""
    th = inp.theta if kind != "plain" else None
    al = inp.alpha if kind == "admm" else None
    W, mom, out = inp.W, inp.mom, []
    for s in range(len(inp.X) if steps is None else steps):
        loss, g, buf, W = mlp_step_ref(W, inp.X[s], inp.y[s], d, h, c, theta=th, alpha=al, mom=mom, lr=lr,
                                       momentum=momentum, rho=rho if th is not None else 0.0, first_step=(s == 0),
                                       update=True, mutate=mutate, dtype=dtype)
        mom = buf
        out.append((loss, g, buf, W))
    return out


def tol_ratio(got: torch.Tensor, want: torch.Tensor, rtol: float, atol: float) -> float:
    """max |got - want| / (atol + rtol |want|): <= 1 is what assert_close accepts."""
    got, want = got.double(), want.double()
    r = (got - want).abs() / (atol + rtol * want.abs())
    r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
    return float(r.max()) if r.numel() else 0.0


# ---- the case list shared by the host check and the GPU tests (n, B, d, h, c)
MATRIX_SHAPES = [
    (3, 32, 784, 128, 10),   # config 5's tile shape
    (3, 33, 100, 96, 17),    # KS = 32, h not dividing 256, NT = 4
    (2, 64, 36, 64, 3),      # KS = 32, NT = 1, partial k chunk
    (2, 64, 40, 256, 32),    # every limit at once; c h > 2048, B h > 4096, LDS above 64 KiB
    (2, 8, 4, 224, 9),       # d = one partial chunk, h = 224, c h = 2016 <= 2048
    (2, 8, 4, 224, 10),      # one class past the 2048 edge
    (13, 7, 20, 32, 5),      # two XCD groups, ragged last one, B < 8
    (17, 1, 32, 32, 1),      # B = 1, c = 1, d = one full chunk, three groups
]
MATRIX_VARIANTS = [(k, m, wg) for k in KINDS for m in (0.0, MU) for wg in (False, True)]
EDGE_SHAPE = (5, 8, 36, 64, 3)         # the ABI-edge tests (admm, momentum)
SMALL_ROWS = (8, 36, 64, 3)            # the every-agent launch at n = 4 n_cu + 3
CHILD_PIN_SHAPE = (13, 7, 100, 128, 5)  # the bit-identity children's member checked against fp64
CHILD_LR, CHILD_STEPS = 0.1, 3


def child_inputs(n: int, B: int, d: int, h: int, c: int) -> MlpInputs:
    """Inputs of the bit-identity children (tests/test_mlp_gpu.py): the same
    distributions as make_inputs, three steps, W / X / y in the RNG order those
    children have always used."""
    P = mlp_P(d, h, c)
    torch.manual_seed(n * 1000 + d)
    W = torch.randn(n, P) * 0.05
    g = torch.Generator().manual_seed(d)
    X, y = [], []
    for _ in range(CHILD_STEPS):
        X.append(torch.randn(n, B, d, generator=g))
        y.append(torch.randint(0, c, (n, B), generator=g))
    g2 = torch.Generator().manual_seed(7 * d + n)
    theta, alpha, mom = (0.05 * torch.randn(*s, generator=g2) for s in ((P,), (n, P), (n, P)))
    return MlpInputs(W, theta, alpha, mom, X, y)
