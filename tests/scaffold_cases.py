"""The SCAFFOLD least-squares round restated on the host, and the inputs the
CPU and GPU tiers share (tests/test_scaffold_host.py, tests/test_scaffold_gpu.py).

scaffold_ls_round_ref is what dol_scaffold_ls_round_f32 is held to, bit for
bit.  Every separately rounded term is one numpy float32 operation; the SGD
step is oracle.prox_admm_sgd with theta = alpha = None (the golden-pinned
momentum + fma(-lr, d, w)), and the two chains over the sampled clients are
oracle.ordered_sum (acc = x[o0]; acc = fl(acc + x[ok])).
"""
import numpy as np
import torch

import oracle

N = 9
ORDER = np.array([7, 2, 0, 8, 5, 3, 6, 4, 1], np.int32)
FIRST = np.array([1, 0, 1, 0, 0, 1, 1, 0, 0], np.int32)
LR = 0.05


def inv_steps_lr(local_steps, lr):
    """float32(1 / (local_steps * lr)), the quotient taken in double (DEC/clients.py:164)."""
    return np.float32(1.0 / (int(local_steps) * float(lr)))


def scaffold_ls_round_ref(w, buf, ci, target, theta, c, agents, first, lr, momentum, local_steps, global_lr=1.0,
                          scale_w=None, n_total=None):
    """One SCAFFOLD round for the sampled rows `agents`; returns (w', buf',
    ci', theta_out, c_out, resid[2]) on copies (buf' None without momentum).
    scale_w None = m; n_total None = the rows of w.  The agents whose
    first-step flags agree go through the oracle together (the step is
    row-wise)."""
    assert int(local_steps) >= 1
    w = np.array(w, np.float32)
    ci = np.array(ci, np.float32)
    buf = None if buf is None or momentum == 0 else np.array(buf, np.float32)
    T = np.asarray(target, np.float32)
    theta = np.asarray(theta, np.float32)
    c = np.asarray(c, np.float32)
    agents = np.asarray(agents, np.int64)
    m = len(agents)
    first = np.zeros(m, bool) if first is None else np.asarray(first) != 0
    inv = inv_steps_lr(local_steps, lr)
    DL = np.zeros_like(w)
    DC = np.zeros_like(w)
    with np.errstate(invalid="ignore", over="ignore"):  # Inf targets: Inf - Inf is the NaN the kernel gives too
        for flag in (False, True):
            rows = agents[first == flag]
            if rows.size == 0:
                continue
            wk = np.repeat(theta[None, :], rows.size, axis=0)
            bk = None if buf is None else buf[rows]
            for step in range(int(local_steps)):
                g = wk - T[rows]
                gp = (g + c[None, :]) - ci[rows]  # grad + alpha_server - alpha, DEC/clients.py:155
                assert gp.dtype == np.float32
                wk, bk, _ = oracle.prox_admm_sgd(wk, bk, gp, None, None, np.float32(0.0), np.float32(lr),
                                                 np.float32(momentum), flag and step == 0)
            dl = wk - theta[None, :]                 # local_sum, :162
            cn = (ci[rows] - c[None, :]) - dl * inv  # :165
            DL[rows] = dl
            DC[rows] = cn - ci[rows]                 # control_update, :167
            w[rows] = wk
            ci[rows] = cn
            if buf is not None:
                buf[rows] = bk
        acc_w = oracle.ordered_sum(DL, agents)
        acc_c = oracle.ordered_sum(DC, agents)
        sw = np.float32(m if scale_w is None else scale_w)
        sc = np.float32(w.shape[0] if n_total is None else n_total)
        theta_out = theta + np.float32(global_lr) * (acc_w / sw)
        c_out = c + acc_c / sc
        assert theta_out.dtype == np.float32 and c_out.dtype == np.float32
        resid = np.array([(DL[agents].astype(np.float64) ** 2).sum(), (ci[agents].astype(np.float64) ** 2).sum()])
    return w, buf, ci, theta_out, c_out, resid


def inputs(P, seed, n=N):
    """(T, B, CI, theta, c): nonzero control variates, and the Inf / -0 /
    denormal targets of test_admm_gpu.py in row 1."""
    rng = np.random.default_rng(seed)
    T = rng.standard_normal((n, P)).astype(np.float32)
    B = rng.standard_normal((n, P)).astype(np.float32)
    CI = (0.3 * rng.standard_normal((n, P))).astype(np.float32)
    th = rng.standard_normal(P).astype(np.float32)
    c = (0.3 * rng.standard_normal(P)).astype(np.float32)
    T[1, :3] = [np.inf, -0.0, 1e-40][:min(3, P)]
    return T, B, CI, th, c


def cpu_scaffold_round(w, ci, target, theta, c, agents=None, first=None, buf=None, lr=0.1, momentum=0.0,
                       local_steps=1, global_lr=1.0, theta_out=None, c_out=None, scale_w=None, n_total=None,
                       resid_total=None, work=None, P=None, validate=True):
    """A round_fn for SeparableScaffold on CPU tensors: ops.scaffold_ls_round's
    signature on the restatement (theta_out may be theta, c_out may be c)."""
    P = w.shape[1] if P is None else P
    ag = agents.numpy() if agents is not None else np.arange(w.shape[0])
    fs = first.numpy() if first is not None else None
    wn, bn, cn, th1, c1, resid = scaffold_ls_round_ref(
        w[:, :P].numpy(), None if buf is None else buf[:, :P].numpy(), ci[:, :P].numpy(), target[:, :P].numpy(),
        theta[:P].numpy(), c[:P].numpy(), ag, fs, lr, momentum, local_steps, global_lr, scale_w,
        w.shape[0] if n_total is None else n_total)
    w[:, :P] = torch.from_numpy(wn)
    ci[:, :P] = torch.from_numpy(cn)
    if buf is not None and bn is not None:
        buf[:, :P] = torch.from_numpy(bn)
    theta_out = torch.empty(P) if theta_out is None else theta_out
    c_out = torch.empty(P) if c_out is None else c_out
    theta_out[:P] = torch.from_numpy(th1)
    c_out[:P] = torch.from_numpy(c1)
    if resid_total is not None:
        resid_total[:] = torch.from_numpy(resid)
    return theta_out, c_out
