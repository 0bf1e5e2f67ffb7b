"""The one-pass least-squares server round of the three algorithms, in one
process on the same buffers, legs alternating (full participation, `--steps`
local steps, with and without momentum):
  (a) FedADMM   ops.admm_ls_round_mean                      (the yardstick)
  (b) FedProx   ops.fed_ls_round_mean(algorithm="fedprox")
  (c) FedAvg    ops.fed_ls_round_mean(algorithm="fedavg")
  (d) with --composed: the FedProx round without the fused entry point -- w =
      theta, then per local step torch.sub(w, t, out=g) + ops.prox_admm_sgd(theta),
      then ops.ordered_mean -- whose bits must equal (b)'s.
ms by HIP events, the median of `--reps` windows of `--inner` calls after a
warm-up; `frac` = the leg's algorithmic bytes, (rows)*4*P*m + 2*4*P with rows =
2 (t in, w out) + 2 with momentum + 2 with duals, over its time, as a share of
8 TB/s; `ratio` = the leg over (a), beside the ratio of the bytes; `spread_a` =
(a)'s own window-to-window range, the allowance `not_slower` gives (b) and (c).
Before any timing the one-pass rows and theta of (b) and (c) are compared bit
for bit with the two-kernel round's (ops.fed_ls_round + ops.ordered_sum), and
(d)'s with (b)'s.
  python tools/fed_ls_ab.py --agents 1024 [--params 1048576] [--composed] [--out profiles/fed_ls_ab.jsonl]
  python tools/fed_ls_ab.py --agents 1024 --only fedprox     (that leg alone, untimed: for a counter run)
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "distributed-optimization-and-learning_amd"))

import torch  # noqa: E402

from dolhip import ops  # noqa: E402
from dolhip.bank import row_stride  # noqa: E402

PEAK = 8e12
RHO, LR = 0.1, 0.1


def timed(fn, inner):
    """ms per call over `inner` back-to-back calls between two events."""
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(inner):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / inner


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def bits(t):
    """A 64-bit sum over the bit patterns of t, in chunks of rows (no copy of the matrix)."""
    t = t.view(torch.int32)
    if t.dim() == 1:
        return int(t.sum(dtype=torch.int64))
    return sum(int(t[i:i + 256].sum(dtype=torch.int64)) for i in range(0, t.shape[0], 256))


def algorithmic_bytes(m, P, momentum, duals):
    return (2 + 2 * (momentum != 0.0) + 2 * duals) * 4 * P * m + 2 * 4 * P


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=1024)
    ap.add_argument("--params", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=10, help="local steps per round")
    ap.add_argument("--momenta", type=float, nargs="+", default=[0.5, 0.0])
    ap.add_argument("--reps", type=int, default=5, help="timed windows per leg")
    ap.add_argument("--inner", type=int, default=5, help="rounds per timed window")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--composed", action="store_true", help="also leg (d), the per-step composition (one more matrix)")
    ap.add_argument("--only", choices=sorted(ops.FED_ALGORITHMS), default=None,
                    help="run this one-pass leg alone, --inner times, untimed (for a counter run)")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    a = ap.parse_args()
    dev = torch.device("cuda")
    out = open(a.out, "a") if a.out else None

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    m, P, steps = a.agents, a.params, a.steps
    ld = row_stride(P)
    gen = torch.Generator(device=dev).manual_seed(2028)
    w = torch.zeros(m, ld, device=dev)
    t = torch.empty(m, ld, device=dev).normal_(generator=gen)
    buf = torch.zeros(m, ld, device=dev)
    need_alpha = a.only in (None, "fedadmm")
    alpha = torch.zeros(m, ld, device=dev) if need_alpha else None
    g = torch.zeros(m, ld, device=dev) if a.composed else None
    theta = torch.empty(ld, device=dev).normal_(generator=gen)
    theta_out = torch.zeros(ld, device=dev)
    agents = torch.arange(m, dtype=torch.int32, device=dev)
    first = torch.zeros(m, dtype=torch.int32, device=dev)  # every optimizer has stepped before
    tot = torch.zeros(2, dtype=torch.float64, device=dev)

    def one_pass(algorithm, mu):
        kw = dict(agents=agents, first=first if mu else None, buf=buf if mu else None, rho=RHO, lr=LR, momentum=mu,
                  local_steps=steps, out=theta_out, resid_total=tot, P=P, validate=False)
        if algorithm == "fedadmm":
            ops.admm_ls_round_mean(w, alpha, t, theta, **kw)
        else:
            ops.fed_ls_round_mean(w, None, t, theta, algorithm=algorithm, **kw)

    def two_kernel(algorithm, mu):
        ops.fed_ls_round(w, None, t, theta, algorithm=algorithm, agents=agents, first=first if mu else None,
                         buf=buf if mu else None, rho=RHO, lr=LR, momentum=mu, local_steps=steps, P=P)
        ops.ordered_sum(w, agents, out=theta_out, scale=float(m), P=P)

    def composed(mu):  # (d): FedProx from the per-step call
        w[:, :P] = theta[:P]
        for _ in range(steps):
            torch.sub(w, t, out=g)
            ops.prox_admm_sgd(w, g, buf if mu else None, theta=theta, rho=RHO, lr=LR, momentum=mu, first_step=False,
                              write_grad=False, P=P)
        ops.ordered_mean(w, agents, out=theta_out, P=P)

    def state_bits(run):
        """The bits of (w, buf, theta_out) after `run` from the same momentum rows."""
        buf.copy_(t)
        w.zero_()
        theta_out.zero_()
        run()
        torch.cuda.synchronize()
        return bits(w[:, :P]), bits(buf[:, :P]), bits(theta_out[:P])

    if a.only:
        mu = a.momenta[0]
        for _ in range(a.inner):
            one_pass(a.only, mu)
        torch.cuda.synchronize()
        emit({"leg": a.only, "agents": m, "params": P, "steps": steps, "momentum": mu, "calls": a.inner,
              "algorithmic_bytes_per_call": algorithmic_bytes(m, P, mu, a.only == "fedadmm"),
              "algorithmic_read_bytes_per_call": (1 + (mu != 0.0) + (a.only == "fedadmm")) * 4 * P * m + 4 * P,
              "algorithmic_write_bytes_per_call": (1 + (mu != 0.0) + (a.only == "fedadmm")) * 4 * P * m + 4 * P})
        return

    for mu in a.momenta:
        same = {}
        for algorithm in ("fedprox", "fedavg"):
            same[algorithm] = state_bits(lambda: one_pass(algorithm, mu)) == state_bits(lambda: two_kernel(algorithm, mu))
        if a.composed:
            same["composed"] = state_bits(lambda: one_pass("fedprox", mu)) == state_bits(lambda: composed(mu))
        legs = [("a_fedadmm", lambda: one_pass("fedadmm", mu), True), ("b_fedprox", lambda: one_pass("fedprox", mu), False),
                ("c_fedavg", lambda: one_pass("fedavg", mu), False)]
        if a.composed:
            legs.append(("d_fedprox_composed", lambda: composed(mu), False))
        for _ in range(a.warmup):  # clocks up, code objects loaded
            for _, fn, _ in legs:
                fn()
        torch.cuda.synchronize()
        ms = {name: [] for name, _, _ in legs}
        for _ in range(a.reps):  # the legs alternate: one window each per repetition
            for name, fn, _ in legs:
                ms[name].append(timed(fn, a.inner))
        med = {k: median(v) for k, v in ms.items()}
        spread_a = max(ms["a_fedadmm"]) - min(ms["a_fedadmm"])
        row = {"agents": m, "params": P, "steps": steps, "momentum": mu, "bits_equal": same, "ms": med, "ms_all": ms,
               "spread_a_ms": spread_a, "frac": {}, "ratio": {}, "byte_ratio": {}, "not_slower": {}}
        bytes_a = algorithmic_bytes(m, P, mu, True)
        for name, _, duals in legs:
            nbytes = algorithmic_bytes(m, P, mu, duals)
            row["frac"][name] = nbytes / (med[name] / 1e3) / PEAK
            if name != "a_fedadmm":
                row["ratio"][name] = med[name] / med["a_fedadmm"]
            if name in ("b_fedprox", "c_fedavg"):
                row["byte_ratio"][name] = nbytes / bytes_a
                row["not_slower"][name] = med[name] <= med["a_fedadmm"] + spread_a
        emit(row)


if __name__ == "__main__":
    main()
