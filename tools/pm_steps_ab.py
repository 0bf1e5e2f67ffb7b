"""Multi-step consensus on the parameter-major bank, fused against unfused, in
one process on the same buffers, legs alternating (random 4-regular W):
  (a) eps back-to-back ops.mix_csr_pm calls (one HBM pass per step),
  (b) one ops.mix_csr_pm_steps call (dol_mix_csr_pm_steps_f32: one pass),
for eps in --eps, and the fused round (SeparableDGDPM) with consensus_steps 1
and --round-eps against the same round as eps - 1 plain mixes + round().
ms by HIP events after a clock warm-up; `ratio` = (b) / (a); `frac` = 2 N P 4
bytes (one pass) over (b)'s time, as a share of 8 TB/s.  Before timing, (b)'s
result is compared bit for bit with (a)'s on the whole bank.
  python tools/pm_steps_ab.py --agents 1024 [--params 1048576] [--reps 5] [--inner 10] [--rounds] [--out profiles/x.jsonl]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "distributed-optimization-and-learning_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from dolhip import graph as G  # noqa: E402
from dolhip import ops  # noqa: E402
from dolhip.synthetic import SeparableDGDPM  # noqa: E402

PEAK = 8e12


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


def mix_legs(a, dev, emit):
    n, P = a.agents, a.params
    c = G.random_regular_csr(n, 4, seed=2028)
    rp, col, val = (torch.as_tensor(np.asarray(x, t), device=dev)
                    for x, t in ((c.rowptr, np.int32), (c.col, np.int32), (c.val, np.float32)))
    g = torch.Generator(device=dev).manual_seed(9)
    ld = (n + 3) // 4 * 4
    XT = torch.zeros(P, ld, device=dev)
    XT[:, :n].normal_(generator=g)
    YT, ZT = torch.zeros_like(XT), torch.zeros_like(XT)

    def unfused(eps):
        A, B = XT, YT
        for _ in range(eps):
            ops.mix_csr_pm(A, B, rp, col, val)
            A, B = B, A
        return A

    for _ in range(a.warmup):  # clocks up, stage order tuned for this buffer pair, code objects loaded
        unfused(2)
        ops.mix_csr_pm_steps(XT, YT, rp, col, val, 2)
    torch.cuda.synchronize()
    bytes_pass = 2 * n * P * 4
    for eps in a.eps:
        ops.mix_csr_pm_steps(XT, ZT, rp, col, val, eps, nseg=0)
        same = torch.equal(unfused(eps).view(torch.int32), ZT.view(torch.int32))
        ta, tb = [], []
        for _ in range(a.reps):
            ta.append(timed(lambda: unfused(eps), a.inner))
            tb.append(timed(lambda: ops.mix_csr_pm_steps(XT, YT, rp, col, val, eps), a.inner))
        ma, mb = median(ta), median(tb)
        emit({"leg": "mix", "agents": n, "params": P, "eps": eps, "unfused_ms": ma, "fused_ms": mb,
              "ratio": mb / ma, "frac": bytes_pass / (mb / 1e3) / PEAK, "unfused_all": ta, "fused_all": tb,
              "bits_equal": same})


def round_legs(a, dev, emit):
    n, P, k = a.agents, a.params, a.round_eps
    plan = G.MixingPlan(G.random_regular_csr(n, 4, seed=2028), dev)
    for objective, mom in (("least_squares", 0.9), ("logistic", 0.0)):
        one = SeparableDGDPM(plan, P, objective=objective, lr=0.01, momentum=mom, local_steps=1, seed=7)
        many = SeparableDGDPM(plan, P, objective=objective, lr=0.01, momentum=mom, local_steps=1, seed=7,
                              consensus_steps=k)

        def chained():
            for _ in range(k - 1):
                ops.mix_csr_pm(one.XT, one.YT, plan.rowptr, plan.col, plan.val, P=P)
                one.XT, one.YT = one.YT, one.XT
            one.round()

        for _ in range(a.warmup):
            one.round()
            many.round()
            chained()
        torch.cuda.synchronize()
        t1, tk, tc = [], [], []
        for _ in range(a.reps):
            t1.append(timed(one.round, a.inner))
            tc.append(timed(chained, a.inner))
            tk.append(timed(many.round, a.inner))
        m1, mk, mc = median(t1), median(tk), median(tc)
        emit({"leg": "round", "agents": n, "params": P, "objective": objective, "momentum": mom, "eps": k,
              "round_eps1_ms": m1, "fused_ms": mk, "unfused_ms": mc, "ratio": mk / mc, "fused_over_eps1": mk / m1,
              "eps1_all": t1, "fused_all": tk, "unfused_all": tc})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=1024)
    ap.add_argument("--params", type=int, default=1 << 20)
    ap.add_argument("--eps", type=int, nargs="+", default=[2, 3, 5, 8])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10, help="calls per timed window")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", action="store_true", help="also time the fused round (<= 4096 agents)")
    ap.add_argument("--round-eps", type=int, default=5)
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

    mix_legs(a, dev, emit)
    if a.rounds:
        round_legs(a, dev, emit)


if __name__ == "__main__":
    main()
