"""The EXTRA round on the agent-major bank (ops.extra_csr, ops.extra_ring)
against its two yardsticks and against the round composed from existing ops,
in one process on the same buffers, legs alternating.  A random 4-regular graph
(--seed) with Metropolis weights for the CSR legs, the ring with Metropolis
weights (1/3, 1/3, 1/3) for the ring legs; ms by HIP events after a warm-up,
per window of --inner calls, --reps windows per leg, medians.  ld = --params +
--pad.
  (a) one ops.extra_csr call (X gathered, T and corr in, X' and corr out);
  (b) one ops.gt_csr call on the same graph: two gathered matrices, the round
      EXTRA is meant to undercut;
  (c) one ops.dgd_csr call with momentum 0.5 on the same graph: the same five
      streams (corr's buffer as the momentum), the yardstick for the bytes;
  (d) the round composed from ops.mix_csr, ops.separable_grad,
      ops.prox_admm_sgd and torch elementwise ops into (a)'s output matrix and
      two scratch matrices.  A sample of 64 rows is kept and compared with
      (a)'s from the same zero correction (`bits_equal`; torch's scaled add is
      not pinned to be an fma, so this is recorded, not required).
  (e) / (f) / (g) ops.extra_ring, ops.gt_ring, ops.dgd_ring with momentum 0.5
      on the n-agent ring, on the same buffers.
The correction is updated in place, so it keeps growing over a leg's calls (X
is not swapped): the values stay finite and far from denormal, which is all a
timing needs.  `frac` = 5 N P 4 bytes over a leg's median as a share of 8 TB/s.
  python tools/extra_ab.py --agents 1024 [--params 1048576] [--pad 0] [--legs abcdefg] [--objectives least_squares,logistic] [--reps 5] [--inner 10] [--note TEXT] [--out profiles/extra_ab.jsonl]

--layout pm: the round on the parameter-major bank (ops.extra_csr_pm), the same
graph and weights, matrices [params, round_up(agents, 4)], the stage order left
to the ops (tuned for the XT / YT pair on first use, as a caller gets it)
(profiles/extra_pm_ab.jsonl; the recorded runs: 1024 x 2^20 and 4096 x 2^18):
  (a) one ops.extra_csr_pm call;
  (b) one ops.gt_csr_pm call on the same graph (X and S gathered);
  (c) one ops.dgd_csr_pm call with momentum 0.5: the same five streams (corr's
      buffer as the momentum) through the pipeline (a) is built on;
  (d) one ops.extra_csr call on the same problem agent-major (transposed copies
      of X and T, a Y and a corr of their own).  Its first call from a zero
      correction is compared with (a)'s (`bits_equal_agent_major`: all of X'
      and corr).
  python tools/extra_ab.py --layout pm --agents 1024 [--params 1048576] [--legs abcd] [--objectives least_squares,logistic] [--reps 5] [--inner 10] [--note TEXT] [--out profiles/extra_pm_ab.jsonl]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "distributed-optimization-and-learning_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from dolhip import graph as G  # noqa: E402
from dolhip import ops  # noqa: E402
from dolhip.synthetic import ring_gt_weights  # noqa: E402
from gt_ab import PEAK, csr_dev, median, ring_csr, same_bits, timed  # noqa: E402

PM_NAMES = {"a": "extra_csr_pm", "b": "gt_csr_pm", "c": "dgd_csr_pm_momentum", "d": "extra_csr"}
NAMES = {"a": "extra_csr", "b": "gt_csr", "c": "dgd_csr_momentum", "d": "composed", "e": "extra_ring", "f": "gt_ring",
         "g": "dgd_ring_momentum"}


def pm_main(a):
    dev = torch.device("cuda")
    n, P, lr = a.agents, a.params, a.lr
    ld = (n + 3) // 4 * 4
    w_off, d = G.metropolis_weights(G.random_regular_csr(n, 4, seed=a.seed))
    rp, col, val = csr_dev(w_off, dev)
    ws = torch.as_tensor(d, device=dev)

    def matrix():
        return torch.zeros(P, ld, device=dev)[:, :n]
    g = torch.Generator(device=dev).manual_seed(9)
    XT, TT, YT, CT = (matrix() for _ in range(4))
    XT.normal_(generator=g)
    TT.normal_(generator=g)
    if "b" in a.legs:
        ST, SO = matrix(), matrix()
    if "d" in a.legs:  # the same problem agent-major
        X, T, Y, C = (torch.zeros(n, P, device=dev) for _ in range(4))
    out = open(a.out, "a") if a.out else None

    for objective in a.objectives.split(","):
        if objective == "logistic":  # targets +-feature, in p-row blocks: no bank-sized temporaries
            for r in range(0, P, 1 << 16):
                blk = TT[r:r + (1 << 16)]
                blk.mul_(torch.where(torch.rand(blk.shape, generator=g, device=dev) < 0.5, -1.0, 1.0))
        kw = dict(objective=objective, lr=lr)
        legs = {
            "a": lambda: ops.extra_csr_pm(XT, YT, rp, col, val, TT, CT, self_weight=ws, **kw),
            "b": lambda: ops.gt_csr_pm(XT, ST, YT, SO, rp, col, val, TT, self_weight=ws, **kw),
            "c": lambda: ops.dgd_csr_pm(XT, YT, rp, col, val, TT, CT, steps=1, momentum=0.5, **kw),
            "d": lambda: ops.extra_csr(X, Y, rp, col, val, T, C, self_weight=ws, **kw),
        }
        legs = {k: f for k, f in legs.items() if k in a.legs}
        same = None
        if "d" in legs:
            ops.transpose(XT, X, P, n)
            ops.transpose(TT, T, P, n)
        if "a" in legs and "d" in legs:
            C.zero_()
            legs["d"]()
            ops.transpose(Y, YT, n, P)  # YT as the transposes' landing place: (a) overwrites it below
            want_x = YT.clone()
            ops.transpose(C, YT, n, P)
            want_c = YT.clone()
            CT.zero_()
            legs["a"]()
            same = same_bits(YT, want_x) and same_bits(CT, want_c)
            del want_x, want_c
        t = {k: [] for k in legs}
        for k, f in legs.items():  # each leg from its own start state: zero corr / momentum, s = g(x, t)
            CT.zero_()
            if k == "d":
                C.zero_()
            if k == "b":
                ops.separable_grad(XT, TT, ST, objective)
            for _ in range(a.warmup):  # clocks up, code objects loaded, the stage order tuned
                f()
        torch.cuda.synchronize()
        for _ in range(a.reps):
            for k, f in legs.items():
                t[k].append(timed(f, a.inner))
        m = {k: median(x) for k, x in t.items()}
        r = {"layout": "pm", "agents": n, "params": P, "ld": ld,
             "graph": f"random 4-regular, seed {a.seed}, Metropolis weights", "objective": objective, "lr": lr,
             "bits_equal_agent_major": same, "note": a.note}
        for k in legs:
            r[PM_NAMES[k] + "_ms"], r[PM_NAMES[k] + "_all"] = m[k], t[k]
            r[PM_NAMES[k] + "_frac"] = 5 * n * P * 4 / (m[k] / 1e3) / PEAK
        for num, den in (("a", "b"), ("a", "c"), ("a", "d")):
            if num in m and den in m:
                r[f"{num}_over_{den}"] = m[num] / m[den]
                r[f"{num}_over_{den}_pairs"] = [x / y for x, y in zip(t[num], t[den])]
        line = json.dumps(r)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layout", default="am", choices=("am", "pm"), help="am: the agent-major legs; pm: the "
                    "parameter-major ones")
    ap.add_argument("--agents", type=int, default=1024)
    ap.add_argument("--params", type=int, default=1 << 20)
    ap.add_argument("--pad", type=int, default=0, help="ld = params + pad")
    ap.add_argument("--seed", type=int, default=2028, help="of the random 4-regular graph")
    ap.add_argument("--lr", type=float, default=0.1)
    ap.add_argument("--legs", default=None, help="default: abcdefg (am), abcd (pm)")
    ap.add_argument("--objectives", default="least_squares,logistic")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10, help="calls per timed window")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--note", default=None, help="free text kept in every row (e.g. the build measured)")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    a = ap.parse_args()
    if a.legs is None:
        a.legs = "abcd" if a.layout == "pm" else "abcdefg"
    if a.layout == "pm":
        return pm_main(a)
    dev = torch.device("cuda")
    n, P, lr, ld = a.agents, a.params, a.lr, a.params + a.pad
    w_off, d = G.metropolis_weights(G.random_regular_csr(n, 4, seed=a.seed))
    rp, col, val = csr_dev(w_off, dev)
    ws = torch.as_tensor(d, device=dev)
    wp, wn, wr = (torch.as_tensor(w, device=dev) for w in ring_gt_weights(ring_csr(n)))

    def matrix():
        return torch.zeros(n, ld, device=dev)[:, :P]
    g = torch.Generator(device=dev).manual_seed(9)
    X, T, Y, C = (matrix() for _ in range(4))
    X.normal_(generator=g)
    T.normal_(generator=g)
    if set(a.legs) & set("bdf"):  # the trackers of the gradient-tracking legs; (d)'s two scratch matrices
        S, SO = matrix(), matrix()
    rows = torch.arange(0, n, max(1, n // 64), device=dev)[:64]  # of (d)'s comparison
    out = open(a.out, "a") if a.out else None

    for objective in a.objectives.split(","):
        if objective == "logistic":  # targets +-feature, in row blocks: no bank-sized temporaries
            for r in range(0, n, 256):
                blk = T[r:r + 256]
                blk.mul_(torch.where(torch.rand(blk.shape, generator=g, device=dev) < 0.5, -1.0, 1.0))
        kw = dict(objective=objective, lr=lr)

        def composed():
            ops.mix_csr(X, Y, rp, col, val)
            torch.mul(X, ws[:, None], out=S)
            Y.add_(S)  # ax
            torch.sub(X, Y, out=SO)  # r
            ops.separable_grad(X, T, S, objective)
            ops.prox_admm_sgd(Y, S, lr=lr, write_grad=False)  # elementwise: fma(-lr, g, ax)
            Y.sub_(C)
            C.add_(SO, alpha=0.5)

        legs = {
            "a": lambda: ops.extra_csr(X, Y, rp, col, val, T, C, self_weight=ws, **kw),
            "b": lambda: ops.gt_csr(X, S, Y, SO, rp, col, val, T, self_weight=ws, **kw),
            "c": lambda: ops.dgd_csr(X, Y, rp, col, val, T, mom=C, steps=1, momentum=0.5, **kw),
            "d": composed,
            "e": lambda: ops.extra_ring(X, Y, wp, wn, T, C, self_weight=wr, **kw),
            "f": lambda: ops.gt_ring(X, S, Y, SO, wp, wn, T, self_weight=wr, **kw),
            "g": lambda: ops.dgd_ring(X, Y, wp, wn, T, mom=C, steps=1, momentum=0.5, **kw),
        }
        legs = {k: f for k, f in legs.items() if k in a.legs}
        same = None
        if "a" in legs and "d" in legs:
            C.zero_()
            composed()
            want = (Y[rows].clone(), C[rows].clone())
            C.zero_()
            legs["a"]()
            same = same_bits(Y[rows], want[0]) and same_bits(C[rows], want[1])
        t = {k: [] for k in legs}
        for k, f in legs.items():  # each leg from its own start state: zero corr / momentum, s = g(x, t)
            C.zero_()
            if k in "bf":
                ops.separable_grad(X, T, S, objective)
            for _ in range(a.warmup):  # clocks up, code objects loaded
                f()
        torch.cuda.synchronize()
        for _ in range(a.reps):
            for k, f in legs.items():
                if k in "bf":  # (d) uses S as scratch
                    ops.separable_grad(X, T, S, objective)
                    torch.cuda.synchronize()
                t[k].append(timed(f, a.inner))
        m = {k: median(x) for k, x in t.items()}
        r = {"agents": n, "params": P, "ld": ld, "graph": f"random 4-regular, seed {a.seed}, Metropolis weights; ring legs: "
             "Metropolis ring", "objective": objective, "lr": lr, "bits_equal_composed_sample": same, "note": a.note}
        for k in legs:
            r[NAMES[k] + "_ms"], r[NAMES[k] + "_all"] = m[k], t[k]
            r[NAMES[k] + "_frac"] = 5 * n * P * 4 / (m[k] / 1e3) / PEAK
        for num, den in (("a", "b"), ("a", "c"), ("a", "d"), ("e", "f"), ("e", "g")):
            if num in m and den in m:
                r[f"{num}_over_{den}"] = m[num] / m[den]
                r[f"{num}_over_{den}_pairs"] = [x / y for x, y in zip(t[num], t[den])]
        line = json.dumps(r)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()


if __name__ == "__main__":
    main()
