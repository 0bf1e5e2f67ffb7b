"""The gradient-tracking round on the parameter-major bank, fused against
composed, in one process on the same buffers, legs alternating (random
4-regular W with Metropolis weights, so W = W_off + diag(d)):
  (a) the round composed from today's ops: two ops.mix_csr_pm (X and S), the
      self-weight terms (a multiply and an add each), x' by ops.prox_admm_sgd
      (fma(-lr, s, ax)), ops.separable_grad twice, an add and a subtract;
  (b) one ops.gt_csr_pm call (dol_gt_csr_pm_f32: X, S, T in, X', S' out);
  (c) the ops.dgd_csr_pm least-squares momentum round on the same X / Y / T
      buffers: the same five streams (X, T, M in, Y, M out), the yardstick for
      what this kernel structure reaches on the box at hand.
Both objectives.  ms by HIP events after a warm-up, median of --reps windows of
--inner calls; `b_over_a`, `b_over_c`; `frac` = 5 N P 4 bytes over (b)'s time
as a share of 8 TB/s.  Before timing, (b)'s X' and S' are compared bit for bit
with (a)'s on the whole bank.
  python tools/gt_pm_ab.py --agents 1024 [--params 1048576] [--reps 5] [--inner 10] [--legs abc] [--note TEXT] [--out profiles/x.jsonl]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=1024)
    ap.add_argument("--params", type=int, default=1 << 20)
    ap.add_argument("--lr", type=float, default=0.1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10, help="calls per timed window")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--legs", default="abc", help="which legs to time (the bit comparison needs a and b)")
    ap.add_argument("--note", default=None, help="free text kept in every row (e.g. the build measured)")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    a = ap.parse_args()
    dev = torch.device("cuda")
    out = open(a.out, "a") if a.out else None
    n, P, lr = a.agents, a.params, a.lr

    W, d = G.metropolis_weights(G.random_regular_csr(n, 4, seed=2028))
    rp, col, val = (torch.as_tensor(np.asarray(x, t), device=dev)
                    for x, t in ((W.rowptr, np.int32), (W.col, np.int32), (W.val, np.float32)))
    ld = (n + 3) // 4 * 4
    dw = torch.zeros(ld, device=dev)
    dw[:n] = torch.as_tensor(d, device=dev)
    g = torch.Generator(device=dev).manual_seed(9)
    XT, TT = torch.zeros(P, ld, device=dev), torch.zeros(P, ld, device=dev)
    XT[:, :n].normal_(generator=g)
    TT[:, :n].normal_(generator=g)
    ST, XO, SO = (torch.zeros_like(XT) for _ in range(3))
    if "a" in a.legs:
        AX, AS, G0, G1 = (torch.zeros_like(XT) for _ in range(4))
    if "c" in a.legs:
        MT = torch.zeros_like(XT)
    bytes_round = 5 * n * P * 4

    for objective in ("least_squares", "logistic"):
        if objective == "logistic":  # targets +-feature
            TT.copy_(torch.where(torch.rand(TT.shape, generator=g, device=dev) < 0.5, -TT, TT))
        ops.separable_grad(XT, TT, ST, objective)

        def composed():
            """X', S' into AX, AS (G0, G1 scratch)."""
            ops.mix_csr_pm(XT, AX, rp, col, val)
            ops.mix_csr_pm(ST, AS, rp, col, val)
            torch.mul(XT, dw, out=G0)
            AX.add_(G0)
            torch.mul(ST, dw, out=G0)
            AS.add_(G0)
            ops.prox_admm_sgd(AX, ST, lr=lr, write_grad=False)  # elementwise: x' = fma(-lr, s, ax)
            ops.separable_grad(AX, TT, G1, objective)
            ops.separable_grad(XT, TT, G0, objective)
            AS.add_(G1)
            AS.sub_(G0)

        def fused():
            ops.gt_csr_pm(XT, ST, XO, SO, rp, col, val, TT, self_weight=dw[:n], objective=objective, lr=lr)

        def dgd():
            ops.dgd_csr_pm(XT, XO, rp, col, val, TT, MT, objective="least_squares", lr=0.01, momentum=0.9)

        legs = {k: f for k, f in (("a", composed), ("b", fused), ("c", dgd)) if k in a.legs}
        for _ in range(a.warmup):  # clocks up, stage order tuned for the buffer pairs, code objects loaded
            for f in legs.values():
                f()
        torch.cuda.synchronize()
        same = None
        if "a" in legs and "b" in legs:
            composed()
            fused()
            same = bool(torch.equal(AX[:, :n].view(torch.int32), XO[:, :n].view(torch.int32))
                        and torch.equal(AS[:, :n].view(torch.int32), SO[:, :n].view(torch.int32)))
        t = {k: [] for k in legs}
        for _ in range(a.reps):
            for k, f in legs.items():
                t[k].append(timed(f, a.inner))
        m = {k: median(v) for k, v in t.items()}
        row = {"agents": n, "params": P, "objective": objective, "lr": lr, "bits_equal": same, "note": a.note}
        for k, name in (("a", "composed"), ("b", "fused"), ("c", "dgd_ls_momentum")):
            if k in m:
                row[name + "_ms"], row[name + "_all"] = m[k], t[k]
        if "b" in m:
            row["frac"] = bytes_round / (m["b"] / 1e3) / PEAK
            if "a" in m:
                row["b_over_a"] = m["b"] / m["a"]
            if "c" in m:
                row["b_over_c"] = m["b"] / m["c"]
        line = json.dumps(row)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()


if __name__ == "__main__":
    main()
