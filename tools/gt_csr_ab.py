"""The gradient-tracking round on the agent-major CSR bank, fused against
composed and against its yardsticks, in one process on one bank, legs
alternating (a random 4-regular graph with Metropolis weights: 1/5 per edge and
a self weight of 1/5):
  (a) one ops.gt_csr call (dol_gt_csr_f32: X, S, T in, X', S' out);
  (b) the round composed from the ops the library had before it: two
      ops.mix_csr (X and S), the self-weight terms (a multiply and an add
      each), x' by ops.prox_admm_sgd (fma(-lr, s, ax)), ops.separable_grad
      twice, an add and a subtract -- at least fourteen row streams against
      (a)'s five.  It writes X', S' into (a)'s output matrices and needs one
      scratch matrix more, so six bank matrices in all;
  (c) ops.dgd_csr with momentum 0.5 on the same bank: the same five streams (X,
      T, mom in, Y, mom out) through csr_xcd_kernel, the yardstick for "these
      bytes at the CSR mix's rate" on the box at hand;
  (d) ops.gt_csr_pm on the same graph and values in the parameter-major layout
      (five more matrices; at most ops.GT_MAX_AGENTS agents, skipped beyond).
Least squares and logistic for (a), (b), (d); (c) is least squares.  ms by HIP
events after a warm-up, per window of --inner calls, --reps windows per leg
with the legs alternating, so window i of (a) and of (b) are an A/B pair.
`frac` = 5 N P 4 bytes over (a)'s median time as a share of 8 TB/s.  Before
timing, a sample of 64 rows of (a)'s X' and S' is compared bit for bit with
(b)'s and, where it runs, all of (d)'s.
  python tools/gt_csr_ab.py --agents 1024 [--params 1048576] [--pad 0] [--legs abcd] [--reps 5] [--inner 10] [--note TEXT] [--out profiles/gt_csr_ab.jsonl]
The recorded runs: --agents 1024, and --agents 8192 --pad 2048.
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


def same_bits(a, b):
    return bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=1024)
    ap.add_argument("--params", type=int, default=1 << 20)
    ap.add_argument("--pad", type=int, default=0, help="ld = params + pad")
    ap.add_argument("--lr", type=float, default=0.1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10, help="calls per timed window")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--legs", default="abcd")
    ap.add_argument("--objectives", default="least_squares,logistic")
    ap.add_argument("--seed", type=int, default=2028, help="of the random 4-regular graph")
    ap.add_argument("--note", default=None, help="free text kept in every row (e.g. the build measured)")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    a = ap.parse_args()
    dev = torch.device("cuda")
    out = open(a.out, "a") if a.out else None
    n, P, lr, ld = a.agents, a.params, a.lr, a.params + a.pad
    legs_asked = "".join(k for k in a.legs if not (k == "d" and n > ops.GT_MAX_AGENTS))

    w_off, d = G.metropolis_weights(G.random_regular_csr(n, 4, seed=a.seed))
    rp, col, val = (torch.as_tensor(np.asarray(x, t), device=dev)
                    for x, t in ((w_off.rowptr, np.int32), (w_off.col, np.int32), (w_off.val, np.float32)))
    ws = torch.as_tensor(d, device=dev)

    def matrix():
        return torch.zeros(n, ld, device=dev)[:, :P]
    g = torch.Generator(device=dev).manual_seed(9)
    X, T, S, XO, SO = (matrix() for _ in range(5))
    X.normal_(generator=g)
    T.normal_(generator=g)
    if "b" in legs_asked:
        G0 = matrix()
    if "d" in legs_asked:
        ldp = (n + 3) // 4 * 4
        XT, ST, TT, XOT, SOT = (torch.zeros(P, ldp, device=dev) for _ in range(5))
        back = matrix()
    sample = torch.arange(0, n, max(1, n // 64), device=dev)[:64]
    bytes_round = 5 * n * P * 4

    for objective in a.objectives.split(","):
        if objective == "logistic":  # targets +-feature
            for r in range(0, n, 256):  # in row blocks: no bank-sized temporaries
                blk = T[r:r + 256]
                blk.mul_(torch.where(torch.rand(blk.shape, generator=g, device=dev) < 0.5, -1.0, 1.0))
        ops.separable_grad(X, T, S, objective)
        if "d" in legs_asked:
            for src, dst in ((X, XT), (S, ST), (T, TT)):
                ops.transpose(src, dst, n, P)

        def fused():
            ops.gt_csr(X, S, XO, SO, rp, col, val, T, self_weight=ws, objective=objective, lr=lr)

        def composed():
            """X', S' into XO, SO (G0 scratch)."""
            ops.mix_csr(X, XO, rp, col, val)
            ops.mix_csr(S, SO, rp, col, val)
            torch.mul(X, ws[:, None], out=G0)
            XO.add_(G0)
            torch.mul(S, ws[:, None], out=G0)
            SO.add_(G0)
            ops.prox_admm_sgd(XO, S, lr=lr, write_grad=False)  # elementwise: x' = fma(-lr, s, ax)
            ops.separable_grad(XO, T, G0, objective)
            SO.add_(G0)
            ops.separable_grad(X, T, G0, objective)
            SO.sub_(G0)

        def dgd():  # SO as the momentum buffer: read and written, like S' -- (a) rewrites it before it is compared
            ops.dgd_csr(X, XO, rp, col, val, T, mom=SO, objective="least_squares", lr=0.01, momentum=0.5)

        def pm():
            ops.gt_csr_pm(XT, ST, XOT, SOT, rp, col, val, TT, self_weight=ws, objective=objective, lr=lr)

        legs = {k: f for k, f in (("a", fused), ("b", composed), ("c", dgd), ("d", pm))
                if k in legs_asked and not (k == "c" and objective != "least_squares")}
        for _ in range(a.warmup):  # clocks up, stage order tuned, code objects loaded
            for f in legs.values():
                f()
        torch.cuda.synchronize()
        same = {}
        if "a" in legs:
            if "b" in legs:
                composed()
                want = XO[sample].clone(), SO[sample].clone()
            fused()
            if "b" in legs:
                same["b"] = same_bits(XO[sample], want[0]) and same_bits(SO[sample], want[1])
            if "d" in legs:
                pm()
                same["d"] = same_bits(ops.transpose(XOT, back, P, n), XO) and \
                    same_bits(ops.transpose(SOT, back, P, n), SO)
        t = {k: [] for k in legs}
        for _ in range(a.reps):
            for k, f in legs.items():
                t[k].append(timed(f, a.inner))
        m = {k: median(v) for k, v in t.items()}
        row = {"agents": n, "params": P, "ld": ld, "graph": f"random 4-regular, seed {a.seed}, Metropolis weights",
               "objective": objective, "lr": lr, "bits_equal": same, "note": a.note}
        for k, name in (("a", "fused"), ("b", "composed"), ("c", "dgd_csr_momentum"), ("d", "gt_csr_pm")):
            if k in m:
                row[name + "_ms"], row[name + "_all"] = m[k], t[k]
        if "a" in m:
            row["frac"] = bytes_round / (m["a"] / 1e3) / PEAK
            if "b" in m:
                row["a_over_b"] = m["a"] / m["b"]
                row["a_over_b_pairs"] = [x / y for x, y in zip(t["a"], t["b"])]
            if "c" in m:
                row["a_over_c"] = m["a"] / m["c"]
                row["a_over_c_pairs"] = [x / y for x, y in zip(t["a"], t["c"])]
                row["c_spread"] = max(t["c"]) / min(t["c"])
            if "d" in m:
                row["a_over_d"] = m["a"] / m["d"]
        line = json.dumps(row)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()


if __name__ == "__main__":
    main()
