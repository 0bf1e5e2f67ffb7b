"""The push-sum gradient-tracking round on the agent-major CSR bank
(ops.gt_push_csr) against its yardstick and against the round composed from
existing ops, in one process on the same buffers, legs alternating.  A random
4-regular graph (--seed) with out-degree weights (graph.push_sum_weights: 1/5
per edge and a self weight of 1/5), both objectives; ms by HIP events after a
warm-up, per window of --inner calls, --reps windows per leg, medians.
ld = --params + --pad.
  (a) one ops.gt_push_csr call (U, S, T in, U', S' out, and the n-vectors v, v');
  (b) one ops.gt_csr call on the same matrices and weights: the same five
      streams without the two divisions per coordinate and the v reads, the
      yardstick;
  (c) the round composed from existing ops into (a)'s output matrices and one
      scratch matrix: two ops.mix_csr (U and S), a third on v as an [n, 1]
      matrix, the self-weight terms, u' by ops.prox_admm_sgd, two torch
      divisions, ops.separable_grad twice, an add and a subtract.  A sample of
      64 rows is kept and compared with (a)'s (`bits_equal`; torch's division
      is not pinned to be correctly rounded, so this is recorded, not required).
`a_over_b` is the cost of the divisions and the v reads, `a_over_c` must be
below 1, `frac` = 5 N P 4 bytes over (a)'s median as a share of 8 TB/s.
  python tools/gt_push_ab.py --agents 1024 [--params 1048576] [--pad 0] [--legs abc] [--objectives least_squares,logistic] [--reps 7] [--inner 10] [--note TEXT] [--out profiles/gt_push_ab.jsonl]
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
from gt_ab import PEAK, csr_dev, median, same_bits, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=1024)
    ap.add_argument("--params", type=int, default=1 << 20)
    ap.add_argument("--pad", type=int, default=0, help="ld = params + pad")
    ap.add_argument("--seed", type=int, default=2028, help="of the random 4-regular graph")
    ap.add_argument("--lr", type=float, default=0.1)
    ap.add_argument("--legs", default="abc")
    ap.add_argument("--objectives", default="least_squares,logistic")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10, help="calls per timed window")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--note", default=None, help="free text kept in every row (e.g. the build measured)")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    a = ap.parse_args()
    dev = torch.device("cuda")
    n, P, lr, ld = a.agents, a.params, a.lr, a.params + a.pad
    c_off, d = G.push_sum_weights(G.random_regular_csr(n, 4, seed=a.seed))
    rp, col, val = csr_dev(c_off, dev)
    ws = torch.as_tensor(d, device=dev)

    def matrix():
        return torch.zeros(n, ld, device=dev)[:, :P]
    g = torch.Generator(device=dev).manual_seed(9)
    U, T, S, UO, SO = (matrix() for _ in range(5))
    U.normal_(generator=g)
    T.normal_(generator=g)
    v = torch.rand(n, generator=g, device=dev) + 0.5  # an arbitrary positive v: the divisions are real ones
    vo = torch.zeros(n, device=dev)
    if "c" in a.legs:
        G0, av = matrix(), torch.zeros(n, 1, device=dev)
    rows = torch.arange(0, n, max(1, n // 64), device=dev)[:64]  # of (c)'s comparison
    out = open(a.out, "a") if a.out else None

    for objective in a.objectives.split(","):
        if objective == "logistic":  # targets +-feature, in row blocks: no bank-sized temporaries
            for r in range(0, n, 256):
                blk = T[r:r + 256]
                blk.mul_(torch.where(torch.rand(blk.shape, generator=g, device=dev) < 0.5, -1.0, 1.0))
        ops.separable_grad(U, T, S, objective)

        def push():
            ops.gt_push_csr(U, S, UO, SO, rp, col, val, T, v, vo, self_weight=ws, objective=objective, lr=lr)

        def plain():
            ops.gt_csr(U, S, UO, SO, rp, col, val, T, self_weight=ws, objective=objective, lr=lr)

        def composed():
            ops.mix_csr(U, UO, rp, col, val)
            ops.mix_csr(S, SO, rp, col, val)
            ops.mix_csr(v[:, None], av, rp, col, val)
            av.add_((ws * v)[:, None])
            torch.mul(U, ws[:, None], out=G0)
            UO.add_(G0)
            torch.mul(S, ws[:, None], out=G0)
            SO.add_(G0)
            ops.prox_admm_sgd(UO, S, lr=lr, write_grad=False)  # elementwise: u' = fma(-lr, s, au)
            torch.div(UO, av, out=G0)
            ops.separable_grad(G0, T, G0, objective)
            SO.add_(G0)
            torch.div(U, v[:, None], out=G0)
            ops.separable_grad(G0, T, G0, objective)
            SO.sub_(G0)

        legs = {k: f for k, f in (("a", push), ("b", plain), ("c", composed)) if k in a.legs}
        for _ in range(a.warmup):  # clocks up, code objects loaded
            for f in legs.values():
                f()
        torch.cuda.synchronize()
        same = None
        if "a" in legs and "c" in legs:
            composed()
            want = (UO[rows].clone(), SO[rows].clone(), av[:, 0].clone())
            push()
            same = same_bits(UO[rows], want[0]) and same_bits(SO[rows], want[1]) and same_bits(vo, want[2])
        t = {k: [] for k in legs}
        for _ in range(a.reps):
            for k, f in legs.items():
                t[k].append(timed(f, a.inner))
        m = {k: median(x) for k, x in t.items()}
        r = {"agents": n, "params": P, "ld": ld, "graph": f"random 4-regular, seed {a.seed}, out-degree weights",
             "objective": objective, "lr": lr, "bits_equal_composed_sample": same, "note": a.note}
        for k, name in (("a", "gt_push_csr"), ("b", "gt_csr"), ("c", "composed")):
            if k in m:
                r[name + "_ms"], r[name + "_all"] = m[k], t[k]
        if "a" in m:
            r["frac"] = 5 * n * P * 4 / (m["a"] / 1e3) / PEAK
            if "b" in m:
                r["a_over_b"] = m["a"] / m["b"]
                r["a_over_b_pairs"] = [x / y for x, y in zip(t["a"], t["b"])]
                r["b_spread"] = max(t["b"]) / min(t["b"])
            if "c" in m:
                r["a_over_c"] = m["a"] / m["c"]
        line = json.dumps(r)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()


if __name__ == "__main__":
    main()
