"""The gradient-fed exact rounds (ops.gt_grad_csr, ops.extra_grad_csr,
dolhip.ExactMLPGossip) against their yardsticks, in one process on the same
buffers, legs alternating.  A random 4-regular graph (--seed) with Metropolis
weights; rows of --params floats, the bank's stride apart (bank.row_stride: 1024
x 101,770 is config 5's bank); ms by HIP events after a warm-up, per window of
--inner calls, --reps windows per leg, medians, and every window kept.
  (a) one ops.gt_grad_csr call: X and S gathered, G and Gprev in, X' and S' out
      (six streams);
  (b) one ops.gt_csr call on the same bank, least squares (five streams);
  (c) (a)'s round composed from existing ops: two ops.mix_csr calls and torch
      elementwise ops into (a)'s output matrices and one scratch matrix.  A
      sample of 64 rows is compared with (a)'s (`bits_equal_composed_sample`;
      torch's scaled add is not pinned to be an fma: recorded, not required);
  (d) one ops.extra_grad_csr call (X gathered, G and corr in, X' and corr out);
  (e) one ops.extra_csr call on the same bank, least squares (the same streams);
  (f) (d)'s round composed from ops.mix_csr, ops.prox_admm_sgd and torch
      elementwise ops, compared with (d) the same way.
The inputs are not swapped between calls (corr, updated in place, keeps
growing: finite and far from denormal, which is all a timing needs).  `frac` =
the leg's algorithmic bytes (6 or 5 N P 4) over its median as a share of 8 TB/s.
Two conditions are evaluated per row: `fed_beats_composed_every_pair` (a < c and
d < f in every pair of windows) and `gt_grad_over_1p2_gt_csr` with the spread of
its pairs (six streams to five).
  --mlp AGENTS: at AGENTS MLP agents 784-128-10, B = 32, one ExactMLPGossip
      round of each method (forward_backward + the fed round) against the
      existing round on the same graph, bank.mix with W_off + diag(d) as one CSR
      + BatchedMLP.step with momentum 0.
  python tools/grad_rounds_ab.py [--agents 1024] [--params 101770,1048576] [--mlp 1024] [--legs abcdef] [--reps 7] [--inner 10] [--note TEXT] [--out profiles/grad_rounds_ab.jsonl]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "distributed-optimization-and-learning_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from dolhip import AgentBank, ExactMLPGossip, graph as G, ops  # noqa: E402
from dolhip.bank import row_stride  # noqa: E402
from dolhip.mlp import BatchedMLP, mlp_layout  # noqa: E402
from gt_ab import PEAK, csr_dev, median, same_bits, timed  # noqa: E402

NAMES = {"a": "gt_grad_csr", "b": "gt_csr", "c": "gt_grad_composed", "d": "extra_grad_csr", "e": "extra_csr",
         "f": "extra_grad_composed"}
STREAMS = {"a": 6, "b": 5, "c": 6, "d": 5, "e": 5, "f": 5}


def emit(r, out):
    line = json.dumps(r)
    print(line, flush=True)
    if out:
        out.write(line + "\n")
        out.flush()


def alternate(legs, reps, inner, warmup):
    for f in legs.values():  # clocks up, code objects loaded
        for _ in range(warmup):
            f()
    torch.cuda.synchronize()
    t = {k: [] for k in legs}
    for _ in range(reps):
        for k, f in legs.items():
            t[k].append(timed(f, inner))
    return t


def spread(v):
    return max(v) - min(v)


def bank_main(a, n, P, out):
    dev = torch.device("cuda")
    lr, ld = a.lr, row_stride(P)
    w_off, d = G.metropolis_weights(G.random_regular_csr(n, 4, seed=a.seed))
    rp, col, val = csr_dev(w_off, dev)
    ws = torch.as_tensor(d, device=dev)

    def matrix():
        return torch.zeros(n, ld, device=dev)[:, :P]
    g = torch.Generator(device=dev).manual_seed(9)
    X, S, Gr, Gp, T, C, XO, SO, tmp = (matrix() for _ in range(9))
    for m in (X, S, Gr, Gp, T):
        m.normal_(generator=g)
    rows = torch.arange(0, n, max(1, n // 64), device=dev)[:64]  # of the composed rounds' comparisons

    def gt_composed():
        ops.mix_csr(X, XO, rp, col, val)
        ops.mix_csr(S, SO, rp, col, val)
        torch.mul(X, ws[:, None], out=tmp)
        XO.add_(tmp)  # ax
        torch.mul(S, ws[:, None], out=tmp)
        SO.add_(tmp)  # as
        SO.add_(Gr)
        SO.sub_(Gp)  # s'
        XO.add_(SO, alpha=-lr)  # x'

    def extra_composed():
        ops.mix_csr(X, XO, rp, col, val)
        torch.mul(X, ws[:, None], out=tmp)
        XO.add_(tmp)  # ax
        torch.sub(X, XO, out=tmp)  # r
        ops.prox_admm_sgd(XO, Gr, lr=lr, write_grad=False)  # elementwise: fma(-lr, g, ax)
        XO.sub_(C)
        C.add_(tmp, alpha=0.5)

    legs = {
        "a": lambda: ops.gt_grad_csr(X, S, XO, SO, rp, col, val, Gr, Gp, self_weight=ws, lr=lr),
        "b": lambda: ops.gt_csr(X, S, XO, SO, rp, col, val, T, self_weight=ws, lr=lr),
        "c": gt_composed,
        "d": lambda: ops.extra_grad_csr(X, XO, rp, col, val, Gr, C, self_weight=ws, lr=lr),
        "e": lambda: ops.extra_csr(X, XO, rp, col, val, T, C, self_weight=ws, lr=lr),
        "f": extra_composed,
    }
    legs = {k: f for k, f in legs.items() if k in a.legs}
    same_gt = same_extra = None
    if "a" in legs and "c" in legs:
        gt_composed()
        want = (XO[rows].clone(), SO[rows].clone())
        legs["a"]()
        same_gt = same_bits(XO[rows], want[0]) and same_bits(SO[rows], want[1])
    if "d" in legs and "f" in legs:
        C.zero_()
        extra_composed()
        want = (XO[rows].clone(), C[rows].clone())
        C.zero_()
        legs["d"]()
        same_extra = same_bits(XO[rows], want[0]) and same_bits(C[rows], want[1])
    C.zero_()
    t = alternate(legs, a.reps, a.inner, a.warmup)
    m = {k: median(x) for k, x in t.items()}
    r = {"part": "bank", "agents": n, "params": P, "ld": ld,
         "graph": f"random 4-regular, seed {a.seed}, Metropolis weights", "lr": lr, "reps": a.reps, "inner": a.inner,
         "bits_equal_composed_sample": {"gt_grad": same_gt, "extra_grad": same_extra}, "note": a.note}
    for k in legs:
        r[NAMES[k] + "_ms"], r[NAMES[k] + "_all"] = m[k], t[k]
        r[NAMES[k] + "_frac"] = STREAMS[k] * n * P * 4 / (m[k] / 1e3) / PEAK
    for num, den in (("a", "b"), ("a", "c"), ("d", "e"), ("d", "f")):
        if num in m and den in m:
            pairs = [x / y for x, y in zip(t[num], t[den])]
            r[f"{NAMES[num]}_over_{NAMES[den]}"] = m[num] / m[den]
            r[f"{NAMES[num]}_over_{NAMES[den]}_pairs"] = pairs
    beats = [x < y for num, den in (("a", "c"), ("d", "f")) if num in t and den in t for x, y in zip(t[num], t[den])]
    r["fed_beats_composed_every_pair"] = all(beats) if beats else None
    if "a" in t and "b" in t:
        pairs = r["gt_grad_csr_over_gt_csr_pairs"]
        r["gt_grad_over_1p2_gt_csr"] = {"median_ratio": median(pairs), "pair_spread": spread(pairs),
                                        "slower_than_1p2_by_more_than_the_spread": median(pairs) - 1.2 > spread(pairs)}
    emit(r, out)
    del X, S, Gr, Gp, T, C, XO, SO, tmp
    torch.cuda.empty_cache()


def mlp_main(a, n, out):
    dev = torch.device("cuda")
    d_in, h, c, B, lr = 784, 128, 10, 32, 0.05
    w_off, d = G.metropolis_weights(G.random_regular_csr(n, 4, seed=a.seed))
    plan = G.MixingPlan(w_off, dev, allow_ring=False)
    full = G.MixingPlan(G.csr_from_dense(w_off.dense() + np.diag(d).astype(np.float32)), dev, allow_ring=False)
    g = torch.Generator(device=dev).manual_seed(9)
    Xb = torch.randn(n, B, d_in, generator=g, device=dev)
    yb = torch.randint(0, c, (n, B), generator=g, device=dev, dtype=torch.int64)
    sims = {m: ExactMLPGossip(plan, d_in, h, c, method=m, lr=lr, self_weight=d) for m in ("gt", "extra")}
    for s in sims.values():
        s.batch(Xb, yb)
    bank = AgentBank(n, mlp_layout(d_in, h, c), dev)
    bank.rows()[:] = sims["gt"].params()
    bank.buffer("y").zero_()
    mlp = BatchedMLP(bank, d_in, h, c)

    def existing():
        bank.mix(full)
        mlp.step(Xb, yb, lr=lr, momentum=0.0, first_step=False)

    legs = {"exact_gt_round": sims["gt"].round, "exact_extra_round": sims["extra"].round,
            "mix_plus_step": existing, "forward_backward": lambda: sims["gt"].mlp.forward_backward(Xb, yb)}
    t = alternate(legs, a.reps, a.inner, a.warmup)
    m = {k: median(x) for k, x in t.items()}
    r = {"part": "mlp", "agents": n, "mlp": [d_in, h, c], "batch": B, "params": bank.P, "ld": bank.ld,
         "graph": f"random 4-regular, seed {a.seed}, Metropolis weights", "lr": lr, "reps": a.reps, "inner": a.inner,
         "note": a.note}
    for k in legs:
        r[k + "_ms"], r[k + "_all"] = m[k], t[k]
    for k in ("exact_gt_round", "exact_extra_round"):
        r[k + "_over_mix_plus_step"] = m[k] / m["mix_plus_step"]
        r[k + "_over_mix_plus_step_pairs"] = [x / y for x, y in zip(t[k], t["mix_plus_step"])]
    emit(r, out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=1024)
    ap.add_argument("--params", default="101770,1048576", help="comma-separated row lengths; empty: skip the bank legs")
    ap.add_argument("--mlp", type=int, default=1024, help="agents of the MLP part; 0: skip it")
    ap.add_argument("--seed", type=int, default=2028, help="of the random 4-regular graph")
    ap.add_argument("--lr", type=float, default=0.1)
    ap.add_argument("--legs", default="abcdef")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10, help="calls per timed window")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--note", default=None, help="free text kept in every row (e.g. the build measured)")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    a = ap.parse_args()
    out = open(a.out, "a") if a.out else None
    for P in (int(p) for p in a.params.split(",") if p):
        bank_main(a, a.agents, P, out)
    if a.mlp:
        mlp_main(a, a.mlp, out)


if __name__ == "__main__":
    main()
