"""The boundary rows of a sharded ring block's gradient-tracking round: one
ops.gt_ring_edges call (dol_gt_ring_edges_f32) against the two one-row
ops.gt_ring calls it replaces in ShardedRing.gt_step, in one process on the
same buffers, legs alternating.  A block of --rows rows of --params floats, ld =
params + pad, Metropolis ring weights (1/3, 1/3 and a self weight of 1/3),
four halo rows of their own.  Both objectives; ms per call by HIP events over
windows of --inner back-to-back calls after a warm-up, --reps windows per leg,
medians, and the ratio of each alternating pair with the spread of each leg
(max / min) beside it.  Before timing, rows 0 and rows - 1 of the two legs are
compared bit for bit.  The calls are a few tens of microseconds, so a window
times the host's enqueue rate as much as the kernels: that is what a round
pays.  One JSON row per objective (profiles/gt_ring_edges_ab.jsonl).

  python tools/gt_edges_ab.py [--rows 1024] [--params 1048576] [--pad 2048] [--reps 7] [--inner 200] [--note TEXT] [--out profiles/x.jsonl]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "distributed-optimization-and-learning_amd"))

import torch  # noqa: E402

from dolhip import ops  # noqa: E402


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
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--params", type=int, default=1 << 20)
    ap.add_argument("--pad", type=int, default=2048, help="ld = params + pad")
    ap.add_argument("--lr", type=float, default=0.1)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=200, help="calls per timed window")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--objectives", default="least_squares,logistic")
    ap.add_argument("--note", default=None, help="free text kept in every row (e.g. the build measured)")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    a = ap.parse_args()
    dev = torch.device("cuda")
    n, P, ld, lr = a.rows, a.params, a.params + a.pad, a.lr
    if n < 2:
        raise SystemExit("--rows must be >= 2 (two boundary rows)")
    g = torch.Generator(device=dev).manual_seed(9)
    X, S, T, XO, SO, XR, SR = (torch.zeros(n, ld, device=dev)[:, :P] for _ in range(7))
    touched = sorted({0, 1, n - 2, n - 1})
    for M in (X, S, T):
        for r in touched:
            M[r].normal_(generator=g)
    H = torch.randn(4, ld, generator=g, device=dev)
    halos = tuple(H[k, :P] for k in range(4))
    wp, wn, ws = (torch.full((n,), 1.0 / 3.0, device=dev) for _ in range(3))
    out = open(a.out, "a") if a.out else None
    for objective in a.objectives.split(","):
        if objective == "logistic":  # targets +-feature
            for r in touched:
                T[r].mul_(torch.where(torch.rand(P, generator=g, device=dev) < 0.5, -1.0, 1.0))
        kw = dict(objective=objective, lr=lr, P=P)

        def one_launch():
            ops.gt_ring_edges(X, S, XO, SO, wp, wn, T, halos, self_weight=ws, n_rows=n, **kw)

        def two_calls(XO=XR, SO=SR):
            ops.gt_ring(X[0:1], S[0:1], XO[0:1], SO[0:1], wp[0:1], wn[0:1], T[0:1], self_weight=ws[0:1],
                        halos=(halos[0], X[1], halos[2], S[1]), n_rows=1, **kw)
            ops.gt_ring(X[n - 1:n], S[n - 1:n], XO[n - 1:n], SO[n - 1:n], wp[n - 1:n], wn[n - 1:n], T[n - 1:n],
                        self_weight=ws[n - 1:n], halos=(X[n - 2], halos[1], S[n - 2], halos[3]), n_rows=1, **kw)

        legs = {"a": one_launch, "b": two_calls}
        for _ in range(a.warmup):
            for f in legs.values():
                f()
        torch.cuda.synchronize()
        edge = [0, n - 1]
        same = same_bits(XO[edge].contiguous(), XR[edge].contiguous()) and \
            same_bits(SO[edge].contiguous(), SR[edge].contiguous()) and bool(XO[edge].abs().sum() > 0)
        t = {k: [] for k in legs}
        for _ in range(a.reps):
            for k, f in legs.items():
                t[k].append(timed(f, a.inner))
        row = {"rows": n, "params": P, "ld": ld, "objective": objective, "lr": lr, "bits_equal": same,
               "inner": a.inner, "note": a.note,
               "edges_ms": median(t["a"]), "edges_all": t["a"], "two_calls_ms": median(t["b"]), "two_calls_all": t["b"],
               "a_over_b": median(t["a"]) / median(t["b"]),
               "a_over_b_pairs": [x / y for x, y in zip(t["a"], t["b"])],
               "a_spread": max(t["a"]) / min(t["a"]), "b_spread": max(t["b"]) / min(t["b"])}
        line = json.dumps(row)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()


if __name__ == "__main__":
    main()
