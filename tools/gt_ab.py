"""The gradient-tracking round of one layout, fused against composed and against
its yardsticks, in one process on the same buffers, legs alternating.  Both
objectives; ms by HIP events after a warm-up, per window of --inner calls,
--reps windows per leg, medians; `frac` = 5 N P 4 bytes over the fused leg's
median as a share of 8 TB/s.  Before timing, the fused X' and S' are compared
bit for bit with the other legs' where those run (`bits_equal`).  --note
records what build was measured.  One JSON row per objective; the rows of each
layout keep the keys of its file under profiles/.

--layout pm: the parameter-major bank, a random 4-regular W (seed 2028) with
Metropolis weights, so W = W_off + diag(d) (profiles/gt_pm_ab.jsonl):
  (a) the round composed from the other ops: two ops.mix_csr_pm (X and S), the
      self-weight terms (a multiply and an add each), x' by ops.prox_admm_sgd
      (fma(-lr, s, ax)), ops.separable_grad twice, an add and a subtract;
  (b) one ops.gt_csr_pm call (dol_gt_csr_pm_f32: X, S, T in, X', S' out);
  (c) the ops.dgd_csr_pm least-squares momentum round on the same X / Y / T
      buffers: the same five streams (X, T, M in, Y, M out), the yardstick for
      what this kernel structure reaches on the box at hand.
  `b_over_a`, `b_over_c`; (b)'s X' and S' are compared with (a)'s on the whole
  bank.
  python tools/gt_ab.py --layout pm --agents 1024 [--params 1048576] [--reps 5] [--inner 10] [--legs abc] [--note TEXT] [--out profiles/x.jsonl]

--layout ring: the agent-major ring with Metropolis weights (1/3, 1/3 and a self
weight of 1/3; profiles/gt_ring_ab.jsonl).  --layout csr: the agent-major CSR
bank, a random 4-regular graph (--seed) with Metropolis weights (1/5 per edge
and a self weight of 1/5; profiles/gt_csr_ab.jsonl; the recorded runs: --agents
1024, and --agents 8192 --pad 2048).  ld = --params + --pad.
  (a) one ops.gt_ring / ops.gt_csr call (X, S, T in, X', S' out);
  (b) the round composed as above from two ops.mix_ring / ops.mix_csr -- at
      least fourteen row streams against (a)'s five.  Ring: into two matrices of
      its own and one scratch, compared with (a)'s on the whole bank.  CSR: into
      (a)'s output matrices and one scratch, so a sample of 64 rows is kept and
      compared;
  (c) ops.dgd_ring (momentum 0.9) / ops.dgd_csr (momentum 0.5) on the same bank:
      the same five streams (X, T, mom in, Y, mom out) through
      ring_mix_dma_kernel / csr_xcd_kernel, the yardstick for "these bytes at
      the mix's rate" on the box at hand; least squares only;
  (d) ops.gt_csr_pm on the same graph and values in the parameter-major layout
      (five more matrices; at most ops.GT_MAX_AGENTS agents, skipped beyond),
      all of it compared with (a).
  The legs alternate, so window i of (a) and of another leg are an A/B pair:
  `a_over_c_pairs` with (c)'s own spread max / min beside it, and on the CSR
  bank `a_over_b_pairs`.  (Tile heights, block orders and tile widths were
  compared as builds of their own, see csrc/gt_ring.hip and csrc/gt_csr.hip.)
  python tools/gt_ab.py --layout ring|csr --agents 1024 [--params 1048576] [--pad 0] [--legs abcd] [--objectives least_squares,logistic] [--reps 5] [--inner 10] [--note TEXT] [--out profiles/x.jsonl]
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
from dolhip.synthetic import ring_gt_weights  # noqa: E402

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


def csr_dev(c, dev):
    return tuple(torch.as_tensor(np.asarray(x, t), device=dev)
                 for x, t in ((c.rowptr, np.int32), (c.col, np.int32), (c.val, np.float32)))


def ring_csr(n):
    """The n-agent ring's pattern as a CSR (values unused: ring_gt_weights takes the pattern)."""
    i = np.arange(n)
    col = np.sort(np.stack([(i - 1) % n, (i + 1) % n], 1), 1).reshape(-1).astype(np.int32)
    return G.CSR(n, n, (2 * np.arange(n + 1)).astype(np.int32), col, np.ones(2 * n, np.float32))


def composed_round(mix, X, S, T, ws, CX, CS, G0, objective, lr):
    """X', S' into CX, CS from the other ops (G0 scratch); ws broadcasts against X."""
    mix(X, CX)
    mix(S, CS)
    torch.mul(X, ws, out=G0)
    CX.add_(G0)
    torch.mul(S, ws, out=G0)
    CS.add_(G0)
    ops.prox_admm_sgd(CX, S, lr=lr, write_grad=False)  # elementwise: x' = fma(-lr, s, ax)
    ops.separable_grad(CX, T, G0, objective)
    CS.add_(G0)
    ops.separable_grad(X, T, G0, objective)
    CS.sub_(G0)


def pm_layout(a, dev):
    """(objectives, round(objective) -> (legs, check), row(objective, same, m, t)) on the parameter-major bank."""
    n, P, lr = a.agents, a.params, a.lr
    W, d = G.metropolis_weights(G.random_regular_csr(n, 4, seed=2028))
    rp, col, val = csr_dev(W, dev)
    ld = (n + 3) // 4 * 4
    dw = torch.zeros(ld, device=dev)
    dw[:n] = torch.as_tensor(d, device=dev)
    g = torch.Generator(device=dev).manual_seed(9)
    XT, TT = torch.zeros(P, ld, device=dev), torch.zeros(P, ld, device=dev)
    XT[:, :n].normal_(generator=g)
    TT[:, :n].normal_(generator=g)
    ST, XO, SO = (torch.zeros_like(XT) for _ in range(3))
    if "a" in a.legs:
        AX, AS, G0 = (torch.zeros_like(XT) for _ in range(3))
    if "c" in a.legs:
        MT = torch.zeros_like(XT)

    def round_(objective):
        if objective == "logistic":  # targets +-feature
            TT.copy_(torch.where(torch.rand(TT.shape, generator=g, device=dev) < 0.5, -TT, TT))
        ops.separable_grad(XT, TT, ST, objective)

        def composed():
            composed_round(lambda A, Y: ops.mix_csr_pm(A, Y, rp, col, val), XT, ST, TT, dw, AX, AS, G0, objective, lr)

        def fused():
            ops.gt_csr_pm(XT, ST, XO, SO, rp, col, val, TT, self_weight=dw[:n], objective=objective, lr=lr)

        def dgd():
            ops.dgd_csr_pm(XT, XO, rp, col, val, TT, MT, objective="least_squares", lr=0.01, momentum=0.9)

        def check(legs):
            if "a" not in legs or "b" not in legs:
                return None
            composed()
            fused()
            return same_bits(AX[:, :n], XO[:, :n]) and same_bits(AS[:, :n], SO[:, :n])
        return {k: f for k, f in (("a", composed), ("b", fused), ("c", dgd)) if k in a.legs}, check

    def row(objective, same, m, t):
        r = {"agents": n, "params": P, "objective": objective, "lr": lr, "bits_equal": same, "note": a.note}
        for k, name in (("a", "composed"), ("b", "fused"), ("c", "dgd_ls_momentum")):
            if k in m:
                r[name + "_ms"], r[name + "_all"] = m[k], t[k]
        if "b" in m:
            r["frac"] = 5 * n * P * 4 / (m["b"] / 1e3) / PEAK
            if "a" in m:
                r["b_over_a"] = m["b"] / m["a"]
            if "c" in m:
                r["b_over_c"] = m["b"] / m["c"]
        return r
    return ("least_squares", "logistic"), round_, row


def am_layout(a, dev):
    """The same on the agent-major bank: the ring (a.layout == "ring") or a random 4-regular graph."""
    ring = a.layout == "ring"
    n, P, lr, ld = a.agents, a.params, a.lr, a.params + a.pad
    legs_asked = "".join(k for k in a.legs if not (k == "d" and n > ops.GT_MAX_AGENTS))
    pattern = ring_csr(n) if ring else G.random_regular_csr(n, 4, seed=a.seed)
    w_off, d = G.metropolis_weights(pattern)
    rp, col, val = csr_dev(w_off, dev)
    ws = torch.as_tensor(d, device=dev)
    if ring:
        wp, wn = (torch.as_tensor(w, device=dev) for w in ring_gt_weights(pattern)[:2])

    def matrix():
        return torch.zeros(n, ld, device=dev)[:, :P]
    g = torch.Generator(device=dev).manual_seed(9)
    X, T, S, XO, SO = (matrix() for _ in range(5))
    X.normal_(generator=g)
    T.normal_(generator=g)
    if "b" in legs_asked:
        CX, CS, G0 = (matrix(), matrix(), matrix()) if ring else (XO, SO, matrix())
    if "d" in legs_asked:
        ldp = (n + 3) // 4 * 4
        XT, ST, TT, XOT, SOT = (torch.zeros(P, ldp, device=dev) for _ in range(5))
        back = matrix()
    rows = slice(None) if ring else torch.arange(0, n, max(1, n // 64), device=dev)[:64]  # of (b)'s comparison

    def round_(objective):
        if objective == "logistic":  # targets +-feature
            for r in range(0, n, 256):  # in row blocks: no bank-sized temporaries
                blk = T[r:r + 256]
                blk.mul_(torch.where(torch.rand(blk.shape, generator=g, device=dev) < 0.5, -1.0, 1.0))
        ops.separable_grad(X, T, S, objective)
        if "d" in legs_asked:
            for src, dst in ((X, XT), (S, ST), (T, TT)):
                ops.transpose(src, dst, n, P)

        def fused():
            if ring:
                ops.gt_ring(X, S, XO, SO, wp, wn, T, self_weight=ws, objective=objective, lr=lr)
            else:
                ops.gt_csr(X, S, XO, SO, rp, col, val, T, self_weight=ws, objective=objective, lr=lr)

        def composed():
            mix = (lambda A, Y: ops.mix_ring(A, Y, wp, wn)) if ring else (lambda A, Y: ops.mix_csr(A, Y, rp, col, val))
            composed_round(mix, X, S, T, ws[:, None], CX, CS, G0, objective, lr)

        def dgd():  # SO as the momentum buffer: read and written, like S' -- (a) rewrites it before it is compared
            if ring:
                ops.dgd_ring(X, XO, wp, wn, T, mom=SO, objective="least_squares", lr=0.01, momentum=0.9)
            else:
                ops.dgd_csr(X, XO, rp, col, val, T, mom=SO, objective="least_squares", lr=0.01, momentum=0.5)

        def pm():
            ops.gt_csr_pm(XT, ST, XOT, SOT, rp, col, val, TT, self_weight=ws, objective=objective, lr=lr)

        def check(legs):
            same = {}
            if "a" in legs:
                if "b" in legs:
                    composed()
                    want = (CX, CS) if ring else (XO[rows].clone(), SO[rows].clone())
                fused()
                if "b" in legs:
                    same["b"] = same_bits(XO[rows], want[0]) and same_bits(SO[rows], want[1])
                if "d" in legs:
                    pm()
                    same["d"] = same_bits(ops.transpose(XOT, back, P, n), XO) and \
                        same_bits(ops.transpose(SOT, back, P, n), SO)
            return same
        return {k: f for k, f in (("a", fused), ("b", composed), ("c", dgd), ("d", pm))
                if k in legs_asked and not (k == "c" and objective != "least_squares")}, check

    def row(objective, same, m, t):
        r = {"agents": n, "params": P, "ld": ld}
        if not ring:
            r["graph"] = f"random 4-regular, seed {a.seed}, Metropolis weights"
        r.update(objective=objective, lr=lr, bits_equal=same, note=a.note)
        for k, name in (("a", "fused"), ("b", "composed"), ("c", f"dgd_{a.layout}_momentum"), ("d", "gt_csr_pm")):
            if k in m:
                r[name + "_ms"], r[name + "_all"] = m[k], t[k]
        if "a" in m:
            r["frac"] = 5 * n * P * 4 / (m["a"] / 1e3) / PEAK
            if "b" in m:
                r["a_over_b"] = m["a"] / m["b"]
                if not ring:
                    r["a_over_b_pairs"] = [x / y for x, y in zip(t["a"], t["b"])]
            if "c" in m:
                r["a_over_c"] = m["a"] / m["c"]
                r["a_over_c_pairs"] = [x / y for x, y in zip(t["a"], t["c"])]
                r["c_spread"] = max(t["c"]) / min(t["c"])
            if "d" in m:
                r["a_over_d"] = m["a"] / m["d"]
        return r
    return a.objectives.split(","), round_, row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layout", required=True, choices=("pm", "ring", "csr"))
    layout = ap.parse_known_args()[0].layout
    ap.add_argument("--agents", type=int, default=1024)
    ap.add_argument("--params", type=int, default=1 << 20)
    ap.add_argument("--lr", type=float, default=0.1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10, help="calls per timed window")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--note", default=None, help="free text kept in every row (e.g. the build measured)")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    if layout == "pm":
        ap.add_argument("--legs", default="abc", help="which legs to time (the bit comparison needs a and b)")
    else:
        ap.add_argument("--legs", default="abcd")
        ap.add_argument("--pad", type=int, default=0, help="ld = params + pad")
        ap.add_argument("--objectives", default="least_squares,logistic")
    if layout == "csr":
        ap.add_argument("--seed", type=int, default=2028, help="of the random 4-regular graph")
    a = ap.parse_args()
    dev = torch.device("cuda")
    out = open(a.out, "a") if a.out else None
    objectives, round_, row = (pm_layout if layout == "pm" else am_layout)(a, dev)
    for objective in objectives:
        legs, check = round_(objective)
        for _ in range(a.warmup):  # clocks up, stage order tuned for the buffer pairs, code objects loaded
            for f in legs.values():
                f()
        torch.cuda.synchronize()
        same = check(legs)
        t = {k: [] for k in legs}
        for _ in range(a.reps):
            for k, f in legs.items():
                t[k].append(timed(f, a.inner))
        line = json.dumps(row(objective, same, {k: median(v) for k, v in t.items()}, t))
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()


if __name__ == "__main__":
    main()
