"""Gradient tracking on the agent-major CSR bank (dol_gt_csr_f32, ops.gt_csr,
MixingPlan.apply_gt, SeparableGTCSR, ColumnSharded.gt_step), CPU tier: nothing
is launched.

* The surface: the SIGNATURES row, the ops re-export, the package export.
* Every argument rule of the entry point, called through the library with
  addresses that are never dereferenced (each refusal returns before a launch
  and names the entry), and DOL_OK for the empty shapes.
* MixingPlan.apply_gt's routing by kind and SeparableGTCSR's refusals, with
  ops._native.call replaced by test_ops_args_gpu.Recorder.  (The rules of
  ops.gt_csr that a CPU tensor can reach are the ones it shares with
  ops.gt_csr_pm and ops.gt_ring: tests/test_gt_host.py.  A CPU matrix is refused
  before the square-W and row-count rules are looked at; those and the accepted
  call's argument tuple are pinned with the Recorder on device tensors in
  tests/test_gt_csr_gpu.py.)
* ColumnSharded.gt_step with tests/gt_cases.py::gt_round injected as the
  arithmetic: world 1 in-process, worlds 2 and 3 over gloo; the gathered
  parameters and trackers equal the unsharded host rounds bit for bit.
* The launch geometry and indexing of csrc/gt_csr.hip restated in the manner
  of tests/test_kernel_extents.py: gt_csr_xcd_kernel<R, 32, 2, OBJ, SELF> (from
  512 rows and 32 f4 columns: grid cdiv(nt, 8) * 8 * cdiv(n, 16), tile = (b >>
  3) / nrb * 8 + (b & 7); rows clamped to n - 1 for rowptr, the gathers, the
  centre rows and the target row; stores r < n) and gt_csr_kernel<R, f4 /
  float, OBJ, SELF> (the columns the pinned tiles leave over, small graphs,
  scalar columns: 16 rows per block, row group fastest).  Both entry points
  run these kernels (R = GtPlain for dol_gt_csr_f32, GtPushSum for
  dol_gt_push_csr_f32); the push-sum round also reads v and v_out at the rows
  of the self weights, after gt_push_v_kernel (one thread per row).  Every
  buffer's touched range must lie in [0, n * ld), or [0, n) for a vector: on
  an exact-size mapped block an over-read faults.
* The emitted code: 2 rounds x 2 objectives x 2 self-weight forms of each
  kernel form and the 2 forms of gt_push_v_kernel, none with a private segment
  (no scratch).
* tests/gt_cases.py::gt_round replayed on the 16-agent random 4-regular graph
  with Metropolis weights, least squares, lr 0.1, 200 rounds, P = 8: every
  agent within 1e-5 of the mean of the targets, where DGD with the same W and
  lr stays above it."""
import functools
import os
import re
import socket
import subprocess
import types

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import dolhip
import gt_cases
import oracle
from dolhip import _native, graph as G, gt, ops, parallel
from dolhip.bank import row_stride
from dolhip.synthetic import SeparableGT, SeparableGTCSR
from test_codegen_pins import LLVM, _kernels, _unbundle
from test_kernel_extents import KT, Ext, cdiv
from test_ops_args_gpu import mat, vec

CPU = torch.device("cpu")
F32 = np.float32
I32 = torch.int32
RPB = 16           # kRows, and the rows of one block of the pinned kernel ((256 / XW) * XPASSES)
XW, XPASSES = 32, 2  # the pinned tile: 32 f4 = 512 B of a row
MIN_XCD_ROWS = 512   # kMinXcdRows


# ---------------------------------------------------------------------------
# the surface
# ---------------------------------------------------------------------------
def test_surface():
    assert len(_native.SIGNATURES["dol_gt_csr_f32"]) == 19
    assert ops.gt_csr is gt.gt_csr and "gt_csr" not in ops.__all__
    assert dolhip.SeparableGTCSR is SeparableGTCSR and issubclass(SeparableGT, SeparableGTCSR)
    assert callable(G.MixingPlan.apply_gt) and callable(parallel.ColumnSharded.gt_step)


# ---------------------------------------------------------------------------
# the entry point's argument rules, without a launch
# ---------------------------------------------------------------------------
def test_entry_point_checks_arguments_without_launch():
    L = _native.lib()
    fake = 1 << 20  # never dereferenced: every call below returns from its argument checks
    X, S, XO, SO, T, RP, COL, VAL, WS = (fake + (k << 16) for k in range(9))

    def call(x=X, s=S, xo=XO, so=SO, n=8, P=8, ld=8, lds=None, ldxo=None, ldso=None, ldt=None, rp=RP, col=COL,
             val=VAL, ws=None, t=T, objective=0):
        pick = lambda v: ld if v is None else v  # noqa: E731
        return L.dol_gt_csr_f32(x, ld, s, pick(lds), xo, pick(ldxo), so, pick(ldso), n, P, rp, col, val, ws, t,
                                pick(ldt), objective, 0.1, None)

    def refused(word, **kw):
        assert call(**kw) == -1, kw
        msg = L.dol_last_error()
        assert b"dol_gt_csr_f32" in msg and word in msg, (kw, msg)

    for name in ("x", "s", "xo", "so", "t", "rp", "col", "val"):  # self_w alone may be null
        refused(b"null pointer", **{name: None})
        refused(b"null pointer", ws=WS, **{name: None})
    for name in ("ld", "lds", "ldxo", "ldso", "ldt"):
        refused(b"ld < P", **{name: 7})
    for kw in (dict(s=X), dict(xo=X), dict(so=X), dict(xo=S), dict(so=S), dict(so=XO)):
        refused(b"alias", **kw)
    refused(b"objective must be 0 or 1", objective=2)
    refused(b"objective must be 0 or 1", objective=-1)
    refused(b"too large", n=1 << 20, P=1 << 40, ld=1 << 40)  # 2^30 column tiles x 2^16 row groups
    refused(b"too large", n=(1 << 28) + 16, P=1, ld=1)  # the scalar kernel's grid: 1 x (2^24 + 1)
    refused(b"too large", n=(1 << 28) + 16, P=1, ld=1, ws=WS)
    refused(b"negative size", n=-1)
    refused(b"negative size", P=-1)
    refused(b"size above 2^40", ld=(1 << 40) + 4)
    # nothing to do: DOL_OK whatever else is passed, nothing launched
    assert call(n=0) == 0 and call(P=0) == 0 and call(n=0, x=None, objective=5) == 0
    assert L.dol_last_error() == b""


# ---------------------------------------------------------------------------
# ops.gt_csr, MixingPlan.apply_gt and SeparableGTCSR, before the library is reached
# ---------------------------------------------------------------------------
@pytest.fixture
def rec(monkeypatch):
    return gt_cases.recorder(monkeypatch)


def _ring_pattern(n):
    torch.manual_seed(2028)
    return G.communication_csr("circle", "stochastic", n)[0]


def test_apply_gt_routes_by_kind(monkeypatch, rec):
    seen = []
    monkeypatch.setattr(ops, "gt_ring", lambda *a, **k: seen.append(("gt_ring", a, k)) or (a[2], a[3]))
    monkeypatch.setattr(ops, "gt_csr", lambda *a, **k: seen.append(("gt_csr", a, k)) or (a[2], a[3]))
    monkeypatch.setattr(ops, "mix_csr_slab", lambda *a, **k: seen.append(("slab", a, k)))
    c9 = _ring_pattern(9)
    t = gt_cases.host_args("gt_csr", CPU, n=9)
    d = vec(CPU, 9)
    kw = dict(self_weight=d, objective="logistic", lr=0.5, P=10)
    five = (t["X"], t["S"], t["XO"], t["SO"])

    ring = G.MixingPlan(c9, CPU)
    assert ring.kind == "ring"
    out = ring.apply_gt(*five, t["target"], **kw)
    assert out[0] is t["XO"] and out[1] is t["SO"]
    name, a, k = seen.pop()
    assert name == "gt_ring" and all(x is y for x, y in zip(a, five + (ring.w_prev, ring.w_next, t["target"])))
    assert k == dict(kw, n_rows=9) and "halos" not in k  # the wrap-around ring

    csr = G.MixingPlan(c9, CPU, allow_ring=False)
    assert csr.kind == "csr"
    csr.apply_gt(*five, t["target"], **kw)
    name, a, k = seen.pop()
    assert name == "gt_csr" and k == kw
    assert all(x is y for x, y in zip(a, five + (csr.rowptr, csr.col, csr.val, t["target"])))

    csr.ent = csr.hdr = vec(CPU, 4, I32)  # a plan that carries a slab pack still runs gt_csr
    csr.apply_gt(*five, t["target"])
    assert seen.pop()[0] == "gt_csr" and seen == []

    dense = G.MixingPlan(c9, CPU, dense=True)
    with pytest.raises(NotImplementedError, match="gradient-tracking rounds are fused into the sparse mixes; use a "
                                                  "ring/CSR plan"):
        dense.apply_gt(*five, t["target"])
    csr._retire()
    with pytest.raises(RuntimeError, match="no longer holds its W"):
        csr.apply_gt(*five, t["target"])
    with pytest.raises(ValueError, match="X has 4 rows; W has 9 columns"):
        ring.apply_gt(*(mat(CPU, 4, 10, 12) for _ in range(5)))
    assert seen == [] and rec.calls == []


def test_problem_class_refusals(rec):
    c = G.random_regular_csr(8, 4, seed=1)
    with pytest.raises(ValueError, match="sparse"):
        SeparableGTCSR(G.MixingPlan(c, CPU, dense=True), 8)
    with pytest.raises(ValueError, match="objective must be one of"):
        SeparableGTCSR(G.MixingPlan(c, CPU), 8, objective="hinge")
    with pytest.raises(ValueError, match="self_weight: expected 8 weights"):
        SeparableGTCSR(G.MixingPlan(c, CPU), 8, self_weight=np.zeros(9, F32))
    # the ring-only subclass keeps its message; the base class takes the ring plan too
    with pytest.raises(ValueError, match="ring plan .got kind 'csr'.; SeparableGTPM"):
        SeparableGT(G.MixingPlan(c, CPU), 8)
    with pytest.raises(ValueError, match="objective must be one of"):
        SeparableGTCSR(G.MixingPlan(_ring_pattern(9), CPU), 8, objective="hinge")
    assert rec.calls == []


def test_problem_round_calls_apply_gt_and_swaps():
    """round() on stand-ins for the plan and the bank: one apply_gt call on
    (x, s, y, s_out, target), then both swaps."""
    calls = []
    prob = SeparableGTCSR.__new__(SeparableGTCSR)
    prob.plan = types.SimpleNamespace(apply_gt=lambda *a, **k: calls.append((a, k)))
    prob.bank = types.SimpleNamespace(buffer=lambda name: name, swap=lambda a, b: calls.append(("swap", a, b)))
    prob.self_weight, prob.objective, prob.lr, prob.P, prob.rounds = "d", "logistic", 0.5, 10, 0
    prob.round()
    assert calls == [(("x", "s", "y", "s_out", "target"), dict(self_weight="d", objective="logistic", lr=0.5, P=10)),
                     ("swap", "x", "y"), ("swap", "s", "s_out")]
    assert prob.rounds == 1


# ---------------------------------------------------------------------------
# ColumnSharded.gt_step with the host round injected
# ---------------------------------------------------------------------------
SH_N, SH_P, SH_ROUNDS = 24, 130, 3  # column cuts on 64 floats: (0, 130) / (0, 64, 130) / (0, 64, 128, 130)


def cpu_apply_gt(csr):
    """tests/gt_cases.py::gt_round with MixingPlan.apply_gt's signature."""
    def apply_gt(X, S, XO, SO, target, self_weight=None, objective="least_squares", lr=0.01, P=None):
        assert objective == "least_squares"
        n = csr.n_rows
        d = None if self_weight is None else self_weight.numpy()
        xn, sn = gt_cases.gt_round(X[:n, :P].numpy(), S[:n, :P].numpy(), target[:n, :P].numpy(), csr, d, lr)
        XO[:n, :P] = torch.from_numpy(xn)
        SO[:n, :P] = torch.from_numpy(sn)
        return XO, SO
    return apply_gt


def _sharded_problem():
    csr = G.random_regular_csr(SH_N, 4, seed=5)
    rng = np.random.default_rng(8)
    X, S, T = (rng.standard_normal((SH_N, SH_P)).astype(F32) for _ in range(3))
    return csr, np.linspace(0.05, 0.45, SH_N).astype(F32), X, S, T


def _sharded_rounds():
    """(x, s) gathered on rank 0 (None elsewhere) after SH_ROUNDS gt_step rounds."""
    csr, d, X, S, T = _sharded_problem()
    plan = type("Plan", (), {"n_rows": SH_N})()  # host stand-in: the arithmetic is injected
    sh = parallel.ColumnSharded(plan, SH_P, "cpu", apply=lambda *a, **k: None, apply_dgd=lambda *a, **k: None,
                                apply_gt=cpu_apply_gt(csr))
    cut = lambda A: torch.from_numpy(np.ascontiguousarray(A[:, sh.c0:sh.c1]))  # noqa: E731
    sh.x[:, :sh.Pl] = cut(X)
    s, t = cut(S), cut(T)
    s_out = torch.zeros_like(s)
    for _ in range(SH_ROUNDS):
        x_before = sh.x
        s, s_out = sh.gt_step(s, s_out, t, self_weight=torch.from_numpy(d), lr=0.1)
        assert sh.y is x_before
    return sh.gather(0), sh.gather(0, src=s)


def _unsharded_rounds():
    csr, d, X, S, T = _sharded_problem()
    for _ in range(SH_ROUNDS):
        X, S = gt_cases.gt_round(X, S, T, csr, d, 0.1)
    return X, S


def test_column_sharded_gt_step_in_one_process():
    x, s = _sharded_rounds()
    want_x, want_s = _unsharded_rounds()
    assert oracle.bits_equal(x.numpy(), want_x) and oracle.bits_equal(s.numpy(), want_s)


def test_column_sharded_gt_step_needs_an_entry():
    plan = types.SimpleNamespace(n_rows=6, n_cols=6, apply=lambda *a, **k: None, apply_dgd=lambda *a, **k: None)
    sh = parallel.ColumnSharded(plan, 10, "cpu")
    z = torch.zeros(6, sh.ld)
    with pytest.raises(NotImplementedError, match="gt_step"):
        sh.gt_step(z, z.clone(), z.clone())
    calls = []
    sh.set_plan(plan, apply_gt=lambda *a, **k: calls.append(k))
    sh.set_plan(plan)  # an injected entry survives set_plan
    assert sh.gt_step(z, z.clone(), z.clone(), lr=0.5)[1] is z and calls == [dict(P=10, lr=0.5)]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _gt_column_worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    parallel.init_process_group("gloo", rank=rank, world_size=world, timeout_s=120)
    try:
        x, s = _sharded_rounds()
        q.put((rank, None if x is None else x.numpy(), None if s is None else s.numpy()))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_column_sharded_gt_step_over_gloo(world):
    """Column cuts at 64 (and 128): every rank runs the round on its block, no
    data-path communication; the gathered result is the unsharded host round's."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_gt_column_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = {r: (x, s) for r, x, s in (q.get(timeout=120) for _ in range(world))}
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    want_x, want_s = _unsharded_rounds()
    assert oracle.bits_equal(res[0][0], want_x) and oracle.bits_equal(res[0][1], want_s)
    assert all(res[r] == (None, None) for r in range(1, world))


# ---------------------------------------------------------------------------
# extents: csrc/gt_csr.hip's geometry and indexing restated
# ---------------------------------------------------------------------------
def _row_neighbour_range(csr, n):
    """(lo, hi) per row: the lowest and highest neighbour row, the row itself where it has none."""
    rowptr, col = np.asarray(csr.rowptr, np.int64), np.asarray(csr.col, np.int64)
    lo, hi = np.arange(n, dtype=np.int64), np.arange(n, dtype=np.int64)
    has = np.diff(rowptr) > 0
    if has.any():
        starts = rowptr[:-1][has]
        lo[has] = np.minimum.reduceat(col, starts)
        hi[has] = np.maximum.reduceat(col, starts)
    assert col.size == 0 or (col.min() >= 0 and col.max() < n)
    return lo, hi


def _block_neighbour_range(csr, n):
    """The same per 16-row block (both kernel forms walk 16 rows per block)."""
    lo, hi = _row_neighbour_range(csr, n)
    starts = np.arange(0, n, RPB)
    return np.minimum.reduceat(lo, starts), np.maximum.reduceat(hi, starts)


def gt_csr_extents(n, P, ld, csr, vec_ok=True, push=False):
    """dol_gt_csr_f32 (push: dol_gt_push_csr_f32) -> gt_csr_xcd_kernel<R, 32, 2,
    *, *> over whole pinned tiles (from 512 rows), gt_csr_kernel<R, f4, *, *>
    over the f4 columns left, then gt_csr_kernel<R, float, *, *> over the scalar
    ones (all of them when !vec_ok).  push: gt_push_v_kernel first, and the
    main kernels read v and v_out at the rows where they read the self weights
    W."""
    e = Ext()
    blk_lo, blk_hi = _block_neighbour_range(csr, n)
    row_w = ("W", "v", "v_out") if push else ("W",)
    if push:  # gt_push_v_kernel: one thread per row r < n, cdiv(n, 256) blocks
        r = np.arange(cdiv(n, KT) * KT, dtype=np.int64)
        r = r[r < n]
        lo, hi = _row_neighbour_range(csr, n)
        e.add("rowptr", r, r + 1)
        e.add("v", np.minimum(lo[r], r), np.maximum(hi[r], r))  # v[col[e]] and v[r]
        e.add("W", r, r)
        e.add("v_out", r, r)
    n4, tail = (P // 4, P % 4) if vec_ok else (0, P)
    assert cdiv(n4, KT) * cdiv(n, RPB) <= 1 << 24 and cdiv(tail, KT) * cdiv(n, RPB) <= 1 << 24
    done4 = 0
    if n4 >= XW and n >= MIN_XCD_ROWS:
        nt = n4 // XW
        RB = (KT // XW) * XPASSES
        assert RB == RPB
        nrb = cdiv(n, RB)
        grid = cdiv(nt, 8) * 8 * nrb
        assert grid <= 8 << 24
        b = np.arange(grid, dtype=np.int64)
        xcd, local = b & 7, b >> 3
        ct, rb = (local // nrb) * 8 + xcd, local % nrb
        live = ct < nt
        ct, rb = ct[live], rb[live]
        assert np.unique(ct * nrb + rb).size == nt * nrb  # every (tile, row block) once
        c_lo, c_hi = 4 * ct * XW, 4 * (ct * XW + XW - 1) + 3  # element columns of the tile
        # rows rb * RB + j, j < RB, clamped to n - 1 for every load; stores only rows < n
        rc_lo, rc_hi = np.minimum(rb * RB, n - 1), np.minimum(rb * RB + RB - 1, n - 1)
        assert (rb * RB < n).all()
        e.add("rowptr", rc_lo, rc_hi + 1)
        for m in ("X", "S"):  # the gathers and the centre rows
            e.add(m, np.minimum(blk_lo[rb], rc_lo) * ld + c_lo, np.maximum(blk_hi[rb], rc_hi) * ld + c_hi)
        for m in row_w:
            e.add(m, rc_lo, rc_hi)
        for m in ("T", "XO", "SO"):  # the target rows (clamped) and the stores (r < n): the same rows
            e.add(m, rc_lo * ld + c_lo, rc_hi * ld + c_hi)
        done4 = nt * XW
    for V, c_off, ncols in ((4, done4 * 4, n4 - done4), (1, n4 * 4, tail)):
        if ncols <= 0:
            continue
        n_rg = cdiv(n, RPB)
        b = np.arange(cdiv(ncols, KT) * n_rg, dtype=np.int64)
        rg, ct = b % n_rg, b // n_rg
        r0, r1 = rg * RPB, np.minimum(rg * RPB + RPB, n)
        assert (r0 < r1).all()
        c_first, c_last = ct * KT, np.minimum(ct * KT + KT - 1, ncols - 1)  # lanes with c < ncols_v
        assert (c_first <= c_last).all()
        lo, hi = c_off + c_first * V, c_off + c_last * V + V - 1
        e.add("rowptr", r0, r1)
        for m in row_w:
            e.add(m, r0, r1 - 1)
        for m in ("X", "S"):
            e.add(m, np.minimum(blk_lo[rg], r0) * ld + lo, np.maximum(blk_hi[rg], r1 - 1) * ld + hi)
        for m in ("T", "XO", "SO"):
            e.add(m, r0 * ld + lo, (r1 - 1) * ld + hi)
    return e


def _sizes(n, ld):
    return dict({m: n * ld for m in ("X", "S", "T", "XO", "SO")}, rowptr=n + 1, W=n, v=n, v_out=n)


def _check_whole(e, n, P, ld, push=False):
    e.check(_sizes(n, ld))
    for m in ("T", "XO", "SO"):  # and nothing is left out
        assert e.r[m] == (0, (n - 1) * ld + P - 1), m
    assert e.r["rowptr"] == (0, n) and e.r["W"] == (0, n - 1)
    assert ("v" in e.r, "v_out" in e.r) == (push, push)
    if push:
        assert e.r["v"] == (0, n - 1) and e.r["v_out"] == (0, n - 1)


@pytest.mark.parametrize("n", [1024, 8192])
def test_extents_at_the_headline_shapes(n):
    """Exact-size mapped blocks: n * row_stride(P) floats per matrix."""
    P = 1 << 20
    ld = row_stride(P)
    csr = G.random_regular_csr(n, 4, seed=n + 3)
    for push in (False, True):
        _check_whole(gt_csr_extents(n, P, ld, csr, push=push), n, P, ld, push)


@functools.lru_cache(maxsize=None)
def _ragged_csr(n):
    return gt_cases.irregular(n, values=False) if n in (37, 520) else G.random_regular_csr(n, 4, seed=n + 3)


@pytest.mark.parametrize("P", [1, 7, 128, 131, 132, 300, 1031])
@pytest.mark.parametrize("n", [5, 16, 17, 33, 37, 512, 513, 520, 527, 4100])
def test_extents_at_ragged_shapes(n, P):
    """The shapes of tests/test_gt_csr_gpu.py: at ld = row_stride(P), at the
    tests' ld = round_up(P, 4), and with every column scalar (odd ld, or an
    unaligned base)."""
    csr = _ragged_csr(n)
    for push in (False, True):
        for ld, vec_ok in ((row_stride(P), True), ((P + 3) // 4 * 4, True), (P + 8 | 1, False), (P, False)):
            _check_whole(gt_csr_extents(n, P, ld, csr, vec_ok, push), n, P, ld, push)
        if P == 131 and n >= MIN_XCD_ROWS:  # one pinned tile, no left-over f4, a 3-float tail
            e = gt_csr_extents(n, P, 132, csr, push=push)
            assert e.r["X"][1] <= (n - 1) * 132 + 130


def test_extents_of_rows_past_element_2_pow_31():
    for n, ld in ((5, (1 << 29) + 64), (520, (1 << 22) + 64)):
        for push in (False, True):
            e = gt_csr_extents(n, 1031, ld, G.random_regular_csr(n, 4, seed=n + 3), push=push)
            e.check(_sizes(n, ld))
            assert e.r["SO"][1] == (n - 1) * ld + 1030 >= 1 << 31
            assert not push or e.r["v"] == e.r["v_out"] == (0, n - 1)


# ---------------------------------------------------------------------------
# the emitted code
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gt_csr_code_object(tmp_path_factory):
    return _unbundle("gt_csr.o", tmp_path_factory)


def _private_segment_sizes(co):
    """kernel name -> .private_segment_fixed_size of the code object's metadata"""
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True,
                           text=True).stdout
    sizes, name = {}, None
    for ln in notes.splitlines():
        m = re.match(r"\s*\.(name|private_segment_fixed_size):\s*(\S+)", ln)
        if m and m.group(1) == "name":
            name = m.group(2)
        elif m and name is not None:
            sizes[name] = int(m.group(2))
    return sizes


def test_gt_csr_kernels_are_counted_and_scratch_free(gt_csr_code_object):
    """{plain, push-sum} x {least squares, logistic} x {no self weights, self
    weights} of each kernel form: the pinned tiles, the 4 KiB f4 tiles, the
    scalar columns; gt_push_v_kernel with and without self weights; no private
    segment (nothing in scratch)."""
    co = gt_csr_code_object
    xcd = _kernels(co, "gt_csr_xcd_kernel")
    small = _kernels(co, "gt_csr_kernel")
    f4, scalar = [k for k in small if "Dv4_f" in k], [k for k in small if "Dv4_f" not in k]
    vk = _kernels(co, "gt_push_v_kernel")
    assert len(xcd) == 8 and len(f4) == 8 and len(scalar) == 8 and len(vk) == 2, (xcd, f4, scalar, vk)
    for form in (xcd, f4, scalar):  # 4 per round
        assert sum("GtPlain" in k for k in form) == 4 and sum("GtPushSum" in k for k in form) == 4, form
    sizes = _private_segment_sizes(co)
    for k in xcd + f4 + scalar + vk:
        assert sizes[k] == 0, f"{k}: a private segment of {sizes[k]} bytes (scratch)"


# ---------------------------------------------------------------------------
# convergence, by replaying the host restatement
# ---------------------------------------------------------------------------
def test_host_round_reaches_the_optimum_that_dgd_misses():
    n, P, lr = 16, 8, 0.1
    w_off, d = G.metropolis_weights(G.random_regular_csr(n, 4, seed=5))
    assert (np.diff(w_off.rowptr) == 4).all() and (w_off.val == F32(1) / F32(5)).all() and (d > 0).all()
    rng = np.random.default_rng(3)
    X0, T = (rng.standard_normal((n, P)).astype(F32) for _ in range(2))
    opt = T.astype(np.float64).mean(0)
    X, S = X0, gt_cases.ls_grad(X0, T)
    for _ in range(200):
        X, S = gt_cases.gt_round(X, S, T, w_off, d, lr)
    err = np.abs(X.astype(np.float64) - opt).max()
    # DGD with the same W and lr: consensus with W, then one SGD step on the local gradient
    Y = X0
    for _ in range(200):
        mixed = gt_cases.add_self(oracle.mix_csr(Y, w_off.rowptr, w_off.col, w_off.val), d, Y)
        Y = gt_cases.sgd_step(mixed, gt_cases.ls_grad(mixed, T), lr)
    err_dgd = np.abs(Y.astype(np.float64) - opt).max()
    print(f"max |x - mean t| after 200 rounds: gradient tracking {err:.3g}, DGD {err_dgd:.3g}")
    assert err <= 1e-5
    assert err_dgd > 1e-5
