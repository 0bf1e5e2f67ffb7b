"""Gradient tracking on the sharded ring (dol_gt_ring_edges_f32,
ops.gt_ring_edges, ShardedRing.gt_step), CPU tier: nothing is launched.

* The surface: the SIGNATURES row (dol_gt_ring_f32's), the ops re-export, the
  method on ShardedRing.
* Every argument rule of the entry point, called through the library with
  addresses that are never dereferenced, and DOL_OK for the empty shapes.
* The rules of ops.gt_ring_edges with ops._native.call replaced by a recorder.
* The edge kernel's geometry and indexing restated in the manner of
  tests/test_gt_ring_host.py: gt_ring_edges_kernel<V, OBJ, SELF> over a grid of
  cdiv(columns, 256) x (1 or 2) blocks; y = 0 is row 0, y = 1 row n - 1; each
  lane reads rows r - 1, r, r + 1 of X and S (the halo below 0 / from n) and
  row r of the targets, and writes row r of XO and SO.
* The emitted code: eight instantiations, seven loads and two stores per lane,
  no scratch.
* gt_step with CPU entries (tests/gt_sharded_cases.py) at world 1 in process
  and at worlds 2 and 3 over gloo, with and without the one-launch edge entry:
  every rank's rows of x and of the tracker carry the bits of
  gt_cases.gt_round iterated on the whole ring's CSR; each round posts four
  point-to-point ops of round_up(P, 4) + P floats.
* Convergence at world 3: the 9-agent Metropolis ring, least squares, lr 0.1,
  zero start, 200 rounds: within 1e-5 of the mean of the targets (the bound of
  test_gt_ring_gpu.test_problem_reaches_the_optimum_that_dgd_misses; a CPU run
  of the block-wise round measured 5.8e-7) where extra_cases.dgd_round on the
  same W stays above 0.1 (0.68 there)."""
import re

import numpy as np
import pytest
import torch

import extra_cases as E
import gt_cases
import gt_sharded_cases as C
import oracle
from dolhip import _native, gt, ops, parallel
from test_codegen_pins import _disasm, _kernels, _unbundle
from test_gt_ring_host import _sizes, _window
from test_kernel_extents import KT, Ext, cdiv
from test_ops_args_gpu import vec

CPU = torch.device("cpu")
F32 = np.float32


# ---------------------------------------------------------------------------
# the surface
# ---------------------------------------------------------------------------
def test_surface():
    assert len(_native.SIGNATURES["dol_gt_ring_edges_f32"]) == len(_native.SIGNATURES["dol_gt_ring_f32"]) == 22
    assert _native.SIGNATURES["dol_gt_ring_edges_f32"] == _native.SIGNATURES["dol_gt_ring_f32"]
    assert ops.gt_ring_edges is gt.gt_ring_edges
    assert callable(parallel.ShardedRing.gt_step)


# ---------------------------------------------------------------------------
# the entry point's argument rules, without a launch
# ---------------------------------------------------------------------------
def test_entry_point_checks_arguments_without_launch():
    L = _native.lib()
    fake = 1 << 20  # never dereferenced: every call below returns from its argument checks
    X, S, XO, SO, T, WP, WN, H0, H1, H2, H3 = (fake + (k << 16) for k in range(11))

    def call(x=X, s=S, xo=XO, so=SO, n=8, P=8, ld=8, lds=None, ldxo=None, ldso=None, ldt=None, halos=(H0, H1, H2, H3),
             wp=WP, wn=WN, ws=None, t=T, objective=0):
        pick = lambda v: ld if v is None else v  # noqa: E731
        return L.dol_gt_ring_edges_f32(x, ld, s, pick(lds), xo, pick(ldxo), so, pick(ldso), n, P, *halos, wp, wn, ws,
                                       t, pick(ldt), objective, 0.1, None)

    def refused(word, **kw):
        assert call(**kw) == -1, kw
        msg = L.dol_last_error()
        assert b"dol_gt_ring_edges_f32" in msg and word in msg, (kw, msg)

    for ws in (None, fake + (12 << 16)):  # the self weights alone may be null
        for name in ("x", "s", "xo", "so", "wp", "wn", "t"):
            refused(b"null pointer", ws=ws, **{name: None})
        for k in range(4):  # each halo is required; there is no wrap-around form
            refused(b"null pointer", ws=ws, halos=tuple(None if j == k else h for j, h in enumerate((H0, H1, H2, H3))))
    refused(b"null pointer", halos=(None,) * 4)
    refused(b"null pointer", halos=(None,) * 4, n=1)
    for name in ("ld", "lds", "ldxo", "ldso", "ldt"):
        refused(b"ld < P", **{name: 7})
    for kw in (dict(s=X), dict(xo=X), dict(so=X), dict(xo=S), dict(so=S), dict(so=XO)):
        refused(b"alias", **kw)
    refused(b"objective must be 0 or 1", objective=2)
    refused(b"objective must be 0 or 1", objective=-1)
    refused(b"negative size", n=-1)
    refused(b"negative size", P=-1)
    refused(b"size above 2^40", ld=(1 << 40) + 4)
    refused(b"size above 2^40", P=(1 << 40) + 1, ld=(1 << 40) + 1)
    refused(b"too large", P=1 << 40, ld=1 << 40, x=X + 4)  # scalar columns: 2^32 column tiles
    # nothing to do: DOL_OK whatever else is passed, nothing launched
    assert call(n=0) == 0 and call(P=0) == 0 and call(n=0, x=None, halos=(None,) * 4, objective=5) == 0
    assert L.dol_last_error() == b""


# ---------------------------------------------------------------------------
# ops.gt_ring_edges before the library is reached
# ---------------------------------------------------------------------------
@pytest.fixture
def rec(monkeypatch):
    return gt_cases.recorder(monkeypatch)


def _call(t, halos, **kw):
    return ops.gt_ring_edges(*(t[k] for k in ("X", "S", "XO", "SO", "w_prev", "w_next", "target")), halos, **kw)


def test_unknown_objective_is_refused(rec):
    with pytest.raises(ValueError, match="gt_ring_edges: objective must be one of"):
        _call(gt_cases.host_args("gt_ring", CPU), (vec(CPU, 10),) * 4, objective="hinge")
    assert rec.calls == []


@pytest.mark.parametrize("a,b", [("X", "S"), ("X", "XO"), ("X", "SO"), ("S", "XO"), ("S", "SO"), ("XO", "SO")])
def test_aliasing_state_is_refused(a, b, rec):
    t = gt_cases.host_args("gt_ring", CPU)
    t[b] = t[a]
    with pytest.raises(ValueError, match=f"gt_ring_edges: {a} and {b} alias"):
        _call(t, (vec(CPU, 10),) * 4)
    assert rec.calls == []


def test_fewer_than_four_halos_is_refused(rec):
    h = vec(CPU, 10)
    for halos in (None, (), (h, h), (h, h, h), (h, h, h, None), (None, h, h, h), (h,) * 5):
        with pytest.raises(ValueError, match="gt_ring_edges needs all four halos"):
            _call(gt_cases.host_args("gt_ring", CPU), halos)
    assert rec.calls == []


def test_cpu_tensors_are_refused(rec):
    with pytest.raises(ops.DolNativeError, match="cpu"):
        _call(gt_cases.host_args("gt_ring", CPU), (vec(CPU, 10),) * 4, self_weight=vec(CPU, 4), objective="logistic",
              lr=0.5, P=10, n_rows=4)
    with pytest.raises(ops.DolNativeError, match="cpu"):  # one row is a valid block
        _call(gt_cases.host_args("gt_ring", CPU, n=1), (vec(CPU, 10),) * 4)
    assert rec.calls == []


# ---------------------------------------------------------------------------
# extents: gt_ring_edges_kernel's geometry and indexing restated
# ---------------------------------------------------------------------------
def gt_ring_edges_extents(n, P, ld, vec_ok=True):
    """dol_gt_ring_edges_f32 -> gt_ring_edges_kernel<f4, *, *> over the f4
    columns, then <float, *, *> from column 4 * n4 on (every column when
    !vec_ok).  Returns the extents and the set of XO / SO rows stored."""
    e, stored = Ext(), set()
    n4, tail = (P // 4, P % 4) if vec_ok else (0, P)
    ny = 1 if n == 1 else 2
    for c_off, ncols, w in ((0, n4, 4), (4 * n4, tail, 1)):
        if not ncols:
            continue
        gx = cdiv(ncols, KT)
        assert gx <= 1 << 24
        bx = np.arange(gx, dtype=np.int64)
        c_lo, c_hi = bx * KT, np.minimum(bx * KT + KT - 1, ncols - 1)  # lanes with c < ncols_v
        assert (c_lo < ncols).all()
        lo, hi = c_off + w * c_lo, c_off + w * c_hi + (w - 1)
        for y in range(ny):
            r = 0 if y == 0 else n - 1
            for m in ("X", "S"):
                for k in (-1, 0, 1):
                    _window(e, m, np.full(gx, r + k), n, ld, lo, hi, halos=True)
            for m in ("T", "XO", "SO"):
                e.add(m, r * ld + lo, r * ld + hi)
            stored.add(r)
    return e, stored


@pytest.mark.parametrize("ld_of", [lambda P: (P + 3) // 4 * 4, lambda P: (1 << 20) + 2048],
                         ids=["ld = P rounded up to 4", "ld = 2^20 + 2048"])
@pytest.mark.parametrize("P", [7, 1031, 1 << 20])
@pytest.mark.parametrize("n", [1, 2, 1024])
def test_edge_kernel_extents(n, P, ld_of):
    ld = ld_of(P)
    for vec_ok in (True, False):
        e, stored = gt_ring_edges_extents(n, P, ld, vec_ok)
        e.check(_sizes(n, P, ld))
        assert stored == {0, n - 1}
        # the stores span exactly columns [0, P) of rows 0 and n - 1 ...
        assert e.r["XO"] == e.r["SO"] == e.r["T"] == (0, (n - 1) * ld + P - 1)
        # ... the loads of X and S rows 0, 1, n - 2, n - 1 and all four halos, whole
        assert e.r["X"] == e.r["S"] == (0, (n - 1) * ld + P - 1)
        assert all(e.r[h] == (0, P - 1) for h in ("XHP", "XHN", "SHP", "SHN"))


# ---------------------------------------------------------------------------
# the emitted code
# ---------------------------------------------------------------------------
def test_edge_kernels_are_counted_and_spill_free(tmp_path_factory):
    """{f4, float} x {least squares, logistic} x {no self weights, self weights};
    each lane loads seven values (three rows of X, three of S, one target row)
    and stores two; nothing in scratch.  The ring entry's eight kernels stay."""
    co = _unbundle("gt_ring.o", tmp_path_factory)
    ks = _kernels(co, "gt_ring_edges_kernel")
    assert len(ks) == 8 and sum("Dv4_f" in k for k in ks) == 4, ks
    for k in ks:
        asm = _disasm(co, k)
        wide = "Dv4_f" in k
        loads = len(re.findall(r"global_load_dwordx4" if wide else r"global_load_dword\s", asm))
        stores = len(re.findall(r"global_store_dwordx4" if wide else r"global_store_dword\s", asm))
        # (the compiler may emit the body more than once)
        assert loads >= 7 and loads % 7 == 0 and stores * 7 == loads * 2, (k, loads, stores)
        assert "scratch_" not in asm, f"{k}: spills to scratch"
    assert len(_kernels(co, "gt_ring_dma_kernel")) == 4 and len(_kernels(co, "gt_ring_kernel")) == 4


# ---------------------------------------------------------------------------
# gt_step with CPU entries
# ---------------------------------------------------------------------------
SH_ROUNDS = 3
RING_N, RING_P = 11, 130
MSG = (RING_P + 3) // 4 * 4 + RING_P  # floats per halo message: x's row in [0, P), s's from round_up(P, 4) on


def _ring_rounds(edges):
    """This rank's row range, its rows of (x, s) after SH_ROUNDS gt_step rounds,
    and what each batch_isend_irecv call posted."""
    _, d, wp, wn = E.metropolis_ring(RING_N)
    X, S, T = gt_cases.problem(RING_N, RING_P, 21)
    sh = parallel.ShardedRing(RING_N, RING_P, wp, wn, "cpu", ld=RING_P + 3)
    rows = slice(sh.lo, sh.hi)
    sh.x[:, :RING_P] = torch.from_numpy(X[rows])
    s, t, dl = (torch.from_numpy(np.ascontiguousarray(a[rows])) for a in (S, T, d))
    s_out = torch.full_like(s, float("nan"))
    with C.CountedBatches() as posted:
        for _ in range(SH_ROUNDS):
            x_before, pair = sh.x, (s, s_out)
            s, s_out = sh.gt_step(s, s_out, t, dl, gt_ring=C.cpu_gt_ring,
                                  gt_edges=C.cpu_gt_ring_edges if edges else None, lr=0.1)
            assert sh.y is x_before and s is pair[1] and s_out is pair[0]
    return sh.lo, sh.hi, sh.x[:, :RING_P].numpy().copy(), s.numpy().copy(), posted.calls


def _want():
    c, d = E.metropolis_ring(RING_N)[:2]
    X, S, T = gt_cases.problem(RING_N, RING_P, 21)
    return C.unsharded(X, S, T, c, d, 0.1, SH_ROUNDS)


def test_cpu_entries_are_the_restatement_on_the_whole_ring():
    """One wrap-around cpu_gt_ring call, and cpu_gt_ring_edges with the ring's
    own last and first rows as halos, against gt_round on the ring's CSR."""
    c, d, wp, wn = E.metropolis_ring(RING_N)
    X, S, T = gt_cases.problem(RING_N, RING_P, 21)
    want_x, want_s = gt_cases.gt_round(X, S, T, c, d, 0.1)
    Xt, St, Tt, wpt, wnt, dt = (torch.from_numpy(np.ascontiguousarray(a)) for a in (X, S, T, wp, wn, d))
    XO, SO = torch.zeros_like(Xt), torch.zeros_like(Xt)
    C.cpu_gt_ring(Xt, St, XO, SO, wpt, wnt, Tt, self_weight=dt, lr=0.1, P=RING_P, n_rows=RING_N)
    assert oracle.bits_equal(XO.numpy(), want_x) and oracle.bits_equal(SO.numpy(), want_s)
    XE, SE = torch.full_like(Xt, 7.0), torch.full_like(Xt, 7.0)
    C.cpu_gt_ring_edges(Xt, St, XE, SE, wpt, wnt, Tt, (Xt[-1], Xt[0], St[-1], St[0]), self_weight=dt, lr=0.1, P=RING_P,
                        n_rows=RING_N)
    edge = [0, RING_N - 1]
    assert oracle.bits_equal(XE.numpy()[edge], want_x[edge]) and oracle.bits_equal(SE.numpy()[edge], want_s[edge])
    assert (XE[1:-1] == 7.0).all() and (SE[1:-1] == 7.0).all()


def test_sharded_ring_gt_step_in_one_process():
    lo, hi, x, s, posted = _ring_rounds(edges=True)
    want_x, want_s = _want()
    assert (lo, hi) == (0, RING_N) and posted == []  # one wrap-around call, nothing exchanged
    assert oracle.bits_equal(x, want_x) and oracle.bits_equal(s, want_s)


@pytest.mark.parametrize("edges", [True, False], ids=["edge entry", "edges through the ring entry"])
@pytest.mark.parametrize("world", [2, 3])
def test_sharded_ring_gt_step_over_gloo(world, edges):
    """The boundary rows of x and s travel in one message per direction;
    targets and self weights are sliced per rank.  Every rank's rows are the
    single-process restatement's."""
    want_x, want_s = _want()
    res = C.spawn(_ring_rounds, world, edges)
    assert sorted((lo, hi) for lo, hi, *_ in res) == [parallel.shard_bounds(RING_N, world, r) for r in range(world)]
    for lo, hi, x, s, posted in res:
        assert oracle.bits_equal(x, want_x[lo:hi]) and oracle.bits_equal(s, want_s[lo:hi])
        assert posted == [(4, [MSG] * 4)] * SH_ROUNDS


def test_gt_step_defaults_to_the_hip_ops(monkeypatch):
    """Without injected entries the round goes through ops.gt_ring (world 1:
    one wrap-around call on x, s, y, s_out) -- no eager fall-back."""
    seen = []
    monkeypatch.setattr(ops, "gt_ring", lambda *a, **k: seen.append((a, k)))
    wp, wn = E.metropolis_ring(RING_N)[2:]
    sh = parallel.ShardedRing(RING_N, RING_P, wp, wn, "cpu")
    x, y = sh.x, sh.y
    s, s_out, t = (torch.zeros(RING_N, RING_P) for _ in range(3))
    got = sh.gt_step(s, s_out, t, lr=0.5)
    assert got[0] is s_out and got[1] is s and sh.x is y and sh.y is x
    (a, k), = seen
    assert all(p is q for p, q in zip(a, (x, s, y, s_out, sh.w_prev, sh.w_next, t)))
    assert k == dict(self_weight=None, P=RING_P, n_rows=RING_N, lr=0.5)


# ---------------------------------------------------------------------------
# convergence at world 3
# ---------------------------------------------------------------------------
CONV_N, CONV_P, CONV_ROUNDS, CONV_LR = 9, 8, 200, 0.1


def _conv_targets():
    return np.random.default_rng(2028).standard_normal((CONV_N, CONV_P)).astype(F32)


def _conv_rounds():
    _, d, wp, wn = E.metropolis_ring(CONV_N)
    T = _conv_targets()
    sh = parallel.ShardedRing(CONV_N, CONV_P, wp, wn, "cpu")
    rows = slice(sh.lo, sh.hi)
    sh.x.zero_()
    t, dl = (torch.from_numpy(np.ascontiguousarray(a[rows])) for a in (T, d))
    s = torch.from_numpy(gt_cases.ls_grad(np.zeros_like(T[rows]), T[rows]))  # s(0) = g(x(0))
    s_out = torch.zeros_like(s)
    for _ in range(CONV_ROUNDS):
        s, s_out = sh.gt_step(s, s_out, t, dl, gt_ring=C.cpu_gt_ring, gt_edges=C.cpu_gt_ring_edges, lr=CONV_LR)
    return sh.lo, sh.hi, sh.x[:, :CONV_P].numpy().copy()


def test_sharded_round_reaches_the_optimum_that_dgd_misses():
    c, d = E.metropolis_ring(CONV_N)[:2]
    T = _conv_targets()
    opt = T.astype(np.float64).mean(0)
    res = sorted(C.spawn(_conv_rounds, 3), key=lambda r: r[0])
    assert [(lo, hi) for lo, hi, _ in res] == [(0, 3), (3, 6), (6, 9)]
    X = np.concatenate([x for _, _, x in res])
    err = np.abs(X.astype(np.float64) - opt).max()
    Y = np.zeros_like(T)
    for _ in range(CONV_ROUNDS):
        Y = E.dgd_round(Y, T, c, d, CONV_LR)
    err_dgd = np.abs(Y.astype(np.float64) - opt).max()
    print(f"max |x - mean t| after {CONV_ROUNDS} rounds at world 3: gradient tracking {err:.3g}, DGD {err_dgd:.3g}")
    assert err <= 1e-5
    assert err_dgd > 0.1
