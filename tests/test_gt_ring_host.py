"""Gradient tracking on the agent-major ring (dol_gt_ring_f32, ops.gt_ring,
SeparableGT), CPU tier: nothing is launched.

* The surface: the SIGNATURES row, the ops re-export, the package export.
* Every argument rule of the entry point, called through the library with
  addresses that are never dereferenced (each refusal returns before a launch
  and names the entry), and DOL_OK for the empty shapes.
* The rules of ops.gt_ring that are the ring's own (halos, three rows) and of
  SeparableGT, with ops._native.call replaced by test_ops_args_gpu.Recorder;
  the rules it shares with ops.gt_csr_pm and ops.gt_csr (objective, aliased
  state, weight vectors, CPU tensors) are in tests/test_gt_host.py.
* The launch geometry and indexing of csrc/gt_ring.hip restated in the manner
  of tests/test_kernel_extents.py: gt_ring_dma_kernel<4, OBJ, SELF> (grid
  nct * cdiv(n, 4) in panels of 512 column tiles; R + 2 window rows of X and of S per block at
  min(r0 - 1 + k, r1) through the halo pointers below 0 / from n; target rows
  at min(r0 + k, r1 - 1); stores r < r1) and gt_ring_kernel<OBJ, SELF> (the
  scalar columns: rows r0 - 1 .. r1 of a 4-row block).  Every buffer's touched
  range must lie in [0, rows * ld): on an exact-size mapped block an over-read
  faults.
* The emitted code: four f4 and four scalar instantiations, the LDS-DMA loads
  present, no scratch.
* tests/gt_cases.py::gt_round replayed on the 9-agent ring with Metropolis
  weights (1/3, 1/3, 1/3), least squares, lr 0.1, 200 rounds, P = 8: every
  agent within 1e-5 of the mean of the targets (a float32 numpy simulation of
  this arithmetic gives 2.6e-7), where DGD with the same W and lr stays above
  0.1 (0.36 there).  lr 0.3 diverges and a 33-agent ring needs far more
  rounds, so neither is a case here."""
import types

import numpy as np
import pytest
import torch

import dolhip
import gt_cases
import oracle
from dolhip import _native, graph as G, gt, ops
from dolhip.ops import DolNativeError
from dolhip.synthetic import SeparableGT, ring_gt_weights
from test_codegen_pins import _disasm, _kernels, _unbundle
from test_kernel_extents import KT, Ext, cdiv
from test_ops_args_gpu import vec

CPU = torch.device("cpu")
F32 = np.float32
R = 4  # kGtRows, gt_ring_dma_kernel's tile height, and kGtTailRows
PANEL = 512  # kGtPanel


def ring_pattern(n):
    torch.manual_seed(2028)
    return G.communication_csr("circle", "stochastic", n)[0]


# ---------------------------------------------------------------------------
# the surface
# ---------------------------------------------------------------------------
def test_surface():
    assert len(_native.SIGNATURES["dol_gt_ring_f32"]) == 22
    assert ops.gt_ring is gt.gt_ring and "gt_ring" not in ops.__all__
    assert dolhip.SeparableGT is SeparableGT


def test_ring_gt_weights_are_metropolis_thirds():
    wp, wn, ws = ring_gt_weights(ring_pattern(9))
    third = F32(1) / F32(3)
    assert all(a.dtype == F32 and a.shape == (9,) for a in (wp, wn, ws))
    assert (wp == third).all() and (wn == third).all() and (ws == F32(F32(1) - F32(third + third))).all()
    with pytest.raises(ValueError, match="not a ring"):
        ring_gt_weights(G.random_regular_csr(8, 4, seed=1))


# ---------------------------------------------------------------------------
# the entry point's argument rules, without a launch
# ---------------------------------------------------------------------------
def test_entry_point_checks_arguments_without_launch():
    L = _native.lib()
    fake = 1 << 20  # never dereferenced: every call below returns from its argument checks
    X, S, XO, SO, T, WP, WN, H0, H1, H2, H3 = (fake + (k << 16) for k in range(11))

    def call(x=X, s=S, xo=XO, so=SO, n=8, P=8, ld=8, lds=None, ldxo=None, ldso=None, ldt=None, halos=(None,) * 4,
             wp=WP, wn=WN, ws=None, t=T, objective=0):
        pick = lambda v: ld if v is None else v  # noqa: E731
        return L.dol_gt_ring_f32(x, ld, s, pick(lds), xo, pick(ldxo), so, pick(ldso), n, P, *halos, wp, wn, ws, t,
                                 pick(ldt), objective, 0.1, None)

    def refused(word, **kw):
        assert call(**kw) == -1, kw
        msg = L.dol_last_error()
        assert b"dol_gt_ring_f32" in msg and word in msg, (kw, msg)

    for name in ("x", "s", "xo", "so", "wp", "wn", "t"):
        refused(b"null pointer", **{name: None})
    for name in ("ld", "lds", "ldxo", "ldso", "ldt"):
        refused(b"ld < P", **{name: 7})
    for n_set in range(1, 4):  # one, two or three of the four halos
        for first in range(4):
            halos = tuple(h if (k - first) % 4 < n_set else None for k, h in enumerate((H0, H1, H2, H3)))
            refused(b"all four halos or none", halos=halos)
    refused(b"n_rows >= 3", n=2)
    refused(b"n_rows >= 3", n=1)
    for kw in (dict(s=X), dict(xo=X), dict(so=X), dict(xo=S), dict(so=S), dict(so=XO)):
        refused(b"alias", **kw)
    refused(b"objective must be 0 or 1", objective=2)
    refused(b"objective must be 0 or 1", objective=-1)
    refused(b"too large", n=1 << 20, P=1 << 40, ld=1 << 40)  # 2^30 column tiles x 2^18 row tiles
    refused(b"too large", n=1 << 28, P=1, ld=1)  # the scalar kernel's grid: 1 x 2^26
    refused(b"negative size", n=-1)
    refused(b"size above 2^40", ld=(1 << 40) + 4)
    # nothing to do: DOL_OK whatever else is passed, nothing launched
    assert call(n=0) == 0 and call(P=0) == 0 and call(n=0, x=None, objective=5) == 0
    assert L.dol_last_error() == b""


# ---------------------------------------------------------------------------
# ops.gt_ring and SeparableGT, before the library is reached
# ---------------------------------------------------------------------------
@pytest.fixture
def rec(monkeypatch):
    return gt_cases.recorder(monkeypatch)


def _args(dev, n=4):
    return gt_cases.host_args("gt_ring", dev, n)


def _call(t, **kw):
    return gt_cases.host_call("gt_ring", t, **kw)


def test_halos_come_as_four_or_not_at_all(rec):
    h = vec(CPU, 10)
    for halos in ((h, h, h), (h, h, h, None), (h, None, h, None), (h,) * 5):
        with pytest.raises(ValueError, match="all four or None"):
            _call(_args(CPU), halos=halos)
    assert rec.calls == []


def test_a_wrap_around_ring_needs_three_rows(rec):
    with pytest.raises(ValueError, match="needs >= 3 rows"):
        _call(_args(CPU, n=2))
    with pytest.raises(ValueError, match="needs >= 3 rows"):
        _call(_args(CPU), n_rows=2)
    # with halos one row is a valid block: the next refusal is the CPU tensor's
    with pytest.raises(DolNativeError, match="cpu"):
        _call(_args(CPU, n=1), halos=(vec(CPU, 10),) * 4)
    assert rec.calls == []


def test_problem_class_takes_ring_plans_only(rec):
    c = G.random_regular_csr(8, 4, seed=1)
    with pytest.raises(ValueError, match="ring plan .got kind 'csr'.; SeparableGTPM"):
        SeparableGT(G.MixingPlan(c, CPU), 8)
    with pytest.raises(ValueError, match="SeparableGTPM"):
        SeparableGT(types.SimpleNamespace(n_rows=8, kind="dense", device=CPU), 8)
    ring = G.MixingPlan(ring_pattern(9), CPU)
    assert ring.kind == "ring"
    with pytest.raises(ValueError, match="objective must be one of"):
        SeparableGT(ring, 8, objective="hinge")
    with pytest.raises(ValueError, match="self_weight: expected 9 weights"):
        SeparableGT(ring, 8, self_weight=np.zeros(8, F32))
    assert rec.calls == []


# ---------------------------------------------------------------------------
# extents: csrc/gt_ring.hip's geometry and indexing restated
# ---------------------------------------------------------------------------
def _window(e, mat_name, r, n, ld, lo, hi, halos):
    """Loads of logical rows r (arrays, in [-1, n]) of X or S over element
    columns [lo, hi]: xrow() / srow() -- halo pointers below 0 and from n, which
    are the wrap-around rows of the matrix itself without halos."""
    r = np.asarray(r, np.int64)
    inside = (r >= 0) & (r < n)
    if inside.any():
        e.add(mat_name, r[inside] * ld + lo[inside], r[inside] * ld + hi[inside])
    for mask, wrap_row, halo in ((r < 0, n - 1, "HP"), (r >= n, 0, "HN")):
        if mask.any():
            if halos:
                e.add(mat_name + halo, lo[mask], hi[mask])
            else:
                e.add(mat_name, wrap_row * ld + lo[mask], wrap_row * ld + hi[mask])


def block_order(b, nct, nrt):
    """(column tile, row tile) of block b in gt_ring_dma_kernel: whole panels of
    PANEL column tiles first (row tiles in order inside a panel, the panel's
    column tiles inside a row tile), then the narrower last panel."""
    full = nct // PANEL * PANEL
    in_full = b < full * nrt
    in_panel = b % (PANEL * nrt)
    rem, w = b - full * nrt, max(nct - full, 1)
    ct = np.where(in_full, b // (PANEL * nrt) * PANEL + in_panel % PANEL, full + rem % w)
    rt = np.where(in_full, in_panel // PANEL, rem // w)
    return ct, rt


@pytest.mark.parametrize("nct,nrt", [(1, 1), (3, 5), (511, 2), (512, 3), (513, 3), (1024, 256), (1300, 3)])
def test_block_order_visits_every_tile_once(nct, nrt):
    ct, rt = block_order(np.arange(nct * nrt, dtype=np.int64), nct, nrt)
    assert ct.min() == 0 and ct.max() == nct - 1 and rt.min() == 0 and rt.max() == nrt - 1
    assert np.unique(ct * nrt + rt).size == nct * nrt
    # the vertical neighbour of a tile in a whole panel is PANEL blocks on: the same XCD, 64 of its blocks later
    if nct >= PANEL and nrt > 1:
        assert ct[PANEL] == ct[0] and rt[PANEL] == rt[0] + 1 and PANEL % 8 == 0


def gt_ring_extents(n, P, ld, halos=False, vec_ok=True):
    """dol_gt_ring_f32 -> gt_ring_dma_kernel<4, *, *> over the f4 columns, then
    gt_ring_kernel<*, *> over the scalar ones (all of them when !vec_ok)."""
    e = Ext()
    n4, tail = (P // 4, P % 4) if vec_ok else (0, P)
    if n4:
        nct = cdiv(n4, KT)
        b = np.arange(nct * cdiv(n, R), dtype=np.int64)
        assert b.size <= 1 << 24
        ct, rt = block_order(b, nct, cdiv(n, R))
        r0 = rt * R
        r1 = np.minimum(r0 + R, n)
        c_lo, c_hi = ct * KT, np.minimum(ct * KT + KT - 1, n4 - 1)  # lanes with c < ncols_v
        assert (c_lo < n4).all() and (r0 < n).all()
        for k in range(R + 2):  # the DMA's window rows of both matrices
            for m in ("X", "S"):
                _window(e, m, np.minimum(r0 - 1 + k, r1), n, ld, 4 * c_lo, 4 * c_hi + 3, halos)
        for k in range(R):
            r = np.minimum(r0 + k, r1 - 1)  # the target rows ride with the DMA
            e.add("T", r * ld + 4 * c_lo, r * ld + 4 * c_hi + 3)
            st = r0 + k < r1
            if st.any():
                rs = (r0 + k)[st]
                for m in ("XO", "SO"):
                    e.add(m, rs * ld + 4 * c_lo[st], rs * ld + 4 * c_hi[st] + 3)
    if tail:
        c_off, nct = 4 * n4, cdiv(tail, KT)
        b = np.arange(nct * cdiv(n, R), dtype=np.int64)
        assert b.size <= 1 << 24
        ct, r0 = b % nct, (b // nct) * R
        r1 = np.minimum(r0 + R, n)
        lo, hi = c_off + ct * KT, c_off + np.minimum(ct * KT + KT - 1, tail - 1)
        for k in range(-1, R + 1):  # xat / sat: r0 - 1, r0, then r + 1 for r0 <= r < r1
            live = r0 + k <= r1
            for m in ("X", "S"):
                _window(e, m, (r0 + k)[live], n, ld, lo[live], hi[live], halos)
        for k in range(R):
            st = r0 + k < r1
            if st.any():
                rs = (r0 + k)[st]
                for m in ("T", "XO", "SO"):
                    e.add(m, rs * ld + lo[st], rs * ld + hi[st])
    return e


def _sizes(n, P, ld):
    sizes = {m: n * ld for m in ("X", "S", "T", "XO", "SO")}
    sizes.update({m: P for m in ("XHP", "XHN", "SHP", "SHN")})
    return sizes


@pytest.mark.parametrize("n,P,ld", [(1024, 1 << 20, (1 << 20) + 2048), (8192, 1 << 20, 1 << 20)],
                         ids=["1024 x 2^20, padded rows", "8192 x 2^20"])
def test_extents_at_the_headline_shapes(n, P, ld):
    e = gt_ring_extents(n, P, ld)
    e.check(_sizes(n, P, ld))
    assert e.r["X"] == (0, (n - 1) * ld + P - 1) and e.r["SO"] == (0, (n - 1) * ld + P - 1)  # and nothing is left out


RAGGED = [(3, 1031, 1032), (5, 7, 7), (9, 2055, 2063), (7, 1024, 1024), (4, 1, 1), (6, 4099, 4100)]


@pytest.mark.parametrize("halos", [False, True], ids=["wrap-around", "halos"])
@pytest.mark.parametrize("n,P,ld,vec_ok", [s + (v,) for s in RAGGED for v in (True, False) if not (v and s[2] % 4)])
def test_extents_at_ragged_shapes(n, P, ld, vec_ok, halos):
    """P % 4 != 0, n not a multiple of R, n < R, one element per row; the f4
    body with its scalar tail where ld % 4 == 0, and all columns scalar."""
    e = gt_ring_extents(n, P, ld, halos, vec_ok)
    e.check(_sizes(n, P, ld))
    for m in ("X", "S", "T", "XO", "SO"):
        assert e.r[m] == (0, (n - 1) * ld + P - 1), m
    assert ("XHP" in e.r) == halos
    if halos:
        assert all(e.r[h] == (0, P - 1) for h in ("XHP", "XHN", "SHP", "SHN"))


@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("P", [1031, 3])
def test_extents_of_one_and_two_row_blocks_with_halos(n, P):
    ld = (P + 3) // 4 * 4
    e = gt_ring_extents(n, P, ld, halos=True)
    e.check(_sizes(n, P, ld))
    assert all(e.r[h] == (0, P - 1) for h in ("XHP", "XHN", "SHP", "SHN"))
    assert e.r["X"] == (0, (n - 1) * ld + P - 1)


# ---------------------------------------------------------------------------
# the emitted code
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gt_ring_code_object(tmp_path_factory):
    return _unbundle("gt_ring.o", tmp_path_factory)


def test_gt_ring_kernels_are_counted_and_spill_free(gt_ring_code_object):
    """{least squares, logistic} x {no self weights, self weights}, once on f4
    columns through LDS-DMA and once on scalar columns; R + 2 = 6 window rows
    of two matrices = 12 DMA loads per wave and copy of the tile body, four of
    them nontemporal; nontemporal target loads and stores; nothing in scratch."""
    co = gt_ring_code_object
    dma, scalar = _kernels(co, "gt_ring_dma_kernel"), _kernels(co, "gt_ring_kernel")
    assert len(dma) == 4 and len(scalar) == 4, (dma, scalar)
    for k in dma:
        asm = _disasm(co, k)
        dma_loads = asm.count("global_load_lds_dwordx4")  # the compiler may emit the tile body more than once
        assert dma_loads >= 2 * (R + 2) and dma_loads % (2 * (R + 2)) == 0, (k, dma_loads)
        nt = [ln for ln in asm.splitlines() if ln.split("//")[0].rstrip().endswith(" nt")]
        # the rows no other tile reads, R - 2 of the R + 2 window rows of each matrix, and the target rows
        assert sum("global_load_lds_dwordx4" in ln for ln in nt) * (R + 2) == dma_loads * (R - 2), k
        assert sum("global_load_dwordx4" in ln for ln in nt) >= R, k
        assert sum("global_store_dwordx4" in ln for ln in nt) >= 2, k  # x' and s'
        assert not [ln for ln in asm.splitlines() if "global_store" in ln and ln not in nt], k
        assert "scratch_" not in asm, f"{k}: spills to scratch"
        assert "s_barrier" not in asm, f"{k}: a wave only reads what it loaded"
    for k in scalar:
        assert "scratch_" not in _disasm(co, k), f"{k}: spills to scratch"


# ---------------------------------------------------------------------------
# convergence, by replaying the host restatement
# ---------------------------------------------------------------------------
def test_host_round_reaches_the_optimum_that_dgd_misses():
    n, P, lr = 9, 8, 0.1
    w_off, d = G.metropolis_weights(ring_pattern(n))
    third = F32(1) / F32(3)
    assert (w_off.val == third).all() and (d == F32(F32(1) - F32(third + third))).all()
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
    assert err_dgd > 0.1
