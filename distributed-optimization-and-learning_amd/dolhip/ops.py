"""Tensor-level wrappers over the C-ABI (include/dol_hip.h).

Every function takes CUDA(HIP) fp32 tensors, validates shapes/strides on the
host (the kernels trust their arguments), and enqueues on the current torch
stream.  There is deliberately no CPU path: a CPU tensor raises.

Each kind of argument has one validator (below, before the ops); an op states
which of them apply to it.  Where ops disagree on a rule the difference is a
flag at the call site (same_length=, jacobi=, ld4_of_one_row=, fresh=, ...),
not a second copy of the check.  tests/test_ops_args_gpu.py pins every rule's
exception and message and every op's arguments to the library.
"""
from __future__ import annotations

import os as _os
from typing import Optional

import torch

from . import _native
from ._native import DolNativeError

__all__ = [
    "DolNativeError", "pm_stage_order", "tune_pm_stage_order", "ring_steps_variant", "tune_ring_steps_variant",
    "RING_STEPS_VARIANTS", "PM_STAGE_ORDERS", "tuned_choices", "autotune_enabled", "ring_steps_choice",
    "pm_stage_order_choice", "mix_csr", "mix_ring", "mix_dense", "mix_dense_split3", "dense_split3_workspace_bytes", "split3_x_flags", "er_stochastic",
    "mix_ring_steps", "mix_ring_edges", "dgd_ring_edges", "prox_admm_sgd", "admm_dual", "ordered_mean",
    "ordered_sum", "stream_copy", "dual_workspace_bytes", "prox_grad", "admm_step_dual", "mlp_step",
    "dgd_ring", "dgd_csr", "OBJECTIVES", "admm_ls_round", "admm_ls_round_workspace_bytes", "mix_csr_pm",
    "transpose", "PM_MAX_AGENTS", "stream_copy_rows", "dgd_csr_pm", "PM_DGD_MAX_AGENTS",
    "SLAB_CHUNK", "SLAB_ROWS", "csr_slab_pack", "mix_csr_slab", "slab_layout_ok", "dense_to_csr",
    "admm_ls_round_mean", "slab_variant", "SLAB_VARIANTS", "SPLIT3_FUSE_MAX_M", "SPLIT3_W_READY",
    "SPLIT3_X_ROWS_PADDED", "SPLIT3_FUSE_X", "AUTOTUNE_MIN_BYTES", "AUTOTUNE_REPS", "PM_MAX_FUSED_STEPS",
    "FED_ALGORITHMS", "GT_MAX_AGENTS",
]

PM_MAX_AGENTS = 8192  # dol_mix_csr_pm_f32: one p-row image (<= 32 KiB) per LDS stage
PM_DGD_MAX_AGENTS = 4096  # dol_dgd_csr_pm_f32: X, target and momentum p-rows share a 64 KiB stage
PM_MAX_FUSED_STEPS = 64  # DOL_PM_MAX_FUSED_STEPS: mixing steps in one dol_mix_csr_pm_steps_f32 launch
GT_MAX_AGENTS = 4096  # dol_gt_csr_pm_f32: one quad of agents per thread; X, S and T p-rows share a stage
RING_STEPS_VARIANTS = (1, 2, 3, 4, 5)
PM_STAGE_ORDERS = (8, 16, 32)
AUTOTUNE_MIN_BYTES = 1 << 30  # below this one pass is too short to be worth timing
AUTOTUNE_REPS = 3
SLAB_CHUNK = 64  # DOL_SLAB_CHUNK: agents per LDS chunk of dol_mix_csr_slab_f32
SLAB_ROWS = 128  # DOL_SLAB_ROWS: rows per row group of the chunk-major packing
SLAB_VARIANTS = (2, 3)  # 2: the wave's pairs as one pipelined stream (r06); 3: that stream hand-scheduled (asm); 1 (a loop per row, r03) was retired
SPLIT3_W_READY, SPLIT3_X_ROWS_PADDED, SPLIT3_FUSE_X = 1, 2, 4  # dol_hip.h flags
SPLIT3_FUSE_MAX_M = 2048  # auto-fused X split up to this many output rows (agents)
OBJECTIVES = {"least_squares": 0, "logistic": 1}
FED_ALGORITHMS = {"fedavg": 0, "fedprox": 1, "fedadmm": 2}  # DOL_FED_AVG / _PROX / _ADMM

_TUNED: dict = {}  # launch choices tuned on the product path (see _auto_choice)
_WORK: dict = {}  # per-device scratch (see _workspace)


# ---------------------------------------------------------------------------
# Argument validators: one per kind of argument.
# ---------------------------------------------------------------------------
def _stream(t: torch.Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _ptr_unless_empty(t: torch.Tensor) -> Optional[int]:
    return t.data_ptr() if t.numel() else None


def _no_cpu_path(name: str, t: torch.Tensor) -> DolNativeError:
    return DolNativeError(f"{name}: tensor is on {t.device}; the HIP engine has no CPU path")


def _ld(t: torch.Tensor) -> int:
    """The ld that _check_rows returns, of a matrix not checked here (the *_choice lookups)."""
    return int(t.stride(0) if t.shape[0] > 1 else max(t.shape[1], 1))


def _check_rows(name: str, t: torch.Tensor, P: Optional[int] = None, rows: int = 0, short: Optional[str] = None,
                cols: int = 0, device=None) -> int:
    """Validate a stacked [rows, >=P] fp32 device matrix; return its ld.  With
    `short`: it also has at least `rows` rows (and `cols` columns, and is on
    `device`, where given), or ValueError(short); a {} in `short` stands for
    `device`, whose text is only made when the message is."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a torch.Tensor")
    if t.device.type != "cuda":
        raise _no_cpu_path(name, t)
    if t.dtype != torch.float32:
        raise TypeError(f"{name}: expected float32, got {t.dtype}")
    if t.dim() != 2:
        raise ValueError(f"{name}: expected a 2-D [rows, P] tensor, got shape {tuple(t.shape)}")
    have_rows, have_cols = t.shape
    if have_cols > 1 and t.stride(1) != 1:
        raise ValueError(f"{name}: rows must be contiguous (stride(1) == 1)")
    if P is not None and have_cols < P:
        raise ValueError(f"{name}: has {have_cols} columns < P={P}")
    if short is not None and (have_rows < rows or have_cols < cols or (device is not None and t.device != device)):
        raise ValueError(short.format(device))
    return int(t.stride(0) if have_rows > 1 else max(have_cols, 1))


def _check_xy(X: torch.Tensor, Y: torch.Tensor, P: Optional[int], jacobi: bool = True, nx: str = "X", ny: str = "Y"):
    """The input / output pair of a mix: two row matrices that must not be the
    same buffer (every output row reads several input rows); returns (ldx,
    ldy).  jacobi: whether this op's message says why."""
    ldx = _check_rows(nx, X, P)
    ldy = _check_rows(ny, Y, P)
    if X.data_ptr() == Y.data_ptr():
        raise ValueError(f"{nx} and {ny} alias" + (": the Jacobi mix needs two buffers" if jacobi else ""))
    return ldx, ldy


def _check_momentum(name: str, buf: Optional[torch.Tensor], momentum: float, P: Optional[int], rows: int, short: str,
                    cols: int = 0, device=None) -> int:
    """ld of the momentum buffer (_check_rows), or 0 when momentum == 0: the
    buffer is then neither needed nor looked at, and the op passes NULL."""
    if momentum == 0.0:
        return 0
    if buf is None:
        raise ValueError(f"momentum != 0 needs {name}")
    return _check_rows(name, buf, P, rows, short, cols, device)


def _check_vec(name: str, t: Optional[torch.Tensor], P: int, device) -> None:
    if t is None:
        return
    if t.device != device:
        raise DolNativeError(f"{name}: on {t.device}, expected {device}")
    if t.dtype != torch.float32 or t.dim() != 1 or t.shape[0] < P or (t.shape[0] > 1 and t.stride(0) != 1):
        raise ValueError(f"{name}: expected a contiguous float32 vector of >= {P} elements")


def _check_prox_terms(theta: Optional[torch.Tensor], alpha: Optional[torch.Tensor], P: int, n: int, device) -> int:
    """The optional prox centre theta [>= P] and dual rows alpha [>= n, >= P]
    of a local step (alpha only with theta); returns alpha's ld, 0 without."""
    lda = 0
    if alpha is not None:
        if theta is None:
            raise ValueError("alpha needs theta")
        lda = _check_rows("alpha", alpha, P, n, "alpha has fewer rows than w")
    _check_vec("theta", theta, P, device)
    return lda


def _check_array(name: str, t: torch.Tensor, dtype, n: int, device, what: str = "contiguous") -> None:
    """A contiguous 1-D device array of >= n elements of `dtype` (index lists,
    per-agent flags and norms)."""
    if t.device != device or t.dtype != dtype or t.numel() < n or not t.is_contiguous():
        raise ValueError(f"{name}: expected {what} {str(dtype)[6:]} [{n}] on {device}")


def _check_csr(rowptr: torch.Tensor, col: torch.Tensor, val: torch.Tensor, device, same_length: bool) -> None:
    """The CSR triple on `device`.  same_length: col and val must be equally
    long (mix_csr, csr_slab_pack); the other ops accept a longer one."""
    for nm, t, dt in (("rowptr", rowptr, torch.int32), ("col", col, torch.int32), ("val", val, torch.float32)):
        if t.device != device or t.dtype != dt or not t.is_contiguous():
            raise ValueError(f"{nm}: expected contiguous {dt} on {device}")
    if same_length and col.numel() != val.numel():
        raise ValueError("col and val lengths differ")


def _check_order(order: torch.Tensor, device) -> None:
    if order.device != device or order.dtype != torch.int32 or not order.is_contiguous():
        raise ValueError("order: expected contiguous int32 on the rows' device")


def _ring_args(X, Y, w_prev, w_next, P, n_rows, jacobi: bool = True):
    """(P, n, ldx, ldy) of a ring op: the X / Y pair with at least n rows each
    and the two weight vectors [n]."""
    P = X.shape[1] if P is None else P
    n = X.shape[0] if n_rows is None else n_rows
    ldx, ldy = _check_xy(X, Y, P, jacobi)
    if X.shape[0] < n or Y.shape[0] < n:
        raise ValueError("X/Y have fewer rows than n_rows")
    for nm, t in (("w_prev", w_prev), ("w_next", w_next)):
        if t.device != X.device or t.dtype != torch.float32 or t.numel() < n or not t.is_contiguous():
            raise ValueError(f"{nm}: expected contiguous float32 [{n}] on {X.device}")
    return P, n, ldx, ldy


def _check_halos(halo_prev, halo_next, P: int, device, required_by: Optional[str] = None) -> bool:
    """The rows before / after the local block, [>= P] each: both or neither,
    or both where `required_by` names an op that cannot do without.  Returns
    whether they are there."""
    if required_by is not None and (halo_prev is None or halo_next is None):
        raise ValueError(f"{required_by} needs both halos")
    if (halo_prev is None) != (halo_next is None):
        raise ValueError("pass both halos or neither")
    _check_vec("halo_prev", halo_prev, P, device)
    _check_vec("halo_next", halo_next, P, device)
    return halo_prev is not None


def _dgd_args(device, target, mom, objective, steps, momentum, P, n, pm: bool = False):
    """(ldt, ldm) of the local-step arguments of a DGD round on n agents of P
    parameters.  pm: the parameter-major layout (TT / MT are [P, >= n], their
    columns the agents) instead of the agent-major one ([>= n, >= P])."""
    if objective not in OBJECTIVES:
        raise ValueError(f"objective must be one of {sorted(OBJECTIVES)}")
    if int(steps) < 1:
        raise ValueError("local steps must be >= 1")
    if pm:
        return (_check_rows("TT", target, None, P, f"TT: expected [>= {P}, >= {n}] on {{}}", n, device),
                _check_momentum("MT", mom, momentum, None, P, f"MT: expected [>= {P}, >= {n}] on {{}}", n, device))
    return (_check_rows("target", target, P, n, f"target: expected >= {n} rows on {{}}", 0, device),
            _check_momentum("mom", mom, momentum, P, n, f"mom: expected >= {n} rows on {{}}", 0, device))


def _workspace(work: Optional[torch.Tensor], nbytes: int, device, fresh: int = 0, uint8: bool = False,
               any_device: bool = False) -> torch.Tensor:
    """`work`, checked to hold nbytes bytes on `device`; or when None the
    per-device scratch, grown on demand and reused (stream-ordered on the
    current stream like every other op).  fresh: allocate a buffer of its own
    of at least this many bytes instead of the shared scratch.  uint8: `work`
    must be a uint8 tensor.  any_device: its device is not looked at."""
    if work is None:
        if fresh:
            return torch.empty(max(nbytes, fresh), dtype=torch.uint8, device=device)
        work = _WORK.get(device)
        if work is None or work.numel() < nbytes:
            work = _WORK[device] = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=device)
        return work
    if uint8:
        fits = work.dtype == torch.uint8 and work.numel() >= nbytes
    else:
        fits = work.numel() * work.element_size() >= nbytes
    if not fits or not (any_device or work.device == device):
        raise ValueError("work: need " + (f"a uint8 tensor of >= {nbytes} bytes" if uint8 else f"{nbytes} bytes")
                         + ("" if any_device else f" on {device}"))
    return work


def _rows_padded(X: torch.Tensor, P: int, ld4_of_one_row: bool) -> bool:
    """Whether X's rows can be read in whole 16-B pieces up to round_up(P, 4)
    floats: aligned rows, ld % 4 == 0, storage present behind the last row.
    ld4_of_one_row: whether a one-row X (which has no stride to speak of)
    must be a multiple of 4 wide as well."""
    if X.dim() != 2 or X.data_ptr() % 16:
        return False
    ld = X.stride(0) if X.shape[0] > 1 else X.shape[1]
    p4 = -(-P // 4) * 4
    if ld < p4 or (ld % 4 and (ld4_of_one_row or X.shape[0] > 1)):
        return False
    return (X.storage_offset() + (X.shape[0] - 1) * ld + p4) * 4 <= X.untyped_storage().nbytes()


# ---------------------------------------------------------------------------
# Process-wide kernel settings.
# ---------------------------------------------------------------------------
def _set_or_raise(setter: str, value: int, returned: bool = False) -> int:
    """Call a dol_*_set_* entry point; the previous setting, or DolNativeError
    with the library's message when it refuses the value."""
    L = _native.lib()
    prev = int(getattr(L, setter)(int(value)))
    if prev < 0:
        raise DolNativeError(setter + (f" returned {prev}: " if returned else ": ")
                             + L.dol_last_error().decode(errors="replace"))
    return prev


def pm_stage_order(nseg: int) -> int:
    """Set the parameter-major kernels' stage order for this process (nseg
    regions streamed at once; 0 = the default) and return the previous setting
    (dol_pm_set_stage_order).  Same bits for every order."""
    return _set_or_raise("dol_pm_set_stage_order", nseg)


def ring_steps_variant(variant: int) -> int:
    """Kernel of mix_ring_steps for this process: 1 register tiles, 2 streaming,
    3 / 4 / 5 streaming by LDS-DMA (plain / block-synchronised / 64-row sweep),
    0 default; returns the previous setting (dol_ring_steps_set_variant)."""
    return _set_or_raise("dol_ring_steps_set_variant", variant)


def slab_variant(variant: int) -> int:
    """Kernel of mix_csr_slab for this process (dol_slab_set_variant; 0 =
    the default, 3).  Same bits for every variant.  Returns the previous
    setting; a variant the library refuses raises DolNativeError."""
    return _set_or_raise("dol_slab_set_variant", variant, returned=True)


def _time_each(run_with, candidates, reps, device=None):
    """{candidate: mean ms of `reps` calls of run_with(candidate)} on the
    current stream of `device` (default: the current device) -- the stream the
    ops launch on for tensors there.  Events bracket the calls on that stream
    and the host waits on the closing event only: no device-wide
    synchronisation, so work on other streams (a side stream's W draw, another
    rank's buffers) is neither waited for nor serialised."""
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    times = {}
    with torch.cuda.device(device):
        stream = torch.cuda.current_stream(device)
        for c in candidates:
            run_with(c)  # warm (first launch of this variant on these buffers)
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record(stream)
            for _ in range(reps):
                run_with(c)
            e.record(stream)
            e.synchronize()
            times[c] = s.elapsed_time(e) / reps
    return times


def _tune(setter, run, candidates, reps):
    def run_with(c):
        setter(c)
        run()
    times = _time_each(run_with, candidates, reps)
    best = min(times, key=times.get)
    setter(best)
    return best, times


def tune_pm_stage_order(run, candidates=(8, 16, 32), reps: int = 3) -> dict:
    """Time `run()` (a parameter-major mix on the buffers it will keep using)
    under each stage order and keep the fastest for this process: which order
    balances the HBM channels best depends on where those buffers' pages
    landed (profiles/r03_pm_stage_order.txt).  Returns {"nseg": best, "ms":
    {nseg: ms}}.  Setup-time only; results are bit-identical under every order."""
    best, times = _tune(pm_stage_order, run, candidates, reps)
    return {"nseg": best, "ms": times}


def tune_ring_steps_variant(run, reps: int = 3) -> dict:
    """Time `run()` (a mix_ring_steps call on the buffers it will keep using)
    with the register-tile and the streaming kernel and keep the faster for
    this process; which wins depends on where the buffers' pages landed.
    Returns {"variant": 1 | 2, "ms": {variant: ms}}.  Same bits either way."""
    best, times = _tune(ring_steps_variant, run, RING_STEPS_VARIANTS, reps)
    return {"variant": best, "ms": times}


# ---------------------------------------------------------------------------
# Launch choices tuned on the product path.  Which ring-steps kernel / which
# parameter-major stage order is fastest follows where a bank's pages landed
# (DESIGN.md §4.1, §4.4), so the first large call on a pair of buffers times
# every candidate on THOSE buffers (the calls are pure X -> Y mixes: re-running
# them only rewrites Y) and caches the winner for that (buffer pair, geometry);
# later calls pass it per call (the _ex entry points), so nothing process-wide
# changes and the results are the same bits whatever is picked.  A stale entry
# after the memory is reused can only cost speed.  DOL_AUTOTUNE=0 turns it off
# (every call then takes the library default).
# ---------------------------------------------------------------------------
def autotune_enabled() -> bool:
    return _os.environ.get("DOL_AUTOTUNE", "1") != "0"


def tuned_choices() -> dict:
    """{key: {"choice": c, "ms": {candidate: ms}}} of every launch choice this process tuned."""
    return {repr(k): dict(v) for k, v in _TUNED.items()}


def _auto_choice(key, run_with, candidates, nbytes: int, device) -> int:
    """The cached pick for `key`, or time every candidate on `device`'s current
    stream (where the buffers live and the ops launch), cache and return the
    fastest; 0 (the library default) when tuning is off, the buffers are small
    or that stream is being captured into a graph."""
    if not autotune_enabled() or nbytes < AUTOTUNE_MIN_BYTES:
        return 0
    hit = _TUNED.get(key)
    if hit is not None:
        return hit["choice"]
    with torch.cuda.device(device):
        if torch.cuda.is_current_stream_capturing():  # no timing inside a graph capture
            return 0
    times = _time_each(run_with, candidates, AUTOTUNE_REPS, device=device)
    best = min(times, key=times.get)
    _TUNED[key] = {"choice": best, "ms": times}
    return best


def _pair_key(kind, A: torch.Tensor, B: torch.Tensor, *geometry):
    return (kind, A.device.index, frozenset((A.data_ptr(), B.data_ptr())), *geometry)


def ring_steps_choice(X: torch.Tensor, Y: torch.Tensor, steps: int, P: Optional[int] = None,
                      n_rows: Optional[int] = None) -> Optional[dict]:
    """The tuned mix_ring_steps entry ({"choice", "ms"}) for this buffer pair, or None."""
    P = X.shape[1] if P is None else P
    n = X.shape[0] if n_rows is None else n_rows
    return _TUNED.get(_pair_key("ring_steps", X, Y, _ld(X), _ld(Y), n, P, int(steps)))


def pm_stage_order_choice(XT: torch.Tensor, YT: torch.Tensor, n: int, x_agents: Optional[int] = None,
                          P: Optional[int] = None) -> Optional[dict]:
    """The tuned mix_csr_pm / dgd_csr_pm entry ({"choice", "ms"}) for this buffer pair, or None."""
    P = XT.shape[0] if P is None else P
    x_agents = n if x_agents is None else int(x_agents)
    return _TUNED.get(_pair_key("pm", XT, YT, _ld(XT), _ld(YT), x_agents, n, P))


# ---------------------------------------------------------------------------
# Copies and layout.
# ---------------------------------------------------------------------------
def stream_copy(src: torch.Tensor, dst: torch.Tensor) -> torch.Tensor:
    if src.device.type != "cuda" or dst.device != src.device:
        raise DolNativeError("stream_copy: device tensors required")
    if not (src.is_contiguous() and dst.is_contiguous()) or src.numel() != dst.numel():
        raise ValueError("stream_copy: contiguous tensors of equal size required")
    _native.call("dol_stream_copy_f32", src.data_ptr(), dst.data_ptr(), src.numel(), _stream(src))
    return dst


def stream_copy_rows(X: torch.Tensor, Y: torch.Tensor, P: Optional[int] = None) -> torch.Tensor:
    """Y[:, :P] = X[:, :P] in the ring mix's tile geometry (roofline calibration)."""
    P = X.shape[1] if P is None else P
    ldx = _check_rows("X", X, P)
    ldy = _check_rows("Y", Y, P, X.shape[0], "Y has fewer rows than X")
    _native.call("dol_stream_copy_rows_f32", X.data_ptr(), ldx, Y.data_ptr(), ldy, X.shape[0], P, _stream(X))
    return Y


def transpose(A: torch.Tensor, B: torch.Tensor, rows: Optional[int] = None, cols: Optional[int] = None) -> torch.Tensor:
    """B[c, r] = A[r, c] for r < rows, c < cols (tiled through LDS): converts the
    agent-major bank [N, ld] to the parameter-major one [P, ldt] and back."""
    rows = A.shape[0] if rows is None else rows
    cols = A.shape[1] if cols is None else cols
    lda = _check_rows("A", A, cols)
    ldb = _check_rows("B", B, rows)
    if A.shape[0] < rows or B.shape[0] < cols:
        raise ValueError(f"shapes: A {tuple(A.shape)}, B {tuple(B.shape)}, rows {rows}, cols {cols}")
    if A.device != B.device:
        raise ValueError("A and B on different devices")
    _native.call("dol_transpose_f32", A.data_ptr(), lda, B.data_ptr(), ldb, rows, cols, _stream(A))
    return B


# ---------------------------------------------------------------------------
# Ring (circle topology).
# ---------------------------------------------------------------------------
def mix_ring(X: torch.Tensor, Y: torch.Tensor, w_prev: torch.Tensor, w_next: torch.Tensor,
             halo_prev: Optional[torch.Tensor] = None, halo_next: Optional[torch.Tensor] = None,
             P: Optional[int] = None, n_rows: Optional[int] = None) -> torch.Tensor:
    """Ring (circle topology) mix; halos are the rows before/after the local block."""
    P, n, ldx, ldy = _ring_args(X, Y, w_prev, w_next, P, n_rows)
    if not _check_halos(halo_prev, halo_next, P, X.device) and n < 3:
        raise ValueError("a wrap-around ring needs >= 3 rows (use mix_csr)")
    _native.call("dol_mix_ring_f32", X.data_ptr(), ldx, Y.data_ptr(), ldy, n, P, _ptr(halo_prev),
                 _ptr(halo_next), w_prev.data_ptr(), w_next.data_ptr(), _stream(X))
    return Y


def mix_ring_edges(X: torch.Tensor, Y: torch.Tensor, w_prev: torch.Tensor, w_next: torch.Tensor,
                   halo_prev: torch.Tensor, halo_next: torch.Tensor, P: Optional[int] = None,
                   n_rows: Optional[int] = None) -> torch.Tensor:
    """Rows 0 and n_rows-1 of mix_ring with halos, in one launch (the second
    half of a sharded ring round; dol_mix_ring_edges_f32)."""
    P, n, ldx, ldy = _ring_args(X, Y, w_prev, w_next, P, n_rows)
    _check_halos(halo_prev, halo_next, P, X.device, required_by="mix_ring_edges")
    _native.call("dol_mix_ring_edges_f32", X.data_ptr(), ldx, Y.data_ptr(), ldy, n, P, halo_prev.data_ptr(),
                 halo_next.data_ptr(), w_prev.data_ptr(), w_next.data_ptr(), _stream(X))
    return Y


def mix_ring_steps(X: torch.Tensor, Y: torch.Tensor, w_prev: torch.Tensor, w_next: torch.Tensor, steps: int,
                   P: Optional[int] = None, n_rows: Optional[int] = None,
                   variant: Optional[int] = None) -> torch.Tensor:
    """Y = W^steps X for the wrap-around ring in one HBM pass (bit-identical to
    `steps` mix_ring calls).  Needs P % 4 == 0 and 16-B aligned rows.
    variant: the kernel (RING_STEPS_VARIANTS; None = tuned for these buffers
    on first use, 0 = the process setting)."""
    P, n, ldx, ldy = _ring_args(X, Y, w_prev, w_next, P, n_rows, jacobi=False)

    def launch(v):
        _native.call("dol_mix_ring_steps_ex_f32", X.data_ptr(), ldx, Y.data_ptr(), ldy, n, P, int(steps),
                     w_prev.data_ptr(), w_next.data_ptr(), int(v), _stream(X))
    if variant is None:
        variant = _auto_choice(_pair_key("ring_steps", X, Y, ldx, ldy, n, P, int(steps)), launch,
                               RING_STEPS_VARIANTS, 2 * n * P * 4, X.device) if steps > 1 else 0
    launch(variant)
    return Y


def dgd_ring(X: torch.Tensor, Y: torch.Tensor, w_prev: torch.Tensor, w_next: torch.Tensor, target: torch.Tensor,
             mom: Optional[torch.Tensor] = None, objective: str = "least_squares", steps: int = 1, lr: float = 0.01,
             momentum: float = 0.0, first_step: bool = False, halo_prev: Optional[torch.Tensor] = None,
             halo_next: Optional[torch.Tensor] = None, P: Optional[int] = None,
             n_rows: Optional[int] = None) -> torch.Tensor:
    """One fused DGD round on a ring: Y = W X (bit-exact mix), then `steps` local
    momentum-SGD iterations per row on a separable loss (BASELINE config 3;
    round order of DIST/simulators.py:147-162)."""
    P, n, ldx, ldy = _ring_args(X, Y, w_prev, w_next, P, n_rows)
    if not _check_halos(halo_prev, halo_next, P, X.device) and n < 3:
        raise ValueError("a wrap-around ring needs >= 3 rows (use dgd_csr)")
    ldt, ldm = _dgd_args(X.device, target, mom, objective, steps, momentum, P, n)
    _native.call("dol_dgd_ring_f32", X.data_ptr(), ldx, Y.data_ptr(), ldy, n, P, _ptr(halo_prev), _ptr(halo_next),
                 w_prev.data_ptr(), w_next.data_ptr(), target.data_ptr(), ldt, _ptr(mom) if ldm else None, ldm,
                 OBJECTIVES[objective], int(steps), float(lr), float(momentum), int(bool(first_step)), _stream(X))
    return Y


def dgd_ring_edges(X: torch.Tensor, Y: torch.Tensor, w_prev: torch.Tensor, w_next: torch.Tensor,
                   target: torch.Tensor, halo_prev: torch.Tensor, halo_next: torch.Tensor,
                   mom: Optional[torch.Tensor] = None, objective: str = "least_squares", steps: int = 1,
                   lr: float = 0.01, momentum: float = 0.0, first_step: bool = False, P: Optional[int] = None,
                   n_rows: Optional[int] = None) -> torch.Tensor:
    """Rows 0 and n_rows-1 of dgd_ring with halos, in one launch (dol_dgd_ring_edges_f32)."""
    P, n, ldx, ldy = _ring_args(X, Y, w_prev, w_next, P, n_rows)
    _check_halos(halo_prev, halo_next, P, X.device, required_by="dgd_ring_edges")
    ldt, ldm = _dgd_args(X.device, target, mom, objective, steps, momentum, P, n)
    _native.call("dol_dgd_ring_edges_f32", X.data_ptr(), ldx, Y.data_ptr(), ldy, n, P, halo_prev.data_ptr(),
                 halo_next.data_ptr(), w_prev.data_ptr(), w_next.data_ptr(), target.data_ptr(), ldt,
                 _ptr(mom) if ldm else None, ldm, OBJECTIVES[objective], int(steps), float(lr), float(momentum),
                 int(bool(first_step)), _stream(X))
    return Y


# ---------------------------------------------------------------------------
# Sparse W (CSR): agent-major, parameter-major, and the LDS slab.
# ---------------------------------------------------------------------------
def _csr_args(X, Y, rowptr, col, val, P, same_length: bool):
    """(P, n, ldx, ldy) of an agent-major CSR op: n = rowptr length - 1 output rows."""
    P = X.shape[1] if P is None else P
    ldx, ldy = _check_xy(X, Y, P)
    n = rowptr.shape[0] - 1
    if Y.shape[0] < n:
        raise ValueError(f"Y has {Y.shape[0]} rows < {n}")
    _check_csr(rowptr, col, val, X.device, same_length)
    return P, n, ldx, ldy


def mix_csr(X: torch.Tensor, Y: torch.Tensor, rowptr: torch.Tensor, col: torch.Tensor,
            val: torch.Tensor, P: Optional[int] = None) -> torch.Tensor:
    """Y[i] = sum_e val[e] * X[col[e]] (ascending e, +0 start, no FMA).

    Reference: DIST/simulators.py:91-97 + DIST/clients.py:61-69."""
    P, n, ldx, ldy = _csr_args(X, Y, rowptr, col, val, P, same_length=True)
    _native.call("dol_mix_csr_f32", X.data_ptr(), ldx, X.shape[0], Y.data_ptr(), ldy, n, P,
                 rowptr.data_ptr(), _ptr_unless_empty(col), _ptr_unless_empty(val), _stream(X))
    return Y


def dgd_csr(X: torch.Tensor, Y: torch.Tensor, rowptr: torch.Tensor, col: torch.Tensor, val: torch.Tensor,
            target: torch.Tensor, mom: Optional[torch.Tensor] = None, objective: str = "least_squares",
            steps: int = 1, lr: float = 0.01, momentum: float = 0.0, first_step: bool = False,
            P: Optional[int] = None) -> torch.Tensor:
    """dgd_ring for any W (CSR mix, bit-exact), then the same local steps."""
    P, n, ldx, ldy = _csr_args(X, Y, rowptr, col, val, P, same_length=False)
    ldt, ldm = _dgd_args(X.device, target, mom, objective, steps, momentum, P, n)
    _native.call("dol_dgd_csr_f32", X.data_ptr(), ldx, X.shape[0], Y.data_ptr(), ldy, n, P, rowptr.data_ptr(),
                 _ptr_unless_empty(col), _ptr_unless_empty(val),
                 target.data_ptr(), ldt, _ptr(mom) if ldm else None, ldm, OBJECTIVES[objective], int(steps),
                 float(lr), float(momentum), int(bool(first_step)), _stream(X))
    return Y


def _pm_args(XT, YT, rowptr, col, val, x_agents, P):
    """(P, n, x_agents, ldx, ldy) of a parameter-major op: XT [P, >= x_agents],
    YT [P, >= n], n = rowptr length - 1."""
    P = XT.shape[0] if P is None else P
    n = rowptr.shape[0] - 1
    x_agents = n if x_agents is None else int(x_agents)
    ldx, ldy = _check_xy(XT, YT, None, nx="XT", ny="YT")
    if XT.shape[0] < P or YT.shape[0] < P:
        raise ValueError(f"XT/YT need >= {P} parameter rows")
    if XT.shape[1] < x_agents or YT.shape[1] < n:
        raise ValueError(f"XT needs >= {x_agents} agent columns, YT >= {n}")
    _check_csr(rowptr, col, val, XT.device, same_length=False)
    return P, n, x_agents, ldx, ldy


def _pm_mix(XT, YT, rowptr, col, val, ldx, ldy, x_agents, n, P):
    """launch(nseg): the parameter-major mix under one stage order."""
    def launch(ns):
        _native.call("dol_mix_csr_pm_ex_f32", XT.data_ptr(), ldx, x_agents, YT.data_ptr(), ldy, n, P,
                     rowptr.data_ptr(), _ptr_unless_empty(col), _ptr_unless_empty(val), int(ns), _stream(XT))
    return launch


def _pm_auto(mix, XT, YT, ldx, ldy, x_agents, n, P) -> int:
    key = _pair_key("pm", XT, YT, ldx, ldy, x_agents, n, P)
    return _auto_choice(key, mix, PM_STAGE_ORDERS, (x_agents + n) * P * 4, XT.device)


def mix_csr_pm(XT: torch.Tensor, YT: torch.Tensor, rowptr: torch.Tensor, col: torch.Tensor, val: torch.Tensor,
               x_agents: Optional[int] = None, P: Optional[int] = None, nseg: Optional[int] = None) -> torch.Tensor:
    """The gossip mix on the parameter-major bank: YT[p, i] = sum_e val[e] *
    XT[p, col[e]] for every parameter row p (bit-identical to mix_csr on the
    transposed matrices).  XT [P, >= x_agents], YT [P, >= n] (n = rowptr
    length - 1), row strides multiples of 4, 16-B aligned; at most
    PM_MAX_AGENTS agents.  nseg: the stage order (None = tuned for these
    buffers on first use, 0 = the process setting).  Reference:
    DIST/simulators.py:91-97 + DIST/clients.py:61-69."""
    P, n, x_agents, ldx, ldy = _pm_args(XT, YT, rowptr, col, val, x_agents, P)
    mix = _pm_mix(XT, YT, rowptr, col, val, ldx, ldy, x_agents, n, P)
    mix(_pm_auto(mix, XT, YT, ldx, ldy, x_agents, n, P) if nseg is None else nseg)
    return YT


def dgd_csr_pm(XT: torch.Tensor, YT: torch.Tensor, rowptr: torch.Tensor, col: torch.Tensor, val: torch.Tensor,
               TT: torch.Tensor, MT: Optional[torch.Tensor] = None, objective: str = "least_squares",
               steps: int = 1, lr: float = 0.01, momentum: float = 0.0, first_step: bool = False,
               x_agents: Optional[int] = None, P: Optional[int] = None, nseg: Optional[int] = None) -> torch.Tensor:
    """dgd_csr on the parameter-major bank: XT/YT as mix_csr_pm, TT [P, >= n]
    the targets and MT [P, >= n] the momentum (transposed like XT); the same
    mix and local steps, bit-identical to dgd_csr on the transposed matrices.
    At most PM_DGD_MAX_AGENTS agents.  nseg as mix_csr_pm (None: the order
    tuned for XT / YT, timed on the plain mix, which only writes YT)."""
    P, n, x_agents, ldx, ldy = _pm_args(XT, YT, rowptr, col, val, x_agents, P)
    ldt, ldm = _dgd_args(XT.device, TT, MT, objective, steps, momentum, P, n, pm=True)
    if nseg is None:
        nseg = _pm_auto(_pm_mix(XT, YT, rowptr, col, val, ldx, ldy, x_agents, n, P), XT, YT, ldx, ldy, x_agents, n, P)
    _native.call("dol_dgd_csr_pm_ex_f32", XT.data_ptr(), ldx, x_agents, YT.data_ptr(), ldy, n, P, rowptr.data_ptr(),
                 _ptr_unless_empty(col), _ptr_unless_empty(val), TT.data_ptr(),
                 ldt, _ptr(MT) if ldm else None, ldm, OBJECTIVES[objective], int(steps), float(lr), float(momentum),
                 int(bool(first_step)), int(nseg), _stream(XT))
    return YT


def csr_slab_pack(rowptr: torch.Tensor, col: torch.Tensor, val: torch.Tensor, x_rows: int,
                  ent: Optional[torch.Tensor] = None, hdr: Optional[torch.Tensor] = None, balance: bool = False):
    """(ent, hdr) of a device CSR for mix_csr_slab (dol_csr_slab_pack): the
    rows of each group of SLAB_ROWS dealt to slots (balanced per-chunk wave
    loads), the entries re-packed chunk-major as (weight bits, LDS byte offset)
    pairs, every (slot, chunk) segment padded to an even length; hdr[g][k][s] =
    first entry of slot s in chunk k, bit 0 = the segment ends in a pad, then
    perm[g][s] = row and inv[row] = slot (include/dol_hip.h).  col/val may be
    longer than nnz (a capacity); ent is sized from it.  balance: deal the
    rows to the kernel's waves by greedy packing of their per-chunk loads
    (same bits; worth it when one W is mixed many times)."""
    n = rowptr.numel() - 1
    if rowptr.device.type != "cuda":
        raise _no_cpu_path("rowptr", rowptr)
    _check_csr(rowptr, col, val, rowptr.device, same_length=True)
    L = _native.lib()
    need_e = int(L.dol_csr_slab_ent_len(col.numel(), n, int(x_rows)))
    need_h = int(L.dol_csr_slab_hdr_len(n, int(x_rows)))
    if ent is None or ent.numel() < need_e:
        ent = torch.empty(max(need_e, 4), dtype=torch.int32, device=rowptr.device)
    if hdr is None or hdr.numel() < need_h:
        hdr = torch.empty(max(need_h, 4), dtype=torch.int32, device=rowptr.device)
    _native.call("dol_csr_slab_pack", rowptr.data_ptr(), _ptr_unless_empty(col), _ptr_unless_empty(val), n,
                 int(x_rows), int(bool(balance)), ent.data_ptr(), hdr.data_ptr(), _stream(rowptr))
    return ent, hdr


def slab_layout_ok(X: torch.Tensor, Y: torch.Tensor, P: int) -> bool:
    """Whether mix_csr_slab accepts these matrices: 16-B aligned rows, row
    strides multiples of 4, X rows readable up to round_up(P, 4) floats."""
    if Y.dim() != 2 or Y.data_ptr() % 16 or (Y.stride(0) if Y.shape[0] > 1 else Y.shape[1]) % 4:
        return False
    return _rows_padded(X, P, ld4_of_one_row=True)


def mix_csr_slab(X: torch.Tensor, Y: torch.Tensor, ent: torch.Tensor, hdr: torch.Tensor, n_rows: int,
                 x_rows: Optional[int] = None, P: Optional[int] = None) -> torch.Tensor:
    """mix_csr for high-degree graphs (dol_mix_csr_slab_f32): the same sum in
    the same order, bit-identical, with X's columns staged through LDS.
    (ent, hdr) from csr_slab_pack.  Reference: DIST/simulators.py:91-97 +
    DIST/clients.py:61-69."""
    P = X.shape[1] if P is None else P
    x_rows = X.shape[0] if x_rows is None else int(x_rows)
    ldx, ldy = _check_xy(X, Y, P)
    if Y.shape[0] < n_rows or X.shape[0] < x_rows:
        raise ValueError(f"X has {X.shape[0]} rows (need {x_rows}), Y {Y.shape[0]} (need {n_rows})")
    if not slab_layout_ok(X, Y, P):
        raise ValueError("mix_csr_slab: X, Y need 16-B aligned rows with strides % 4 == 0 and X readable to "
                         "round_up(P, 4) floats per row")
    for nm, t in (("ent", ent), ("hdr", hdr)):
        if t.device != X.device or t.dtype != torch.int32 or not t.is_contiguous():
            raise ValueError(f"{nm}: expected contiguous int32 on {X.device}")
    if hdr.numel() < int(_native.lib().dol_csr_slab_hdr_len(int(n_rows), x_rows)):
        raise ValueError("hdr too short for these row counts (rebuild with csr_slab_pack)")
    _native.call("dol_mix_csr_slab_f32", X.data_ptr(), ldx, x_rows, Y.data_ptr(), ldy, int(n_rows), P,
                 ent.data_ptr(), hdr.data_ptr(), _stream(X))
    return Y


def dense_to_csr(W: torch.Tensor, rowptr: Optional[torch.Tensor] = None, col: Optional[torch.Tensor] = None,
                 val: Optional[torch.Tensor] = None):
    """Neighbors (DIST/simulators.py:91-97) of every row of a dense device W, on
    the device (dol_dense_to_csr_f32): (rowptr, col, val) with col/val of
    capacity n*m (nnz = rowptr[-1], not synchronised to the host)."""
    ld = _check_rows("W", W)
    n, m = W.shape
    cap = n * m
    if rowptr is None or rowptr.numel() < n + 1:
        rowptr = torch.empty(n + 1, dtype=torch.int32, device=W.device)
    if col is None or col.numel() < cap:
        col = torch.empty(max(cap, 1), dtype=torch.int32, device=W.device)
    if val is None or val.numel() < cap:
        val = torch.empty(max(cap, 1), dtype=torch.float32, device=W.device)
    _native.call("dol_dense_to_csr_f32", W.data_ptr(), ld, n, m, rowptr.data_ptr(), col.data_ptr(), val.data_ptr(),
                 col.numel() if val.numel() >= col.numel() else val.numel(), _stream(W))
    return rowptr, col, val


# ---------------------------------------------------------------------------
# Dense W.
# ---------------------------------------------------------------------------
def _dense_args(W, X, Y, P, jacobi_pair: bool):
    """(P, ldw, ldx, ldy, M, K) of Y[M, P] = W[M, K] X[K, P].  jacobi_pair:
    X / Y are checked as a mix pair (mix_dense); else the op has an aliasing
    rule of its own."""
    P = X.shape[1] if P is None else P
    ldw = _check_rows("W", W)
    if jacobi_pair:
        ldx, ldy = _check_xy(X, Y, P, jacobi=False)
    else:
        ldx, ldy = _check_rows("X", X, P), _check_rows("Y", Y, P)
    M, K = W.shape
    if X.shape[0] < K or Y.shape[0] < M:
        raise ValueError(f"shapes: W {tuple(W.shape)}, X {tuple(X.shape)}, Y {tuple(Y.shape)}")
    return P, ldw, ldx, ldy, M, K


def mix_dense(W: torch.Tensor, X: torch.Tensor, Y: torch.Tensor, P: Optional[int] = None) -> torch.Tensor:
    """Y = W X on fp32 MFMA (fma chain over k; tolerance path, see dol_hip.h)."""
    P, ldw, ldx, ldy, M, K = _dense_args(W, X, Y, P, jacobi_pair=True)
    _native.call("dol_mix_dense_f32", W.data_ptr(), ldw, X.data_ptr(), ldx, Y.data_ptr(), ldy, M, K, P, _stream(X))
    return Y


def split3_x_flags(X: torch.Tensor, P: int) -> int:
    """DOL_SPLIT3_X_ROWS_PADDED when the GEMM may read X's rows in whole 16-B
    pieces up to round_up(P, 4) floats (aligned rows, ld % 4 == 0, storage
    present): X is then split in registers, with no split pass."""
    return SPLIT3_X_ROWS_PADDED if _rows_padded(X, P, ld4_of_one_row=False) else 0


def dense_split3_workspace_bytes(M: int, K: int, P: int, flags: int = 0) -> int:
    return int(_native.lib().dol_mix_dense_split3_workspace_bytes(int(M), int(K), int(P), int(flags)))


def mix_dense_split3(W: torch.Tensor, X: torch.Tensor, Y: torch.Tensor, P: Optional[int] = None,
                     work: Optional[torch.Tensor] = None, w_ready: bool = False,
                     fuse: Optional[bool] = None) -> torch.Tensor:
    """Y = W X on the bf16 matrix cores at fp32 accuracy (dol_mix_dense_split3_f32:
    three-piece bf16 split of both operands, six piece products per term).
    fuse (None = when X's rows allow it, split3_x_flags, and M <=
    SPLIT3_FUSE_MAX_M): X is split inside the GEMM (dense_split3_fxw_kernel:
    no split pass, no X workspace; same bits) instead of by a split pass.  Its
    GEMM runs ~6-8 % slower than the record-staged one, so it pays where the
    pass is a large share of the round, i.e. few output rows per X value:
    1024 x 1024 x 101,770 0.94-0.95 vs 1.04 ms, 8192 x 8192 x 101,770 56.2
    vs 53.1 ms (tools/split3_ab.py, profiles/r05m_split3_ab.jsonl,
    r05n_split3_ab_8192.jsonl).  fuse=False forces the split pass.  `work`: a uint8 device
    buffer of >= dense_split3_workspace_bytes(M, K, P, flags) bytes (allocated
    per call when None); w_ready=True reuses the split W that a previous call
    with the same W left in `work`."""
    P, ldw, ldx, ldy, M, K = _dense_args(W, X, Y, P, jacobi_pair=False)
    if Y.data_ptr() in (X.data_ptr(), W.data_ptr()):
        raise ValueError("Y aliases an input")
    if fuse is None:
        fuse = None if W.shape[0] <= SPLIT3_FUSE_MAX_M else False
    xf = split3_x_flags(X, P) if fuse is not False else 0
    fused = bool(xf) or (fuse is True and P % 4 == 0)
    flags = ((SPLIT3_FUSE_X | xf) if fused else 0) | (SPLIT3_W_READY if w_ready else 0)
    if work is None and w_ready:
        raise ValueError("w_ready needs the workspace of the call that split W")
    work = _workspace(work, dense_split3_workspace_bytes(M, K, P, flags), X.device, fresh=1, uint8=True)
    _native.call("dol_mix_dense_split3_f32", W.data_ptr(), ldw, X.data_ptr(), ldx, Y.data_ptr(), ldy, M, K, P,
                 work.data_ptr(), work.numel(), flags, _stream(X))
    return Y


def er_stochastic(W: torch.Tensor, p: float, seed: int) -> torch.Tensor:
    """W[n, >=n] <- a fresh Erdos-Renyi G(n, p) mixing matrix under the
    reference's 'stochastic' weighting, in one kernel (dol_er_stochastic_f32)."""
    ld = _check_rows("W", W)
    n = W.shape[0]
    if W.shape[1] < n:
        raise ValueError(f"W: expected [n, >= n], got {tuple(W.shape)}")
    _native.call("dol_er_stochastic_f32", W.data_ptr(), ld, n, float(p), int(seed) & (2**64 - 1), _stream(W))
    return W


# ---------------------------------------------------------------------------
# Primal / dual steps (FedProx, FedADMM).
# ---------------------------------------------------------------------------
def prox_admm_sgd(w: torch.Tensor, g: torch.Tensor, buf: Optional[torch.Tensor] = None,
                  theta: Optional[torch.Tensor] = None, alpha: Optional[torch.Tensor] = None,
                  rho: float = 0.0, lr: float = 0.01, momentum: float = 0.0, first_step: bool = False,
                  write_grad: bool = True, P: Optional[int] = None) -> None:
    """Fused FedProx/FedADMM gradient term + torch.optim.SGD(momentum) step, in place.

    Reference: DEC/clients.py:101-115, :125-139 and SGD.step (:44)."""
    P = w.shape[1] if P is None else P
    n = w.shape[0]
    ldw = _check_rows("w", w, P)
    ldg = _check_rows("g", g, P, n, "g has fewer rows than w")
    ldb = _check_momentum("buf", buf, momentum, P, n, "buf has fewer rows than w")
    lda = _check_prox_terms(theta, alpha, P, n, w.device)
    _native.call("dol_prox_admm_sgd_f32", w.data_ptr(), ldw, _ptr(buf) if ldb else None, ldb,
                 g.data_ptr(), ldg, _ptr(theta), _ptr(alpha), lda, float(rho), float(lr), float(momentum),
                 int(bool(first_step)), int(bool(write_grad)), n, P, _stream(w))


def admm_step_dual(w: torch.Tensor, g: torch.Tensor, theta: torch.Tensor, alpha: torch.Tensor,
                   buf: Optional[torch.Tensor] = None, rho: float = 0.0, lr: float = 0.01, momentum: float = 0.0,
                   first_step: bool = False, write_grad: bool = True, P: Optional[int] = None) -> None:
    """Last FedADMM local step + dual ascent in one pass (bit-identical to
    prox_admm_sgd(theta, alpha) followed by admm_dual)."""
    P = w.shape[1] if P is None else P
    n = w.shape[0]
    ldw = _check_rows("w", w, P)
    ldg = _check_rows("g", g, P, n, "g/alpha have fewer rows than w")
    lda = _check_rows("alpha", alpha, P, n, "g/alpha have fewer rows than w")
    ldb = _check_momentum("buf", buf, momentum, P, n, "buf has fewer rows than w")
    _check_vec("theta", theta, P, w.device)
    _native.call("dol_admm_step_dual_f32", w.data_ptr(), ldw, _ptr(buf) if ldb else None, ldb,
                 g.data_ptr(), ldg, theta.data_ptr(), alpha.data_ptr(), lda, float(rho), float(lr), float(momentum),
                 int(bool(first_step)), int(bool(write_grad)), n, P, _stream(w))


def prox_grad(g: torch.Tensor, w: torch.Tensor, theta: torch.Tensor, rho: float,
              alpha: Optional[torch.Tensor] = None, P: Optional[int] = None) -> None:
    """g += rho*(w - theta) (+ alpha), in place: the update_model gradient term alone
    (DEC/clients.py:108-111, :132-135)."""
    P = g.shape[1] if P is None else P
    n = g.shape[0]
    ldg = _check_rows("g", g, P)
    ldw = _check_rows("w", w, P, n, "w has fewer rows than g")
    lda = 0 if alpha is None else _check_rows("alpha", alpha, P, n, "alpha has fewer rows than g")
    _check_vec("theta", theta, P, g.device)
    _native.call("dol_prox_grad_f32", g.data_ptr(), ldg, w.data_ptr(), ldw, theta.data_ptr(), _ptr(alpha), lda,
                 float(rho), n, P, _stream(g))


def dual_workspace_bytes(n_agents: int, P: int) -> int:
    return int(_native.lib().dol_admm_dual_workspace_bytes(n_agents, P))


def admm_dual(alpha: torch.Tensor, w: torch.Tensor, theta: torch.Tensor, rho: float,
              resid_sq: Optional[torch.Tensor] = None, work: Optional[torch.Tensor] = None,
              P: Optional[int] = None) -> None:
    """alpha += rho*(w - theta) for every row (DEC/clients.py:141-144), in place."""
    P = alpha.shape[1] if P is None else P
    n = alpha.shape[0]
    lda = _check_rows("alpha", alpha, P)
    ldw = _check_rows("w", w, P, n, "w has fewer rows than alpha")
    _check_vec("theta", theta, P, alpha.device)
    if resid_sq is not None:
        if resid_sq.dtype != torch.float64 or resid_sq.numel() < n or resid_sq.device != alpha.device:
            raise ValueError("resid_sq: expected float64 [n_agents] on the same device")
        work = _workspace(work, dual_workspace_bytes(n, P), alpha.device, fresh=8, any_device=True)
    _native.call("dol_admm_dual_f32", alpha.data_ptr(), lda, w.data_ptr(), ldw, theta.data_ptr(), float(rho),
                 n, P, _ptr(resid_sq), _ptr(work) if resid_sq is not None else None, _stream(alpha))


def admm_ls_round_workspace_bytes(m: int, P: int) -> int:
    return int(_native.lib().dol_admm_ls_round_workspace_bytes(int(m), int(P)))


def _ls_round_args(w, alpha, target, theta, agents, buf, momentum, local_steps, P, duals: bool = True):
    """(P, n, ldw, lda, ldt, ldb) of a least-squares client round: the state
    matrices of w's n rows, theta, the step count and the sampled `agents`.
    duals=False (FedAvg / FedProx, fed_ls.py): alpha is not looked at, lda 0."""
    P = w.shape[1] if P is None else P
    n = w.shape[0]
    ldw = _check_rows("w", w, P)
    lda = _check_rows("alpha", alpha, P, n, "alpha/target have fewer rows than w") if duals else 0
    ldt = _check_rows("target", target, P, n, "alpha/target have fewer rows than w")
    _check_vec("theta", theta, P, w.device)
    if int(local_steps) < 0:
        raise ValueError("local_steps must be >= 0")
    ldb = _check_momentum("buf", buf, momentum, P, n, "buf has fewer rows than w")
    if agents is not None:
        _check_order(agents, w.device)
    return P, n, ldw, lda, ldt, ldb


def _check_distinct_agents(name: str, agents: Optional[torch.Tensor], n: int, validate: bool) -> int:
    """m of a round + mean: the number of sampled `agents` (None: all n rows),
    at least one and at most n.  validate: also that they are distinct rows
    in [0, n), on the host (one device-to-host copy of the m ids) -- except
    while the stream is being captured into a graph, where a copy to the host
    cannot be made: capture with ids that the caller has checked."""
    if agents is None:
        m = n
    else:
        m = agents.numel()
        if m > n:
            raise ValueError(f"{name}: {m} agents but w has {n} rows (agents must be distinct)")
        if validate and m:
            with torch.cuda.device(agents.device):
                capturing = torch.cuda.is_current_stream_capturing()
            if not capturing:
                ids = agents.cpu()
                if int(ids.min()) < 0 or int(ids.max()) >= n or torch.unique(ids).numel() != m:
                    raise ValueError(f"{name}: agents must be distinct rows in [0, {n})")
    if m < 1:
        raise ValueError(f"{name} needs at least one agent (the average indexes w[0])")
    return m


def _one_pass_outputs(w: torch.Tensor, m: int, P: int, first: Optional[torch.Tensor], outs, resid_total, work):
    """What the one-pass wrappers (round + mean, SCAFFOLD) share after their
    row checks: `first` is int32 [m]; each (name, vector) of `outs` is a float32
    [P] device vector, a fresh one where None; resid_total is float64 [2] and
    brings the workspace with it.  Returns (the output vectors, work)."""
    if first is not None:
        _check_array("first", first, torch.int32, m, w.device)
    vecs = [torch.empty(P, dtype=torch.float32, device=w.device) if t is None else t for _, t in outs]
    for (name, _), t in zip(outs, vecs):
        _check_vec(name, t, P, w.device)
    if resid_total is not None:
        _check_array("resid_total", resid_total, torch.float64, 2, w.device)
        work = _workspace(work, int(_native.lib().dol_admm_ls_round_mean_workspace_bytes(int(P))), w.device)
    return vecs, work


def _ls_round(entry: str, alg: Optional[int], w, alpha, target, theta, agents, first, buf, rho, lr, momentum,
              local_steps, resid_sq, alpha_sq, work, P) -> None:
    """The body of admm_ls_round (alg None: `entry` takes no algorithm) and of
    fed_ls.fed_ls_round (alg = DOL_FED_*, passed on to `entry`)."""
    duals = alg is None or alg == 2
    P, n, ldw, lda, ldt, ldb = _ls_round_args(w, alpha, target, theta, agents, buf, momentum, local_steps, P,
                                              duals=duals)
    m = n if agents is None else agents.numel()
    if first is not None:
        _check_array("first", first, torch.int32, m, w.device)
    if duals and (resid_sq is None) != (alpha_sq is None):
        raise ValueError("pass both resid_sq and alpha_sq or neither")
    if resid_sq is not None:
        _check_array("resid_sq", resid_sq, torch.float64, m, w.device)
        if duals:
            _check_array("alpha_sq", alpha_sq, torch.float64, m, w.device)
        work = _workspace(work, admm_ls_round_workspace_bytes(m, P), w.device)
    _native.call(entry, w.data_ptr(), ldw, _ptr(buf) if ldb else None, ldb, _ptr(alpha), lda, target.data_ptr(), ldt,
                 theta.data_ptr(), _ptr(agents), _ptr(first), m, P, *(() if alg is None else (alg,)), float(rho),
                 float(lr), float(momentum), int(local_steps), _ptr(resid_sq), _ptr(alpha_sq),
                 _ptr(work) if resid_sq is not None else None, _stream(w))


def _ls_round_mean(name: str, entry: str, alg: Optional[int], w, alpha, target, theta, agents, first, buf, rho, lr,
                   momentum, local_steps, out, scale, resid_total, work, P, validate) -> torch.Tensor:
    """The body of admm_ls_round_mean and of fed_ls.fed_ls_round_mean; `name`
    is the wrapper's, for the messages, and alg as in _ls_round."""
    P, n, ldw, lda, ldt, ldb = _ls_round_args(w, alpha, target, theta, agents, buf, momentum, local_steps, P,
                                              duals=alg is None or alg == 2)
    m = _check_distinct_agents(name, agents, n, validate)
    (out,), work = _one_pass_outputs(w, m, P, first, (("out", out),), resid_total, work)
    _native.call(entry, w.data_ptr(), ldw, _ptr(buf) if ldb else None, ldb, _ptr(alpha), lda, target.data_ptr(), ldt,
                 theta.data_ptr(), _ptr(agents), _ptr(first), m, P, *(() if alg is None else (alg,)), float(rho),
                 float(lr), float(momentum), int(local_steps), out.data_ptr(), float(m if scale is None else scale),
                 _ptr(resid_total), _ptr(work) if resid_total is not None else None, _stream(w))
    return out


def admm_ls_round(w: torch.Tensor, alpha: torch.Tensor, target: torch.Tensor, theta: torch.Tensor,
                  agents: Optional[torch.Tensor] = None, first: Optional[torch.Tensor] = None,
                  buf: Optional[torch.Tensor] = None, rho: float = 0.1, lr: float = 0.1, momentum: float = 0.0,
                  local_steps: int = 1, resid_sq: Optional[torch.Tensor] = None,
                  alpha_sq: Optional[torch.Tensor] = None, work: Optional[torch.Tensor] = None,
                  P: Optional[int] = None) -> None:
    """One FedADMM client round on f_a(w) = 1/2 ||w - t_a||^2 for the sampled
    rows `agents` (int32 device [m]; None = rows 0..n-1), fused per row
    (dol_admm_ls_round_f32): w = theta, `local_steps` x (LS gradient + ADMM
    term + momentum SGD), then the dual ascent.  first: int32 device [m],
    nonzero where that agent's optimizer takes its first step ever.
    resid_sq / alpha_sq: float64 [m] outputs (||w - theta||^2, ||alpha||^2).
    Reference: DEC/clients.py:36-53, :125-144 (update_weights, update_model,
    update_duals) with the CNN loss replaced by least squares."""
    _ls_round("dol_admm_ls_round_f32", None, w, alpha, target, theta, agents, first, buf, rho, lr, momentum,
              local_steps, resid_sq, alpha_sq, work, P)


def admm_ls_round_mean(w: torch.Tensor, alpha: torch.Tensor, target: torch.Tensor, theta: torch.Tensor,
                       agents: Optional[torch.Tensor] = None, first: Optional[torch.Tensor] = None,
                       buf: Optional[torch.Tensor] = None, rho: float = 0.1, lr: float = 0.1, momentum: float = 0.0,
                       local_steps: int = 1, out: Optional[torch.Tensor] = None, scale: Optional[float] = None,
                       resid_total: Optional[torch.Tensor] = None, work: Optional[torch.Tensor] = None,
                       P: Optional[int] = None, validate: bool = True) -> torch.Tensor:
    """admm_ls_round + the server's ordered average in ONE pass
    (dol_admm_ls_round_mean_f32): the rows come out as admm_ls_round leaves
    them and `out` = ordered_sum(w, agents, scale=scale) of the new rows, the
    same bits, without reading w back.  scale None = m (the mean,
    DEC/servers.py:42-48); 1.0 = the raw ordered sum.  agents: DISTINCT rows in
    the sampled order (None = 0..n-1).  resid_total: float64 [2] output, the
    round's sums over the agents of ||w - theta||^2 and ||alpha||^2.
    validate (default): check on the host that `agents` are distinct rows of w
    (one device-to-host copy of m ids).  The kernel loads the next agents'
    rows before it stores the current ones, so a repeated id would read a
    stale row, and an out-of-range id would read and write out of bounds
    (ADVICE r05).  Callers that drew the ids themselves on the host and
    checked them (SeparableADMM.round) pass validate=False.  The check is not
    made while the stream is being captured into a graph.
    Reference: DEC/servers.py:50-81 (Server.run's round) on least squares."""
    return _ls_round_mean("admm_ls_round_mean", "dol_admm_ls_round_mean_f32", None, w, alpha, target, theta, agents,
                          first, buf, rho, lr, momentum, local_steps, out, scale, resid_total, work, P, validate)


# ---------------------------------------------------------------------------
# Ordered reductions (the server's average).
# ---------------------------------------------------------------------------
def ordered_mean(W: torch.Tensor, order: torch.Tensor, out: Optional[torch.Tensor] = None,
                 P: Optional[int] = None) -> torch.Tensor:
    """theta = (((w[o0] + w[o1]) + ...) / m (DEC/servers.py:42-48)."""
    P = W.shape[1] if P is None else P
    ldw = _check_rows("W", W, P)
    _check_order(order, W.device)
    m = order.numel()
    if m < 1:
        raise ValueError("ordered_mean needs at least one row (the reference indexes w[0])")
    if out is None:
        out = torch.empty(P, dtype=torch.float32, device=W.device)
    _check_vec("out", out, P, W.device)
    _native.call("dol_ordered_mean_f32", W.data_ptr(), ldw, order.data_ptr(), m, P, out.data_ptr(), _stream(W))
    return out


def ordered_sum(W: torch.Tensor, order: torch.Tensor, acc_in: Optional[torch.Tensor] = None,
                out: Optional[torch.Tensor] = None, scale: float = 1.0, P: Optional[int] = None) -> torch.Tensor:
    P = (W.shape[1] if W is not None else acc_in.shape[0]) if P is None else P
    device = W.device if W is not None else acc_in.device
    ldw = _check_rows("W", W, P) if W is not None else P
    m = 0 if order is None else order.numel()
    if m:
        _check_order(order, device)
    _check_vec("acc_in", acc_in, P, device)
    if out is None:
        out = torch.empty(P, dtype=torch.float32, device=device)
    _check_vec("out", out, P, device)
    _native.call("dol_ordered_sum_f32", _ptr(W) if m else None, ldw, _ptr(order) if m else None, m, P,
                 _ptr(acc_in), out.data_ptr(), float(scale), torch.cuda.current_stream(device).cuda_stream)
    return out


# ---------------------------------------------------------------------------
# The fused MLP step.
# ---------------------------------------------------------------------------
def mlp_step(w: torch.Tensor, X: torch.Tensor, y: torch.Tensor, d: int, h: int, c: int,
             grad: Optional[torch.Tensor] = None, mom: Optional[torch.Tensor] = None,
             theta: Optional[torch.Tensor] = None, alpha: Optional[torch.Tensor] = None,
             loss: Optional[torch.Tensor] = None, lr: float = 0.01, momentum: float = 0.0, rho: float = 0.0,
             first_step: bool = False, update: bool = True,
             work: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
    """Fused forward + CE + backward + (prox/ADMM) momentum-SGD step of every
    agent's MLP Linear(d,h)-ReLU-Linear(h,c) (rows of w, state_dict order).

    X [n, B, d] fp32, y [n, B] int64.  update=False only writes the raw
    gradients into grad.  Reference: DIST/clients.py:34-59 (one local
    iteration per agent), DEC/clients.py:101-139 (prox / ADMM terms)."""
    P = h * d + h + c * h + c
    n = w.shape[0]
    ldw = _check_rows("w", w, P)
    if X.device != w.device or X.dtype != torch.float32 or X.dim() != 3 or X.shape[0] != n or X.shape[2] != d:
        raise ValueError(f"X: expected float32 [{n}, B, {d}] on {w.device}")
    if X.stride(2) != 1:
        raise ValueError("X: samples must be contiguous")
    B = X.shape[1]
    if y.device != w.device or y.dtype != torch.int64 or tuple(y.shape) != (n, B) or (B > 1 and y.stride(1) != 1):
        raise ValueError(f"y: expected int64 [{n}, {B}] on {w.device}")
    ldg = 0 if grad is None else _check_rows("grad", grad, P, n, "grad has fewer rows than w")
    ldm = _check_momentum("mom", mom, momentum if update else 0.0, P, n, "mom has fewer rows than w")
    lda = _check_prox_terms(theta, alpha, P, n, w.device)
    if loss is not None:
        _check_array("loss", loss, torch.float32, n, w.device, what="a contiguous")
    work = _workspace(work, int(_native.lib().dol_mlp_step_workspace_bytes(n, B, h)), w.device)
    ldxa = X.stride(0) if n > 1 else B * X.stride(1)
    ldxb = X.stride(1) if B > 1 else d
    _native.call("dol_mlp_step_f32", w.data_ptr(), ldw, _ptr(grad), ldg, _ptr(mom) if ldm else None, ldm,
                 _ptr(theta), _ptr(alpha), lda, X.data_ptr(), ldxa, ldxb, y.data_ptr(),
                 y.stride(0) if n > 1 else B, _ptr(loss), n, B, d, h, c, float(lr), float(momentum), float(rho),
                 int(bool(first_step)), int(bool(update)), work.data_ptr(), _stream(w))
    return loss


# ---------------------------------------------------------------------------
# The least-squares round of FedAvg / FedProx / FedADMM (fed_ls.py, which
# builds on the validators above): fed_ls_round, fed_ls_round_mean.
# ---------------------------------------------------------------------------
from .fed_ls import fed_ls_round, fed_ls_round_mean  # noqa: E402,F401

# ---------------------------------------------------------------------------
# The SCAFFOLD least-squares round beside them (scaffold.py, on the same
# validators; its own entry point, not a fourth FED_ALGORITHMS value):
# scaffold_ls_round.
# ---------------------------------------------------------------------------
from .scaffold import scaffold_ls_round  # noqa: E402,F401

# ---------------------------------------------------------------------------
# Multi-step consensus on the parameter-major bank (pm_steps.py, which builds
# on the validators above): mix_csr_pm_steps, dgd_csr_pm_steps.
# ---------------------------------------------------------------------------
from .pm_steps import dgd_csr_pm_steps, mix_csr_pm_steps, pm_steps_passes  # noqa: E402,F401

# ---------------------------------------------------------------------------
# Gradient tracking on the parameter-major bank, on the agent-major ring and
# on the agent-major bank with any sparse W (gt.py, which builds on the
# validators above and on pm_steps' square-W check): gt_csr_pm, gt_ring,
# gt_ring_edges (a sharded ring block's two boundary rows), gt_csr,
# separable_grad; gt_csr's push-sum form for column-stochastic weights,
# gt_push_csr; and its form with the gradient fed as a row matrix, gt_grad_csr.
# ---------------------------------------------------------------------------
from .gt import gt_csr, gt_csr_pm, gt_grad_csr, gt_push_csr, gt_ring, gt_ring_edges, separable_grad  # noqa: E402,F401

# ---------------------------------------------------------------------------
# EXTRA, the exact round that mixes the parameters only, on the agent-major
# bank and ring and on the parameter-major bank (extra.py, on the validators
# above and gt.py's): extra_csr, extra_ring, extra_ring_edges, extra_csr_pm;
# and extra_csr with the gradient fed as a row matrix, extra_grad_csr.
# ---------------------------------------------------------------------------
from .extra import extra_csr, extra_csr_pm, extra_grad_csr, extra_ring, extra_ring_edges  # noqa: E402,F401
