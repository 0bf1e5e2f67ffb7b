"""Multi-step consensus on the parameter-major bank: X <- W^k X, the inner loop
of FedLCon's round (DIST/simulators.py:190-196, each step the consensus of
DIST/clients.py:61-69), in one HBM pass for any sparse W
(dol_mix_csr_pm_steps_f32), and that loop fused with config 3's local steps
(dol_dgd_csr_pm_steps_f32).  ops re-exports both calls as
ops.mix_csr_pm_steps / ops.dgd_csr_pm_steps.  Their argument rules are the
validators of ops.py (_pm_args, _dgd_args) plus the three stated here: a step
count >= 1, a square W, and the split of a count above
ops.PM_MAX_FUSED_STEPS into passes; tests/test_pm_steps_args_host.py pins
them without a launch.
"""
from __future__ import annotations

from typing import List, Optional

import torch

from . import _native
from . import ops as _ops

_SQUARE_OK: dict = {}  # CSR triples whose columns were checked against n (see _check_square)


def pm_steps_fused(n: int, steps: int) -> bool:
    """Whether `steps` > 1 mixing rounds on n agents run as one fused pass (the
    measured table of DESIGN.md §4.1: the fused pass won at every agent count
    and step count measured, so this is true wherever the kernel applies)."""
    return steps > 1 and n <= _ops.PM_MAX_AGENTS


def pm_steps_passes(n: int, steps: int) -> List[int]:
    """The launches that make up `steps` mixing rounds on n agents: fused
    passes of at most ops.PM_MAX_FUSED_STEPS steps each, full ones first
    (130 -> [64, 64, 2]); single steps where pm_steps_fused says the fused
    pass does not pay.  Pass i reads what pass i - 1 wrote."""
    steps = int(steps)
    if steps < 1:
        raise ValueError("steps must be >= 1")
    if not pm_steps_fused(n, steps):
        return [1] * steps
    cap = _ops.PM_MAX_FUSED_STEPS
    return [cap] * (steps // cap) + ([steps % cap] if steps % cap else [])


def _check_square(rowptr: torch.Tensor, col: torch.Tensor, n: int) -> None:
    """W^k needs a square W: every column index below n = rowptr length - 1
    (the kernel gathers step t + 1 from step t's n outputs).  The indices live
    on the device, so the first call with a CSR reads them back once; the
    answer is kept per (buffers, versions).  Not looked at while the stream is
    being captured into a graph (no read-back there): capture a W that an
    earlier call has checked."""
    key = (rowptr.data_ptr(), col.data_ptr(), n, rowptr._version, col._version)
    if key in _SQUARE_OK:
        return
    with torch.cuda.device(col.device):
        if torch.cuda.is_current_stream_capturing():
            return
    nnz = int(rowptr[n]) if n > 0 else 0
    if nnz > col.numel():
        raise ValueError(f"col: {col.numel()} entries < rowptr[-1] = {nnz}")
    if nnz:
        lo, hi = (int(v) for v in torch.aminmax(col[:nnz]))
        if lo < 0 or hi >= n:
            raise ValueError(f"multi-step mixing needs a square W: column indices in [{lo}, {hi}], agents {n}")
    if len(_SQUARE_OK) >= 256:
        _SQUARE_OK.clear()
    _SQUARE_OK[key] = True


def _steps_args(XT, YT, rowptr, col, val, steps, P):
    """(P, n, ldx, ldy, passes) of a multi-step parameter-major op."""
    if int(steps) < 1:
        raise ValueError("steps must be >= 1")
    P, n, _, ldx, ldy = _ops._pm_args(XT, YT, rowptr, col, val, None, P)
    if int(steps) > 1:
        _check_square(rowptr, col, n)
    return P, n, ldx, ldy, pm_steps_passes(n, steps)


def _auto_nseg(XT, YT, rowptr, col, val, ldx, ldy, n, P) -> int:
    return _ops._pm_auto(_ops._pm_mix(XT, YT, rowptr, col, val, ldx, ldy, n, n, P), XT, YT, ldx, ldy, n, n, P)


def _mix_pass(src, lds, dst, ldd, n, P, rowptr, col, val, k, nseg) -> None:
    _native.call("dol_mix_csr_pm_steps_ex_f32", src.data_ptr(), lds, dst.data_ptr(), ldd, n, P, rowptr.data_ptr(),
                 _ops._ptr_unless_empty(col), _ops._ptr_unless_empty(val), int(k), int(nseg), _ops._stream(src))


def mix_csr_pm_steps(XT: torch.Tensor, YT: torch.Tensor, rowptr: torch.Tensor, col: torch.Tensor, val: torch.Tensor,
                     steps: int, P: Optional[int] = None, nseg: Optional[int] = None) -> torch.Tensor:
    """W^steps XT on the parameter-major bank (buffers as ops.mix_csr_pm, W
    square), bit-identical to `steps` mix_csr_pm calls, the bank crossing HBM
    once per pass instead of once per step.  Returns the buffer that holds the
    result.  Up to ops.PM_MAX_FUSED_STEPS steps are one pass: the result is
    in YT and XT is untouched.  More steps run as several passes
    (pm_steps_passes) that swap the two buffers, so XT is overwritten and the
    result is in YT after an odd number of passes, in XT after an even one.
    nseg as mix_csr_pm (None: the order tuned for this buffer pair on the
    plain mix).  Reference: DIST/simulators.py:190-196 + DIST/clients.py:61-69."""
    P, n, ldx, ldy, passes = _steps_args(XT, YT, rowptr, col, val, steps, P)
    if nseg is None:
        nseg = _auto_nseg(XT, YT, rowptr, col, val, ldx, ldy, n, P)
    src, lds, dst, ldd = XT, ldx, YT, ldy
    for k in passes:
        _mix_pass(src, lds, dst, ldd, n, P, rowptr, col, val, k, nseg)
        src, lds, dst, ldd = dst, ldd, src, lds
    return src


def dgd_csr_pm_steps(XT: torch.Tensor, YT: torch.Tensor, rowptr: torch.Tensor, col: torch.Tensor, val: torch.Tensor,
                     TT: torch.Tensor, MT: Optional[torch.Tensor] = None, objective: str = "least_squares",
                     mix_steps: int = 1, steps: int = 1, lr: float = 0.01, momentum: float = 0.0,
                     first_step: bool = False, P: Optional[int] = None, nseg: Optional[int] = None) -> torch.Tensor:
    """FedLCon's round on the parameter-major bank: mix_steps mixing rounds,
    then `steps` local momentum-SGD iterations (arguments as ops.dgd_csr_pm, W
    square), bit-identical to mix_steps - 1 mix_csr_pm calls and one
    dgd_csr_pm.  Up to ops.PM_MAX_FUSED_STEPS mixing steps are one kernel;
    beyond that the leading passes are plain mixes (mix_csr_pm_steps) and the
    last pass carries the local steps.  Returns the buffer that holds the
    result, by the same rule as mix_csr_pm_steps.  At most
    ops.PM_DGD_MAX_AGENTS agents."""
    P, n, ldx, ldy, passes = _steps_args(XT, YT, rowptr, col, val, mix_steps, P)
    ldt, ldm = _ops._dgd_args(XT.device, TT, MT, objective, steps, momentum, P, n, pm=True)
    if n > _ops.PM_DGD_MAX_AGENTS:
        raise ValueError(f"the fused round takes at most {_ops.PM_DGD_MAX_AGENTS} agents (got {n})")
    if nseg is None:
        nseg = _auto_nseg(XT, YT, rowptr, col, val, ldx, ldy, n, P)
    src, lds, dst, ldd = XT, ldx, YT, ldy
    for k in passes[:-1]:
        _mix_pass(src, lds, dst, ldd, n, P, rowptr, col, val, k, nseg)
        src, lds, dst, ldd = dst, ldd, src, lds
    _native.call("dol_dgd_csr_pm_steps_ex_f32", src.data_ptr(), lds, dst.data_ptr(), ldd, n, P, rowptr.data_ptr(),
                 _ops._ptr_unless_empty(col), _ops._ptr_unless_empty(val), TT.data_ptr(), ldt,
                 _ops._ptr(MT) if ldm else None, ldm, _ops.OBJECTIVES[objective], int(passes[-1]), int(steps),
                 float(lr), float(momentum), int(bool(first_step)), int(nseg), _ops._stream(src))
    return dst
