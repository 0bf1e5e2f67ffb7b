"""ops.mix_csr_pm_steps / ops.dgd_csr_pm_steps on a machine without a GPU,
launch-free like tests/test_ops_args_host.py (ops._native.call is replaced by
a recorder): the surface is there, bad arguments are refused before the
library is reached, the split of a step count above the cap into passes is
right, and the chained passes swap the buffers and report the one that holds
the result."""
import os
import re

import pytest
import torch

from conftest import ROOT
from dolhip import _native, ops, pm_steps
from dolhip.ops import DolNativeError
from test_ops_args_gpu import Recorder, mat, vec

CPU = torch.device("cpu")
I32 = torch.int32


@pytest.fixture
def rec(monkeypatch):
    r = Recorder()
    monkeypatch.setattr(ops._native, "call", r)
    return r


def _args(dev):
    return dict(XT=mat(dev, 10, 2, 4), YT=mat(dev, 10, 2, 4), rowptr=vec(dev, 3, I32), col=vec(dev, 4, I32),
                val=vec(dev, 4))


def test_surface():
    assert ops.PM_MAX_FUSED_STEPS == 64 and "PM_MAX_FUSED_STEPS" in ops.__all__
    assert ops.mix_csr_pm_steps is pm_steps.mix_csr_pm_steps and ops.dgd_csr_pm_steps is pm_steps.dgd_csr_pm_steps
    with open(os.path.join(ROOT, "include", "dol_hip.h")) as f:
        assert re.search(r"#define DOL_PM_MAX_FUSED_STEPS (\d+)", f.read()).group(1) == "64"


def test_native_table_carries_the_four_signatures():
    want = {"dol_mix_csr_pm_steps_f32": 11, "dol_mix_csr_pm_steps_ex_f32": 12, "dol_dgd_csr_pm_steps_f32": 20,
            "dol_dgd_csr_pm_steps_ex_f32": 21}
    table = next(v for v in vars(_native).values() if isinstance(v, dict) and "dol_mix_csr_pm_ex_f32" in v)
    assert {k: len(table[k]) for k in want} == want
    # the _ex calls take the single-step signature minus x_rows plus the step count
    assert len(table["dol_mix_csr_pm_steps_ex_f32"]) == len(table["dol_mix_csr_pm_ex_f32"])
    assert len(table["dol_dgd_csr_pm_steps_ex_f32"]) == len(table["dol_dgd_csr_pm_ex_f32"])


@pytest.mark.parametrize("steps,want", [(1, [1]), (2, [2]), (64, [64]), (65, [64, 1]), (128, [64, 64]),
                                        (130, [64, 64, 2])])
def test_split_into_passes(steps, want):
    assert ops.pm_steps_passes(1024, steps) == want
    assert sum(want) == steps and max(want) <= ops.PM_MAX_FUSED_STEPS


@pytest.mark.parametrize("steps", [0, -3])
def test_step_counts_below_one_are_refused(steps, rec):
    t = _args(CPU)
    with pytest.raises(ValueError, match="steps must be >= 1"):
        ops.pm_steps_passes(1024, steps)
    with pytest.raises(ValueError, match="steps must be >= 1"):
        ops.mix_csr_pm_steps(t["XT"], t["YT"], t["rowptr"], t["col"], t["val"], steps)
    with pytest.raises(ValueError, match="steps must be >= 1"):
        ops.dgd_csr_pm_steps(t["XT"], t["YT"], t["rowptr"], t["col"], t["val"], t["XT"].clone(), mix_steps=steps)
    assert rec.calls == []


def test_cpu_tensors_are_refused(rec):
    t = _args(CPU)
    for call in (lambda: ops.mix_csr_pm_steps(t["XT"], t["YT"], t["rowptr"], t["col"], t["val"], 3, P=10, nseg=8),
                 lambda: ops.dgd_csr_pm_steps(t["XT"], t["YT"], t["rowptr"], t["col"], t["val"], mat(CPU, 10, 2, 4),
                                              mat(CPU, 10, 2, 4), mix_steps=3, steps=2, momentum=0.5, P=10, nseg=8)):
        with pytest.raises(DolNativeError, match="cpu"):
            call()
    assert rec.calls == []


@pytest.fixture
def no_device(monkeypatch):
    """Let the two ops run to their (recorded) library calls on CPU tensors:
    the per-tensor validators and the read-back of W's columns are ops.py's
    and the GPU suite's business; here only the chaining of passes is."""
    monkeypatch.setattr(ops, "_pm_args", lambda XT, YT, rowptr, col, val, x_agents, P: (P, 2, 2, 4, 4))
    monkeypatch.setattr(ops, "_dgd_args", lambda *a, **k: (4, 4))
    monkeypatch.setattr(ops, "_stream", lambda t: 0)
    monkeypatch.setattr(pm_steps, "_check_square", lambda rowptr, col, n: None)


@pytest.mark.parametrize("steps,holder", [(5, "YT"), (65, "XT"), (130, "YT")])
def test_mix_passes_swap_buffers_and_report_the_holder(steps, holder, rec, no_device):
    t = _args(CPU)
    out = ops.mix_csr_pm_steps(t["XT"], t["YT"], t["rowptr"], t["col"], t["val"], steps, P=10, nseg=8)
    assert out is t[holder]
    x, y = t["XT"].data_ptr(), t["YT"].data_ptr()
    passes = ops.pm_steps_passes(2, steps)
    assert [(n, a[0], a[2], a[9], a[10]) for n, a in rec.calls] == [
        ("dol_mix_csr_pm_steps_ex_f32", (x, y)[i % 2], (y, x)[i % 2], k, 8) for i, k in enumerate(passes)]
    assert rec.calls[-1][1][2] == out.data_ptr()


def test_round_runs_plain_passes_then_one_fused_pass(rec, no_device):
    t = _args(CPU)
    TT, MT = mat(CPU, 10, 2, 4), mat(CPU, 10, 2, 4)
    out = ops.dgd_csr_pm_steps(t["XT"], t["YT"], t["rowptr"], t["col"], t["val"], TT, MT, objective="logistic",
                               mix_steps=130, steps=2, lr=0.5, momentum=0.25, first_step=True, P=10, nseg=16)
    x, y = t["XT"].data_ptr(), t["YT"].data_ptr()
    assert out is t["YT"]
    assert [(n, a[0], a[2]) for n, a in rec.calls] == [
        ("dol_mix_csr_pm_steps_ex_f32", x, y), ("dol_mix_csr_pm_steps_ex_f32", y, x),
        ("dol_dgd_csr_pm_steps_ex_f32", x, y)]
    assert [a[9] for _, a in rec.calls[:2]] == [64, 64]
    last = rec.calls[-1][1]
    assert last[9:] == (TT.data_ptr(), 4, MT.data_ptr(), 4, 1, 2, 2, 0.5, 0.25, 1, 16, 0)
