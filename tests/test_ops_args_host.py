"""dolhip.ops on a machine without a GPU: the public surface is complete and
every op that takes tensors refuses CPU tensors before it reaches the library
(ops._native.call is replaced by a recorder; nothing is launched)."""
import inspect

import pytest
import torch

from dolhip import ops
from dolhip.ops import DolNativeError
from test_ops_args_gpu import CALLS, Recorder

CPU = torch.device("cpu")


def _defined_public_names():
    names = set()
    for name, obj in vars(ops).items():
        if name.startswith("_") or inspect.ismodule(obj):
            continue
        if callable(obj):
            if getattr(obj, "__module__", None) == ops.__name__:
                names.add(name)
        elif name.isupper():
            names.add(name)
    return names


def test_all_lists_every_public_name():
    assert sorted(_defined_public_names() - set(ops.__all__)) == []


def test_all_names_exist():
    assert len(set(ops.__all__)) == len(ops.__all__)
    assert [n for n in ops.__all__ if not hasattr(ops, n)] == []


@pytest.fixture
def rec(monkeypatch):
    r = Recorder()
    monkeypatch.setattr(ops._native, "call", r)
    return r


@pytest.mark.parametrize("op", sorted(CALLS))
def test_cpu_tensors_are_refused(op, rec):
    make, call = CALLS[op]
    with pytest.raises(DolNativeError) as e:
        call(make(CPU))
    assert "cpu" in str(e.value) or str(e.value) == "stream_copy: device tensors required"
    assert rec.calls == []


def test_ordered_sum_without_rows_refuses_a_cpu_accumulator(rec):
    """W=None leaves acc_in as the only tensor: it is a valid vector on its own
    device, so the refusal is torch's own, from the lookup of that device's
    stream: a RuntimeError without a GPU, a ValueError ("expected a cuda
    device") with one."""
    with pytest.raises((RuntimeError, ValueError)) as e:
        ops.ordered_sum(None, None, torch.zeros(8), torch.zeros(8))
    assert type(e.value) in (RuntimeError, ValueError)
    assert rec.calls == []
