"""Pins on the emitted gfx950 code of the one-pass SCAFFOLD round (CPU tier:
reads the code object hipcc built, runs nothing).  scaffold_ls_round_kernel is
a sibling of admm_ls_round_mean_kernel, not a further instantiation of it, so
test_codegen_pins.py::test_admm_round_mean_is_packed_and_counted does not see
it; the same three pins are made here for every f4 instantiation."""
import re

import pytest

from test_codegen_pins import _disasm, _kernels, _unbundle


@pytest.fixture(scope="module")
def admm_code_object(tmp_path_factory):
    return _unbundle("admm.o", tmp_path_factory)


def test_scaffold_round_is_packed_and_counted(admm_code_object):
    """Packed fp32 local steps (v_pk_fma_f32 for the SGD update), row stores as
    buffer stores (dead lanes dropped out of range, so every lane issues the
    same memory ops) and counted vmcnt waits inside the agent loop -- not only
    full drains."""
    ks = [k for k in _kernels(admm_code_object, "scaffold_ls_round_kernel") if "Dv4_f" in k]
    assert len(ks) == 8, ks  # momentum x residuals x {1024, 256}-lane strips
    for k in ks:
        asm = _disasm(admm_code_object, k)
        assert "v_pk_fma_f32" in asm, k
        assert asm.count("buffer_store_dwordx4") >= 3, k  # w, c_k, momentum rows
        waits = [int(v) for v in re.findall(r"s_waitcnt vmcnt\((\d+)\)", asm)]
        assert any(w >= 3 for w in waits), f"{k}: no counted vmcnt wait"
        assert "scratch_" not in asm, f"{k}: spills to scratch"


def test_existing_round_template_has_no_new_instantiation(admm_code_object):
    """The FedAvg / FedProx / FedADMM rounds keep their 48 instantiations (f4 and
    scalar x momentum x residuals x strips x TERMS)."""
    assert len(_kernels(admm_code_object, "admm_ls_round_mean_kernel")) == 48
