"""Host-side pieces of bench.py that shape the reported numbers (no GPU):
the a n^2 + b n extrapolation of the CPU baselines, and the JSON contract's
kernel names for every ring-steps variant the product path may pick."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_fit_n2_n_recovers_exact_model(bench):
    a, b = 3e-7, 2e-4
    samples = {n: 1.0 / (a * n * n + b * n) for n in (128, 256)}
    fit = bench._fit_n2_n(samples, 1024)
    assert fit["a_s_per_agent2"] == pytest.approx(a, rel=1e-9)
    assert fit["b_s_per_agent"] == pytest.approx(b, rel=1e-9)
    assert fit["rounds_per_s"] == pytest.approx(1.0 / (a * 1024 ** 2 + b * 1024), rel=1e-9)


def test_fit_n2_n_linear_cost_is_not_squared(bench):
    """a per-agent (linear) cost must extrapolate linearly, not as n^2."""
    samples = {n: 1.0 / (1e-3 * n) for n in (128, 256)}
    fit = bench._fit_n2_n(samples, 1024)
    assert fit["rounds_per_s"] == pytest.approx(1.0 / (1e-3 * 1024), rel=1e-6)


def test_fit_n2_n_noise_cannot_make_a_coefficient_negative(bench):
    """with samples whose exact solve has b < 0 (the middle size
    slow, the largest fast), the fit stays in a, b >= 0 and the extrapolated
    rate stays positive and finite."""
    samples = {64: 1.0 / 0.010, 128: 1.0 / 0.030, 256: 1.0 / 0.050}
    fit = bench._fit_n2_n(samples, 1024)
    assert fit["a_s_per_agent2"] >= 0.0 and fit["b_s_per_agent"] >= 0.0
    assert fit["rounds_per_s"] is not None and 0 < fit["rounds_per_s"] < samples[256]
    # a pure n^2 cost with one noisy point: a > 0 and a rate below the largest sample's
    noisy = {64: 1.0 / (1e-6 * 64 ** 2), 128: 1.0 / (1e-6 * 128 ** 2 * 1.2), 256: 1.0 / (1e-6 * 256 ** 2 * 0.9)}
    f2 = bench._fit_n2_n(noisy, 1024)
    assert f2["a_s_per_agent2"] > 0 and f2["b_s_per_agent"] >= 0 and f2["rounds_per_s"] < noisy[256]


def test_plain_run_is_headline_only_and_full_restores_the_rest(bench, monkeypatch):
    """Without --full every leg beside the headline is off; with it each leg
    follows its own --no-* switch as before."""
    import sys
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    assert a.no_cpu and a.no_copy and a.no_primal_dual
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full"])
    a = bench.parse()
    assert a.full and not (a.no_cpu or a.no_copy or a.no_primal_dual)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--no-cpu", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.no_cpu and not a.no_copy and not a.no_primal_dual and a.dump_outputs == "d"


def _fake_ring(n, P, ld):
    import types

    import torch
    x = torch.arange(n * ld, dtype=torch.float32).reshape(n, ld)
    return types.SimpleNamespace(n_local=n, P=P, x=x)


def test_dump_outputs_small_matrix_is_written_whole(bench, tmp_path):
    import numpy as np
    ring = _fake_ring(5, 37, 40)
    info = bench.dump_outputs(str(tmp_path / "o"), ring, 1, 0)
    x = np.load(tmp_path / "o" / "x.npy")
    assert x.dtype == np.float32 and x.shape == (5, 37)
    assert np.array_equal(x, ring.x[:, :37].numpy())
    assert info["arrays"] == {"x": [5, 37]} and info["bytes"] == x.nbytes


def test_dump_outputs_large_matrix_is_a_fixed_sample(bench, tmp_path, monkeypatch):
    """Above the budget: whole rows (first and last among them) and columns over
    all rows, the same indices on every call, within the budget."""
    import numpy as np
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4096)
    ring = _fake_ring(33, 101, 128)
    full = ring.x[:, :101].numpy()
    info = bench.dump_outputs(str(tmp_path / "a"), ring, 1, 0)
    bench.dump_outputs(str(tmp_path / "b"), ring, 2, 1)
    got = {p.name[:-4]: np.load(p) for p in (tmp_path / "a").iterdir()}
    assert set(got) == {"x_rows", "x_cols", "x_rows_index", "x_cols_index"}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    rows, cols = got["x_rows_index"].astype(int), got["x_cols_index"].astype(int)
    assert rows[0] == 0 and rows[-1] == 32 and len(set(rows)) == len(rows) == 2048 // (101 * 4)
    assert len(set(cols)) == len(cols) == 2048 // (33 * 4)
    assert np.array_equal(got["x_rows"], full[rows]) and np.array_equal(got["x_cols"], full[:, cols])
    assert info["bytes"] <= 4096 + 8 * (len(rows) + len(cols))
    for name, a in got.items():  # the other rank's files: same sample, suffixed names
        assert np.array_equal(np.load(tmp_path / "b" / f"{name}.rank1.npy"), a)


def _bench_env(**extra):
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "DOL_BENCH_FAIL_RANK")}
    env.update(DOL_DIST_BACKEND="gloo", DOL_DEVICE_MAP="0", **extra)
    return env


def _run(cmd, env, timeout=240):
    import subprocess
    import sys
    return subprocess.run([sys.executable, *cmd], cwd=ROOT, env=env, capture_output=True, text=True,
                          timeout=timeout)


def test_bench_gpus_n_spawns_n_ranks_itself():
    """`python bench.py --gpus 2` with no launcher around it
    starts two ranks itself and the relayed line says n_gpus 2, with the world
    size and backend each rank saw."""
    import json
    r = _run(["bench.py", "--gpus", "2", "--launch-check"], _bench_env())
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [s for s in r.stdout.splitlines() if s.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2
    par = line["parallel"]
    assert par["world_size"] == 2 and par["backend"] == "gloo"
    assert [i["rank"] for i in par["ranks"]] == [0, 1]
    assert all(i["world_size"] == 2 and i["backend"] == "gloo" for i in par["ranks"])
    assert all(i["launcher"].startswith("bench.py") for i in par["ranks"])
    assert len({i["pid"] for i in par["ranks"]}) == 2


def test_bench_under_torchrun_keeps_working():
    import json
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    r = _run(["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
              "--master-port", str(port), "bench.py", "--gpus", "2", "--launch-check"], _bench_env())
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([s for s in r.stdout.splitlines() if s.startswith("{")][0])
    assert line["n_gpus"] == 2
    assert all(i["launcher"] == "torch.distributed.run" for i in line["parallel"]["ranks"])


def test_bench_refuses_fewer_ranks_than_asked():
    """A run whose joined world differs from --gpus exits non-zero (it used to
    warn and time one GPU)."""
    r = _run(["bench.py", "--gpus", "2", "--launch-check"], _bench_env(WORLD_SIZE="1", RANK="0", LOCAL_RANK="0"))
    assert r.returncode == 2
    assert not [s for s in r.stdout.splitlines() if s.startswith("{")]


def test_bench_spawned_rank_failure_fails_the_run():
    """A rank that dies makes the launcher stop the others and exit non-zero
    without relaying a line (not after the collective timeout)."""
    import time
    t0 = time.time()
    r = _run(["bench.py", "--gpus", "3", "--launch-check"], _bench_env(DOL_BENCH_FAIL_RANK="1",
                                                                       DOL_COLLECTIVE_TIMEOUT_S="600"))
    assert r.returncode != 0
    assert not [s for s in r.stdout.splitlines() if s.startswith("{")]
    assert time.time() - t0 < 120


def test_every_ring_steps_variant_has_a_kernel_name(bench):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "distributed-optimization-and-learning_amd"))
    from dolhip import ops
    assert set(ops.RING_STEPS_VARIANTS) <= set(bench.RING_STEPS_KERNELS)
