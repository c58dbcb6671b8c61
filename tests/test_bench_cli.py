"""bench.py's command line: a plain run prints the headline line alone, `--steps` sets the timed
steps, `--dump-outputs` writes what the last timed step computed (checked against the oracle), and
the dump stays inside its byte budget with a sample that depends on the seed and the size only."""

import importlib
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

fcg = importlib.import_module("4c_amd").fcg
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return b


def test_dump_sample_is_fixed_sorted_and_bounded():
    b = _bench_module()
    assert b._dump_sample(100, 100) is None  # fits: written whole
    idx = b._dump_sample(1_000_003, 5000)
    assert idx.dtype.kind == "i" and 0 < idx.size <= 5000
    assert idx.min() >= 0 and idx.max() < 1_000_003 and np.all(np.diff(idx) > 0)
    assert np.array_equal(idx, b._dump_sample(1_000_003, 5000))
    assert not np.array_equal(idx, b._dump_sample(1_000_004, 5000)[:idx.size])
    assert b.DUMP_BUDGET_BYTES <= 64 * 10**6


@pytest.mark.parametrize("world", [1, 2])
def test_dump_outputs_keeps_f_whole_samples_k_and_respects_the_budget(tmp_path, monkeypatch, world):
    import torch
    b = _bench_module()
    monkeypatch.setattr(b, "DUMP_BUDGET_BYTES", 8 * 1000 * world)  # 1000 doubles per rank
    rng = np.random.default_rng(7)
    f = torch.from_numpy(rng.standard_normal(300))
    K = torch.from_numpy(rng.standard_normal(5001))
    for d in ("a", "b"):
        for r in range(world):
            b.dump_outputs(str(tmp_path / d), f, K, r, world)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == (["K.npy", "f.npy"] if world == 1 else
                     ["K_rank0.npy", "K_rank1.npy", "f_rank0.npy", "f_rank1.npy"])
    total = 0
    for n in names:
        a = np.load(tmp_path / "a" / n)
        assert a.dtype == np.float64 and a.ndim == 1
        assert np.array_equal(a, np.load(tmp_path / "b" / n))
        total += a.nbytes
    assert total <= 8 * 1000 * world
    sfx = "" if world == 1 else "_rank0"
    assert np.array_equal(np.load(tmp_path / "a" / f"f{sfx}.npy"), f.numpy())
    Ks = np.load(tmp_path / "a" / f"K{sfx}.npy")
    assert np.array_equal(Ks, K.numpy()[b._dump_sample(5001, 700)])


@pytest.mark.gpu
def test_plain_run_prints_the_headline_alone_and_dumps_the_last_step(tmp_path):
    from parity_util import oracle_evaluate, rel_err
    n, steps = 6, 3
    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps",
                        str(steps), "--warmup", "1", "--elems-per-dir", str(n),
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == steps and d["warmup"] == 1 and d["dtype"] == "f64"
    assert d["unit"] == "element-evaluations/s" and d["higher_is_better"] is True
    assert d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(n ** 3 / (d["ms_per_step"] * 1e-3), rel=1e-9)
    # nothing beyond the headline was measured
    for k in ("secondary", "cpu_baseline", "roofline", "ranks"):
        assert k not in d
    mesh = fcg.BoxMesh(fcg.HEX8, (n, n, n), jitter=0.1, seed=20251015)
    err, _, Kr, fr = oracle_evaluate(mesh, fcg.LINEAR, 210.0, 0.3, mesh.u_col(1e-3))
    assert err == 0
    assert sorted(os.listdir(out)) == ["K.npy", "f.npy"]
    f, K = np.load(out / "f.npy"), np.load(out / "K.npy")
    assert f.dtype == np.float64 and K.dtype == np.float64
    assert f.shape == fr.shape and K.shape == Kr.shape  # small enough to be written whole
    assert rel_err(f, fr) <= 1e-10 and rel_err(K, Kr) <= 1e-12
