"""CPU: bench.py's multi-rank launcher: `--gpus N`
without torchrun spawns N ranks itself and the emitted line reports them;
a --gpus / WORLD_SIZE mismatch fails loudly. The step is the --dry-run
stand-in (gloo, no GPU)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env=None):
    e = dict(os.environ)
    e.pop("WORLD_SIZE", None)
    e.update(env or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--dry-run"] + args,
                          capture_output=True, text=True, timeout=240, env=e)


@pytest.mark.timeout(300)
def test_bench_spawns_two_ranks():
    r = _run(["--gpus", "2", "--steps", "5", "--warmup", "1", "--full"])
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(line) == 1
    d = json.loads(line[0])
    assert d["n_gpus"] == 2 and d["world_size"] == 2 and d["backend"] == "gloo" and d["dry_run"]
    # at N > 1 the run measures configs[1] (headline) and configs[3]'s 64/GPU bf16 share
    wl = {w["config"]: w for w in d["workloads"]}
    assert wl["configs[1]"]["global_batch"] == 16 and wl["configs[1]"]["dtype"] == "f32"
    assert wl["configs[3]"]["global_batch"] == 128 and wl["configs[3]"]["dtype"] == "bf16"


def test_bench_rejects_world_mismatch():
    r = _run(["--gpus", "1"], env={"WORLD_SIZE": "2"})
    assert r.returncode != 0 and "WORLD_SIZE=2" in (r.stderr + r.stdout)


def test_plain_dry_run_plans_the_headline_only_and_dumps(tmp_path):
    """Without --full the run measures the headline alone; --dump-outputs
    writes float32 .npy files, identical from run to run."""
    import numpy as np
    outs = []
    for d in ("a", "b"):
        r = _run(["--gpus", "1", "--steps", "3", "--warmup", "1",
                  "--dump-outputs", str(tmp_path / d)])
        assert r.returncode == 0, r.stderr[-2000:]
        line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][0])
        assert [w["role"] for w in line["workloads"]] == ["headline"]
        assert line["steps"] == 3 and line["ms_per_step"] >= 0
        outs.append(np.load(tmp_path / d / "buf.npy"))
    assert outs[0].dtype == np.float32 and np.array_equal(outs[0], outs[1])


def test_dump_array_samples_large_outputs_at_fixed_positions():
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    small = torch.arange(12, dtype=torch.bfloat16).reshape(3, 4)
    a = bench.dump_array(small)
    assert a.dtype == np.float32 and a.shape == (3, 4)
    assert bench.dump_array(small.double()).dtype == np.float64
    n = 3 * bench.DUMP_MAX_ELEMS + 7
    big = torch.arange(n, dtype=torch.float32).reshape(-1, 1)   # n < 2^24: exact
    s1, s2 = bench.dump_array(big), bench.dump_array(big.clone())
    assert s1.shape == (bench.DUMP_MAX_ELEMS,) and s1.nbytes * 5 <= 64e6
    assert np.array_equal(s1, s2) and np.all(np.diff(s1) >= 0)
    assert s1.min() >= 0 and s1.max() < n and s1.max() > 0.99 * n
