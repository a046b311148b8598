"""bench.py's plain run (`--gpus 1 --steps K --warmup W`): only the headline is measured, `--steps` sets the timed steps and
`--dump-outputs DIR` writes what the last timed step computed (a fixed, seeded sample of SA and LCP as float64)."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
BENCH = str(ROOT / "bench.py")


def _run(args, timeout=600):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "SUFR_BENCH_FORCE_DIST"):
        env.pop(k, None)
    return subprocess.run([sys.executable, BENCH] + args, capture_output=True, text=True, timeout=timeout, env=env, cwd=str(ROOT))


def test_steps_below_one_are_refused():
    """(decided while parsing the arguments, before anything touches a GPU: runs in the CPU container too)"""
    r = _run(["--gpus", "1", "--steps", "0", "--warmup", "0"])
    assert r.returncode == 2 and "--steps" in r.stderr


@pytest.mark.gpu
def test_plain_run_times_the_headline_only_and_dumps_the_last_step(tmp_path):
    import torch
    import bench
    import sufr_amd
    out = tmp_path / "out"
    r = _run(["--gpus", "1", "--workload", "ecoli", "--steps", "3", "--warmup", "1", "--dump-outputs", str(out)])
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    j = json.loads(lines[0])
    assert j["steps"] == 3 and j["warmup"] == 1 and j["ms_per_step"] > 0
    assert j["value"] == pytest.approx(j["config"]["num_suffixes"] / (j["ms_per_step"] * 1e-3), rel=1e-9)
    for leg in ("cpu_baseline", "e2e_create", "host_abi", "search"):
        assert leg not in j, leg
    assert j["verified"] is None and "store_floor_ms" not in j["roofline"]
    sa, lcp = np.load(out / "sa.npy"), np.load(out / "lcp.npy")
    s = j["config"]["num_suffixes"]
    assert sa.dtype == lcp.dtype == np.float64 and sa.shape == lcp.shape == (min(s, bench.DUMP_SAMPLES),)
    assert sum((out / f).stat().st_size for f in ("sa.npy", "lcp.npy")) <= 64 * 2**20
    # the same build in this process, sampled the same way: the dumped arrays are what the timed path handed back
    gen, bases, flags, partitions, _ = bench.WORKLOADS["ecoli"]
    text, _ = gen(bases, device=torch.device("cuda", 0))
    db = sufr_amd.DeviceBuilder(0)
    want_sa, want_lcp = db.sort(text, raw_text=True, num_partitions=partitions, **flags)
    assert want_sa.numel() == s
    bench.dump_outputs(str(tmp_path / "want"), [(want_sa, want_lcp)])
    db.close()
    assert np.array_equal(np.load(tmp_path / "want" / "sa.npy"), sa)
    assert np.array_equal(np.load(tmp_path / "want" / "lcp.npy"), lcp)
