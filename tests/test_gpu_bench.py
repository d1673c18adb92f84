"""bench.py's plain run: --steps timed steps in one block, and --dump-outputs writes the records of
the last step, which are the oracle's for that step's text.  7 steps: one library call per block;
5000: beyond bench.PERIOD_STEPS, the block is issued as repeated periods of batches."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("steps", [7, 5000])
def test_plain_run_dumps_last_step(gpu, tmp_path, steps):
    import bench
    texts = 3
    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "2",
                        "--texts", str(texts), "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    rec = json.loads(p.stdout.strip().splitlines()[-1])
    assert rec["metric"] == "input_GB_per_s_scanned" and rec["unit"] == "GB/s" and rec["higher_is_better"] is True
    assert rec["steps"] == steps and rec["warmup"] == 2 and rec["repeats"] == 1 and len(rec["blocks_ms"]) == 1
    assert rec["ms_per_step"] > 0 and rec["value"] > 0
    assert "sub_records" not in rec and "cpu_baseline" not in rec and "roofline" not in rec

    arrays = {n: np.load(str(out / (n + ".npy"))) for n in ("offsets", "patterns", "final_state", "match_count")}
    assert all(a.dtype == np.float64 for a in arrays.values())
    # step k scans text k % texts, base text b generated from seed 7 + 64 b (bench.run_workload)
    wl = bench.Workload("clamav2000", 4096)
    o = wl.oracle()
    epos, epat, elast = o.scan(wl.text(7 + 64 * ((steps - 1) % texts)))
    o.close()
    assert epos.size > 0 and arrays["match_count"][0] == epos.size == rec["matches_per_step"]
    assert np.array_equal(arrays["offsets"], epos.astype(np.float64))
    assert np.array_equal(arrays["patterns"], epat.astype(np.float64))
    assert arrays["final_state"][0] == elast
