"""-m gpu: the plain bench run as it is timed -- the headline line alone, exactly --steps timed steps, and --dump-outputs writing
the records of the last timed step, bit for bit the same from run to run (the inputs are seeded)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_run_dumps_the_same_outputs_twice(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "AGT_DIST_BACKEND")}
    got = []
    for i in range(2):
        d = tmp_path / ("out%d" % i)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "64", "--warmup", "8", "--dump-outputs", str(d)],
                           env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1
        j = json.loads(lines[0])
        assert j["unit"] == "frames/s" and j["higher_is_better"] is True and j["value"] > 0 and j["ms_per_step"] > 0
        assert j["steps"] == 64 and j["timing"]["blocks"] == 1 and j["gathered_shape"] == [1, 64, 1, 16]
        assert j["roofline"] is None and j["cpu_baseline"] is None and "batch64_hbm" not in j       # (--full only)
        assert j["accepted_frac"] == 1.0 and j["chain_timeouts"] == 0
        assert sorted(os.listdir(d)) == ["records.npy"]
        got.append(np.load(d / "records.npy"))
    rec = got[0]
    assert rec.dtype == np.float64 and rec.shape == (1, 1, 16)
    assert rec[0, 0, 6] == 1.0 and rec[0, 0, 8] >= 8           # accepted, from at least the minimum of tracked corners
    assert np.array_equal(got[0].view(np.uint64), got[1].view(np.uint64))
