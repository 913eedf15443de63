"""GPU: a plain `bench.py` run (set-up, warm-up, the timed steps, the line - none of the `--full` legs) and what
`--dump-outputs` writes of the last timed step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_times_the_steps_and_dumps_the_last_ones_outputs(cuda, tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    out_dir = tmp_path / "outputs"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out_dir)], cwd=ROOT, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["steps"] == 3 and out["warmup"] == 1 and out["unit"] == "images/s" and out["higher_is_better"] is True
    assert out["dtype"] == "bf16" and out["ms_per_step"] > 0 and out["value"] > 0
    assert not {"roofline", "roofline_wgrad", "north_star_in_step", "cpu_baseline", "host_fed"} & set(out)
    names = sorted(f[:-4] for f in os.listdir(out_dir))
    assert names == ["grad", "logits_sample", "losses", "moving", "theta"], names
    arrays = {n: np.load(out_dir / f"{n}.npy") for n in names}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    assert arrays["losses"].shape == (8,) and arrays["losses"][6] == np.float32(out["config"]["final_total_loss"])
    assert arrays["theta"].shape == arrays["grad"].shape and np.abs(arrays["grad"]).max() > 0
