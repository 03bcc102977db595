"""bench.py without --full: set-up, warm-up, the timed steps, --dump-outputs and one JSON line whose headline keys mean what
they always did -- and nothing measured after the timed region (stage split, siblings, extras, CPU baseline: those are --full's)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

FULL_ONLY = ("stages_ms", "transformer_ms", "transformer_roofline", "fp32_exact", "parity", "boundary", "batched", "slab512", "sf3d",
             "parity_mode")


def test_plain_run_measures_the_headline_alone(cuda, tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--dump-outputs", str(tmp_path / "out")]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{"metric"')]
    assert len(lines) == 1, p.stdout[-3000:]
    d = json.loads(lines[0])
    assert d["unit"] == "meshes/s" and d["higher_is_better"] is True and d["n_gpus"] == 1
    assert d["steps"] == 3 and d["warmup"] == 1
    assert abs(d["value"] - 3 / (d["ms_per_step"] * 3e-3)) < 1e-6 * d["value"]
    assert "filtered grid" in d["dtype"] and d["config"]["decoder_filter"] is True
    assert d["roofline"]["launch_ms"] > 0
    # the identity check still decides whether the timed steps use the two-pass grid; its pass timings are --full's
    filt = d["density"]["filtered"]
    assert filt["mesh_identical"] is True and filt["sign_mismatches_vs_full"] == 0 and filt["used_for_value"] is True
    assert filt["pass_a_ms"] is None and "full" not in d["density"]
    assert d["cpu_baseline"] is None
    assert not [k for k in FULL_ONLY if k in d], [k for k in FULL_ONLY if k in d]
    shape = np.load(tmp_path / "out" / "mesh_shape.npy")
    assert shape.tolist() == [d["config"]["mesh"]["vertices"], d["config"]["mesh"]["faces"]]
