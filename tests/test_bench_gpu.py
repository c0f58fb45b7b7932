"""bench.py's plain run (the invocation timed for every change) on the MI355X: exactly --steps timed objects, the headline fields
and nothing that --full adds, and --dump-outputs writing the last timed object's mesh.  Small model settings (mini dims, 2 steps,
65^3 grid): a functional test, not a measurement."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_times_its_steps_and_dumps_the_last_mesh(tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--model", "mini", "--inference-steps", "2",
           "--octree-resolution", "64", "--steps", "3", "--warmup", "1", "--objects-per-launch", "2",
           "--dump-outputs", str(tmp_path / "out")]
    p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["steps"] == 3 and out["config"]["objects_total"] == 3 and out["warmup"] == 1
    assert out["unit"] == "objects/sec" and out["higher_is_better"] is True and out["dtype"] == "bf16"
    assert out["value"] > 0 and abs(out["value"] * out["ms_per_step"] / 1000.0 - 1.0) < 1e-6
    assert not {"roofline", "roofline_mc", "cpu_baseline", "mc_parity", "strong"} & set(out)
    v = np.load(tmp_path / "out" / "mesh_vertices.npy")
    f = np.load(tmp_path / "out" / "mesh_faces.npy")
    assert v.dtype == np.float32 and f.dtype == np.float64 and v.shape[1:] == (3,) and f.shape[1:] == (3,)
    assert (len(v), len(f)) == (out["mesh_last"]["V"], out["mesh_last"]["F"])
    assert len(f) > 0 and f.min() >= 0 and f.max() < len(v) and np.array_equal(f, np.round(f))
    assert np.isfinite(v).all()
