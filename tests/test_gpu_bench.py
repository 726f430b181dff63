"""bench.py's plain run on the GPU, in a fresh process: it times the steps it
was asked for, prints the headline line without any of the --full extras, and
--dump-outputs writes the frame the last timed step rendered."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_is_lean_and_dumps_the_last_timed_frame(tmp_path):
    W, H, SPP = 160, 96, 2
    env = dict(os.environ, PT_BENCH_DETAIL=str(tmp_path / "detail.json"))
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2",
           "--width", str(W), "--height", str(H), "--spp", str(SPP), "--dump-outputs", str(tmp_path / "out")]
    res = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    line = json.loads(res.stdout.strip().splitlines()[-1])
    assert line["steps"] == 3 and line["warmup"] == 2 and line["n_gpus"] == 1
    assert line["unit"] == "Mrays/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["ms_per_step"] > 0 and line["value"] > 0
    assert line["config"]["rays_per_frame"] > 0
    # what --full adds is absent from a plain run
    for k in ("cpu_baseline", "verified_vs_oracle", "single_context", "primary_cull_off_ms", "configs", "group_leg"):
        assert k not in line, k
    assert "rays_traced" not in line["config"]
    # the dumped frame: the same frame rendered here, bit for bit
    import ptamd
    import scenes
    scene = ptamd.Scene.load_obj(scenes.BOX_OBJ).build_bvh()
    v, i, n, _, _ = scene.arrays()
    r = ptamd.Renderer(0)
    r.upload_scene(v, i, n)
    r.upload_lights(scenes.REFERENCE_LIGHT)
    r.set_camera(scenes.DEFAULT_CAMERA)
    r.set_params(4, 3)
    r.resize_and_clear(W, H)
    r.render(0, SPP)
    want = r.read_accum()
    got = np.load(tmp_path / "out" / "accum.npy")
    assert got.dtype == np.float32 and got.shape == (H, W, 4)
    assert np.array_equal(got.reshape(-1).view(np.uint32), want.view(np.uint32))
