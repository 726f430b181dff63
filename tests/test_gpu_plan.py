"""GPU: the launch plan as the public API shows it -- the rows of
tests/plan_cases.py that name a real scene, through the library.

What a render's plan leaves visible: pt_last_kernel (wavefront or
path-recursive), the pixels per item of pt_items_live (256 / sample lanes),
pt_sweep_info, pt_mixed_info's schedule, and the exact text of a refusal.
The same rows go through plan_launch on the CPU (tests/test_plan.py), so the
table ties the two together."""
import functools

import numpy as np
import pytest

import plan_cases
import ptamd
import scenes
from support import built, renderer, scene

pytestmark = pytest.mark.gpu

GPU_ROWS = [r for r in plan_cases.ROWS if r["gpu"]]


@functools.lru_cache(maxsize=None)
def _scene(name):
    if name == "box":
        return scene("box")
    return built(*scenes.displaced_sphere(int(name.split(":")[1])))


def _renderer(r):
    v, i, n = _scene(r["gpu"]["scene"])
    assert i.size // 3 == r["facts"]["tris"], "the row's facts are the scene's"
    rd = renderer((v, i, n), scenes.camera((0.0, 0.5, 3.0)) if r["gpu"]["scene"] != "box" else scenes.DEFAULT_CAMERA,
                  options=[(getattr(ptamd, "PT_OPT_" + k), val) for k, val in r["opts"].items()])
    if r["stats"]:
        rd.set_stats_mode(True)
    if r["ranks"] > 1:
        rd.set_partition(r["ranks"], 0)
    rd.resize_and_clear(*r["size"])
    return rd


@pytest.mark.parametrize("r", GPU_ROWS, ids=[r["name"] for r in GPU_ROWS])
def test_row(r):
    rd = _renderer(r)
    want = r["expect"]
    try:
        if isinstance(want, str):
            with pytest.raises(ptamd.PTError) as e:
                rd.render(0, r["batches"])
            assert str(e.value) == f"pt_render failed ({plan_cases.UNSUPPORTED}): {want}"
            if r["gpu"].get("guide"):
                with pytest.raises(ptamd.PTError) as e:
                    rd.render_guide()
                assert str(e.value) == f"pt_render_guide failed ({plan_cases.UNSUPPORTED}): {r['gpu']['guide']}"
            elif "guide" in r["gpu"]:
                rd.render_guide()
                rd.synchronize()
            return
        rd.render(0, r["batches"])
        rd.synchronize()
        assert rd.last_kernel() == (ptamd.KERNEL_WAVEFRONT if want["wf"] else ptamd.KERNEL_RECURSIVE)
        assert rd.items_live(0)[1] == 256 // want["spl"]
        assert rd.sweep_info() == (r["facts"]["sweep"][:2] if want["sweep"] else (0, 0))
        assert rd.mixed_info()[0] == r["gpu"]["mixed"]
        assert np.isfinite(rd.read_accum()).all()
    finally:
        rd.close()
