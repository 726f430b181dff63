"""GPU: small frames of the parked render_kernel around the re-seed (:307),
against the oracle, bitwise.

The re-seed starts path_trace's stream again from the pixel's seed, so at depth
0 it repeats the four draws render_kernel has just made for the aperture and
the jitter: light i takes draws 2i+1 and 2i+2, the first sample_sphere draws
2NL+1 and 2NL+2 and, below two lights, takes sincos_ of bitwise the angle the
aperture (NL = 0) or the jitter (NL = 1) used.  Reading those
values back instead of forming them again was built and measured no faster
(profiles/forms); these frames are the check any such reuse has to pass, and
they run the guarded sqrt_ / rcp_ / x / 1.5f forms of pt_math.h in every place
the light count moves them to.  The cases cross 0, 1 and 2 lights with 0, 1
and 3 SSS steps, depths 1 and 4 and 1 and 4 sample lanes, on the box and on the
cuboid off the origin, from a camera that sees the geometry with background
around it and from one that looks at the geometry through the first light,
where the pre-pass returns the light's colour before anything is drawn.

Every frame with a light must show lit pixels, so that an all-black frame
cannot pass.  Without a light nothing emits, the oracle's frame is (0,0,0,1)
everywhere and so must the kernel's be: those cases only show that such a
frame is left alone.
"""
import numpy as np
import pytest

import ptamd
import scenes
from support import TWO_LIGHTS, lit_pixels, oracle_frame, renderer, same, scene

pytestmark = pytest.mark.gpu

W, H, SPP = 64, 48, 3   # three batches: four sample lanes run a chunk that is not full
MAKERS = {"cuboid": scenes.cuboid}
CENTRE = (scenes.CUBOID_LO.astype(np.float64) + scenes.CUBOID_HI.astype(np.float64)) / 2


def _look(pos, at, fov):
    pos, at = np.asarray(pos, np.float64), np.asarray(at, np.float64)
    ubo = np.zeros(16, np.float32)
    ubo[0:3] = pos
    ubo[4:7] = (at - pos) / np.linalg.norm(at - pos)
    ubo[8:11] = (0, 1, 0)
    ubo[12] = fov
    return ubo


def _light(pos, at, inten, size):
    pos, at = np.asarray(pos, np.float64), np.asarray(at, np.float64)
    return ptamd.pack_light(pos, (at - pos) / np.linalg.norm(at - pos), inten, size)


CUBOID_LIGHTS = np.concatenate([_light(CENTRE + [0.5, 2.0, 1.0], CENTRE, [10, 10, 10], [2.0, 2.0]),
                                _light(CENTRE + [2.5, 0.25, 2.0], CENTRE, [2, 4, 8], [1.0, 1.0])])
# scene -> (two lights, the camera with background around the geometry, the camera behind the first light)
SETUPS = {
    "box": (TWO_LIGHTS, scenes.DEFAULT_CAMERA, _look([1.5, 4.0, 4.0], [0.0, 0.5, 0.0], 60.0)),
    "cuboid": (CUBOID_LIGHTS, _look(CENTRE + [1.5, 1.25, 3.5], CENTRE, 40.0),
               _look(CENTRE + [1.2, 2.2, 3.2], CENTRE, 40.0)),
}


@pytest.mark.parametrize("lanes", [1, 4])
@pytest.mark.parametrize("depth", [1, 4])
@pytest.mark.parametrize("sss", [0, 1, 3])
@pytest.mark.parametrize("n_lights", [0, 1, 2])
@pytest.mark.parametrize("view", ["around", "at-light"])
@pytest.mark.parametrize("name", ["box", "cuboid"])
def test_frame_equals_oracle(name, view, n_lights, sss, depth, lanes):
    two, around, at_light = SETUPS[name]
    lights = np.ascontiguousarray(two[:16 * n_lights])
    cam = around if view == "around" else at_light
    built = scene(name, MAKERS)
    r = renderer(built, cam, lights, depth=depth, sss=sss, size=(W, H), options=[(ptamd.PT_OPT_SAMPLE_LANES, lanes)])
    assert r.sweep_walk() == 3, "the parked kernel of a cube table (render_kernel<false, true, false, 3>) runs"
    r.render(0, SPP)
    out = r.read_accum()
    assert r.last_kernel() == ptamd.KERNEL_RECURSIVE
    r.close()
    ref = oracle_frame(built, cam, lights, W, H, nb=SPP, depth=depth, sss=sss)
    same(out, ref, f"{name} {view} {n_lights} lights sss {sss} depth {depth} lanes {lanes}")
    if n_lights:
        # pixels of exactly the first light's colour are the pre-pass's early return; the other lit ones are
        # geometry (the oracle's counts at depth 1, one light: box 180 / 185, cuboid 275 / 350 lit geometry
        # pixels from the two cameras, 233 and 967 light pixels from the second)
        rgb = out.reshape(-1, 4)[:, :3]
        early = int(np.count_nonzero((rgb == lights[8:11]).all(1)))
        assert lit_pixels(out) - early >= 150, "the frame shows the scene lit"
        if view == "at-light":
            assert early >= 200
    else:
        assert lit_pixels(out) == 0 and lit_pixels(ref) == 0
