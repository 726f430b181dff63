"""GPU: the trace kernels on geometry the rest of the suite does not have, and
with more lights than it uploads.

Every other scene of the suite sits in about [-1, 1]^3 around the origin, with
uniform triangle sizes, non-zero areas and at most three lights.  The culled
wide walk's exactness rests on a floating-point bound whose terms grow with
the distance from ray origin to triangle, with the edge lengths and with the
largest coefficients below a node, and its 64-byte nodes round
their boxes onto a grid of the node's own origin and scale.  The host
restatements of both walks hold on the scenes below (test_wide.py,
test_sweep.py); here the device kernels -- node decode, LDS staging, wave-wide
leaf-queue flushes, the stack overflow area, fused shadow walks, the tail
kernel, the scalar-cache sweep -- render them on every walk, each frame bit
for bit the oracle's.

Frames are 64x48 at 3 spp in two launches (batch 0, then batches 1-2 over the
non-zero accumulator).  Each oracle frame is computed once and must show the
scene lit in at least 100 pixels.
"""
import functools

import numpy as np
import pytest

import oracle_lib as O
import ptamd
import scenes
from cull_support import ring_lights
from support import built, lit_pixels, oracle_frame, renderer, same, scene
from sweep_support import HOSTILE as TINY_HOSTILE, HOSTILE_TABLES

pytestmark = pytest.mark.gpu

W, H = 64, 48
MIN_LIT = 100
SPHERE_CAM = scenes.camera((0.0, 0.5, 3.0))
MISS = np.array([0.0, 0.0, 0.0, 1e30], np.float32)


def _oracle_frame(v, i, n, cam, lights, int_bits=False):
    return oracle_frame((v, i, n), cam, lights, W, H, nb=3, nthreads=8, int_bits=int_bits)


def _moved(cam, scale, offset):
    return scenes.transformed_camera(cam, scale, offset), scenes.transformed_light(scenes.REFERENCE_LIGHT, scale, offset)


# ---- device-memory scenes ---------------------------------------------------

def _big_inputs(name):
    """(vertices, indices, camera, lights, int_bits) of a scene of scenes.WIDE_HOSTILE."""
    if name == "degenerates":   # larger triangles than the CPU case's: more of the frame lit
        v, i = scenes.with_degenerates(*scenes.random_triangles(3000, seed=8, spread=0.5, size=0.05))
        return v, i, scenes.camera((0.3, 0.2, 2.2)), scenes.REFERENCE_LIGHT, False
    v, i = scenes.WIDE_HOSTILE[name]()
    if name == "cloud_far":     # int-encoded links, as the >= 2^24-node trees travel
        return (v, i) + _moved(scenes.camera((0.3, 0.2, 2.2)), 1.0, (1000, -500, 2000)) + (True,)
    if name == "sphere_at_300":
        return (v, i) + _moved(SPHERE_CAM, 1.0, (300, 300, -300)) + (False,)
    if name == "sphere_x50":
        return (v, i) + _moved(SPHERE_CAM, 50.0, (0, 0, 0)) + (False,)
    if name == "sphere_x0.05":
        return (v, i) + _moved(SPHERE_CAM, 0.05, (0, 0, 0)) + (False,)
    if name == "floor_and_cloud":
        return v, i, scenes.camera((0.3, 0.4, 2.2)), scenes.REFERENCE_LIGHT, False
    assert name == "coincident_x6"
    return v, i, SPHERE_CAM, scenes.REFERENCE_LIGHT, False


@functools.lru_cache(maxsize=None)
def _big(name):
    v, i, cam, lights, int_bits = _big_inputs(name)
    v, i, n = built(v, i, int_bits)
    ref = _oracle_frame(v, i, n, cam, lights, int_bits)
    assert lit_pixels(ref) >= MIN_LIT, f"{name}: the oracle's frame shows {lit_pixels(ref)} lit pixels"
    return v, i, n, cam, lights, int_bits, ref


ALL_TAIL, NO_TAIL = 1 << 30, 1
# One option at a time off the defaults, and every one of them at once.  The
# wavefront cases run the whole frame in the tail kernel unless they say
# otherwise (the automatic threshold does the same at this frame size).
BIG_VARIANTS = {
    "recursive": (ptamd.KERNEL_RECURSIVE, {}),
    "wide": (ptamd.KERNEL_WAVEFRONT, {}),
    "exhaustive": (ptamd.KERNEL_WAVEFRONT, {ptamd.PT_OPT_WIDE: 0}),
    "handback": (ptamd.KERNEL_WAVEFRONT, {ptamd.PT_OPT_WIDE: 2}),
    "node128": (ptamd.KERNEL_WAVEFRONT, {ptamd.PT_OPT_WIDE_NODE: 128}),
    "reference_tree": (ptamd.KERNEL_WAVEFRONT, {ptamd.PT_OPT_WIDE_BUILD: 0}),
    "unfused": (ptamd.KERNEL_WAVEFRONT, {ptamd.PT_OPT_WF_FUSE: 0}),
    "rounds": (ptamd.KERNEL_WAVEFRONT, {ptamd.PT_OPT_WF_TAIL: NO_TAIL}),
    "all": (ptamd.KERNEL_WAVEFRONT, {ptamd.PT_OPT_WIDE: 2, ptamd.PT_OPT_WIDE_NODE: 128, ptamd.PT_OPT_WIDE_BUILD: 0,
                                     ptamd.PT_OPT_WF_FUSE: 0, ptamd.PT_OPT_WF_TAIL: NO_TAIL}),
}


def _render_two_launches(r, ref, what):
    r.resize_and_clear(W, H)
    r.render(0, 1)
    r.render(1, 2)
    same(r.read_accum(), ref, what)


def _wide_renderer(v, i, n, cam, lights, int_bits, kernel, opts):
    tail = [(ptamd.PT_OPT_WF_TAIL, ALL_TAIL)] if kernel == ptamd.KERNEL_WAVEFRONT else []
    r = renderer((v, i, n), cam, lights, int_bits=int_bits,   # PT_OPT_WIDE_BUILD is read at the scene's upload
                 options=[(ptamd.PT_OPT_SCENE_IN_LDS, 0), (ptamd.PT_OPT_KERNEL, kernel)] + tail + list(opts.items()))
    info = r.wide_info()
    assert info[0] > 0 and info[1] > 0, f"no wide tree: {info}"   # a refused tree would pass on the exact walk
    return r


@pytest.mark.parametrize("variant", list(BIG_VARIANTS))
@pytest.mark.parametrize("name", sorted(scenes.WIDE_HOSTILE))
def test_device_memory_scene(name, variant):
    v, i, n, cam, lights, int_bits, ref = _big(name)
    kernel, opts = BIG_VARIANTS[variant]
    r = _wide_renderer(v, i, n, cam, lights, int_bits, kernel, opts)
    _render_two_launches(r, ref, f"{name} {variant}")
    assert r.last_kernel() == kernel
    r.close()


def test_coincident_copies_tie_break_decides_the_image():
    """Every hit of the six-copy sphere ties across six triangles of
    alternating winding: the winner's geometric normal, and with it the pixel,
    is the visit order's.  The oracle's frame of it differs from its frame of
    the single sphere nearly everywhere the sphere is lit."""
    v, i, n, cam, lights, _, ref = _big("coincident_x6")
    sv, si, sn = built(*scenes.displaced_sphere(2))
    single = _oracle_frame(sv, si, sn, cam, lights)
    a, b = ref.reshape(-1, 4)[:, :3], single.reshape(-1, 4)[:, :3]
    lit = np.any(a != 0, axis=1) | np.any(b != 0, axis=1)
    differ = np.any(a.view(np.uint32) != b.view(np.uint32), axis=1)
    assert lit.sum() >= MIN_LIT and differ.sum() > 0.5 * lit.sum(), (int(lit.sum()), int(differ.sum()))


# ---- tiny scenes (LDS-staged, the sweep walk) --------------------------------

def _aimed(v, i, tri):
    """A camera 3 away from triangle `tri` on its normal, on the side that
    faces the reference light, looking at its centroid (test_gpu_sweep._aimed)
    through a field of view of 0.35 degrees: the generator's triangles, 0.01
    to 0.02 across, then cover a tenth of a 64x48 frame."""
    p = v.reshape(-1, 3)[i.reshape(-1, 3)[tri]].astype(np.float64)
    c = p.mean(0)
    d = np.cross(p[1] - p[0], p[2] - p[0])
    d /= np.linalg.norm(d)
    if np.dot(d, scenes.REFERENCE_LIGHT[0:3] - c) < 0:
        d = -d
    ubo = np.zeros(16, np.float32)
    ubo[0:3] = c + 3.0 * d
    ubo[4:7] = -d
    ubo[8 + int(np.argmin(np.abs(d)))] = 1.0
    ubo[12] = 0.35
    return ubo


def _facing_light(v, i):
    """Triangles (BVH order) with a non-zero area whose geometric normal faces the reference light."""
    p = v.reshape(-1, 3)[i.reshape(-1, 3)].astype(np.float64)
    nrm = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    to_light = scenes.REFERENCE_LIGHT[0:3] - p.mean(1)
    with np.errstate(invalid="ignore", divide="ignore"):
        cos = (nrm * to_light).sum(1) / (np.linalg.norm(nrm, axis=1) * np.linalg.norm(to_light, axis=1))
    return [int(t) for t in np.flatnonzero(np.nan_to_num(cos) > 0.2)]


@functools.lru_cache(maxsize=None)
def _tiny(name):
    v, i, n = built(*TINY_HOSTILE[name]())
    if name == "box@300":
        cam, lights = _moved(scenes.DEFAULT_CAMERA, 1.0, (300, 300, -300))
    elif name == "box*50":
        cam, lights = _moved(scenes.DEFAULT_CAMERA, 50.0, (0, 0, 0))
    elif name == "box*0.01":
        cam, lights = _moved(scenes.DEFAULT_CAMERA, 0.01, (0, 0, 0))
    elif name in ("tri4:copies8", "tri8:degenerate"):
        cam, lights = _aimed(v, i, _facing_light(v, i)[0]), scenes.REFERENCE_LIGHT
    else:
        cam, lights = scenes.DEFAULT_CAMERA, scenes.REFERENCE_LIGHT
    ref = _oracle_frame(v, i, n, cam, lights)
    assert lit_pixels(ref) >= MIN_LIT, f"{name}: the oracle's frame shows {lit_pixels(ref)} lit pixels"
    return v, i, n, cam, lights, ref


SWEEP, THREADED, DEVICE_MEMORY = "sweep", "threaded", "device memory"
# (options, the walk the launch must take, kernel)
TINY_VARIANTS = {
    "sweep": ({ptamd.PT_OPT_SMALL_SWEEP: 1}, SWEEP, ptamd.KERNEL_RECURSIVE),
    "threaded": ({ptamd.PT_OPT_SMALL_SWEEP: 0}, THREADED, ptamd.KERNEL_RECURSIVE),
    "lds0": ({ptamd.PT_OPT_SMALL_SWEEP: 1, ptamd.PT_OPT_SCENE_IN_LDS: 0}, DEVICE_MEMORY, ptamd.KERNEL_RECURSIVE),
    "lds2": ({ptamd.PT_OPT_SMALL_SWEEP: 1, ptamd.PT_OPT_SCENE_IN_LDS: 2}, SWEEP, ptamd.KERNEL_RECURSIVE),
    "hull0": ({ptamd.PT_OPT_SMALL_SWEEP: 1, ptamd.PT_OPT_SWEEP_HULL: 0}, SWEEP, ptamd.KERNEL_RECURSIVE),
    "hull1": ({ptamd.PT_OPT_SMALL_SWEEP: 1, ptamd.PT_OPT_SWEEP_HULL: 1}, SWEEP, ptamd.KERNEL_RECURSIVE),
    "lanes1": ({ptamd.PT_OPT_SMALL_SWEEP: 1, ptamd.PT_OPT_SAMPLE_LANES: 1}, SWEEP, ptamd.KERNEL_RECURSIVE),
    "lanes4": ({ptamd.PT_OPT_SMALL_SWEEP: 1, ptamd.PT_OPT_SAMPLE_LANES: 4}, SWEEP, ptamd.KERNEL_RECURSIVE),
    "threaded_lanes4": ({ptamd.PT_OPT_SMALL_SWEEP: 0, ptamd.PT_OPT_SAMPLE_LANES: 4}, THREADED, ptamd.KERNEL_RECURSIVE),
    "wavefront": ({ptamd.PT_OPT_KERNEL: 3}, THREADED, ptamd.KERNEL_WAVEFRONT),
    "wavefront_wide": ({ptamd.PT_OPT_KERNEL: 3, ptamd.PT_OPT_SCENE_IN_LDS: 0}, DEVICE_MEMORY, ptamd.KERNEL_WAVEFRONT),
}


@pytest.mark.parametrize("variant", list(TINY_VARIANTS))
@pytest.mark.parametrize("name", sorted(TINY_HOSTILE))
def test_tiny_scene(name, variant):
    v, i, n, cam, lights, ref = _tiny(name)
    opts, walk, kernel = TINY_VARIANTS[variant]
    r = renderer((v, i, n), cam, lights, options=opts)
    boxes, leaves = r.sweep_info()
    if walk == SWEEP:
        assert leaves == i.size // 3 and 1 <= boxes <= 2 * leaves - 1
        if name in HOSTILE_TABLES:
            assert (boxes, leaves) == HOSTILE_TABLES[name]
    else:
        assert (boxes, leaves) == (0, 0)
    if variant == "wavefront_wide":
        assert r.wide_info()[0] > 0, r.wide_info()
    _render_two_launches(r, ref, f"{name} {variant}")
    assert r.last_kernel() == kernel
    r.close()


# ---- guide image --------------------------------------------------------------

def _check_guide(v, i, n, cam, lights, int_bits, what, GW=32, GH=24):
    """render_guide against oracle_lib.trace of pt_guide_ray (as
    test_gpu_denoise._oracle_guide), on every walk the guide kernel has for a
    device-memory scene."""
    want = np.zeros((GH, GW, 4), np.float32)
    for y in range(GH):
        for x in range(GW):
            o, d = ptamd.guide_ray(cam, GW, GH, x, y)
            hit, t, _, nrm, _ = O.trace(v, i, n.reshape(-1), o, d)
            want[y, x] = np.concatenate([nrm, [np.float32(t)]]) if hit else MISS
    hits = int(np.count_nonzero(want[..., 3] < 1e30))
    assert 50 <= hits < GW * GH, hits
    r = renderer((v, i, n), cam, lights, size=(GW, GH), int_bits=int_bits)
    assert r.wide_info()[0] > 0, r.wide_info()
    for key, value in [(ptamd.PT_OPT_WIDE, 1), (ptamd.PT_OPT_WIDE_NODE, 128), (ptamd.PT_OPT_WIDE, 0)]:
        r.set_option(key, value)
        r.render_guide()
        same(r.read_guide(), want, f"guide {what}, option {key} = {value}")
    r.close()


@pytest.mark.parametrize("name", ["sphere_at_300", "coincident_x6"])
def test_guide_image(name):
    v, i, n, cam, lights, int_bits, _ = _big(name)
    _check_guide(v, i, n, cam, lights, int_bits, name)


def test_guide_image_from_far_away():
    """The hostile scenes move the camera with the geometry, and a path-traced
    frame from far away is all aperture blur (the shader focuses at 3).  The
    guide's pinhole rays are not: a dense cloud of 30,000 small triangles seen
    from 1,100 away through a field of view of 0.027 degrees -- S = |o - v0|,
    which the cull bound's error terms multiply, is 2,000 times the scene's
    size on every ray (test_wide.test_wide_walk_far_origins on the device)."""
    v, i, n = built(*scenes.random_triangles(30000, seed=9, spread=0.2, size=0.004))
    cam = scenes.camera((300.0, 200.0, 1000.0), fov=0.027)
    _check_guide(v, i, n, cam, scenes.REFERENCE_LIGHT, False, "far camera")


# ---- many lights ----------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _many(which, n_lights):
    if which == "box":
        (v, i, n), cam = scene("box"), scenes.DEFAULT_CAMERA
    else:
        (v, i, n), cam = scene("sphere"), SPHERE_CAM
    lights = ring_lights(n_lights)
    ref = _oracle_frame(v, i, n, cam, lights)
    assert lit_pixels(ref) >= MIN_LIT, f"{which}, {n_lights} lights: the oracle's frame shows {lit_pixels(ref)} lit pixels"
    return v, i, n, cam, lights, ref


@pytest.mark.parametrize("n_lights", [7, 8, 9])
@pytest.mark.parametrize("kernel,sweep", [(1, 1), (1, 0), (3, 0)], ids=["recursive-sweep", "recursive-threaded",
                                                                          "wavefront"])
def test_many_lights_box(kernel, sweep, n_lights):
    """7 lights fill the cull-rectangle table (kMaxCullRects = 8), 8 and 9
    switch primary culling off; the per-light loops run 7 to 9 turns."""
    v, i, n, cam, lights, ref = _many("box", n_lights)
    r = renderer((v, i, n), cam, lights, options=[(ptamd.PT_OPT_KERNEL, kernel), (ptamd.PT_OPT_SMALL_SWEEP, sweep)])
    if kernel == 1 and sweep:
        assert r.sweep_info() == (7, 12)
    else:
        assert r.sweep_info() == (0, 0)
    _render_two_launches(r, ref, f"box, {n_lights} lights, kernel {kernel}, sweep {sweep}")
    assert r.last_kernel() == kernel
    r.close()


@pytest.mark.parametrize("n_lights", [7, 8, 9])
@pytest.mark.parametrize("fuse", [0, 1])
def test_many_lights_sphere_wide_walk(fuse, n_lights):
    v, i, n, cam, lights, ref = _many("sphere", n_lights)
    for tail in (ALL_TAIL, NO_TAIL):
        r = _wide_renderer(v, i, n, cam, lights, False, ptamd.KERNEL_WAVEFRONT,
                           {ptamd.PT_OPT_WF_FUSE: fuse, ptamd.PT_OPT_WF_TAIL: tail})
        _render_two_launches(r, ref, f"sphere, {n_lights} lights, fuse {fuse}, tail {tail}")
        assert r.last_kernel() == ptamd.KERNEL_WAVEFRONT
        r.close()


@pytest.mark.parametrize("kernel", [ptamd.KERNEL_RECURSIVE, ptamd.KERNEL_WAVEFRONT])
def test_many_lights_primaries(kernel):
    """Counting mode: with 8 or 9 lights no rectangles derive and every sample
    generates its primary ray; with 7 the culled pixels' samples do not."""
    nb = 3
    primaries = {}
    for n_lights in (7, 8, 9):
        v, i, n, cam, lights, ref = _many("box", n_lights)
        r = renderer((v, i, n), cam, lights, size=(W, H),
                     options=[(ptamd.PT_OPT_KERNEL, kernel), (ptamd.PT_OPT_COUNT_TRACED, 1)])
        r.reset_stats()
        r.render(0, nb)
        same(r.read_accum(), ref, f"counting mode, {n_lights} lights, kernel {kernel}")
        assert r.last_kernel() == kernel
        primaries[n_lights] = r.traced()["primaries"]
        r.close()
    assert primaries[8] == primaries[9] == W * H * nb
    assert 0 < primaries[7] < W * H * nb, primaries
