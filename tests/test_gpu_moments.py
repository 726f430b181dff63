"""GPU: the per-pixel luminance moments (PT_OPT_MOMENTS) the render kernels fold.

Against the oracle where the oracle can say: a lone batch b in {0, 1, 3, 7}
into a cleared accumulator leaves c_b / (b + 1), an exact scaling (b + 1 is a
power of two), so the sample colours c_b are known and the moments follow from
the definition in numpy float32.  Longer runs are held to each other bitwise on
every path the kernels have, the accumulator staying the oracle's throughout.
Then the bookkeeping, the refused combinations, and that the option at 0
changes nothing."""
import functools

import numpy as np
import pytest
import torch

import denoise_var_ref as R
import ptamd
import scenes
from support import bits, oracle_frame, renderer, same, scene

pytestmark = pytest.mark.gpu

PT_OK, PT_ERR_INVALID, PT_ERR_UNSUPPORTED = 0, -1, -5
CAM_324 = scenes.camera((3, 2, 4))
CAM_FAR = scenes.camera((0.0, 0.0, 14.0))      # the box small in the middle: most of the old image is culled
FRAMES = {"box": (scenes.DEFAULT_CAMERA, 64, 48), "sphere": (CAM_324, 67, 45)}   # edge tiles in both directions
TINY = np.float32(np.finfo(np.float32).tiny)


def _oracle(name, first, nb, cam_key="own"):
    cam, W, H = FRAMES[name]
    return oracle_frame(scene(name), CAM_FAR if cam_key == "far" else cam, scenes.REFERENCE_LIGHT, W, H, first, nb)


def _renderer(name, opts=(), moments=1, cam=None):
    own_cam, W, H = FRAMES[name]
    return renderer(scene(name), own_cam if cam is None else cam, size=(W, H),
                    options=list(opts) + [(ptamd.PT_OPT_MOMENTS, moments)])


def _sample_colours(name, b, cam_key="own"):
    """c_b of every pixel, (H, W, 3), and the pixels where it is known exactly."""
    _, W, H = FRAMES[name]
    a = _oracle(name, b, 1, cam_key).reshape(H, W, 4)
    c = (a[..., :3] * np.float32(b + 1)).astype(np.float32)
    exact = np.all((a[..., :3] == 0) | (np.abs(a[..., :3]) >= TINY), axis=-1)   # no subnormal quotient
    return c, exact


@pytest.mark.parametrize("name", ["box", "sphere"])
def test_lone_batch_moments_match_the_definition(name):
    _, W, H = FRAMES[name]
    r = _renderer(name)
    for b in (0, 1, 3, 7):
        assert (b + 1) & b == 0
        r.clear()
        r.dispatch(b)
        same(r.read_accum(), _oracle(name, b, 1), f"{name}: accumulator of the lone batch {b}")
        got, n = r.read_moments()
        assert n == (1 if b == 0 else 0)          # only batch 0 alone is "batches 0..n-1"
        c, exact = _sample_colours(name, b)
        live = np.any(c != 0, axis=-1)
        assert np.count_nonzero(live) >= 100
        assert np.count_nonzero(live & ~exact) < 0.01 * np.count_nonzero(live)
        want = R.fold_moments(np.zeros((H, W, 2), np.float32), c, b)
        same(got[exact], want[exact], f"{name}: moments of the lone batch {b}")
        assert np.all(bits(got[~live]) == 0)     # L = +0 wherever nothing was seen


@pytest.mark.parametrize("name", ["box", "sphere"])
def test_two_batches_match_the_two_step_fold(name):
    _, W, H = FRAMES[name]
    r = _renderer(name)
    r.render(0, 2)
    same(r.read_accum(), _oracle(name, 0, 2), f"{name}: accumulator")
    got, n = r.read_moments()
    assert n == 2 and r.moments_ptr()
    c0, e0 = _sample_colours(name, 0)
    c1, e1 = _sample_colours(name, 1)
    want = R.fold_moments(R.fold_moments(np.zeros((H, W, 2), np.float32), c0, 0), c1, 1)
    ok = e0 & e1
    assert np.count_nonzero(~ok) < 0.01 * np.count_nonzero(np.any(c0 != 0, axis=-1))
    same(got[ok], want[ok], f"{name}: moments of batches 0 and 1")
    assert np.any(got[..., 1] > got[..., 0] * got[..., 0])   # some pixel has a variance


def _baseline(name, nb):
    r = _renderer(name)
    r.render(0, nb)
    same(r.read_accum(), _oracle(name, 0, nb), f"{name}: accumulator, {nb} batches")
    m, n = r.read_moments()
    assert n == nb
    return m


@functools.lru_cache(maxsize=None)
def _base(name, nb):
    m = _baseline(name, nb)
    m.setflags(write=False)
    return m


def _check_run(name, r, nb, what):
    same(r.read_accum(), _oracle(name, 0, nb), f"{name}, {what}: accumulator")
    m, n = r.read_moments()
    assert n == nb, what
    same(m, _base(name, nb), f"{name}, {what}: moments")


@pytest.mark.parametrize("name", ["box", "sphere"])
def test_dispatches_and_split_renders_agree(name):
    for nb in (8, 5):
        r = _renderer(name)
        for b in range(nb):
            r.dispatch(b)
        _check_run(name, r, nb, f"{nb} dispatches")
    r = _renderer(name)
    r.render(0, 3)
    r.render(3, 5)
    _check_run(name, r, 8, "render(0, 3) then render(3, 5)")
    r.render(0, 5)                                  # from 0 again over the old image
    _check_run(name, r, 5, "render(0, 5) over an older run")


LANES = ptamd.PT_OPT_SAMPLE_LANES
MIX = ptamd.PT_OPT_MIXED_LANES
BOX_PATHS = {
    "lanes 1": [(MIX, 0), (LANES, 1)],
    "lanes 2": [(MIX, 0), (LANES, 2)],
    "lanes 4": [(MIX, 0), (LANES, 4)],
    "lanes 8": [(MIX, 0), (LANES, 8)],
    "mixed 50, lanes 4": [(MIX, 50), (LANES, 4)],
    "mixed 50, lanes 8": [(MIX, 50), (LANES, 8)],
    "sweep off": [(ptamd.PT_OPT_SMALL_SWEEP, 0)],
    "sweep off, lanes 2": [(ptamd.PT_OPT_SMALL_SWEEP, 0), (MIX, 0), (LANES, 2)],
    "sweep without hull faces": [(ptamd.PT_OPT_SWEEP_HULL, 0)],
    "sweep without hull faces, lanes 8": [(ptamd.PT_OPT_SWEEP_HULL, 0), (MIX, 0), (LANES, 8)],
    "tight cull off": [(ptamd.PT_OPT_CULL_TIGHT, 0)],
    "primary cull off": [(ptamd.PT_OPT_PRIMARY_CULL, 0)],
    "primary cull off, lanes 4": [(ptamd.PT_OPT_PRIMARY_CULL, 0), (LANES, 4)],
    "scene not in LDS": [(ptamd.PT_OPT_SCENE_IN_LDS, 0)],
    "scene not in LDS, lanes 4": [(ptamd.PT_OPT_SCENE_IN_LDS, 0), (LANES, 4)],
    "stale start": [(ptamd.PT_OPT_FRESH_BATCH0, 0)],
}


@pytest.mark.parametrize("path", sorted(BOX_PATHS))
def test_box_paths_agree(path):
    for nb in (8, 5):
        r = _renderer("box", BOX_PATHS[path])
        r.render(0, nb)
        _check_run("box", r, nb, path)
    if path.startswith("sweep"):                    # the walk the case is named for
        assert (r.sweep_info()[0] > 0) == (not path.startswith("sweep off")), r.sweep_info()


def test_box_measured_mixed_schedule_agrees():
    r = _renderer("box", [(MIX, -1)])
    seen = set()
    for _ in range(8):                              # the first frames measure the block costs
        r.render(0, 8)
        r.synchronize()
        seen.add(r.mixed_info()[0])
    print("mixed schedules seen:", sorted(seen), "last:", r.mixed_info())
    _check_run("box", r, 8, f"measured mixed schedule {r.mixed_info()}")


SPHERE_PATHS = {
    "path-recursive": [(ptamd.PT_OPT_KERNEL, 1)],
    "path-recursive, lanes 1": [(ptamd.PT_OPT_KERNEL, 1), (LANES, 1)],
    "path-recursive, lanes 4": [(ptamd.PT_OPT_KERNEL, 1), (LANES, 4)],
    "wavefront": [(ptamd.PT_OPT_KERNEL, 3)],
    "wavefront, primary cull off": [(ptamd.PT_OPT_KERNEL, 3), (ptamd.PT_OPT_PRIMARY_CULL, 0)],
    "path-recursive, tight cull off": [(ptamd.PT_OPT_KERNEL, 1), (ptamd.PT_OPT_CULL_TIGHT, 0)],
}


@pytest.mark.parametrize("path", sorted(SPHERE_PATHS))
def test_sphere_paths_agree(path):
    r = _renderer("sphere", SPHERE_PATHS[path])
    r.render(0, 8)
    assert r.last_kernel() == (3 if path.startswith("wavefront") else 1)
    _check_run("sphere", r, 8, path)
    r.render(0, 3)                                  # wavefront: continues the moments chunk by chunk too
    r.render(3, 2)
    _check_run("sphere", r, 5, path + ", 3 + 2")


def test_camera_change_leaves_zero_moments_on_culled_pixels():
    name = "box"
    _, W, H = FRAMES[name]
    for fresh in (1, 0):
        r = _renderer(name, [(ptamd.PT_OPT_FRESH_BATCH0, fresh)])
        r.render(0, 2)
        old, _ = r.read_moments()
        r.set_camera(CAM_FAR)
        r.render(0, 2)
        same(r.read_accum(), _oracle(name, 0, 2, "far"), f"fresh {fresh}: accumulator under the new camera")
        new, n = r.read_moments()
        assert n == 2
        c0, e0 = _sample_colours(name, 0, "far")
        c1, e1 = _sample_colours(name, 1, "far")
        want = R.fold_moments(R.fold_moments(np.zeros((H, W, 2), np.float32), c0, 0), c1, 1)
        assert np.all(e0 & e1)
        same(new, want, f"fresh {fresh}: moments under the new camera")
        gone = np.any(old != 0, axis=-1) & np.all(bits(new) == 0, axis=-1)
        assert np.count_nonzero(gone) >= 100, "part of the old image is culled now"


def test_bookkeeping_off_gap_and_clear():
    L = ptamd.lib()
    name = "box"
    _, W, H = FRAMES[name]
    buf = np.zeros(W * H * 2, np.float32)
    r = _renderer(name, moments=0)
    r.render(0, 4)
    assert not r.moments_ptr()
    assert L.pt_read_moments(r._c, buf.ctypes.data, buf.size, None) == PT_ERR_INVALID
    assert L.pt_denoise_var(r._c, None, None) == PT_ERR_INVALID
    r.set_option(ptamd.PT_OPT_MOMENTS, 1)
    r.render(4, 2)                                  # on, but not from 0: still nothing valid
    assert not r.moments_ptr() and L.pt_denoise_var(r._c, None, None) == PT_ERR_INVALID
    r.render(0, 1)
    assert r.moments_ptr()
    assert L.pt_denoise_var(r._c, None, None) == PT_ERR_INVALID      # n = 1: no variance of the mean yet
    r.render(1, 3)
    assert r.moments_ptr() and L.pt_denoise_var(r._c, None, None) == PT_OK
    r.render(6, 1)                                  # a gap
    assert not r.moments_ptr() and L.pt_denoise_var(r._c, None, None) == PT_ERR_INVALID
    assert r.read_moments()[1] == 0
    r.render(0, 2)
    assert r.moments_ptr() and r.read_moments()[1] == 2
    r.set_option(ptamd.PT_OPT_MOMENTS, 0)
    r.render(2, 1)                                  # the accumulator moves on without the moments
    r.set_option(ptamd.PT_OPT_MOMENTS, 1)
    assert not r.moments_ptr()
    r.render(3, 1)
    assert not r.moments_ptr() and L.pt_denoise_var(r._c, None, None) == PT_ERR_INVALID
    r.render(0, 2)
    assert r.moments_ptr()
    for clear in (r.clear, lambda: r.resize_and_clear(W, H)):
        clear()
        assert not r.moments_ptr()
        m, n = r.read_moments()
        assert n == 0 and np.all(bits(m) == 0)
        r.render(0, 2)
        assert r.moments_ptr()
    frame = torch.zeros(H, W, 4, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    r.bind_accum(frame.data_ptr(), W, H)
    m, n = r.read_moments()
    assert n == 0 and np.all(bits(m) == 0) and not r.moments_ptr()
    r.render(0, 8)
    r.synchronize()
    same(frame.cpu().numpy(), _oracle(name, 0, 8), "bound accumulator")
    same(r.read_moments()[0], _base(name, 8), "moments beside a bound accumulator")
    assert L.pt_set_option(r._c, ptamd.PT_OPT_MOMENTS, 2) == PT_ERR_INVALID
    small = np.zeros(8, np.float32)
    assert L.pt_read_moments(r._c, small.ctypes.data, small.size, None) == PT_ERR_INVALID
    assert L.pt_read_moments(r._c, None, buf.size, None) == PT_ERR_INVALID


def test_unsupported_combinations_are_refused():
    L = ptamd.lib()
    name = "box"
    _, W, H = FRAMES[name]
    g = ptamd.Renderer(devices=[0, 0])
    assert L.pt_set_option(g._c, ptamd.PT_OPT_MOMENTS, 1) == PT_ERR_UNSUPPORTED
    assert not L.pt_moments_device_ptr(g._c)
    buf = np.zeros(W * H * 2, np.float32)
    assert L.pt_read_moments(g._c, buf.ctypes.data, buf.size, None) == PT_ERR_UNSUPPORTED
    assert L.pt_denoise_var(g._c, None, None) == PT_ERR_UNSUPPORTED
    r = _renderer(name)
    r.set_partition(2, 0)
    assert L.pt_render(r._c, 0, 2) == PT_ERR_UNSUPPORTED
    r.set_partition(1, 0)
    packed = torch.zeros(W * H * 4 + 4096, dtype=torch.float32, device="cuda")
    assert L.pt_render_packed(r._c, 2, packed.data_ptr(), None, 0, None) == PT_ERR_UNSUPPORTED
    assert L.pt_dist_run(r._c, 2, 1, 1, packed.data_ptr(), 1) == PT_ERR_UNSUPPORTED
    r.set_stats_mode(True)
    assert L.pt_render(r._c, 0, 2) == PT_ERR_UNSUPPORTED
    r.set_stats_mode(False)
    r.set_option(ptamd.PT_OPT_COUNT_TRACED, 1)
    assert L.pt_render(r._c, 0, 2) == PT_ERR_UNSUPPORTED
    r.set_option(ptamd.PT_OPT_COUNT_TRACED, 0)
    r.render(0, 8)                                  # and with them gone it renders again
    _check_run(name, r, 8, "after the refusals")


@pytest.mark.parametrize("name", ["box", "sphere"])
def test_moments_off_changes_nothing(name):
    r = _renderer(name, moments=0)
    r.render(0, 8)
    same(r.read_accum(), _oracle(name, 0, 8), f"{name}: option never set to 1")
    r.set_option(ptamd.PT_OPT_MOMENTS, 1)
    r.render(0, 2)
    r.set_option(ptamd.PT_OPT_MOMENTS, 0)
    r.clear()
    r.render(0, 3)
    r.render(3, 5)
    same(r.read_accum(), _oracle(name, 0, 8), f"{name}: option back at 0")
    for b in (1, 7):
        r.clear()
        r.dispatch(b)
        same(r.read_accum(), _oracle(name, b, 1), f"{name}: lone batch {b}, option at 0")
