"""Radiance queries on the GPU: pt_trace_radiance against pt_trace_radiance_host
bit for bit on every scene of tests/rays_support.py, general rays and the
camera's own; query counts around the wave and the workgroup with several
sample counts; chunk seams; the same bytes from every kernel family and walk;
pt_camera_rays against the host; the queries of four batches folded against
pt_render's frame; hostile rays; and the plumbing: a render left untouched, a
context without a frame, a second upload, torch tensors on a stream, buffers
reused, the refusals and the driver's -radiance."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import ptamd
import radiance_support as RS
import rays_support as R
import scenes
import support
from support import PKG, same, same_nan

pytestmark = pytest.mark.gpu

PT_ERR_INVALID, PT_ERR_UNSUPPORTED = -1, -5
F32 = np.float32
O = ptamd
W, H = RS.W, RS.H


def _ctx(name, n_lights, options=(), depth=4, sss=3):
    """A context with a scene, lights and parameters: no camera, no frame."""
    r = ptamd.Renderer(0)
    for key, value in options:
        r.set_option(key, value)
    r.upload_scene(*support.scene(name))
    if n_lights:
        r.upload_lights(RS.lights(n_lights))
    r.set_params(depth, sss)
    return r


@pytest.mark.parametrize("n_lights", [1, 2])
@pytest.mark.parametrize("name", R.SCENES)
def test_device_matches_host(name, n_lights):
    r = _ctx(name, n_lights)
    want = RS.host(name, "general", n_lights)
    assert np.any(want[:, :3] != 0) and np.any((want[:, :3] == 0).all(1)), "lit and black answers"
    got = r.trace_radiance(RS.general_queries(name))
    assert got.tobytes() == want.tobytes(), f"{name}: 600 general rays"
    cam = RS.host(name, "camera", n_lights)
    assert r.trace_radiance(RS.camera_queries("around", 0)).tobytes() == cam.tobytes(), f"{name}: camera rays"
    if name in ("box", "sphere"):   # ... and the oracle's frame directly
        same(cam, support.oracle_frame(support.scene(name), RS.CAMERAS["around"], RS.lights(n_lights), W, H), "oracle")


def _tiled(a, n):
    return np.ascontiguousarray(a[np.arange(n) % len(a)])


@pytest.mark.parametrize("samples", [1, 2, 5])
@pytest.mark.parametrize("name,options", [("box", []), ("sphere", []), ("sphere", [(O.PT_OPT_KERNEL, 3)])])
def test_query_counts_and_samples(name, options, samples):
    """Ragged last waves and workgroups, several workgroups, on the path-recursive kernel (the box's sweep walk, the
    sphere from device memory) and on the wavefront pipeline."""
    r = _ctx(name, 2, options)
    want = RS.host(name, "general", 2, samples, 3)
    q = RS.general_queries(name)
    for n in (1, 63, 64, 65, 255, 256, 257, 4097):
        got = r.trace_radiance(_tiled(q, n), samples, 3)
        assert got.tobytes() == _tiled(want, n).tobytes(), f"{name} n = {n} S = {samples}"
    assert r.trace_radiance(np.zeros((0, 8), F32)).shape == (0, 4)


@pytest.mark.parametrize("chunk", [64, 300, 0])
@pytest.mark.parametrize("name,options", [("box", []), ("sphere", [(O.PT_OPT_KERNEL, 1)]), ("sphere", [(O.PT_OPT_KERNEL, 3)])])
def test_chunk_seams(name, options, chunk):
    """257 queries of 5 samples: chunks of 12 queries (60 paths, seams inside waves), of 60 (300 paths, seams
    between and inside waves), and one chunk."""
    r = _ctx(name, 2, list(options) + [(O.PT_OPT_RADIANCE_CHUNK, chunk)])
    q = _tiled(RS.general_queries(name), 257)
    want = _tiled(RS.host(name, "general", 2, 5, 3), 257)
    assert r.trace_radiance(q, 5, 3).tobytes() == want.tobytes()


OPTION_SETS = {
    "no-lds": [(O.PT_OPT_SCENE_IN_LDS, 0)],
    "lds": [(O.PT_OPT_SCENE_IN_LDS, 1)],
    "recursive": [(O.PT_OPT_KERNEL, 1)],
    "wavefront": [(O.PT_OPT_KERNEL, 3)],
    "wavefront-exact": [(O.PT_OPT_KERNEL, 3), (O.PT_OPT_WIDE, 0)],
    "wavefront-handback": [(O.PT_OPT_KERNEL, 3), (O.PT_OPT_WIDE, 2)],
    "wavefront-128": [(O.PT_OPT_KERNEL, 3), (O.PT_OPT_WIDE_NODE, 128)],
    "wavefront-64": [(O.PT_OPT_KERNEL, 3), (O.PT_OPT_WIDE_NODE, 64)],
    "wavefront-grid-25": [(O.PT_OPT_KERNEL, 3), (O.PT_OPT_WF_GRID, 25)],
    "wavefront-no-tail": [(O.PT_OPT_KERNEL, 3), (O.PT_OPT_WF_TAIL, 0)],
    "wavefront-no-fuse": [(O.PT_OPT_KERNEL, 3), (O.PT_OPT_WF_FUSE, 0)],
    "wavefront-lds": [(O.PT_OPT_KERNEL, 3), (O.PT_OPT_SCENE_IN_LDS, 1)],
    "no-exit-skip": [(O.PT_OPT_EXIT_SKIP, 0)],
    "exit-skip": [(O.PT_OPT_EXIT_SKIP, 1)],
    "wavefront-no-exit-skip": [(O.PT_OPT_KERNEL, 3), (O.PT_OPT_EXIT_SKIP, 0)],
    "no-sweep": [(O.PT_OPT_SMALL_SWEEP, 0)],
    "sweep": [(O.PT_OPT_SMALL_SWEEP, 1)],
    "sweep-no-cube": [(O.PT_OPT_SMALL_SWEEP, 1), (O.PT_OPT_SWEEP_CUBE, 0)],
    "sweep-no-hull": [(O.PT_OPT_SMALL_SWEEP, 1), (O.PT_OPT_SWEEP_HULL, 0)],
}


# the sweep walk's options on the box alone, which has a sweep table
WALK_CASES = [(name, options) for name in ("box", "sphere", "grid:8") for options in OPTION_SETS
              if name == "box" or "sweep" not in options]


@pytest.mark.parametrize("name,options", WALK_CASES)
def test_every_kernel_and_walk_gives_the_same_bytes(name, options):
    r = _ctx(name, 2, OPTION_SETS[options])
    q = np.concatenate([RS.general_queries(name), RS.camera_queries("at-light", 0)])
    want = np.concatenate([RS.host(name, "general", 2, 2, 3), RS.host(name, "camera", 2, 2, 3, view="at-light")])
    assert r.trace_radiance(q, 2, 3).tobytes() == want.tobytes(), f"{name} {options}"


@pytest.mark.parametrize("batch", [0, 3, 0xFFFFFFF0])
def test_camera_rays_against_the_host(batch):
    r = support.renderer(support.scene("box"), RS.CAMERAS["at-light"], size=(W, H))
    want = ptamd.camera_rays_host(RS.CAMERAS["at-light"], W, H, batch)
    got = r.camera_rays(batch)
    r.synchronize()   # the context's stream is not torch's
    assert got.shape == (W * H, 8) and got.cpu().numpy().tobytes() == want.tobytes()
    order = np.random.default_rng(4).permutation(W * H)[:77].astype(np.int32)
    got = r.camera_rays(batch, torch.from_numpy(order).cuda())
    r.synchronize()
    assert got.cpu().numpy().tobytes() == want[order].tobytes()
    assert r.camera_rays(batch, torch.zeros(0, dtype=torch.int32, device="cuda")).shape == (0, 8)


@pytest.mark.parametrize("name,options,kernel", [("box", [], O.KERNEL_RECURSIVE),
                                                 ("sphere", [(O.PT_OPT_KERNEL, 3)], O.KERNEL_WAVEFRONT)])
def test_queries_of_four_batches_fold_to_the_rendered_frame(name, options, kernel):
    """pt_trace_radiance(pt_camera_rays(b)), b = 0 .. 3, folded, is pt_render(0, 4)'s image: on the box (the sweep
    walk of a cube table) and on the sphere (the wavefront pipeline's culled wide walk)."""
    w, h = 32, 24
    cam = RS.CAMERAS["around"] if name == "box" else scenes.camera((0.0, 0.5, 3.0))
    r = support.renderer(support.scene(name), cam, support.TWO_LIGHTS, size=(w, h), options=options)
    colours = [r.trace_radiance(r.camera_rays(b)) for b in range(4)]   # enqueued on the context's stream
    r.synchronize()
    colours = [c.cpu().numpy() for c in colours]
    r.render(0, 4)
    frame = r.read_accum()
    assert r.last_kernel() == kernel
    if name == "box":
        assert r.sweep_walk() == 3
    else:
        assert r.wide_info()[0] > 0
    assert support.lit_pixels(frame) > 0
    same(RS.fold(colours), frame, name)


@pytest.mark.parametrize("options", ["recursive", "wavefront", "wavefront-exact", "no-lds"])
@pytest.mark.parametrize("name", ["box", "sphere"])
def test_hostile_rays(name, options):
    """NaN where NaN, every other float the same bits."""
    r = _ctx(name, 2, OPTION_SETS[options])
    want = RS.host(name, "hostile", 2, 2, 5)
    same_nan(r.trace_radiance(RS.hostile_queries(name), 2, 5), want, f"{name} {options}")


@pytest.mark.parametrize("name,options", [("box", []), ("sphere", [(O.PT_OPT_KERNEL, 3)])])
def test_a_query_between_two_renders_changes_nothing(name, options):
    cam = scenes.DEFAULT_CAMERA if name == "box" else scenes.camera((0.0, 0.5, 3.0))
    frames, stats = [], []
    for query in (False, True):
        r = support.renderer(support.scene(name), cam, size=(64, 48), options=list(options) + [(O.PT_OPT_COUNT_TRACED, 1)])
        r.render(0, 1)
        if query:
            got = r.trace_radiance(RS.general_queries(name), 2, 3)
            assert got.tobytes() == RS.host(name, "general", 1, 2, 3).tobytes()
        r.render(1, 2)
        frames.append(r.read_accum())
        # the walks the renders started and their primaries; the wide walk's node and triangle counts depend on
        # which lanes share a wave (its flush is wave-wide) and so move from run to run without any query
        traced = r.traced()
        stats.append((r.stats(), [traced[k] for k in ("closest_walks", "shadow_walks", "primaries")]))
    same(frames[1], frames[0], "the accumulation image")
    assert stats[0] == stats[1], "pt_get_stats, and the walks pt_get_traced counted"


def test_queries_are_not_counted_in_stats_mode():
    r = _ctx("sphere", 1, [(O.PT_OPT_COUNT_TRACED, 1)])
    r.set_stats_mode(True)
    assert r.trace_radiance(RS.general_queries("sphere")).tobytes() == RS.host("sphere", "general", 1).tobytes()
    assert not any(r.traced().values()) and not any(r.stats().values())


def test_lifetime_no_frame_second_upload_zero_lights_reuse():
    r = _ctx("sphere", 1)   # no camera, no frame
    q = RS.general_queries("sphere")
    want = RS.host("sphere", "general", 1)
    for _ in range(3):   # the library's buffers are reused
        assert r.trace_radiance(q).tobytes() == want.tobytes()
    assert r.trace_radiance(q[:10]).tobytes() == want[:10].tobytes()
    r.upload_scene(*support.scene("tri:2000"))
    assert r.trace_radiance(RS.general_queries("tri:2000")).tobytes() == RS.host("tri:2000", "general", 1).tobytes()
    r.upload_lights(RS.lights(2))
    r.set_params(2, 1)
    assert (r.trace_radiance(RS.general_queries("tri:2000")).tobytes()
            == RS.host("tri:2000", "general", 2, depth=2, sss=1).tobytes())
    z = _ctx("box", 0)   # zero lights are valid: every path is black
    got = z.trace_radiance(RS.general_queries("box"), 2, 1)
    assert got.tobytes() == RS.host("box", "general", 0, 2, 1).tobytes() and not got[:, :3].any()


def test_torch_tensors_on_the_context_s_stream():
    r = _ctx("sphere", 2)
    q = RS.general_queries("sphere")
    want = RS.host("sphere", "general", 2, 2, 3)
    stream = torch.cuda.Stream()
    r.set_stream(stream.cuda_stream)
    with torch.cuda.stream(stream):
        rays = torch.from_numpy(np.array(q)).to("cuda")
        got = r.trace_radiance(rays, 2, 3)
        total = got[:, :3].sum().item()   # torch work behind the query, on the same stream
    stream.synchronize()
    assert got.shape == (len(q), 4) and got.dtype == torch.float32
    assert got.cpu().numpy().tobytes() == want.tobytes()
    assert abs(total - float(want[:, :3].astype(np.float64).sum())) < 1e-2 * max(1.0, abs(total))
    assert r.trace_radiance(rays[:0]).shape == (0, 4)
    with pytest.raises(ptamd.PTError):
        r.trace_radiance(rays.double())
    with pytest.raises(ptamd.PTError):
        r.trace_radiance(rays.cpu())
    r.set_stream(None)


def test_refusals_and_error_paths():
    L = ptamd.lib()
    q = RS.general_queries("box")
    rays = torch.from_numpy(np.array(q[:64])).cuda()
    out = torch.zeros((64, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    P = lambda s, k=1: ctypes.byref(ptamd.RadianceParams(s, k))
    call = lambda r, params=None, rp=rays.data_ptr(), n=64, op=out.data_ptr(): L.pt_trace_radiance(r._c, params, rp, n, op)
    host = np.ascontiguousarray(q[:64])
    hout = np.zeros((64, 4), F32)
    sync = lambda r, params=None, rp=host.ctypes.data, n=64, op=hout.ctypes.data: L.pt_trace_radiance_sync(r._c, params, rp, n, op)
    empty = ptamd.Renderer(0)
    assert call(empty) == PT_ERR_INVALID and b"scene" in L.pt_last_error()
    assert sync(empty) == PT_ERR_INVALID and call(empty, n=0) == PT_ERR_INVALID
    r = _ctx("box", 1)
    assert call(r) == 0 and sync(r) == 0
    r.synchronize()
    assert out.cpu().numpy().tobytes() == hout.tobytes() == RS.host("box", "general", 1)[:64].tobytes()
    for f in (call, sync):
        assert f(r, rp=None) == PT_ERR_INVALID and f(r, op=None) == PT_ERR_INVALID   # a null pointer with n > 0
        assert f(r, params=P(0)) == PT_ERR_INVALID and f(r, params=P(65537)) == PT_ERR_INVALID
        assert f(r, n=2 ** 31 - 255) == PT_ERR_INVALID and b"2^31" in L.pt_last_error()
        assert f(r, n=0) == 0 and f(r, n=0, rp=None, op=None) == 0                    # a successful no-op
    assert call(r, params=P(65536), n=1) == 0
    assert call(r, rp=rays.data_ptr() + 8) == PT_ERR_INVALID and call(r, op=out.data_ptr() + 4) == PT_ERR_INVALID
    assert b"aligned" in L.pt_last_error()
    both = torch.zeros((64, 8), dtype=torch.float32, device="cuda")
    assert call(r, rp=both.data_ptr(), op=both.data_ptr()) == PT_ERR_INVALID and b"overlap" in L.pt_last_error()
    assert call(r, rp=both.data_ptr(), op=both.data_ptr() + 64 * 32 - 16) == PT_ERR_INVALID
    assert call(r, rp=both.data_ptr() + 32 * 32, n=32, op=both.data_ptr()) == 0      # the two halves: disjoint
    with pytest.raises(ptamd.PTError):
        r.set_option(O.PT_OPT_RADIANCE_CHUNK, -1)
    # pt_camera_rays needs a camera and a size
    cr = lambda r, px=None, n=4, op=both.data_ptr(): L.pt_camera_rays(r._c, 0, px, n, op)
    assert cr(r) == PT_ERR_INVALID and b"camera" in L.pt_last_error()
    r.set_camera(scenes.DEFAULT_CAMERA)
    assert cr(r) == PT_ERR_INVALID and b"frame" in L.pt_last_error()
    r.resize_and_clear(W, H)
    assert cr(r) == 0 and cr(r, n=0, op=None) == 0
    assert cr(r, op=None) == PT_ERR_INVALID and cr(r, op=both.data_ptr() + 8) == PT_ERR_INVALID
    assert cr(r, n=W * H + 1) == PT_ERR_INVALID
    g = ptamd.Renderer(devices=[0, 0])                                              # a multi-device context
    g.upload_scene(*support.scene("box"))
    assert call(g) == PT_ERR_UNSUPPORTED and sync(g) == PT_ERR_UNSUPPORTED and cr(g) == PT_ERR_UNSUPPORTED
    big = _ctx("tri:2000", 1, [(O.PT_OPT_SCENE_IN_LDS, 2)])
    assert call(big) == PT_ERR_UNSUPPORTED                                          # the LDS rule, as for a render
    r.synchronize()


def test_driver_radiance_against_the_sync_call(tmp_path):
    """pt_render -radiance: the driver's scene is box.obj under the reference light at -depth / -sss."""
    q = np.concatenate([RS.general_queries("box")[:100], RS.camera_queries("around", 0)[:200]])
    fin, fout = tmp_path / "queries.bin", tmp_path / "answers.bin"
    np.ascontiguousarray(q).tofile(fin)
    exe = os.path.join(PKG, "pt_render")
    res = subprocess.run(["timeout", "-k", "10", "60", exe, scenes.BOX_OBJ, "-w", "32", "-h", "24", "-depth", "3", "-sss", "2",
                          "-radiance", str(fin), str(fout), "-samples", "3", "-seed-stride", "384"],
                         capture_output=True, text=True)
    assert res.returncode == 0 and "radiance: 300 queries x 3 samples" in res.stdout, res.stdout + res.stderr
    got = np.fromfile(fout, F32).reshape(-1, 4)
    r = _ctx("box", 1, depth=3, sss=2)
    assert got.tobytes() == r.trace_radiance(q, 3, 384).tobytes()
    assert got.tobytes() == ptamd.trace_radiance_host(*support.scene("box"), RS.lights(1), q, 3, 384, 3, 2).tobytes()
