"""Radiance queries on the host: pt_trace_radiance_host over pt_camera_rays_host
pinned to the oracle bit for bit (single batches, later batches, the running
mean over four), multi-sample queries against the numpy fold of single-sample
ones with strides that wrap, the pixel list of the camera rays, thread counts,
hostile rays, refusals, defaults, exports and the ABI, and the two stand-alone
programs (tests/radiance_check.cpp, tests/radiance_plan_check.cpp), built
plainly and under the address and undefined-behaviour sanitizers."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import native
import ptamd
import radiance_support as RS
import rays_support as R
import support
from support import oracle_frame, same

F32 = np.float32
W, H = RS.W, RS.H


def _queries(view, batch):
    return RS.camera_queries(view, batch)


@pytest.mark.parametrize("depth", [1, 4])
@pytest.mark.parametrize("sss", [0, 1, 3])
@pytest.mark.parametrize("n_lights", [0, 1, 2])
@pytest.mark.parametrize("view", ["around", "at-light"])
@pytest.mark.parametrize("name", RS.PIN_SCENES)
def test_oracle_pin(name, view, n_lights, sss, depth):
    """Every pixel of a 24x16 frame: the query along main()'s own ray equals the oracle's pixel.

    What the oracle's frames must show for the case to pin anything: black pixels always; with a light,
    shaded pixels (lit geometry); from the camera that looks into the light, pixels of exactly the first
    light's intensity (the pre-pass's early return).  Without lights the frame is black by statement."""
    sc = support.scene(name)
    cam, L = RS.CAMERAS[view], RS.lights(n_lights)
    what = f"{name} {view} {n_lights} lights sss {sss} depth {depth}"
    trace = lambda b: ptamd.trace_radiance_host(*sc, L, _queries(view, b), max_depth=depth, sss_bounces=sss)
    ref0 = oracle_frame(sc, cam, L, W, H, depth=depth, sss=sss)
    rgb = ref0.reshape(-1, 4)[:, :3]
    early = (rgb == L[8:11]).all(1) if n_lights else np.zeros(len(rgb), bool)
    black = (rgb == 0).all(1)
    assert black.any(), what + ": black pixels"
    if n_lights:
        assert (~black & ~early).any(), what + ": shaded pixels"
        if view == "at-light":
            assert early.any(), what + ": pixels of the light itself"
    else:
        assert black.all()
    colours = [trace(b) for b in range(4)]
    same(colours[0], ref0, what + ": batch 0")
    for b in (1, 7):
        c = colours[1] if b == 1 else trace(7)
        same(RS.fold_from(c, b), oracle_frame(sc, cam, L, W, H, first=b, depth=depth, sss=sss), what + f": batch {b}")
    same(RS.fold(colours), oracle_frame(sc, cam, L, W, H, nb=4, depth=depth, sss=sss), what + ": four batches folded")


@pytest.mark.parametrize("stride", [1, W * H, 0xFFFFFFFF])
@pytest.mark.parametrize("samples", [2, 5, 64])
def test_multi_sample_queries_are_the_fold_of_single_ones(samples, stride):
    sc = support.scene("box")
    L = RS.lights(2)
    q = np.array(_queries("at-light", 0)[::3])   # 128 queries, lit, shaded and black among them
    # seeds near the top of the range, so that every stride wraps for some sample
    q = RS.shifted(q, 0xFFFFFFFF - 40)
    got = ptamd.trace_radiance_host(*sc, L, q, samples, stride)
    singles = [ptamd.trace_radiance_host(*sc, L, RS.shifted(q, (s * stride) & 0xFFFFFFFF)) for s in range(samples)]
    same(got, RS.fold(singles), f"S = {samples}, stride {stride:#x}")
    assert np.any(got[:, :3] != 0) and np.all(got[:, 3] == 1)


def test_camera_rays_pixel_lists():
    cam = RS.CAMERAS["around"]
    full = ptamd.camera_rays_host(cam, W, H, 5)
    assert full.shape == (W * H,) and np.all(full["limit"] == F32(1e30))
    y, x = np.divmod(np.arange(W * H), W)
    assert np.array_equal(full["reserved"], ((5 * H + y) * W + x).astype(np.uint32))
    norm = np.linalg.norm(full["d"].astype(np.float64), axis=1)
    assert np.all(np.abs(norm - 1) < 1e-6)
    assert np.array_equal(ptamd.camera_rays_host(cam, W, H, 5, np.arange(W * H)), full), "the list of every pixel"
    order = np.random.default_rng(3).permutation(W * H)[:100]
    assert np.array_equal(ptamd.camera_rays_host(cam, W, H, 5, order), full[order]), "out of order"
    twice = np.array([7, 7, 0, W * H - 1, 7])
    assert np.array_equal(ptamd.camera_rays_host(cam, W, H, 5, twice), full[twice])
    assert len(ptamd.camera_rays_host(cam, W, H, 5, np.zeros(0, np.int32))) == 0
    # the seed wraps in uint32 arithmetic
    big = ptamd.camera_rays_host(cam, W, H, 0xFFFFFFF0, [W * H - 1])
    assert int(big["reserved"][0]) == ((0xFFFFFFF0 * H + H - 1) * W + W - 1) & 0xFFFFFFFF
    for bad in ([-1], [W * H]):
        with pytest.raises(ptamd.PTError):
            ptamd.camera_rays_host(cam, W, H, 0, bad)


@pytest.mark.parametrize("name", ["box", "sphere"])
def test_thread_counts_give_the_same_bytes(name):
    sc = support.scene(name)
    q = RS.general_queries(name)
    L = RS.lights(2)
    one = ptamd.trace_radiance_host(*sc, L, q, 2, 3, threads=1)
    assert np.any(one[:, :3] != 0)
    for t in (3, 16):
        assert ptamd.trace_radiance_host(*sc, L, q, 2, 3, threads=t).tobytes() == one.tobytes(), t


@pytest.mark.parametrize("name", R.SCENES)
def test_hostile_rays_return_and_repeat(name):
    """No oracle exists for these: the host is the definition.  It returns, and its bytes do not depend on
    the thread count."""
    sc = support.scene(name)
    q = RS.hostile_queries(name)
    a = ptamd.trace_radiance_host(*sc, RS.lights(2), q, 2, 5, threads=1)
    b = ptamd.trace_radiance_host(*sc, RS.lights(2), q, 2, 5, threads=16)
    assert a.shape == (len(q), 4) and a.tobytes() == b.tobytes()
    assert np.all(a[:, 3] == 1)


def test_records_and_the_float_layout_are_one():
    sc = support.scene("box")
    q = np.array(_queries("around", 0)[:64])
    rec = ptamd.radiance_queries(q[:, 0:3], q[:, 3:6], q.view(np.uint32)[:, 7])
    assert rec.dtype == ptamd.RAY_DTYPE
    a = ptamd.trace_radiance_host(*sc, RS.lights(1), q)
    assert ptamd.trace_radiance_host(*sc, RS.lights(1), rec).tobytes() == a.tobytes()
    # limit is ignored
    q2 = q.copy()
    q2[:, 6] = [np.nan, -1, 0, 1e-3] * 16
    assert ptamd.trace_radiance_host(*sc, RS.lights(1), q2).tobytes() == a.tobytes()


def test_int_bits_nodes_give_the_same_answers():
    import scenes
    v, i, n = support.built(*scenes.grid_mesh(8), int_bits=True)
    q = RS.general_queries("grid:8")
    got = ptamd.trace_radiance_host(v, i, n, RS.lights(1), q, int_bits=True)
    assert got.tobytes() == RS.host("grid:8", "general", 1).tobytes()


def test_arguments_defaults_and_refusals():
    L = ptamd.lib()
    v, i, n = support.scene("box")
    n = np.ascontiguousarray(n, F32)
    lights = RS.lights(1)
    rays = np.array(_queries("around", 0)[:4])
    out = np.zeros((4, 4), F32)
    p = lambda a: a.ctypes.data
    params = ptamd.RadianceParams()
    assert L.pt_radiance_default_params(ctypes.byref(params)) == 0 and (params.n_samples, params.seed_stride) == (1, 1)
    assert L.pt_radiance_default_params(None) == -1
    host = lambda **kw: L.pt_trace_radiance_host(*[kw.get(k, d) for k, d in (
        ("v", p(v)), ("nv", v.size), ("i", p(i)), ("ni", i.size), ("n", p(n)), ("nn", n.size // 8), ("flags", 0),
        ("lights", p(lights)), ("nl", 1), ("depth", 4), ("sss", 3), ("params", None), ("rays", p(rays)), ("count", 4),
        ("out", p(out)), ("threads", 1))])
    assert host() == 0
    want = out.copy()
    assert host(params=ctypes.byref(ptamd.RadianceParams(1, 1))) == 0 and out.tobytes() == want.tobytes(), "null = the defaults"
    assert host(count=0, rays=None, out=None) == 0, "no queries: a successful no-op"
    assert host(nl=0, lights=None) == 0, "zero lights are valid"
    for bad in (dict(v=None), dict(i=None), dict(n=None), dict(rays=None), dict(out=None), dict(lights=None),
                dict(depth=-1), dict(sss=-1), dict(params=ctypes.byref(ptamd.RadianceParams(0, 1))),
                dict(params=ctypes.byref(ptamd.RadianceParams(65537, 1)))):
        assert host(**bad) == -1, bad   # PT_ERR_INVALID
        assert L.pt_last_error()
    assert host(params=ctypes.byref(ptamd.RadianceParams(65536, 0)), count=1) == 0
    for bad in (dict(ni=i.size - 3), dict(nn=n.size // 8 - 1), dict(nv=v.size - 1), dict(ni=0)):
        assert host(**bad) == -3, bad   # PT_ERR_SCENE
    # the device calls without a context
    assert L.pt_trace_radiance(None, None, None, 0, None) == -1 and L.pt_trace_radiance_sync(None, None, None, 0, None) == -1
    assert L.pt_camera_rays(None, 0, None, 0, None) == -1
    cam = np.ascontiguousarray(RS.CAMERAS["around"], F32)
    rec = np.zeros(4, ptamd.RAY_DTYPE)
    assert L.pt_camera_rays_host(p(cam), W, H, 0, None, 4, p(rec)) == 0
    assert L.pt_camera_rays_host(None, W, H, 0, None, 4, p(rec)) == -1
    assert L.pt_camera_rays_host(p(cam), 0, H, 0, None, 4, p(rec)) == -1
    assert L.pt_camera_rays_host(p(cam), W, H, 0, None, W * H + 1, p(rec)) == -1
    assert L.pt_camera_rays_host(p(cam), W, H, 0, None, 4, None) == -1
    assert L.pt_camera_rays_host(p(cam), W, H, 0, None, 0, None) == 0


def test_abi_is_still_3_and_exports_the_new_names():
    L = ptamd.lib()
    assert L.pt_abi_version() == 3
    names = ("pt_radiance_default_params", "pt_trace_radiance", "pt_trace_radiance_sync", "pt_trace_radiance_host",
             "pt_camera_rays", "pt_camera_rays_host")
    header = open(os.path.join(native.INCLUDE, "pathtracer.h")).read()
    for name in names:
        assert name in ptamd.EXPORTS and hasattr(ctypes.CDLL(ptamd.LIB_PATH), name)
        assert re.search(r"^int " + name + r"\(", header, re.M), name
    assert ptamd.PT_OPT_RADIANCE_CHUNK == 34 and "#define PT_OPT_RADIANCE_CHUNK 34" in header
    taken = [v for k, v in vars(ptamd).items() if k.startswith("PT_OPT_") and k != "PT_OPT_RADIANCE_CHUNK"]
    assert 34 not in taken
    assert "#define PT_ABI_VERSION 3" in header and "typedef struct pt_radiance_params" in header


def _sources():
    scene_dir = os.path.join(native.CSRC, "scene")
    return [os.path.join(native.TESTS, "radiance_check.cpp"), os.path.join(native.CSRC, "pt_radiance_host.cpp"),
            os.path.join(native.CSRC, "pt_rays_host.cpp"), os.path.join(scene_dir, "threaded_bvh.cpp"),
            os.path.join(scene_dir, "bvh.cpp")]


SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


def _run(exe, word):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and word in out.stdout, out.stdout + out.stderr
    return out.stdout.splitlines()


def test_the_stand_alone_host_check_passes():
    exe = native.build("radiance_check", _sources(), ["-O1", "-g"] + native.COMMON + ["-I", native.CSRC], libs=["-lpthread"])
    _run(exe, "radiance_check ok")


def test_the_stand_alone_host_check_under_the_sanitizers(tmp_path):
    exe = native.build("radiance_check", _sources(), ["-O1", "-g"] + native.COMMON + SANITIZE + ["-I", native.CSRC],
                       libs=["-lpthread"], out_dir=tmp_path)
    _run(exe, "radiance_check ok")


def test_plan_radiance_table():
    src = [os.path.join(native.TESTS, "radiance_plan_check.cpp")]
    exe = native.build("radiance_plan_check", src, ["-O1"] + native.COMMON[:2] + ["-I", native.CSRC])
    lines = _run(exe, "radiance_plan_check ok")
    assert sum(1 for ln in lines if ln.startswith("n=")) >= 40 and sum(1 for ln in lines if ln.startswith("wf wide=")) == 16
    assert sum(1 for ln in lines if ln.startswith("lds=")) == 16


def test_plan_radiance_table_under_the_sanitizers(tmp_path):
    src = [os.path.join(native.TESTS, "radiance_plan_check.cpp")]
    exe = native.build("radiance_plan_check", src, ["-O1", "-g"] + native.COMMON[:2] + SANITIZE + ["-I", native.CSRC],
                       out_dir=tmp_path)
    _run(exe, "radiance_plan_check ok")
