"""Batched ray queries on the GPU: pt_trace_rays against pt_trace_rays_host bit
for bit, both kinds, on every scene and ray family of tests/rays_support.py;
the same bits from every walk (the culled wide walk in both its shapes and node
layouts, the exact walk from LDS and from device memory, rays handed back);
batch sizes around the wave, the workgroup and the refill threshold; rays no
renderer would cast; and the plumbing: a context with a scene and nothing
else, a second upload, torch tensors on a stream, the driver's -pick, the
refusals, and a render that a query in its middle leaves untouched."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import ptamd
import rays_support as R
import scenes
import support
from support import PKG, same, same_nan

pytestmark = pytest.mark.gpu

PT_ERR_INVALID, PT_ERR_UNSUPPORTED = -1, -5
F32 = np.float32
O = ptamd
# the walks a query can take, as option lists
WALKS = {
    "defaults": [],
    "exact-lds": [(O.PT_OPT_WIDE, 0), (O.PT_OPT_SCENE_IN_LDS, 1)],
    "exact-device": [(O.PT_OPT_WIDE, 0), (O.PT_OPT_SCENE_IN_LDS, 0)],
    "wide-128": [(O.PT_OPT_WIDE_NODE, 128)],
    "wide-plain": [(O.PT_OPT_RAYS_REFILL, 0)],
    "wide-refill": [(O.PT_OPT_RAYS_REFILL, 1)],
    "wide-128-plain": [(O.PT_OPT_WIDE_NODE, 128), (O.PT_OPT_RAYS_REFILL, 0)],
    "handback-plain": [(O.PT_OPT_WIDE, 2), (O.PT_OPT_RAYS_REFILL, 0)],   # every odd ray marked for the exact kernel
    "handback-refill": [(O.PT_OPT_WIDE, 2), (O.PT_OPT_RAYS_REFILL, 1)],
}


def _ctx(scene, options=()):
    """A context with a scene and nothing else: no camera, no lights, no frame."""
    r = ptamd.Renderer(0)
    for key, value in options:
        r.set_option(key, value)
    r.upload_scene(*scene)
    return r


def _check(r, rays, any_rays, hits, occ, what):
    got = r.trace_rays(rays, O.RAYS_CLOSEST)
    assert np.array_equal(got["tri"], hits["tri"]), f"{what}: tri"
    same_nan(got.view(F32), hits.view(F32), f"{what}: closest")
    assert np.array_equal(r.trace_rays(any_rays, O.RAYS_ANY), occ), f"{what}: occlusion"


@pytest.mark.parametrize("name", R.SCENES)
def test_device_matches_host(name):
    c = R.case(name)
    hits, occ = R.host_answers(name)
    r = _ctx(c["scene"])
    _check(r, c["rays"], c["any_rays"], hits, occ, name)
    got = r.trace_rays(c["rays"])
    assert got.tobytes() == hits.tobytes(), "no NaN among these answers: the records are the host's byte for byte"
    if name in ("box", "sphere"):   # ... and the oracle's directly
        k = slice(0, 1000)
        assert np.array_equal(got["tri"][k] >= 0, c["hit"][k])
        same(got["t"][k], c["t"][k], "t against the oracle")
        same(got["n"][k], c["n"][k], "n against the oracle")
        assert np.array_equal(r.trace_rays(c["any_rays"][k], O.RAYS_ANY), c["occluded"][k])


@pytest.mark.parametrize("walk", list(WALKS))
@pytest.mark.parametrize("name", ["sphere", "grid:8", "box"])
def test_every_walk_gives_the_same_bits(name, walk):
    c = R.case(name)
    r = _ctx(c["scene"], WALKS[walk])
    if name == "sphere":
        assert r.wide_info()[0] > 0, "the sphere has a wide tree: without PT_OPT_WIDE 0 the wide kernel runs"
    _check(r, c["rays"], c["any_rays"], *R.host_answers(name), f"{name} {walk}")


def _tiled(a, n):
    return np.ascontiguousarray(a[np.arange(n) % len(a)])


@pytest.mark.parametrize("refill", [0, 1])
def test_batch_sizes(refill):
    """Below the refill threshold, ragged last waves, several workgroups."""
    c = R.case("sphere")
    hits, occ = R.host_answers("sphere")
    r = _ctx(c["scene"], [(O.PT_OPT_RAYS_REFILL, refill)])
    x = _ctx(c["scene"], [(O.PT_OPT_WIDE, 0)])
    for n in (1, 63, 64, 65, 255, 256, 257, 20000):
        for ctx in (r, x) if n <= 257 else (r,):
            _check(ctx, _tiled(c["rays"], n), _tiled(c["any_rays"], n), _tiled(hits, n), _tiled(occ, n), f"n = {n}")
    assert len(r.trace_rays(np.zeros((0, 8), F32))) == 0 and len(r.trace_rays(np.zeros((0, 8), F32), O.RAYS_ANY)) == 0


@pytest.mark.parametrize("options", [
    [(O.PT_OPT_WF_GRID, 1)], [(O.PT_OPT_WF_GRID, 1), (O.PT_OPT_WF_REFILL, 8)], [(O.PT_OPT_WF_GRID, 1), (O.PT_OPT_WF_REFILL, 16)],
    [(O.PT_OPT_WF_GRID, 1), (O.PT_OPT_RAYS_REFILL, 0)], [(O.PT_OPT_WF_GRID, 1), (O.PT_OPT_WF_REFILL, 64)],
    [(O.PT_OPT_WF_GRID, 1), (O.PT_OPT_WF_REFILL, 1), (O.PT_OPT_WIDE_NODE, 128)]])
def test_a_small_grid_takes_many_rays_per_lane(options):
    """PT_OPT_WF_GRID 1 with 20,000 rays: every lane takes several rays and refills."""
    c = R.case("sphere")
    hits, occ = R.host_answers("sphere")
    n = 20000
    _check(_ctx(c["scene"], options), _tiled(c["rays"], n), _tiled(c["any_rays"], n), _tiled(hits, n), _tiled(occ, n),
           str(options))


def _wide_ok(rays):
    """wide_ray_ok (wide_walk.h) in numpy float32."""
    o, d = rays[:, 0:3], rays[:, 3:6]
    with np.errstate(all="ignore"):
        inv = (F32(1.0) / d).astype(F32)
        d2 = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(F32)
        return (np.abs(inv) <= F32(2.0 ** 40)).all(1) & (np.abs(o) <= F32(1e15)).all(1) & (d2 <= F32(1.00002))


@pytest.mark.parametrize("refill", [0, 1])
def test_batches_all_exact_and_none_exact(refill):
    c = R.case("sphere")
    hits, occ = R.host_answers("sphere")
    ok = _wide_ok(c["rays"])
    assert ok.sum() >= 1000 and (~ok).sum() >= 500
    r = _ctx(c["scene"], [(O.PT_OPT_RAYS_REFILL, refill)])
    for pick, what in ((ok, "no ray needs the exact walk"), (~ok, "every ray needs the exact walk")):
        assert hits["tri"][pick].max() >= 0, what + ": and some hit"
        _check(r, np.ascontiguousarray(c["rays"][pick]), np.ascontiguousarray(c["any_rays"][pick]), hits[pick], occ[pick], what)


@pytest.mark.parametrize("walk", ["defaults", "wide-plain", "exact-device", "exact-lds"])
@pytest.mark.parametrize("name", ["sphere", "box"])
def test_hostile_rays(name, walk):
    scene = support.scene(name)
    rays, scaled, zero = R.hostile_rays(scene)
    hits = ptamd.trace_rays_host(*scene, rays)
    occ = ptamd.trace_rays_host(*scene, rays, O.RAYS_ANY)
    assert (hits["tri"][scaled] >= 0).sum() >= 8, "the non-unit rays include hits"
    assert (hits["tri"][zero] >= 0).sum() >= 8, "the zero-component rays include hits"
    assert occ[scaled].any() and occ[zero].any() and not occ[scaled].all()
    # |d| = 1e3 and a zero component fail wide_ray_ok: the exact walk.  |d| = 1e-3 passes it (the cull bound
    # asks for dot(d, d) <= 1.00002 and |1 / d| <= 2^40 only): the wide walk, where the scene has one
    long = np.linalg.norm(rays[scaled, 3:6].astype(np.float64), axis=1) > 1
    assert long.sum() == 24 and not _wide_ok(rays[scaled][long]).any() and _wide_ok(rays[scaled][~long]).all()
    assert not _wide_ok(rays[zero]).any()
    assert (hits["tri"][scaled][long] >= 0).sum() >= 8 and (hits["tri"][scaled][~long] >= 0).sum() >= 8
    # t scales with 1 / |d|
    t = hits["t"][scaled]
    assert ((t[hits["tri"][scaled] >= 0] > 100) | (t[hits["tri"][scaled] >= 0] < 0.1)).all()
    _check(_ctx(scene, WALKS[walk]), rays, rays, hits, occ, f"{name} {walk}")


def test_a_second_upload_moves_the_rank_table():
    a, b = R.case("sphere"), R.case("tri:2000")
    r = _ctx(a["scene"])
    _check(r, a["rays"], a["any_rays"], *R.host_answers("sphere"), "first scene")
    r.upload_scene(*b["scene"])
    assert r.wide_info()[0] > 0
    _check(r, b["rays"], b["any_rays"], *R.host_answers("tri:2000"), "second scene")
    r.upload_lights(scenes.REFERENCE_LIGHT)   # (bumps the scene serial too)
    r.upload_scene(*a["scene"])
    _check(r, a["rays"], a["any_rays"], *R.host_answers("sphere"), "first scene again")


def test_torch_tensors_on_the_context_s_stream():
    c = R.case("sphere")
    hits, occ = R.host_answers("sphere")
    r = _ctx(c["scene"])
    stream = torch.cuda.Stream()
    r.set_stream(stream.cuda_stream)
    with torch.cuda.stream(stream):
        rays = torch.from_numpy(np.array(c["rays"])).to("cuda")
        any_rays = torch.from_numpy(np.array(c["any_rays"])).to("cuda")
        got = r.trace_rays(rays)
        flags = r.trace_rays(any_rays, O.RAYS_ANY)
        nearer = got[:, 0] < 1e30   # torch work behind the query, on the same stream
        n_hit = int(nearer.sum().item())
    stream.synchronize()
    assert got.shape == (len(c["rays"]), 8) and got.dtype == torch.float32 and flags.dtype == torch.int32
    assert got.cpu().numpy().tobytes() == hits.tobytes()
    assert np.array_equal(flags.cpu().numpy().view(np.uint32), occ)
    assert n_hit == int((hits["tri"] >= 0).sum())
    assert got.cpu().numpy().tobytes() == r.trace_rays(c["rays"]).tobytes(), "the sync path"
    assert r.trace_rays(rays[:0]).shape == (0, 8)
    with pytest.raises(ptamd.PTError):
        r.trace_rays(rays.double())
    with pytest.raises(ptamd.PTError):
        r.trace_rays(rays.cpu())
    r.set_stream(None)


PICK = re.compile(r"pick \((\d+), (\d+)\): (miss|t (\S+) tri (-?\d+) u (\S+) v (\S+) n (\S+) (\S+) (\S+) p (\S+) (\S+) (\S+))")


def test_driver_pick_against_the_guide_image():
    W, H = 64, 48
    v, i, n = support.scene("box")
    r = support.renderer((v, i, n), scenes.DEFAULT_CAMERA, size=(W, H))
    r.render_guide()
    guide = r.read_guide().reshape(H, W, 4)
    exe = os.path.join(PKG, "pt_render")
    # the centre column's rays have a zero direction component; (0, 0) misses
    for x, y in ((W // 2, H // 2), (W // 2, 20), (27, 30), (0, 0)):
        res = subprocess.run(["timeout", "-k", "10", "60", exe, scenes.BOX_OBJ, "-w", str(W), "-h", str(H), "-spp", "0",
                              "-pick", str(x), str(y)], capture_output=True, text=True)
        assert res.returncode == 0, res.stdout + res.stderr
        m = PICK.search(res.stdout)
        assert m and (int(m.group(1)), int(m.group(2))) == (x, y), res.stdout
        g = guide[y, x]
        if m.group(3) == "miss":
            assert g[3] == F32(1e30) and (x, y) == (0, 0)
            continue
        t, tri, u, w = F32(m.group(4)), int(m.group(5)), F32(m.group(6)), F32(m.group(7))
        nrm, pos = F32([m.group(k) for k in (8, 9, 10)]), F32([m.group(k) for k in (11, 12, 13)])
        same(np.concatenate([nrm, [t]]), g, f"pixel ({x}, {y}): n and t")
        o, d = ptamd.guide_ray(scenes.DEFAULT_CAMERA, W, H, x, y)
        if x == W // 2:
            assert d[0] == 0
        same(pos, (o + d * t).astype(F32), "the position")
        h = ptamd.trace_rays_host(v, i, n, np.concatenate([o, d, [0, 0]]).astype(F32)[None])[0]
        assert (tri, u, w) == (h["tri"], h["u"], h["v"])


def test_refusals_and_error_paths():
    L = ptamd.lib()
    c = R.case("box")
    rays = torch.from_numpy(np.array(c["rays"][:64])).cuda()
    out = torch.zeros((64, 8), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    call = lambda r, kind=0, rp=rays.data_ptr(), n=64, op=out.data_ptr(): L.pt_trace_rays(r._c, kind, rp, n, op)
    host = np.ascontiguousarray(c["rays"][:64])
    hout = np.zeros(64, ptamd.HIT_DTYPE)
    sync = lambda r, kind=0, rp=host.ctypes.data, n=64, op=hout.ctypes.data: L.pt_trace_rays_sync(r._c, kind, rp, n, op)
    empty = ptamd.Renderer(0)
    assert call(empty) == PT_ERR_INVALID and b"scene" in L.pt_last_error()          # no scene
    assert sync(empty) == PT_ERR_INVALID and call(empty, n=0) == PT_ERR_INVALID
    r = _ctx(c["scene"])
    assert call(r) == 0 and sync(r) == 0
    r.synchronize()
    assert out.cpu().numpy().tobytes() == hout.tobytes() == R.host_answers("box")[0][:64].tobytes()
    for f in (call, sync):
        assert f(r, rp=None) == PT_ERR_INVALID and f(r, op=None) == PT_ERR_INVALID   # a null pointer with n > 0
        assert f(r, kind=2) == PT_ERR_INVALID and f(r, kind=-1) == PT_ERR_INVALID     # an unknown kind
        assert f(r, n=2 ** 31 - 255) == PT_ERR_INVALID and b"2^31" in L.pt_last_error()
        assert f(r, n=0) == 0 and f(r, n=0, rp=None, op=None) == 0                    # a successful no-op
    assert call(r, rp=rays.data_ptr() + 8) == PT_ERR_INVALID and call(r, op=out.data_ptr() + 4) == PT_ERR_INVALID
    assert b"aligned" in L.pt_last_error()
    assert call(r, rp=rays.data_ptr() + 32, n=63) == 0                              # 16-B aligned is enough
    with pytest.raises(ptamd.PTError):
        r.set_option(O.PT_OPT_RAYS_REFILL, 2)
    g = ptamd.Renderer(devices=[0, 0])                                              # a multi-device context
    g.upload_scene(*c["scene"])
    assert call(g) == PT_ERR_UNSUPPORTED and sync(g) == PT_ERR_UNSUPPORTED
    big = _ctx(R.case("tri:2000")["scene"], [(O.PT_OPT_WIDE, 0), (O.PT_OPT_SCENE_IN_LDS, 2)])
    assert call(big) == PT_ERR_UNSUPPORTED                                          # the LDS rule, as for the guide
    r.synchronize()


@pytest.mark.parametrize("name,options", [("box", []), ("sphere", [(O.PT_OPT_KERNEL, 3)])])
def test_a_query_between_two_renders_changes_nothing(name, options):
    c = R.case(name)
    cam = scenes.DEFAULT_CAMERA if name == "box" else scenes.camera((0.0, 0.5, 3.0))
    frames = []
    for query in (False, True):
        r = support.renderer(c["scene"], cam, size=(64, 48), options=options)
        r.render(0, 1)
        if query:
            _check(r, c["rays"], c["any_rays"], *R.host_answers(name), "between the renders")
        r.render(1, 2)
        frames.append(r.read_accum())
    same(frames[1], frames[0], "the accumulation image")


def test_queries_are_not_counted():
    c = R.case("sphere")
    for options in ([(O.PT_OPT_COUNT_TRACED, 1)], [(O.PT_OPT_COUNT_TRACED, 1), (O.PT_OPT_WIDE, 0)]):
        r = _ctx(c["scene"], options)
        r.set_stats_mode(True)
        _check(r, c["rays"], c["any_rays"], *R.host_answers("sphere"), "counting on")
        assert not any(r.traced().values()) and not any(r.stats().values())
