"""Batched ray queries without a GPU: pt_trace_rays_host, the host statement of
pt_trace_rays, against the oracle's traceRay on every scene and ray family;
what `tri`, `u` and `v` mean, pinned by an independent numpy Moller-Trumbore
on the uploaded arrays; answers known by hand; arguments and refusals; the
ABI's new names; and the stand-alone program meant for host sanitizer runs."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import native
import oracle_lib
import ptamd
import rays_support as R
import support
from support import same

F32 = np.float32


@pytest.mark.parametrize("name", R.SCENES)
def test_host_closest_matches_the_oracle(name):
    c = R.case(name)
    hits, _ = R.host_answers(name)
    assert np.array_equal(hits["tri"] >= 0, c["hit"]), "a miss is a miss"
    same(hits["t"], c["t"], f"{name}: t")
    same(hits["n"], c["n"], f"{name}: n")
    miss = hits[~c["hit"]]
    assert np.all(miss["tri"] == -1) and np.all(miss["reserved"] == 0) and np.all(hits["reserved"] == 0)
    same(miss["t"], np.full(len(miss), 1e30, F32), "a miss's t")
    for f in ("u", "v", "n"):
        assert not np.any(support.bits(miss[f])), f"a miss's {f} is +0"


@pytest.mark.parametrize("name", R.SCENES)
def test_host_occlusion_matches_the_oracle(name):
    c = R.case(name)
    _, occ = R.host_answers(name)
    assert np.array_equal(occ, c["occluded"])
    lim = c["any_rays"][:, 6]
    # the limits around the hits decide both ways: t itself and the float above it do not occlude ...
    k = np.arange(len(lim)) % 8
    assert not np.any(occ[c["hit"] & (k == 0)]) and np.all(occ[c["hit"] & (k == 1)] == 0)
    # ... the float above t does; NaN occludes whenever anything is hit; 0 and -1 never
    assert np.all(occ[c["hit"] & (k == 2)] == 1) and np.all(occ[c["hit"] & (k == 6)] == 1) and np.all(occ[c["hit"] & (k == 5)] == 1)
    assert not np.any(occ[(k == 3) | (k == 4)]) and not np.any(occ[~c["hit"]])
    assert np.isnan(lim[k == 6]).all()


@pytest.mark.parametrize("name", R.SCENES)
def test_tri_u_v_are_the_uploaded_triangle_s(name):
    c = R.case(name)
    hits, _ = R.host_answers(name)
    h = c["hit"]
    rays, rec = c["rays"][h], hits[h]
    n_tris = c["scene"][1].size // 3
    assert np.all((rec["tri"] >= 0) & (rec["tri"] < n_tris))
    ok, t, u, v = R.moller_trumbore(c["scene"], rays, rec["tri"])
    assert ok.all(), "the numpy intersectTriangle accepts every winning triangle"
    same(t, rec["t"], "t of indices[3*tri..]")
    same(u, rec["u"], "u")
    same(v, rec["v"], "v")
    assert np.all(rec["u"] >= 0) and np.all(rec["v"] >= 0) and np.all(rec["u"] + rec["v"] <= 1)
    # and the point the barycentrics name is the hit point, to rounding
    V = c["scene"][0].reshape(-1, 3)
    T = c["scene"][1].reshape(-1, 3)[rec["tri"]]
    w = (1 - rec["u"] - rec["v"])[:, None]
    p = w * V[T[:, 0]] + rec["u"][:, None] * V[T[:, 1]] + rec["v"][:, None] * V[T[:, 2]]
    q = rays[:, 0:3] + rays[:, 3:6] * rec["t"][:, None]
    scale = 1 + np.abs(rays[:, 0:3]).max(1) + rec["t"]
    assert np.all(np.abs(p - q).max(1) <= 1e-4 * scale)


# Families of make_rays that cannot have both hits and misses in a scene, whatever the seed (tried: seeds
# 1-59): a ray aimed at a point of a triangle from outside hits (3; the 0.01-sized triangles of the cloud are
# missed by rounding now and then), an origin inside the closed box hits (2), and a ray lying in a plane of
# the cube's or the grid's vertex coordinates never hits either mesh (6).  There the test pins the one outcome.
ONE_SIDED = {("box", 2): True, ("box", 3): True, ("sphere", 3): True, ("grid:8", 3): True,
             ("box", 6): False, ("grid:8", 6): False}


@pytest.mark.parametrize("name", R.SCENES)
def test_the_rays_reach_what_they_are_meant_to(name):
    """The conditions the other tests rest on, from the oracle's answers."""
    c = R.case(name)
    for j, sl in enumerate(R.families()):
        hit = c["hit"][sl]
        if (name, j + 1) in ONE_SIDED:
            assert hit.all() if ONE_SIDED[(name, j + 1)] else not hit.any(), f"{name}: family {j + 1}"
            continue
        assert hit.any() and not hit.all(), f"{name}: family {j + 1} has {int(hit.sum())} hits of {hit.size}"
    zero = R.families()[3]
    assert (c["rays"][zero, 3:6] == 0).any(1).all() and c["hit"][zero].any()
    assert c["hit"][R.N_MAKE:].any(), "the plane rays hit"


def test_grid_mesh_has_equal_t_ties():
    c = R.case("grid:8")
    tied = R.ties(c["scene"], c["rays"], c["t"]) & c["hit"]
    assert tied.sum() >= 1
    assert (tied & (c["rays"][:, 3:6] != 0).all(1)).sum() >= 1, "... one of them a ray the wide walk takes"
    # ... and the host statement gives them to the oracle's triangle: the same normal and t (above), and a
    # triangle that is accepted at that t
    hits, _ = R.host_answers("grid:8")
    ok, t, _, _ = R.moller_trumbore(c["scene"], c["rays"][tied], hits["tri"][tied])
    assert ok.all()
    same(t, c["t"][tied])


def _box_hit(o, d):
    scene = support.scene("box")
    rays = np.zeros((1, 8), F32)
    rays[0, 0:3], rays[0, 3:6] = o, d
    return ptamd.trace_rays_host(*scene, rays)[0], scene


def test_known_answers_on_the_box():
    # box.obj is the cube [-1, 1]^3, its normals pointing out
    h, scene = _box_hit((0, 0, 5), (0, 0, -1))   # the axis ray: the z = 1 face, 4 away
    V, T = scene[0].reshape(-1, 3), scene[1].reshape(-1, 3)
    assert h["t"] == 4.0 and tuple(h["n"]) == (0.0, 0.0, 1.0) and np.all(V[T[h["tri"]]][:, 2] == 1.0)
    assert h["u"] >= 0 and h["v"] >= 0 and h["u"] + h["v"] <= 1
    h, _ = _box_hit((0.25, 0.5, -0.125), (1, 0, 0))   # from inside: the x = 1 face from behind, 0.75 away
    assert h["t"] == 0.75 and tuple(h["n"]) == (1.0, 0.0, 0.0) and np.all(V[T[h["tri"]]][:, 0] == 1.0)
    # along the edge x = y = 1: the root's slab test already fails -- 1 / d.x = +inf, (1 - 1) * inf = NaN is
    # skipped by min and max, (-1 - 1) * inf = -inf is then both tNear.x and tFar.x, so tMax = -inf < 0: a miss
    h, _ = _box_hit((1, 1, 5), (0, 0, -1))
    assert h["tri"] == -1 and h["t"] == F32(1e30)
    assert not oracle_lib.trace(*scene, (1, 1, 5), (0, 0, -1))[0]
    # ... and 2^-20 inside the edge it is the z = 1 face again, next to its corner; the side faces are parallel
    e = 1 - 2.0 ** -20
    h, _ = _box_hit((e, e, 5), (0, 0, -1))
    assert h["t"] == 4.0 and tuple(h["n"]) == (0.0, 0.0, 1.0) and np.all(V[T[h["tri"]]][:, 2] == 1.0)
    assert min(h["u"], h["v"], 1 - h["u"] - h["v"]) <= 2.0 ** -20 and max(h["u"], h["v"], 1 - h["u"] - h["v"]) >= 1 - 2.0 ** -19
    h, _ = _box_hit((0, 0, 5), (0, 0, 1))    # away from it
    assert h["tri"] == -1 and h["t"] == F32(1e30)
    occ = ptamd.trace_rays_host(*scene, np.array([[0, 0, 5, 0, 0, -1, 4.0, 0], [0, 0, 5, 0, 0, -1, 4.5, 0]], F32), ptamd.RAYS_ANY)
    assert list(occ) == [0, 1]


def test_thread_count_does_not_change_the_output():
    c = R.case("sphere")
    one = ptamd.trace_rays_host(*c["scene"], c["rays"], threads=1)
    for threads in (2, 7, 64):
        assert ptamd.trace_rays_host(*c["scene"], c["rays"], threads=threads).tobytes() == one.tobytes()
    assert R.host_answers("sphere")[0].tobytes() == one.tobytes()   # threads = 0: one per core
    occ = ptamd.trace_rays_host(*c["scene"], c["any_rays"], ptamd.RAYS_ANY, threads=5)
    assert np.array_equal(occ, R.host_answers("sphere")[1])


def test_ray_records_and_the_float_layout_are_one():
    c = R.case("box")
    rec = np.zeros(8, ptamd.RAY_DTYPE)
    rec["o"], rec["d"], rec["limit"] = c["rays"][:8, 0:3], c["rays"][:8, 3:6], c["rays"][:8, 6]
    assert ptamd.RAY_DTYPE.itemsize == 32 and ptamd.HIT_DTYPE.itemsize == 32
    assert ptamd.trace_rays_host(*c["scene"], rec).tobytes() == R.host_answers("box")[0][:8].tobytes()


def test_int_bits_nodes_give_the_same_answers():
    c = R.case("grid:8")
    v, i, n = support.built(*__import__("scenes").grid_mesh(8), int_bits=True)
    assert np.array_equal(i, c["scene"][1])
    got = ptamd.trace_rays_host(v, i, n, c["rays"], int_bits=True)
    assert got.tobytes() == R.host_answers("grid:8")[0].tobytes()


def test_arguments_and_refusals():
    L = ptamd.lib()
    v, i, n = support.scene("box")
    n = np.ascontiguousarray(n, F32)
    rays = np.ascontiguousarray(R.case("box")["rays"][:4])
    out = np.zeros(4, ptamd.HIT_DTYPE)
    p = lambda a: a.ctypes.data
    host = lambda **kw: L.pt_trace_rays_host(*[kw.get(k, d) for k, d in (
        ("v", p(v)), ("nv", v.size), ("i", p(i)), ("ni", i.size), ("n", p(n)), ("nn", n.size // 8), ("flags", 0),
        ("kind", 0), ("rays", p(rays)), ("count", 4), ("out", p(out)), ("threads", 1))])
    assert host() == 0
    assert host(count=0, rays=None, out=None) == 0, "no rays: a successful no-op"
    for bad in (dict(v=None), dict(i=None), dict(n=None), dict(rays=None), dict(out=None), dict(kind=2), dict(kind=-1)):
        assert host(**bad) == -1, bad   # PT_ERR_INVALID
        assert L.pt_last_error()
    for bad in (dict(ni=i.size - 3), dict(nn=n.size // 8 - 1), dict(nv=v.size - 3), dict(ni=0), dict(nv=v.size - 1)):
        assert host(**bad) == -3, bad   # PT_ERR_SCENE
    loop = n.copy()
    loop[0, 3] = 0.0   # the root its own child: not a tree
    assert host(n=p(loop)) == -3 and b"tree" in L.pt_last_error()
    with pytest.raises(ptamd.PTError):
        ptamd.trace_rays_host(v, i, n, rays, kind=5)
    # the device calls without a context
    assert L.pt_trace_rays(None, 0, None, 0, None) == -1 and L.pt_trace_rays_sync(None, 0, None, 0, None) == -1


def test_abi_is_still_3_and_exports_the_new_names():
    L = ptamd.lib()
    assert L.pt_abi_version() == 3
    for name in ("pt_trace_rays", "pt_trace_rays_sync", "pt_trace_rays_host"):
        assert name in ptamd.EXPORTS and hasattr(ctypes.CDLL(ptamd.LIB_PATH), name)
    assert (ptamd.RAYS_CLOSEST, ptamd.RAYS_ANY, ptamd.PT_OPT_RAYS_REFILL) == (0, 1, 32)
    header = open(os.path.join(native.INCLUDE, "pathtracer.h")).read()
    for text in ("#define PT_OPT_RAYS_REFILL 32", "#define PT_RAYS_CLOSEST 0", "#define PT_RAYS_ANY 1"):
        assert text in header


def test_the_stand_alone_host_check_passes():
    """tests/rays_check.cpp, the program a host sanitizer run uses, built plainly."""
    scene_dir = os.path.join(native.CSRC, "scene")
    exe = native.build("rays_check", [os.path.join(native.TESTS, "rays_check.cpp"), os.path.join(native.CSRC, "pt_rays_host.cpp"),
                                      os.path.join(scene_dir, "threaded_bvh.cpp"), os.path.join(scene_dir, "bvh.cpp")],
                       ["-O1", "-g"] + native.COMMON + ["-I", native.CSRC], libs=["-lpthread"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "rays_check ok" in out.stdout, out.stdout + out.stderr
