"""What the radiance-query tests share, on the CPU and on the GPU: the oracle-pin
matrix (scenes, cameras, lights), the camera's own rays of a frame as queries,
the shader's running mean in numpy float32, queries from the ray-query tests'
rays, and the host statement's answers (computed once per process, read-only)."""
import functools

import numpy as np

import ptamd
import rays_support as R
import scenes
import support

F32 = np.float32
W, H = 24, 16


def look(pos, at, fov):
    pos, at = np.asarray(pos, np.float64), np.asarray(at, np.float64)
    ubo = np.zeros(16, F32)
    ubo[0:3] = pos
    ubo[4:7] = (at - pos) / np.linalg.norm(at - pos)
    ubo[8:11] = (0, 1, 0)
    ubo[12] = fov
    return ubo


# the default camera, and one behind and above the geometry that looks into the reference light
# (test_gpu_reseed_reuse.py's second camera of the box)
CAMERAS = {"around": scenes.DEFAULT_CAMERA, "at-light": look([1.5, 4.0, 4.0], [0.0, 0.5, 0.0], 60.0)}
PIN_SCENES = ["box", "sphere"]


def lights(n):
    return np.ascontiguousarray(support.TWO_LIGHTS[:16 * n])


def fold(colours):
    """The shader's running mean (:467-469) of colours[s] (each (n, 3) or (n, 4); alpha folds 1) in order from
    +0, one float32 rounding per operation: (n, 4)."""
    acc = np.zeros((len(colours[0]), 4), F32)
    with np.errstate(all="ignore"):
        for s, c in enumerate(colours):
            fb, fb1 = F32(s), F32(s + 1)
            acc[:, :3] = ((acc[:, :3] * fb).astype(F32) + np.asarray(c, F32)[:, :3]).astype(F32) / fb1
            acc[:, 3] = ((acc[:, 3] * fb).astype(F32) + F32(1)).astype(F32) / fb1
    return acc


def fold_from(colour, batch):
    """float32((0 * fb + c) / fb1) with alpha (0 * fb + 1) / fb1: one batch folded into a cleared image."""
    fb, fb1 = F32(batch), F32(batch + 1)
    out = np.empty((len(colour), 4), F32)
    out[:, :3] = ((F32(0) * fb) + np.asarray(colour, F32)[:, :3]).astype(F32) / fb1
    out[:, 3] = F32((F32(0) * fb + F32(1)) / fb1)
    return out


def with_seeds(rays, seeds):
    """The (n, 8) float32 rays with `seeds` (uint32) in the reserved word."""
    q = np.array(rays, F32).reshape(-1, 8)
    q.view(np.uint32)[:, 7] = np.asarray(seeds, np.uint32)
    return q


def shifted(rays, add):
    """The queries with `add` added to every seed, uint32 wrap-around."""
    q = np.array(rays).view(F32).reshape(-1, 8).copy()
    s = q.view(np.uint32)[:, 7].astype(np.uint64)
    q.view(np.uint32)[:, 7] = ((s + np.uint64(add)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    return q


@functools.lru_cache(maxsize=None)
def camera_queries(view, batch, w=W, h=H):
    q = ptamd.camera_rays_host(CAMERAS[view], w, h, batch).view(F32).reshape(-1, 8)
    q.setflags(write=False)
    return q


@functools.lru_cache(maxsize=None)
def general_queries(name, n=600):
    """n of make_rays' rays of a scene of rays_support.SCENES, seeds 0 .. n-1."""
    q = with_seeds(R.case(name)["rays"][:n], np.arange(n))
    q.setflags(write=False)
    return q


@functools.lru_cache(maxsize=None)
def host(name, which, n_lights, samples=1, stride=1, depth=4, sss=3, view="around"):
    """pt_trace_radiance_host's answers, read-only.  which: "general" (general_queries), "camera" (batch 0 of the
    24x16 frame from `view`) or "hostile" (rays_support.hostile_rays with seeds 0 ..)."""
    sc = support.scene(name)
    if which == "general":
        q = general_queries(name)
    elif which == "camera":
        q = camera_queries(view, 0)
    else:
        q = hostile_queries(name)
    out = ptamd.trace_radiance_host(*sc, lights(n_lights), q, samples, stride, depth, sss)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def hostile_queries(name):
    rays, _, _ = R.hostile_rays(support.scene(name))
    q = with_seeds(rays, np.arange(len(rays)) * 7919)
    q.setflags(write=False)
    return q
