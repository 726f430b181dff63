"""What the test modules share: the one bitwise comparison, image helpers,
built scenes and oracle frames (cached across modules), a renderer set up in
the order every test uses, and device-memory access for the GPU tests."""
import ctypes
import functools
import os

import numpy as np

import oracle_lib
import ptamd
import scenes

# where libptamd.so and pt_render lie
PKG = os.path.dirname(os.path.abspath(ptamd.__file__))
# the reference light and a second one of another colour, size and direction
TWO_LIGHTS = np.concatenate([scenes.REFERENCE_LIGHT,
                             ptamd.pack_light([0.5, 0.5, 1.5], [0, 0, -1], [2, 4, 8], [0.5, 1.0])])


def bits(a):
    """The uint32 view of a contiguous float32 array."""
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(got, want, what=""):
    """got and want hold the same float32 bits.  Sizes must be equal, and shapes
    too unless one side is flat (the oracle's frames are); nothing is broadcast."""
    g, w = bits(got), bits(want)
    assert g.size == w.size, f"{what}: {g.size} floats {g.shape} against {w.size} {w.shape}"
    assert g.shape == w.shape or g.ndim == 1 or w.ndim == 1, f"{what}: shape {g.shape} against {w.shape}"
    bad = np.flatnonzero(g.reshape(-1) != w.reshape(-1))
    if bad.size:
        gf, wf = g.view(np.float32).reshape(-1), w.view(np.float32).reshape(-1)
        at = np.unravel_index(bad[0], g.shape if g.ndim >= w.ndim else w.shape)
        with np.errstate(invalid="ignore"):
            diff = np.abs(gf[bad].astype(np.float64) - wf[bad].astype(np.float64))
        diff = diff[np.isfinite(diff)]
        raise AssertionError(f"{what}: {bad.size} of {g.size} floats differ (max |diff| {diff.max() if diff.size else 0.0}); "
                             f"first at {tuple(int(k) for k in at)}: got {gf[bad[0]]} ({g.reshape(-1)[bad[0]]:#010x}), "
                             f"want {wf[bad[0]]} ({w.reshape(-1)[bad[0]]:#010x})")


def same_nan(got, want, what=""):
    """NaN exactly where NaN (its sign and payload are the platform's), every
    other float the same bits."""
    g, w = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert g.size == w.size, f"{what}: {g.size} floats {g.shape} against {w.size} {w.shape}"
    assert g.shape == w.shape or g.ndim == 1 or w.ndim == 1, f"{what}: shape {g.shape} against {w.shape}"
    nan_g, nan_w = np.isnan(g).reshape(-1), np.isnan(w).reshape(-1)
    bad = np.flatnonzero(nan_g != nan_w)
    if bad.size:
        at = np.unravel_index(bad[0], g.shape if g.ndim >= w.ndim else w.shape)
        raise AssertionError(f"{what}: NaN pattern differs in {bad.size} of {g.size} floats; first at "
                             f"{tuple(int(k) for k in at)}: got {g.reshape(-1)[bad[0]]}, want {w.reshape(-1)[bad[0]]}")
    same(np.where(nan_g, np.float32(0), g.reshape(-1)).reshape(g.shape),
         np.where(nan_w, np.float32(0), w.reshape(-1)).reshape(w.shape), what)


def read_pfm(path):
    """A little-endian colour PFM as (h, w, 3) float32, rows in file order."""
    with open(path, "rb") as f:
        assert f.readline().strip() == b"PF"
        w, h = map(int, f.readline().split())
        assert float(f.readline()) < 0   # little-endian
        return np.fromfile(f, "<f4").reshape(h, w, 3)


def mse(a, b, mask=None):
    """Mean squared rgb difference in float64, over the masked pixels if a mask is given."""
    d = a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)
    if mask is not None:
        d = d[mask]
    return float(np.mean(d * d))


def lit_pixels(frame):
    """Pixels of an rgba frame with a non-zero colour."""
    return int(np.count_nonzero(np.any(frame.reshape(-1, 4)[:, :3] != 0, axis=1)))


def built(v, i, int_bits=False):
    """(vertices, indices, nodes) of the mesh behind the library's own BVH build."""
    v, i, n, _, _ = ptamd.Scene.from_arrays(v, i).build_bvh(int_bits=int_bits).arrays()
    return v, i, n


@functools.lru_cache(maxsize=None)
def _scene(name, make):
    if make is not None:
        return built(*make())
    if name == "box":
        v, i, n, _, _ = ptamd.Scene.load_obj(scenes.BOX_OBJ).build_bvh().arrays()
        return v, i, n
    if name == "sphere":
        return built(*scenes.displaced_sphere(subdiv=3))
    kind, n = name.split(":")
    return built(*{"grid": scenes.grid_mesh, "tri": scenes.random_triangles}[kind](int(n)))


def scene(name, extra=None):
    """The built scene of a name, made once: "box", "sphere" (displaced_sphere(subdiv=3)),
    "grid:N", "tri:N", or a name of `extra`, a module's dict of name -> maker of (vertices, indices)."""
    return _scene(name, extra.get(name) if extra else None)


def box_mesh():
    """(vertices, indices) of tests/golden/box.obj as the oracle parses it."""
    with open(scenes.BOX_OBJ, "rb") as f:
        v, i, _ = oracle_lib.obj_parse(f.read())
    return v, i


def oracle_built(v, i):
    """(vertices, indices, nodes) of the mesh behind the oracle's BVH build."""
    idx, nodes = oracle_lib.bvh_build(v, i)
    return np.ascontiguousarray(v, np.float32), idx, nodes


_FRAMES = {}


def oracle_frame(scene, cam, lights, W, H, first=0, nb=1, depth=4, sss=3, **kw):
    """The oracle's frame of a built scene, read-only, computed once per process: the key is the scene
    tuple itself (scene() hands out the same one every time) and the bits of every other input."""
    key = (id(scene), bits(cam).tobytes(), bits(lights).tobytes(), W, H, first, nb, depth, sss, tuple(sorted(kw.items())))
    if key not in _FRAMES:
        v, i, n = scene
        ref, _ = oracle_lib.render(v, i, n.reshape(-1), cam, lights, W, H, first_batch=first, n_batches=nb,
                                   max_depth=depth, sss_bounces=sss, **kw)
        ref.setflags(write=False)
        _FRAMES[key] = (scene, ref)   # the scene is kept so that its id stays its own
    return _FRAMES[key][1]


def renderer(scene, cam, lights=scenes.REFERENCE_LIGHT, depth=4, sss=3, size=None, options=(), int_bits=False):
    """A Renderer on device 0 set up in the order every test uses: options ((key, value) pairs or a
    dict), scene, lights, camera, parameters, then the frame if a size is given."""
    r = ptamd.Renderer(0)
    for key, value in (options.items() if isinstance(options, dict) else options):
        r.set_option(key, value)
    r.upload_scene(*scene, int_bits=int_bits)
    r.upload_lights(lights)
    r.set_camera(cam)
    r.set_params(depth, sss)
    if size is not None:
        r.resize_and_clear(*size)
    return r


@functools.lru_cache(maxsize=None)
def hip():
    """The HIP runtime this process already holds (torch's)."""
    with open("/proc/self/maps") as f:
        path = next(line.split()[-1] for line in f if "libamdhip64" in line)
    return ctypes.CDLL(path)


def read_device(r, ptr, shape):
    """A library-owned float image, copied behind the context's work."""
    r.synchronize()
    out = np.empty(shape, np.float32)
    assert hip().hipMemcpy(ctypes.c_void_p(out.ctypes.data), ctypes.c_void_p(ptr), ctypes.c_size_t(out.nbytes), 2) == 0
    return out


def write_device(r, ptr, array):
    """read_device's counterpart: the float32 array copied over a library-owned
    image, behind the context's work and done when the call returns."""
    assert ptr, "no such device image"
    r.synchronize()
    a = np.ascontiguousarray(array, np.float32)
    assert hip().hipMemcpy(ctypes.c_void_p(ptr), ctypes.c_void_p(a.ctypes.data), ctypes.c_size_t(a.nbytes), 1) == 0


def dev(a):
    """The array as a float32 tensor on the GPU."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
