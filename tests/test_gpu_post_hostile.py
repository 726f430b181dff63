"""GPU: every kernel downstream of the render on the extreme and non-finite
image sets of tests/hostile_images.py, against the host's run of the same
header code and against the numpy restatement -- NaN where NaN, every other
float bitwise (support.same_nan) -- on every kernel shape: atrous_kernel and
both staged forms (pt_denoise with a caller's source, the crafted guide written
over the rendered one), moments_var_kernel and the variance filter's three
(pt_denoise_var over an overwritten accumulator, moments and guide; then
pt_temporal_denoise and pt_temporal_denoise_spatial over an overwritten
temporal result), reproject_kernel, spatial_var_kernel and
adaptive_select_kernel.  The cases, sizes, pass counts and the condition that
keeps NaN from hiding a failure are tests/test_post_hostile.py's.  Inputs must
come back unchanged.  Last, one frame the renderer itself makes non-finite,
through the whole chain.

adaptive_var_kernel is not reached: after an adaptive render the library hands
out no pointer to the moments (pt_moments_device_ptr is null without a single
sample count); its statement, var_of_mean, runs here in moments_var_kernel."""
import numpy as np
import pytest
import torch

import adaptive_ref as A
import denoise_var_ref as V
import hostile_images as X
import ptamd
import scenes
import spatial_var_ref as S
import temporal_ref as T
import support
from support import oracle_frame, read_device, renderer, same, same_nan, scene, write_device
from test_post_hostile import ADAPTIVE_PARAMS, KINDS, REPROJECT_PARAMS, SIZES, SPATIAL_PARAMS, adaptive_counts
from test_temporal import CAMERAS, CUR

pytestmark = pytest.mark.gpu

F = np.float32
MOMENTS = [(ptamd.PT_OPT_MOMENTS, 1)]
SPATIAL = (4, 1, 0.5, 0.25)


def dev(a):
    """support.dev of a copy: the image sets are read-only, which torch.from_numpy does not take."""
    return support.dev(np.array(a, F))


def _renderer(W, H, options=()):
    """A context with the box and a W x H frame: every size here is accepted."""
    return renderer(scene("box"), CUR, size=(W, H), options=options)


def _both(got, host, ref, what):
    same_nan(got, host, f"{what}: device against host")
    same_nan(got, ref, f"{what}: device against the restatement")


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_atrous_kernels(kind, W, H):
    r = _renderer(W, H)
    r.render_guide()
    n_run = 0
    for seed, plane, k in X.filter_cases("atrous", kind, W, H):
        d = X.images(kind, W, H, seed, plane)
        ref = X.reference("atrous", kind, W, H, seed, plane, k)
        assert (W, H) in X.TINY or X.enough(ref)
        host = ptamd.denoise_host(d["color"], d["guide"], W, H, X.denoise_params(k))
        write_device(r, r.guide_ptr(), d["guide"])
        src = dev(d["color"])
        for staged in (0, 1):
            dst = torch.full((H, W, 4), -7.0, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            r.set_option(ptamd.PT_OPT_DENOISE_LDS, staged)
            assert r.denoise(X.denoise_params(k), src.data_ptr(), dst.data_ptr()) is None
            r.synchronize()
            got = dst.cpu().numpy()
            _both(got, host, ref, f"{kind} {W}x{H} seed {seed} {plane}, {k} passes, staged {staged}")
            if kind == "extremes":
                assert np.isfinite(got).any()
        same(src.cpu().numpy(), d["color"], "the caller's source after the filter")
        same(r.read_guide(), d["guide"], "the guide after the filter")
        n_run += 1
    assert n_run >= len(X.PASSES[kind])


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_variance_filter_kernels(kind, W, H):
    r = _renderer(W, H, MOMENTS)
    r.render(0, X.N_SAMPLES)
    r.render_guide()
    assert r.read_moments()[1] == X.N_SAMPLES
    n_run = 0
    for seed, plane, k in X.filter_cases("var", kind, W, H):
        d = X.images(kind, W, H, seed, plane)
        ref = X.reference("var", kind, W, H, seed, plane, k)
        assert (W, H) in X.TINY or X.enough(ref)
        host = ptamd.denoise_var_host(d["color"], d["moments"], X.N_SAMPLES, d["guide"], W, H, X.var_params(k))
        write_device(r, r.accum_ptr(), d["color"])
        write_device(r, r.moments_ptr(), d["moments"])
        write_device(r, r.guide_ptr(), d["guide"])
        for staged in (0, 1):
            r.set_option(ptamd.PT_OPT_DENOISE_LDS, staged)
            _both(r.denoise_var(X.var_params(k)), host, ref, f"{kind} {W}x{H} seed {seed} {plane}, {k} passes, staged {staged}")
        same(r.read_accum().reshape(H, W, 4), d["color"], "the accumulation image after the filter")
        same(r.read_moments()[0], d["moments"], "the moments after the filter")
        same(r.read_guide(), d["guide"], "the guide after the filter")
        n_run += 1
    assert n_run >= len(X.PASSES[kind])


def test_variance_filter_of_a_bound_accumulator():
    """The same over a caller's accumulation image (pt_bind_accum)."""
    W, H, kind, plane, k = 37, 23, "nonfinite", "all", 3
    seed, = X.seeds(kind, W, H)
    d = X.images(kind, W, H, seed, plane)
    r = _renderer(W, H, MOMENTS)
    acc = torch.zeros(H, W, 4, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    r.bind_accum(acc.data_ptr(), W, H)
    r.render(0, X.N_SAMPLES)
    r.render_guide()
    r.synchronize()
    acc.copy_(torch.from_numpy(np.array(d["color"], F)))               # a copy: the image sets are read-only
    torch.cuda.synchronize()
    write_device(r, r.moments_ptr(), d["moments"])
    write_device(r, r.guide_ptr(), d["guide"])
    ref = X.reference("var", kind, W, H, seed, plane, k)
    host = ptamd.denoise_var_host(d["color"], d["moments"], X.N_SAMPLES, d["guide"], W, H, X.var_params(k))
    _both(r.denoise_var(X.var_params(k)), host, ref, "bound accumulator")
    same(acc.cpu().numpy(), d["color"], "the bound image after the filter")


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_temporal_filters(kind, W, H):
    r = _renderer(W, H, MOMENTS)
    r.temporal_advance(CUR, 2)
    keys = ("color", "moments", "length", "variance")
    n_run = 0
    for seed, plane, k in X.filter_cases("plane", kind, W, H):
        d = X.images(kind, W, H, seed, plane)
        ref = X.reference("plane", kind, W, H, seed, plane, k)
        assert (W, H) in X.TINY or X.enough(ref)
        for which, key in enumerate(keys):
            write_device(r, r.temporal_ptr(which), d[key])
        write_device(r, r.guide_ptr(), d["guide"])
        host = ptamd.denoise_var_plane_host(d["color"], d["variance"], d["guide"], W, H, X.var_params(k))
        est = S.spatial_variance(d["moments"], d["length"], d["variance"], d["guide"], W, H, SPATIAL)
        est_ref = T.atrous_var_plane(d["color"], est, d["guide"], W, H, X.var_params(k))
        est_host = ptamd.denoise_var_plane_host(
            d["color"], ptamd.spatial_variance_host(d["moments"], d["length"], d["variance"], d["guide"], W, H, SPATIAL),
            d["guide"], W, H, X.var_params(k))
        what = f"{kind} {W}x{H} seed {seed} {plane}, {k} passes"
        for staged in (0, 1):
            r.set_option(ptamd.PT_OPT_DENOISE_LDS, staged)
            _both(r.temporal_denoise(X.var_params(k)), host, ref, f"pt_temporal_denoise {what}, staged {staged}")
            if (W, H) in X.TINY or X.enough(est_ref):
                _both(r.temporal_denoise_spatial(X.var_params(k), SPATIAL), est_host, est_ref,
                      f"pt_temporal_denoise_spatial {what}, staged {staged}")
        after = r.read_temporal() + (read_device(r, r.temporal_ptr(3), (H, W)),)
        for a, key in zip(after, keys):
            same(a, d[key], f"the temporal {key} after the filters")
        same(r.read_guide(), d["guide"], "the guide after the filters")
        n_run += 1
    assert n_run >= len(X.PASSES[kind])


def _device_reproject(r, prev, W, H, n, d, hist, params):
    ins = [dev(d["color"]), dev(d["moments"]), dev(d["guide"])] + ([None] * 4 if hist is None else [dev(a) for a in hist])
    outs = [torch.full((H, W, k), -7.0, dtype=torch.float32, device="cuda") for k in (4, 2, 1, 1)]
    torch.cuda.synchronize()
    im = ptamd.ReprojectImages(*[None if t is None else t.data_ptr() for t in ins + outs])
    r.reproject(CUR, prev, W, H, n, im, params)
    r.synchronize()
    got = [o.cpu().numpy() for o in outs]
    want_in = [d["color"], d["moments"], d["guide"]] + ([None] * 4 if hist is None else list(hist))
    for t, a in zip(ins, want_in):
        if t is not None:
            same(t.cpu().numpy().reshape(-1), a, "an input image after the call")
    return got[0], got[1], got[2][..., 0], got[3][..., 0]


@pytest.mark.parametrize("cam", list(CAMERAS))
@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_reproject_kernel(kind, W, H, cam):
    r = ptamd.Renderer(0)
    prev = CAMERAS[cam][0]
    for seed in X.seeds(kind, W, H):
        for plane in (X.planes(kind) if cam == "orbit2" else ("all",)):
            d = X.images(kind, W, H, seed, plane, X.cam_key(CUR, prev))
            for hist in (X.history(d), None):
                for params in (REPROJECT_PARAMS if hist is not None and cam == "orbit2" else (None,)):
                    got = _device_reproject(r, prev, W, H, 2, d, hist, params)
                    host = ptamd.reproject_host(CUR, prev, W, H, 2, d["color"], d["moments"], d["guide"], hist, params)
                    *ref, _ = T.reproject(CUR, prev, W, H, 2, d["color"], d["moments"], d["guide"], hist,
                                          T.DEFAULTS if params is None else params)
                    assert (W, H) in X.TINY or X.enough(*ref)
                    for g, h_, f_, what in zip(got, host, ref, ("colour", "moments", "length", "variance")):
                        _both(g, h_, f_, f"{kind} {cam} {W}x{H} seed {seed} {plane} {params} "
                                         f"{'no ' if hist is None else ''}history: {what}")


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_spatial_var_kernel(kind, W, H):
    r = ptamd.Renderer(0)
    keys = ("moments", "length", "variance", "guide")
    for seed in X.seeds(kind, W, H):
        for plane in X.planes(kind):
            d = X.images(kind, W, H, seed, plane)
            ins = [dev(d[k]) for k in keys]
            for params in SPATIAL_PARAMS:                      # radii 1, 2 and 3
                out = torch.full((H, W), -7.0, dtype=torch.float32, device="cuda")
                torch.cuda.synchronize()
                r.spatial_variance(*[t.data_ptr() for t in ins], W, H, out.data_ptr(), params)
                r.synchronize()
                ref = S.spatial_variance(*[d[k] for k in keys], W, H, params)
                assert (W, H) in X.TINY or X.enough(ref)
                _both(out.cpu().numpy(), ptamd.spatial_variance_host(*[d[k] for k in keys], W, H, params), ref,
                      f"{kind} {W}x{H} seed {seed} {plane} {params}")
            for t, k in zip(ins, keys):
                same(t.cpu().numpy().reshape(-1), d[k], f"input {k} after the calls")


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_adaptive_select_kernel(kind, W, H):
    r = ptamd.Renderer(0)
    bx, by = A.tiles(W, H)
    for seed in X.seeds(kind, W, H):
        d = X.images(kind, W, H, seed, "moments" if kind == "nonfinite" else "all")
        counts = adaptive_counts(W, H, seed)
        dm = dev(d["moments"])
        dn = torch.from_numpy(counts.view(np.int32).copy()).cuda()
        dnext = torch.full((bx * by,), -1, dtype=torch.int32, device="cuda")
        derr = torch.full((bx * by,), -1.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        r.adaptive_select(dm.data_ptr(), dn.data_ptr(), W, H, dnext.data_ptr(), derr.data_ptr(), ADAPTIVE_PARAMS)
        r.synchronize()
        host_n, host_e = ptamd.adaptive_select_host(d["moments"], counts, W, H, ADAPTIVE_PARAMS)
        ref_n, ref_e = A.select(d["moments"], counts, W, H, ADAPTIVE_PARAMS)
        got_n = dnext.cpu().numpy().view(np.uint32)
        assert np.array_equal(got_n, host_n) and np.array_equal(got_n, ref_n), (kind, W, H, seed)
        got_e = derr.cpu().numpy()
        assert not np.isnan(got_e).any()
        same(got_e, host_e, f"{kind} {W}x{H} seed {seed}: E_T against host")
        same(got_e, ref_e, f"{kind} {W}x{H} seed {seed}: E_T against the restatement")
        same(dm.cpu().numpy().reshape(-1), d["moments"], "the moments after the call")


# ---- a frame the renderer itself makes non-finite, through the whole chain ---------------------
HOSTILE_CAM = scenes.camera((0.5, 1.5, 3.5))
PATHS = {"recursive, 1 lane": [(ptamd.PT_OPT_KERNEL, 1), (ptamd.PT_OPT_SAMPLE_LANES, 1)],
         "recursive, 4 lanes": [(ptamd.PT_OPT_KERNEL, 1), (ptamd.PT_OPT_SAMPLE_LANES, 4)],
         "wavefront": [(ptamd.PT_OPT_KERNEL, 3)]}


def _hostile_lights():
    """test_gpu_parity.test_shadow_skip_light_intensities's: the reference light, a negative and an infinite one."""
    return np.concatenate([scenes.REFERENCE_LIGHT,
                           ptamd.pack_light([2.5, 0.5, 0.0], [-1, 0, 0], [-3.0, 0.5, 2.0], [1.0, 1.0]),
                           ptamd.pack_light([-2.5, 0.0, 0.5], [1, 0, 0], [np.inf, 1.0, 0.25], [0.5, 0.5])])


@pytest.mark.parametrize("path", list(PATHS))
def test_a_rendered_frame_with_nan_inf_and_negative_radiance(path):
    W, H, n = 40, 32, 3
    box, lights = scene("box"), _hostile_lights()
    r = renderer(box, HOSTILE_CAM, lights, size=(W, H), options=PATHS[path] + MOMENTS)
    oracle = lambda first, nb: oracle_frame(box, HOSTILE_CAM, lights, W, H, first, nb)
    # the moments of lone batches against the fold of the oracle's sample colours (tests/test_gpu_moments.py)
    tiny = F(np.finfo(F).tiny)
    for b in (0, 1, 3):
        r.clear()
        r.dispatch(b)
        a = oracle(b, 1).reshape(H, W, 4)
        same_nan(r.read_accum(), a, f"{path}: accumulator of the lone batch {b}")
        with np.errstate(all="ignore"):
            c = (a[..., :3] * F(b + 1)).astype(F)
            exact = ~np.any((a[..., :3] != 0) & (np.abs(a[..., :3]) < tiny), axis=-1)     # no subnormal quotient
            want = V.fold_moments(np.zeros((H, W, 2), F), c, b)
        assert np.count_nonzero(~exact) < 0.01 * W * H
        same_nan(r.read_moments()[0][exact], want[exact], f"{path}: moments of the lone batch {b}")
    r.clear()
    r.render(0, n)
    accum = r.read_accum().reshape(H, W, 4)
    same_nan(accum, oracle(0, n), f"{path}: accumulator")
    with np.errstate(invalid="ignore"):
        assert np.isnan(accum).any() and np.isinf(accum).any() and (accum < 0).any() and np.isfinite(accum[..., :3]).any()
    moments, got_n = r.read_moments()
    assert got_n == n and not np.all(np.isfinite(moments))
    r.render_guide()
    guide = r.read_guide()
    for staged in (0, 1):
        r.set_option(ptamd.PT_OPT_DENOISE_LDS, staged)
        same_nan(r.denoise(), ptamd.denoise_host(accum, guide, W, H), f"{path}: pt_denoise, staged {staged}")
        same_nan(r.denoise_var(), ptamd.denoise_var_host(accum, moments, n, guide, W, H), f"{path}: pt_denoise_var, staged {staged}")
    for tonemap in (0, 1, 2):
        for auto in (0, 1):
            params = (tonemap, 1.5, auto, 0.18, 2.0, 1.0)
            r.display_reset()
            want, _ = ptamd.display_host(accum, W, H, params)
            assert np.array_equal(r.display(params), want), f"{path}: pt_display, operator {tonemap}, metering {auto}"
    same_nan(r.read_accum(), accum, "the accumulation image after the filters")
    # two frames of the temporal loop against the chain of plain renders and host reprojections
    plain = renderer(box, HOSTILE_CAM, lights, size=(W, H), options=PATHS[path] + MOMENTS)
    hist, prev_cam = None, None
    for k in range(2):
        cam = T.rotate_y(HOSTILE_CAM, 2.0 * k)
        plain.set_camera(cam)
        plain.set_option(ptamd.PT_OPT_SEED_BASE, k * n)
        plain.clear()
        plain.render(0, n)
        plain.render_guide()
        a, m, g = plain.read_accum().reshape(H, W, 4), plain.read_moments()[0], plain.read_guide()
        want = ptamd.reproject_host(cam, cam if prev_cam is None else prev_cam, W, H, n, a, m, g, hist)
        r.temporal_advance(cam, n)
        c, tm, tl = r.read_temporal()
        tv = read_device(r, r.temporal_ptr(3), (H, W))
        for got, w_, what in zip((c, tm, tl, tv), want, ("colour", "moments", "length", "variance")):
            same_nan(got, w_, f"{path}: temporal frame {k}, {what}")
        hist, prev_cam = (want[0], want[1], want[2], g), cam
    assert np.any(tl > n)                                              # the second frame found history
    same_nan(r.temporal_denoise(), ptamd.denoise_var_plane_host(want[0], want[3], g, W, H), f"{path}: pt_temporal_denoise")
