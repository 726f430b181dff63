#!/usr/bin/env python3
"""Times temporal reprojection at 1920x1080 on box.obj and prints one JSON line:

  reproject_kernel alone (pt_reproject on device images, with history), beside
  its compulsory traffic at 8 TB/s; pt_temporal_advance at 2 spp against
  pt_clear_accum + pt_render(0, 2) with moments, and against that plus
  pt_render_guide; and pt_temporal_denoise beside pt_denoise_var.

Method (as tools/denoise_timing.py): after a warm-up, `--calls` back-to-back
calls and one synchronise, host clock around the lot; `--runs` such windows
per configuration, the configurations interleaved within a run (so drift hits
them alike), the median window reported per call.  Compulsory traffic of the
kernel per pixel: read colour 16, moments 8, guide 16, the history's colour 16,
moments 8, length 4, guide 16 (every history pixel is read about once); written
colour 16, moments 8, length 4, variance 4: 116 B.

  python tools/temporal_timing.py [--out profiles/temporal/timing_1080p.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch   # before libptamd.so, so that both bind to one HIP runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "discovering-path-tracer_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import ptamd   # noqa: E402
import scenes  # noqa: E402

W, H, SPP = 1920, 1080, 2
HBM_BYTES_PER_S = 8e12
PIXEL_BYTES = 16 + 8 + 16 + 16 + 8 + 4 + 16 + 16 + 8 + 4 + 4


def window_ms(r, fn, calls):
    r.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    r.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def orbit(degrees):
    a = np.deg2rad(degrees)
    return scenes.camera((5.0 * np.sin(a), 0.0, 5.0 * np.cos(a)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100, help="back-to-back calls per window (at least 20)")
    ap.add_argument("--runs", type=int, default=7, help="windows per configuration; the median is reported")
    ap.add_argument("--out", default="", help="also write the JSON here")
    a = ap.parse_args()
    if a.calls < 20 or a.runs < 1:
        ap.error("--calls >= 20 and --runs >= 1")
    v, i, n, _, _ = ptamd.Scene.load_obj(scenes.BOX_OBJ).build_bvh().arrays()
    r = ptamd.Renderer(0)
    r.set_option(ptamd.PT_OPT_MOMENTS, 1)
    r.upload_scene(v, i, n)
    r.upload_lights(scenes.REFERENCE_LIGHT)
    r.set_params(4, 3)
    r.resize_and_clear(W, H)
    cams = [orbit(0.0), orbit(2.0)]
    # the kernel alone: the second frame's images against the first frame's result, all in place
    r.temporal_advance(cams[0], SPP)
    hist = [torch.empty(W * H * k, dtype=torch.float32, device="cuda") for k in (4, 2, 1, 4)]
    outs = [torch.empty(W * H * k, dtype=torch.float32, device="cuda") for k in (4, 2, 1, 1)]
    c0, m0, l0 = r.read_temporal()
    g0 = r.read_guide()
    for t, src in zip(hist, (c0, m0, l0, g0)):
        t.copy_(torch.from_numpy(np.ascontiguousarray(src).reshape(-1)))
    torch.cuda.synchronize()
    r.set_camera(cams[1])
    r.clear()
    r.render(0, SPP)
    r.render_guide()
    im = ptamd.ReprojectImages(r.accum_ptr(), r.moments_ptr(), r.guide_ptr(), *[t.data_ptr() for t in hist],
                               *[t.data_ptr() for t in outs])
    step = [0]

    def advance():
        step[0] += 1
        r.temporal_advance(cams[step[0] & 1], SPP)

    def render_only():
        r.clear()
        r.render(0, SPP)

    def render_and_guide():
        step[0] += 1
        r.set_camera(cams[step[0] & 1])
        r.clear()
        r.render(0, SPP)
        r.render_guide()

    L = ptamd.lib()

    def temporal_denoise():
        if L.pt_temporal_denoise(r._c, None, None) != ptamd.PT_OK:
            raise ptamd.PTError(L.pt_last_error().decode())

    def denoise_var():
        if L.pt_denoise_var(r._c, None, None) != ptamd.PT_OK:
            raise ptamd.PTError(L.pt_last_error().decode())

    configs = {
        "reproject_kernel": lambda: r.reproject(cams[1], cams[0], W, H, SPP, im),
        "render_2spp_moments": render_only,
        "render_2spp_moments_and_guide": render_and_guide,
        "temporal_advance_2spp": advance,
        "temporal_denoise": temporal_denoise,
        "denoise_var": denoise_var,
    }
    samples = {k: [] for k in configs}
    for run in range(a.runs + 1):   # run 0 is the warm-up of every configuration
        for key, fn in configs.items():
            if key in ("temporal_denoise", "denoise_var"):
                r.temporal_advance(cams[0], SPP)   # a temporal result, valid moments and the guide for both filters
            ms = window_ms(r, fn, a.calls)
            if run:
                samples[key].append(ms)
    med = {k: statistics.median(s) for k, s in samples.items()}
    floor_ms = W * H * PIXEL_BYTES / HBM_BYTES_PER_S * 1e3
    res = {"tool": "tools/temporal_timing.py", "scene": "box.obj", "width": W, "height": H, "spp": SPP,
           "calls": a.calls, "runs": a.runs,
           "reproject_traffic_bytes_per_pixel": PIXEL_BYTES,
           "reproject_traffic_mb": round(W * H * PIXEL_BYTES / 1e6, 2),
           "reproject_floor_ms_at_8TBps": round(floor_ms, 5),
           "reproject_fraction_of_floor": round(floor_ms / med["reproject_kernel"], 4),
           "ms": {k: round(x, 5) for k, x in med.items()},
           "ms_spread": {k: [round(min(s), 5), round(max(s), 5)] for k, s in samples.items()},
           "advance_minus_render_ms": round(med["temporal_advance_2spp"] - med["render_2spp_moments"], 5),
           "advance_minus_render_and_guide_ms": round(med["temporal_advance_2spp"] - med["render_2spp_moments_and_guide"], 5)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    r.close()


if __name__ == "__main__":
    main()
