#!/usr/bin/env python3
"""Times the spatial variance estimate at 1920x1080 on box.obj and prints one
JSON line:

  spatial_var_kernel alone (pt_spatial_variance on device images) on a first
  frame at 1 spp (every pixel short) and on the eighth frame of an orbit in
  2 degree steps (few short first-hit pixels; a miss never finds history, so
  the background stays short), at radius 1, 2 and 3, and on images without a
  short pixel (the exit alone), beside its compulsory traffic at 8 TB/s; and
  pt_temporal_denoise_spatial beside pt_temporal_denoise on both frames.

Method (as tools/temporal_timing.py): after a warm-up, `--calls` back-to-back
calls and one synchronise, host clock around the lot; `--runs` such windows
per configuration, the configurations interleaved within a run (so drift hits
them alike), the median window reported per call.  Compulsory traffic of the
kernel per pixel: read moments 8, length 4, variance 4, guide 16; written 4:
36 B (a frame with no short pixel moves 12 of them).

  python tools/spatial_var_timing.py [--out profiles/spatial_var/timing_1080p.json]
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

W, H, SPP = 1920, 1080, 1
HBM_BYTES_PER_S = 8e12
PIXEL_BYTES = 8 + 4 + 4 + 16 + 4


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


def loop(frames):
    """A context holding the temporal result of `frames` frames at 1 spp, and
    copies of its images for the kernel alone."""
    v, i, n, _, _ = ptamd.Scene.load_obj(scenes.BOX_OBJ).build_bvh().arrays()
    r = ptamd.Renderer(0)
    r.set_option(ptamd.PT_OPT_MOMENTS, 1)
    r.upload_scene(v, i, n)
    r.upload_lights(scenes.REFERENCE_LIGHT)
    r.set_params(4, 3)
    r.resize_and_clear(W, H)
    for k in range(frames):
        r.temporal_advance(orbit(2.0 * k), SPP)
    _, m, l = r.read_temporal()
    g = r.read_guide()
    var = (np.maximum(np.float32(0), m[..., 1] - m[..., 0] * m[..., 0]) / np.maximum(l - np.float32(1), np.float32(1)))
    hit = g[..., 3] < 1e30
    dev = [torch.from_numpy(np.ascontiguousarray(a, np.float32).reshape(-1)).cuda() for a in (m, l, var, g)]
    out = torch.empty(W * H, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    tiles = (l < 2)[:H // 16 * 16, :W // 16 * 16].reshape(H // 16, 16, W // 16, 16).any(axis=(1, 3))
    stats = {"short_pixels": int(np.count_nonzero(l < 2)), "short_first_hit_pixels": int(np.count_nonzero(hit & (l < 2))),
             "first_hit_pixels": int(np.count_nonzero(hit)), "whole_tiles_with_a_short_pixel": int(np.count_nonzero(tiles)),
             "whole_tiles": int(tiles.size)}
    return r, dev, out, stats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100, help="back-to-back calls per window (at least 20)")
    ap.add_argument("--runs", type=int, default=7, help="windows per configuration; the median is reported")
    ap.add_argument("--out", default="", help="also write the JSON here")
    a = ap.parse_args()
    if a.calls < 20 or a.runs < 1:
        ap.error("--calls >= 20 and --runs >= 1")
    L = ptamd.lib()
    configs, stats, keep = {}, {}, []
    for name, frames in (("first_frame", 1), ("eighth_orbit_frame", 8)):
        r, dev, out, st = loop(frames)
        keep.append((r, dev, out))
        stats[name] = st
        for radius in (1, 2, 3):
            def kernel(r=r, dev=dev, out=out, radius=radius):
                r.spatial_variance(*[t.data_ptr() for t in dev], W, H, out.data_ptr(), (2, radius, 1.0, 1.0))
            configs[f"{name}_kernel_radius_{radius}"] = (r, kernel)
        if frames == 1:   # the exit alone: the same images with every length 8, no pixel short
            long = torch.full_like(dev[1], 8.0)
            torch.cuda.synchronize()

            def exit_only(r=r, dev=dev, out=out, long=long):
                r.spatial_variance(dev[0].data_ptr(), long.data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(), W, H,
                                   out.data_ptr(), (2, 3, 1.0, 1.0))
            configs["no_short_pixel_kernel_radius_3"] = (r, exit_only)

        def plain(r=r):
            if L.pt_temporal_denoise(r._c, None, None) != ptamd.PT_OK:
                raise ptamd.PTError(L.pt_last_error().decode())

        def spatial(r=r):
            if L.pt_temporal_denoise_spatial(r._c, None, None, None) != ptamd.PT_OK:
                raise ptamd.PTError(L.pt_last_error().decode())

        configs[f"{name}_temporal_denoise"] = (r, plain)
        configs[f"{name}_temporal_denoise_spatial"] = (r, spatial)
    samples = {k: [] for k in configs}
    for run in range(a.runs + 1):   # run 0 is the warm-up of every configuration
        for key, (r, fn) in configs.items():
            ms = window_ms(r, fn, a.calls)
            if run:
                samples[key].append(ms)
    med = {k: statistics.median(s) for k, s in samples.items()}
    floor_ms = W * H * PIXEL_BYTES / HBM_BYTES_PER_S * 1e3
    res = {"tool": "tools/spatial_var_timing.py", "scene": "box.obj", "width": W, "height": H, "spp": SPP,
           "calls": a.calls, "runs": a.runs, "frames": stats,
           "kernel_traffic_bytes_per_pixel": PIXEL_BYTES,
           "kernel_traffic_mb": round(W * H * PIXEL_BYTES / 1e6, 2),
           "kernel_floor_ms_at_8TBps": round(floor_ms, 5),
           "kernel_fraction_of_floor": {k: round(floor_ms / x, 4) for k, x in med.items() if "_kernel_" in k},
           "ms": {k: round(x, 5) for k, x in med.items()},
           "ms_spread": {k: [round(min(s), 5), round(max(s), 5)] for k, s in samples.items()},
           "spatial_minus_plain_ms": {n: round(med[f"{n}_temporal_denoise_spatial"] - med[f"{n}_temporal_denoise"], 5)
                                      for n in stats}}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    for r, _, _ in keep:
        r.close()


if __name__ == "__main__":
    main()
