#!/usr/bin/env python3
"""Times guide-driven upsampling to 1920x1080 from 960x540 (scale 2) and 480x270
(scale 4) on box.obj after 8 spp, and prints one JSON line:

  upsample_kernel (a pt_upsample call whose guide is kept) and
  upsample_display_kernel per operator (pt_upsample_display, metering off) in ms
  and against their compulsory traffic at 8 TB/s: the full guide read once, the
  source read once, the result written once (16 + 16 B, or 16 + 4 B, a full
  pixel and 16 B a source pixel); the fused call against pt_upsample followed
  by pt_display at the full size (a second context of that size on the same
  stream, reading the first one's upsampled image); the full-size guide render
  (pt_render_guide of a 1920x1080 context: the launch pt_upsample makes when
  its guide is stale).

Method: as tools/display_timing.py.  After a warm-up, `--calls` back-to-back
calls and one synchronise, host clock around the lot; `--runs` such windows per
configuration, the configurations interleaved within a run, the median window
reported per call with the windows' least and greatest.  A window of
back-to-back calls is a call's time on the host or the device, whichever is
longer; the kernels' own durations come from a profiler run of one
configuration (`--only`), e.g.
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- \\
      python tools/upsample_timing.py --only s2_upsample --calls 50 --runs 3

  python tools/upsample_timing.py [--out profiles/upsample/timing_1080p.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "discovering-path-tracer_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import ptamd   # noqa: E402
import scenes  # noqa: E402

W, H, SPP = 1920, 1080, 8
HBM_BYTES_PER_S = 8e12
OPERATORS = {"clamp": 0, "reinhard": 1, "aces": 2}


def window_ms(stream, fn, calls):
    stream.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    stream.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def traffic_bytes(scale, out_bytes):
    return W * H * (16 + out_bytes) + (W // scale) * (H // scale) * 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200, help="back-to-back calls per window (at least 20)")
    ap.add_argument("--runs", type=int, default=7, help="windows per configuration; the median is reported")
    ap.add_argument("--out", default="", help="also write the JSON here")
    ap.add_argument("--only", default="", help="run this one configuration (s2_upsample, s4_fused_aces, guide_full, ...): "
                    "for a rocprofv3 --kernel-trace --stats run, whose kernel times then belong to it")
    a = ap.parse_args()
    if a.calls < 20 or a.runs < 1:
        ap.error("--calls >= 20 and --runs >= 1")
    v, i, n, _, _ = ptamd.Scene.load_obj(scenes.BOX_OBJ).build_bvh().arrays()
    stream = torch.cuda.Stream()
    L = ptamd.lib()

    def context(w, h, scene=True):
        r = ptamd.Renderer(0)
        r.set_stream(stream.cuda_stream)
        if scene:
            r.upload_scene(v, i, n)
            r.upload_lights(scenes.REFERENCE_LIGHT)
            r.set_camera(scenes.DEFAULT_CAMERA)
            r.set_params(4, 3)
        r.resize_and_clear(w, h)
        return r

    def checked(rc):
        if rc != ptamd.PT_OK:
            raise ptamd.PTError(L.pt_last_error().decode())

    full = context(W, H)
    configs = {"guide_full": (lambda: checked(L.pt_render_guide(full._c)), max(a.calls // 4, 20))}
    low = {}
    for s in (2, 4):
        r = low[s] = context(W // s, H // s)
        r.render(0, SPP)
        up = ptamd.UpsampleParams(s, 0.35, 0.25)
        r.upsample(up)   # renders and keeps the guide; the library-owned image exists from here on
        src = r.upsampled_ptr()

        def upsample(r=r, up=up):
            checked(L.pt_upsample(r._c, up, None, None))
        configs[f"s{s}_upsample"] = (upsample, a.calls)
        for name, tm in OPERATORS.items():
            dp = ptamd.DisplayParams(tm, 1.0, 0, 0.18, 4.0, 1.0)

            def fused(r=r, up=up, dp=dp):
                checked(L.pt_upsample_display(r._c, up, dp, None, None))

            def unfused(r=r, up=up, dp=dp, src=src):
                checked(L.pt_upsample(r._c, up, None, None))
                checked(L.pt_display(full._c, dp, src, None))
            configs[f"s{s}_fused_{name}"] = (fused, a.calls)
            configs[f"s{s}_unfused_{name}"] = (unfused, a.calls)
    if a.only:
        fn, calls = configs[a.only]
        for _ in range(a.runs + 1):
            window_ms(stream, fn, calls)
        return
    samples = {key: [] for key in configs}
    for run in range(a.runs + 1):   # run 0 is the warm-up of every configuration
        for key, (fn, calls) in configs.items():
            ms = window_ms(stream, fn, calls)
            if run:
                samples[key].append(ms)
    med = {key: statistics.median(s) for key, s in samples.items()}
    spread = {key: [round(min(s), 5), round(max(s), 5)] for key, s in samples.items()}
    res = {"tool": "tools/upsample_timing.py", "calls": a.calls, "runs": a.runs, "scene": "box.obj", "width": W,
           "height": H, "spp": SPP,
           "guide_full": {"ms": round(med["guide_full"], 5), "ms_spread": spread["guide_full"],
                          "grays_per_s": round(W * H / med["guide_full"] / 1e6, 3)}}
    for s in (2, 4):
        row = {"source": [W // s, H // s]}
        for key, out_bytes in [("upsample", 16)] + [(f"fused_{name}", 4) for name in OPERATORS]:
            k = f"s{s}_{key}"
            floor_ms = traffic_bytes(s, out_bytes) / HBM_BYTES_PER_S * 1e3
            row[key] = {"ms": round(med[k], 5), "ms_spread": spread[k], "traffic_mb": round(traffic_bytes(s, out_bytes) / 1e6, 2),
                        "floor_ms_at_8TBps": round(floor_ms, 5), "fraction_of_floor": round(floor_ms / med[k], 4)}
        for name in OPERATORS:
            k = f"s{s}_unfused_{name}"
            row[f"unfused_{name}"] = {"ms": round(med[k], 5), "ms_spread": spread[k],
                                      "fused_over_unfused": round(med[f"s{s}_fused_{name}"] / med[k], 4)}
        res[f"scale_{s}"] = row
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
