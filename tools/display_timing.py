#!/usr/bin/env python3
"""Times the display transform at 1920x1080 on box.obj after 8 spp, and prints
one JSON line:

  display_kernel per operator (a pt_display call without metering) in ms and as
  a fraction of its compulsory traffic at 8 TB/s (16 B read and 4 B written a
  pixel); the two metering kernels together (a metering call less the same call
  without); pt_display_readback_begin + end against pt_readback_begin + end of
  the float path, in ms and as a ratio.

Method: after a warm-up, `--calls` back-to-back calls and one synchronise, host
clock around the lot; `--runs` such windows per configuration, the
configurations interleaved within a run (so drift hits them alike), the median
window reported per call with the windows' least and greatest.  A readback is a
begin and its end, which waits: `--calls // 10` of them per window.

A window of back-to-back calls is a call's time on the host or the device,
whichever is longer; the kernels' own durations come from a profiler run of one
configuration (`--only`), e.g.
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- \
      python tools/display_timing.py --only aces_metered --calls 50 --runs 3

  python tools/display_timing.py [--out profiles/display/timing_1080p.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "discovering-path-tracer_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import ptamd   # noqa: E402
import scenes  # noqa: E402

W, H, SPP = 1920, 1080, 8
HBM_BYTES_PER_S = 8e12
PIXEL_BYTES = W * H * (16 + 4)
OPERATORS = {"clamp": 0, "reinhard": 1, "aces": 2}


def window_ms(r, fn, calls):
    r.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    r.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200, help="back-to-back calls per window (at least 20)")
    ap.add_argument("--runs", type=int, default=7, help="windows per configuration; the median is reported")
    ap.add_argument("--out", default="", help="also write the JSON here")
    ap.add_argument("--only", default="", help="run this one configuration (clamp, aces_metered, ...): for a "
                    "rocprofv3 --kernel-trace --stats run, whose kernel times then belong to it")
    a = ap.parse_args()
    if a.calls < 20 or a.runs < 1:
        ap.error("--calls >= 20 and --runs >= 1")
    v, i, n, _, _ = ptamd.Scene.load_obj(scenes.BOX_OBJ).build_bvh().arrays()
    r = ptamd.Renderer(0)
    r.upload_scene(v, i, n)
    r.upload_lights(scenes.REFERENCE_LIGHT)
    r.set_camera(scenes.DEFAULT_CAMERA)
    r.set_params(4, 3)
    r.resize_and_clear(W, H)
    r.render(0, SPP)
    L = ptamd.lib()
    floats = np.empty(W * H * 4, np.float32)
    bytes8 = np.empty(W * H * 4, np.uint8)

    def display(tonemap, auto):
        p = ptamd.DisplayParams(tonemap, 1.0, auto, 0.18, 4.0, 1.0)

        def call():
            if L.pt_display(r._c, p, None, None) != ptamd.PT_OK:
                raise ptamd.PTError(L.pt_last_error().decode())
        return call

    def readback8():
        t = r.display_readback_begin()
        ptamd._check(L.pt_display_readback_end(r._c, t, bytes8.ctypes.data, bytes8.size), "pt_display_readback_end")

    def readback32():
        t = r.readback_begin()
        ptamd._check(L.pt_readback_end(r._c, t, floats.ctypes.data, floats.size), "pt_readback_end")

    configs = {}
    for name, tm in OPERATORS.items():
        configs[name] = (display(tm, 0), a.calls)
        configs[f"{name}_metered"] = (display(tm, 1), a.calls)
    configs["readback_rgba8"] = (readback8, max(a.calls // 10, 5))
    configs["readback_float"] = (readback32, max(a.calls // 10, 5))
    if a.only:
        fn, calls = configs[a.only]
        for _ in range(a.runs + 1):
            window_ms(r, fn, calls)
        r.close()
        return
    samples = {key: [] for key in configs}
    for run in range(a.runs + 1):   # run 0 is the warm-up of every configuration
        for key, (fn, calls) in configs.items():
            ms = window_ms(r, fn, calls)
            if run:
                samples[key].append(ms)
    med = {key: statistics.median(s) for key, s in samples.items()}
    spread = {key: [round(min(s), 5), round(max(s), 5)] for key, s in samples.items()}
    floor_ms = PIXEL_BYTES / HBM_BYTES_PER_S * 1e3
    res = {"tool": "tools/display_timing.py", "calls": a.calls, "runs": a.runs, "scene": "box.obj", "width": W,
           "height": H, "spp": SPP, "traffic_mb": round(PIXEL_BYTES / 1e6, 2), "floor_ms_at_8TBps": round(floor_ms, 5),
           "display_kernel": {}, "metering_kernels": {}}
    for key in configs:
        if key.startswith("readback"):
            continue
        if "_metered" in key:
            plain = key.replace("_metered", "")
            res["metering_kernels"][plain] = {"ms": round(med[key] - med[plain], 5), "metered_call_ms": round(med[key], 5),
                                              "metered_call_ms_spread": spread[key]}
        else:
            res["display_kernel"][key] = {"ms": round(med[key], 5), "ms_spread": spread[key],
                                          "fraction_of_floor": round(floor_ms / med[key], 4)}
    res["readback"] = {"rgba8_begin_end_ms": round(med["readback_rgba8"], 5), "rgba8_ms_spread": spread["readback_rgba8"],
                       "float_begin_end_ms": round(med["readback_float"], 5), "float_ms_spread": spread["readback_float"],
                       "float_over_rgba8": round(med["readback_float"] / med["readback_rgba8"], 3),
                       "bytes_rgba8": W * H * 4, "bytes_float": W * H * 16}
    r.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
