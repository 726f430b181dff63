#!/usr/bin/env python3
"""What the luminance moments and the variance-guided filter cost at
1920x1080 on box.obj, as one JSON line:

  the 8-spp frame (pt_render(0, 8)) with PT_OPT_MOMENTS 0 and 1;
  the 5-pass pt_denoise_var call, plain and LDS-staged (PT_OPT_DENOISE_LDS),
  beside the 5-pass pt_denoise call, and the passes of both.

Method: tools/denoise_timing.py's -- after a warm-up, `--calls` back-to-back
calls and one synchronise, host clock around the lot; `--runs` such windows
per configuration, interleaved within a run, the median window per call; a
k-pass call is timed for k = 1..5, pass i is t(i+1) - t(i).

  python tools/moments_timing.py [--out profiles/moments/timing_1080p.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "discovering-path-tracer_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import ptamd   # noqa: E402
import scenes  # noqa: E402

W, H, SPP, PASSES = 1920, 1080, 8, 5


def window_ms(r, fn, calls):
    r.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    r.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def renderer(moments):
    v, i, n, _, _ = ptamd.Scene.load_obj(scenes.BOX_OBJ).build_bvh().arrays()
    r = ptamd.Renderer(0)
    r.set_option(ptamd.PT_OPT_MOMENTS, moments)
    r.upload_scene(v, i, n)
    r.upload_lights(scenes.REFERENCE_LIGHT)
    r.set_camera(scenes.DEFAULT_CAMERA)
    r.set_params(4, 3)
    r.resize_and_clear(W, H)
    for _ in range(16):   # past the frames that measure the mixed-lane schedule
        r.render(0, SPP)
    r.synchronize()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    L = ptamd.lib()
    off, on = renderer(0), renderer(1)
    fd, vd = ptamd.denoise_default_params(), ptamd.denoise_var_default_params()

    def check(rc):
        if rc != ptamd.PT_OK:
            raise ptamd.PTError(L.pt_last_error().decode())

    def fixed(k):
        p = ptamd.DenoiseParams(k, fd.sigma_color, fd.sigma_normal, fd.sigma_depth)
        return lambda: check(L.pt_denoise(on._c, p, None, None))

    def var(k):
        p = ptamd.DenoiseVarParams(k, vd.sigma_lum, vd.sigma_normal, vd.sigma_depth)
        return lambda: check(L.pt_denoise_var(on._c, p, None))

    configs = {"frame_moments_off": (None, lambda: off.render(0, SPP)),
               "frame_moments_on": (None, lambda: on.render(0, SPP))}
    for staged in (0, 1):
        for k in range(1, PASSES + 1):
            tag = "lds" if staged else "plain"
            configs[f"denoise_{tag}_{k}"] = (staged, fixed(k))
            configs[f"denoise_var_{tag}_{k}"] = (staged, var(k))
    samples = {key: [] for key in configs}
    for run in range(a.runs + 1):   # run 0 warms every configuration up
        for key, (staged, fn) in configs.items():
            if staged is not None:
                on.set_option(ptamd.PT_OPT_DENOISE_LDS, staged)
            ms = window_ms(on if staged is not None or key.endswith("_on") else off, fn, a.calls)
            if run:
                samples[key].append(ms)
    med = {key: statistics.median(v) for key, v in samples.items()}
    res = {"tool": "tools/moments_timing.py", "scene": "box.obj", "width": W, "height": H, "spp": SPP,
           "calls": a.calls, "runs": a.runs}
    for key in ("frame_moments_off", "frame_moments_on"):
        res[key + "_ms"] = round(med[key], 5)
        res[key + "_ms_spread"] = [round(min(samples[key]), 5), round(max(samples[key]), 5)]
    res["frame_moments_cost"] = round(med["frame_moments_on"] / med["frame_moments_off"] - 1.0, 4)
    for name in ("denoise", "denoise_var"):
        for tag in ("plain", "lds"):
            t = [0.0] + [med[f"{name}_{tag}_{k}"] for k in range(1, PASSES + 1)]
            res[f"{name}_{tag}_pass_ms"] = [round(t[k + 1] - t[k], 5) for k in range(PASSES)]
            res[f"{name}_{tag}_{PASSES}pass_call_ms"] = round(t[PASSES], 5)
            s = samples[f"{name}_{tag}_{PASSES}"]
            res[f"{name}_{tag}_call_ms_spread"] = [round(min(s), 5), round(max(s), 5)]
    off.close()
    on.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
