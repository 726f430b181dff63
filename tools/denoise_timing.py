#!/usr/bin/env python3
"""Times the guide image and the a-trous denoiser at 1920x1080 on box.obj and
on tests/scenes.py's displaced sphere, and prints one JSON line:

  per scene: ms for the guide, ms per filter pass for the plain kernel and for
  the LDS-staged one (PT_OPT_DENOISE_LDS 1; it differs in passes 0 and 1 only),
  each pass as a fraction of its compulsory traffic at 8 TB/s, and ms for the
  whole 5-pass call of both.

Method: after a warm-up, `--calls` back-to-back calls and one synchronise,
host clock around the lot; `--runs` such windows per configuration, the
configurations interleaved within a run (so drift hits them alike), the
median window reported per call.  A k-pass call is timed for k = 1..5; pass i
is t(i+1) - t(i).  Compulsory traffic of a pass: 32 B read (colour and guide)
and 16 B written per pixel.

  python tools/denoise_timing.py [--out profiles/denoise/timing.json]
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
HBM_BYTES_PER_S = 8e12
PASS_BYTES = W * H * (32 + 16)


def window_ms(r, fn, calls):
    r.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    r.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def measure(name, scene, cam, calls, runs):
    v, i, n, _, _ = scene.build_bvh().arrays()
    r = ptamd.Renderer(0)
    r.upload_scene(v, i, n)
    r.upload_lights(scenes.REFERENCE_LIGHT)
    r.set_camera(cam)
    r.set_params(4, 3)
    r.resize_and_clear(W, H)
    r.render(0, SPP)
    dflt = ptamd.denoise_default_params()
    sig = (dflt.sigma_color, dflt.sigma_normal, dflt.sigma_depth)
    L = ptamd.lib()

    def denoise(k, staged):
        p = ptamd.DenoiseParams(k, *sig)

        def call():
            if L.pt_denoise(r._c, p, None, None) != ptamd.PT_OK:
                raise ptamd.PTError(L.pt_last_error().decode())
        return staged, call

    configs = {"guide": (None, r.render_guide)}
    for staged in (0, 1):
        for k in range(1, PASSES + 1):
            configs[f"{'lds' if staged else 'plain'}_{k}"] = denoise(k, staged)
    samples = {key: [] for key in configs}
    for run in range(runs + 1):   # run 0 is the warm-up of every configuration
        for key, (staged, fn) in configs.items():
            if staged is not None:
                r.set_option(ptamd.PT_OPT_DENOISE_LDS, staged)
            ms = window_ms(r, fn, max(calls // 4, 20) if key == "guide" else calls)
            if run:
                samples[key].append(ms)
    med = {key: statistics.median(v) for key, v in samples.items()}
    floor_ms = PASS_BYTES / HBM_BYTES_PER_S * 1e3
    out = {"scene": name, "triangles": int(i.size // 3), "width": W, "height": H, "spp": SPP,
           "guide_ms": round(med["guide"], 5), "pass_traffic_mb": round(PASS_BYTES / 1e6, 2),
           "pass_floor_ms_at_8TBps": round(floor_ms, 5)}
    for variant in ("plain", "lds"):
        t = [0.0] + [med[f"{variant}_{k}"] for k in range(1, PASSES + 1)]
        per_pass = [t[k + 1] - t[k] for k in range(PASSES)]
        out[f"{variant}_pass_ms"] = [round(x, 5) for x in per_pass]
        out[f"{variant}_pass_fraction_of_floor"] = [round(floor_ms / x, 4) if x > 0 else None for x in per_pass]
        out[f"{variant}_{PASSES}pass_call_ms"] = round(t[PASSES], 5)
        out[f"{variant}_call_ms_spread"] = [round(min(samples[f"{variant}_{PASSES}"]), 5),
                                            round(max(samples[f"{variant}_{PASSES}"]), 5)]
    r.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200, help="back-to-back calls per window (at least 20)")
    ap.add_argument("--runs", type=int, default=7, help="windows per configuration; the median is reported")
    ap.add_argument("--out", default="", help="also write the JSON here")
    a = ap.parse_args()
    if a.calls < 20 or a.runs < 1:
        ap.error("--calls >= 20 and --runs >= 1")
    sv, si = scenes.displaced_sphere()
    res = {"tool": "tools/denoise_timing.py", "calls": a.calls, "runs": a.runs, "scenes": [
        measure("box.obj", ptamd.Scene.load_obj(scenes.BOX_OBJ), scenes.DEFAULT_CAMERA, a.calls, a.runs),
        measure("displaced_sphere", ptamd.Scene.from_arrays(sv, si), scenes.camera((3, 2, 4)), a.calls, a.runs)]}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
