#!/usr/bin/env python3
"""Times the radiance queries (pt_trace_radiance) on box.obj and on the
displaced sphere of 20,480 triangles, and prints one JSON line.

Workloads per scene, all device memory in and out:
  a  the 2,073,600 camera rays of batch 0 of a 1920x1080 frame (pt_camera_rays)
     through pt_trace_radiance, against pt_render(0, 1) of the same context with
     the primary culling off and PT_OPT_FRESH_BATCH0 on: the same paths.  The
     query reads 32 B and writes 16 + 16 B a path more than the render, and
     folds; `extra_bytes_ms_at_8TBs` is what those bytes cost at 8 TB/s;
  b  a probe: the first 4096 of those rays, 256 samples each.

Method (tools/rays_timing.py's): after a warm-up, `--calls` back-to-back calls
and one synchronise, host clock around the lot; `--runs` such windows per
configuration, the configurations of a scene interleaved within a run, the
median window reported per call with the windows' least and greatest.  A
configuration whose warm-up window shows a call above `--slow-ms` runs
`--slow-calls` calls a window instead.

  python tools/radiance_timing.py [--scenes box,sphere] [--out profiles/radiance/timing.json]
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

W, H = 1920, 1080
PROBE_RAYS, PROBE_SAMPLES = 4096, 256


def build_scene(name, threads):
    if name == "box":
        s = ptamd.Scene.load_obj(scenes.BOX_OBJ).build_bvh()
        cam = scenes.DEFAULT_CAMERA
    else:
        s = ptamd.Scene.from_arrays(*scenes.displaced_sphere(5)).build_bvh(threads=threads)
        cam = scenes.camera((0.0, 0.5, 3.0))
    v, i, n, _, _ = s.arrays()
    return v, i, n, cam


def run(a):
    import torch
    L = ptamd.lib()
    res = {"tool": "tools/radiance_timing.py", "calls": a.calls, "runs": a.runs, "slow_ms": a.slow_ms,
           "slow_calls": a.slow_calls, "frame": [W, H], "extra_bytes_per_path": 64, "scenes": {}}
    for name in a.scenes.split(","):
        v, i, n, cam = build_scene(name, a.threads)
        r = ptamd.Renderer(0)
        r.set_option(ptamd.PT_OPT_PRIMARY_CULL, 0)
        r.set_option(ptamd.PT_OPT_FRESH_BATCH0, 1)
        r.upload_scene(v, i, n)
        r.upload_lights(scenes.REFERENCE_LIGHT)
        r.set_camera(cam)
        r.set_params(4, 3)
        r.resize_and_clear(W, H)
        rays = r.camera_rays(0)
        r.synchronize()
        probe = rays[:PROBE_RAYS].contiguous()
        out = torch.empty((W * H, 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()

        def query(t, samples):
            params = ptamd.RadianceParams(samples, 1)
            rp, m = t.data_ptr(), t.shape[0]

            def call():
                if L.pt_trace_radiance(r._c, params, rp, m, out.data_ptr()) != ptamd.PT_OK:
                    raise ptamd.PTError(L.pt_last_error().decode())
            return call

        def render():
            r.render(0, 1)

        configs = {"render_1spp": (render, W * H), "a_camera_rays": (query(rays, 1), W * H),
                   "b_probe": (query(probe, PROBE_SAMPLES), PROBE_RAYS * PROBE_SAMPLES)}

        def window(key, calls):
            fn = configs[key][0]
            r.synchronize()
            t = time.perf_counter()
            for _ in range(calls):
                fn()
            r.synchronize()
            return (time.perf_counter() - t) * 1e3 / calls

        calls = {key: (a.slow_calls if window(key, 3) > a.slow_ms else a.calls) for key in configs}
        samples = {key: [] for key in configs}
        for _ in range(a.runs):
            for key in configs:
                samples[key].append(window(key, calls[key]))
        # the same paths: the query's answers are the rendered frame's bits
        configs["a_camera_rays"][0]()
        render()
        r.synchronize()
        same = out.cpu().numpy().tobytes() == r.read_accum().tobytes()
        sc = {"triangles": int(i.size // 3), "kernel_of_the_render": r.last_kernel(), "wide_nodes": int(r.wide_info()[0]),
              "query_equals_frame": bool(same), "workloads": {}}
        for key, (_, m) in configs.items():
            med = statistics.median(samples[key])
            sc["workloads"][key] = {"paths": m, "calls_per_window": calls[key], "ms": round(med, 5),
                                    "ms_spread": [round(min(samples[key]), 5), round(max(samples[key]), 5)],
                                    "mpaths_per_s": round(m / med / 1e3, 2)}
        wl = sc["workloads"]
        sc["query_over_render"] = round(wl["a_camera_rays"]["ms"] / wl["render_1spp"]["ms"], 4)
        sc["query_minus_render_ms"] = round(wl["a_camera_rays"]["ms"] - wl["render_1spp"]["ms"], 5)
        sc["extra_bytes_ms_at_8TBs"] = round(W * H * 64 / 8e12 * 1e3, 5)
        res["scenes"][name] = sc
        print(name, json.dumps(sc), flush=True)
        r.close()
        del rays, probe, out
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="box,sphere")
    ap.add_argument("--calls", type=int, default=100, help="back-to-back calls per window")
    ap.add_argument("--runs", type=int, default=7, help="windows per configuration; the median is reported")
    ap.add_argument("--slow-ms", type=float, default=5.0)
    ap.add_argument("--slow-calls", type=int, default=10)
    ap.add_argument("--threads", type=int, default=16, help="host threads of the BVH build")
    ap.add_argument("--out", default="", help="also write the JSON here")
    a = ap.parse_args()
    res = run(a)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
