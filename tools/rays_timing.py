#!/usr/bin/env python3
"""Times the batched ray queries (pt_trace_rays) on the displaced sphere of
20,480 triangles and the cloud of 10M, and prints one JSON line.

Workloads per scene, all device memory in and out:
  a  coherent closest rays: the guide rays of a 1920x1080 frame (recomputed in
     numpy from the camera; pt_guide_ray's to rounding), against pt_render_guide
     of the same frame on the same context -- the query reads 32 B and writes
     32 B a ray where the guide kernel reads nothing and writes 16 B;
  b  incoherent closest rays: families 1-3 and 5 of tests/sweep_support.py
     make_rays, 2M rays;
  c  the occlusion rays of b, their limits drawn around the hit distances
     (t * U(0.5, 1.5) for a hit, U(0, 4) for a miss).
Each under PT_OPT_RAYS_REFILL 0 and 1; Grays/s = rays / median call time.

Method (the project's): after a warm-up, `--calls` back-to-back calls and one
synchronise, host clock around the lot; `--runs` such windows per
configuration, the configurations of a scene interleaved within a run, the
median window reported per call with the windows' least and greatest.  A
configuration whose warm-up window shows a call above `--slow-ms` runs
`--slow-calls` calls a window instead (the count is recorded).

`--counts N` runs no GPU: it walks N rays of each workload through the host's
culled wide walk (tests/wide_check.cpp, the host count tools/walk_counts.py
takes, in the kernel's default variant) and reports wide-node fetches and triangle tests per
ray, every answer checked against the oracle's exhaustive walk where the
oracle can read the scene (float-encoded links: the sphere).

  python tools/rays_timing.py [--scenes sphere,cloud] [--out profiles/rays/timing.json]
  python tools/rays_timing.py --counts 20000 [--out profiles/rays/walk_counts.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "discovering-path-tracer_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import ptamd   # noqa: E402
import scenes  # noqa: E402

W, H = 1920, 1080
F32 = np.float32


def build_scene(name, threads):
    if name == "sphere":
        v, i = scenes.displaced_sphere(5)
        cam, big = scenes.camera((0.0, 0.5, 3.0)), False
    else:
        t = 10_000_000
        v, i = scenes.random_triangles(t, seed=42)
        cam, big = scenes.camera((0.0, 0.0, 2.2)), True
    s = ptamd.Scene.from_arrays(v, i).build_bvh(int_bits=big, threads=threads)
    v, i, n, _, _ = s.arrays()
    return v, i, n, cam, big


def guide_rays(cam):
    """The guide rays of the W x H frame (pt_denoise.h guide_dir), in numpy."""
    pos, d, up = cam[0:3].astype(np.float64), cam[4:7].astype(np.float64), cam[8:11].astype(np.float64)
    right = np.cross(d, -up)
    right /= np.linalg.norm(right)
    upv = np.cross(right, d)
    upv /= np.linalg.norm(upv)
    tan_fov = np.tan(np.radians(float(cam[12]) * 0.5))
    x, y = np.meshgrid(np.arange(W), np.arange(H))
    nx, ny = 2.0 * x / W - 1.0, 2.0 * y / H - 1.0
    dirs = d[None, None] - right[None, None] * (nx * tan_fov * (W / H))[..., None] - upv[None, None] * (ny * tan_fov)[..., None]
    dirs /= np.linalg.norm(dirs, axis=-1, keepdims=True)
    rays = np.zeros((W * H, 8), F32)
    rays[:, 0:3] = pos.astype(F32)
    rays[:, 3:6] = dirs.reshape(-1, 3).astype(F32)
    rays[:, 6] = F32(1e30)
    return rays


def incoherent_rays(v, i, per_family=500_000, seed=7):
    """Families 1-3 and 5 of make_rays: 4 x per_family rays."""
    from sweep_support import make_rays
    k = per_family
    rays = make_rays(v, i, 6 * k, seed)
    return np.ascontiguousarray(np.concatenate([rays[0:3 * k], rays[4 * k:5 * k]]))


def occlusion_rays(rays, t, seed=8):
    rng = np.random.default_rng(seed)
    out = rays.copy()
    hit = t < F32(1e30)
    out[:, 6] = np.where(hit, t * rng.uniform(0.5, 1.5, len(t)), rng.uniform(0.0, 4.0, len(t))).astype(F32)
    return out


def check_guide_rays(cam, rays):
    worst = 0.0
    for x, y in ((0, 0), (W // 2, H // 2), (W - 1, H - 1), (123, 987), (1500, 17)):
        o, d = ptamd.guide_ray(cam, W, H, x, y)
        worst = max(worst, float(np.abs(rays[y * W + x, 3:6] - d).max()), float(np.abs(rays[y * W + x, 0:3] - o).max()))
    return worst


def run_counts(a):
    import test_wide   # its build of tests/wide_check.cpp, the library tools/walk_counts.py counts with
    L = test_wide.lib()
    L.wide_steps.restype = ctypes.c_ulonglong
    res = {"tool": "tools/rays_timing.py --counts", "rays_per_workload": a.counts, "walk": "64-B nodes, queued leaf tests, "
           "wave-flush merge (wide_check variant 64, 2)", "scenes": {}}
    for name in a.scenes.split(","):
        v, i, n, cam, big = build_scene(name, a.threads)
        rng = np.random.default_rng(3)
        ga = guide_rays(cam)
        ga = ga[rng.choice(len(ga), a.counts, replace=False)]
        gb = incoherent_rays(v, i, per_family=max(a.counts // 4, 1))
        t = ptamd.trace_rays_host(v, i, n, gb, int_bits=big)["t"]
        gc = occlusion_rays(gb, t)
        out = {}
        for key, rays, shadow in (("a_guide", ga, 0), ("b_incoherent", gb, 0), ("c_occlusion", gc, 1)):
            r = np.zeros((len(rays), 8), F32)   # wide_check's layout: {o, d, kind, limit}
            r[:, 0:6] = rays[:, 0:6]
            r[:, 6] = shadow
            r[:, 7] = rays[:, 6] if shadow else 0
            L.wide_set_mode(1)
            L.wide_set_variant(64, 2)
            err = ctypes.create_string_buffer(256)
            scene_args = (v, v.size, i, i.size // 3, n.reshape(-1), n.size // 8, 1 if big else 0, r, len(r))
            if big:   # the oracle reads float-encoded links only: count without its check
                nodes, tris = np.zeros(len(r), np.int32), np.zeros(len(r), np.int32)
                assert L.wide_counts(*scene_args, nodes, tris, err, 256) == 0, err.value
                walked = int((nodes >= 0).sum())
                out[key] = {"rays": len(r), "handed_to_exact": len(r) - walked, "mismatches_against_oracle": None,
                            "wide_nodes_per_ray": round(float(nodes[nodes >= 0].sum()) / walked, 3),
                            "tri_tests_per_ray": round(float(tris[tris >= 0].sum()) / walked, 3)}
            else:
                ans = np.zeros(4 * len(r), F32)
                st = np.zeros(8, np.uint64)
                assert L.wide_check(*scene_args, ans, st, err, 256) == 0, err.value
                walked = len(r) - int(st[2])
                out[key] = {"rays": len(r), "handed_to_exact": int(st[2]), "mismatches_against_oracle": int(st[0] + st[1]),
                            "wide_nodes_per_ray": round(float(st[3]) / walked, 3),
                            "tri_tests_per_ray": round(float(st[4]) / walked, 3),
                            "steps_per_ray": round(L.wide_steps() / walked, 3)}
            print(name, key, out[key], flush=True)
        res["scenes"][name] = {"triangles": int(i.size // 3), **out}
    return res


def run_timing(a):
    import torch
    L = ptamd.lib()
    res = {"tool": "tools/rays_timing.py", "calls": a.calls, "runs": a.runs, "slow_ms": a.slow_ms,
           "slow_calls": a.slow_calls, "frame": [W, H], "bytes_per_ray": {"closest": 64, "occlusion": 36, "guide": 16},
           "scenes": {}}
    for name in a.scenes.split(","):
        t0 = time.perf_counter()
        v, i, n, cam, big = build_scene(name, a.threads)
        r = ptamd.Renderer(0)
        r.upload_scene(v, i, n, int_bits=big)
        r.upload_lights(scenes.REFERENCE_LIGHT)
        r.set_camera(cam)
        r.resize_and_clear(W, H)
        info = r.wide_info()
        ga = guide_rays(cam)
        gb = incoherent_rays(v, i)
        hits_b = r.trace_rays(gb)
        gc = occlusion_rays(gb, hits_b["t"])
        dev = {k: torch.from_numpy(x).cuda() for k, x in (("a", ga), ("b", gb), ("c", gc))}
        out_hit = torch.empty((max(len(ga), len(gb)), 8), dtype=torch.float32, device="cuda")
        out_any = torch.empty((len(gc),), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        setup_s = time.perf_counter() - t0

        def query(key, kind, refill):
            rp, m = dev[key].data_ptr(), dev[key].shape[0]
            op = out_any.data_ptr() if kind else out_hit.data_ptr()

            def call():
                if L.pt_trace_rays(r._c, kind, rp, m, op) != ptamd.PT_OK:
                    raise ptamd.PTError(L.pt_last_error().decode())
            return call, refill, m

        def guide():
            if L.pt_render_guide(r._c) != ptamd.PT_OK:
                raise ptamd.PTError(L.pt_last_error().decode())

        configs = {"guide": (guide, None, W * H)}
        for refill in (0, 1):
            configs[f"a_guide_rays_refill{refill}"] = query("a", 0, refill)
            configs[f"b_incoherent_refill{refill}"] = query("b", 0, refill)
            configs[f"c_occlusion_refill{refill}"] = query("c", 1, refill)

        def window(key, calls):
            fn, refill, _ = configs[key]
            if refill is not None:
                r.set_option(ptamd.PT_OPT_RAYS_REFILL, refill)
            r.synchronize()
            t = time.perf_counter()
            for _ in range(calls):
                fn()
            r.synchronize()
            return (time.perf_counter() - t) * 1e3 / calls

        calls = {}
        for key in configs:   # the warm-up, which also sizes the windows
            calls[key] = a.slow_calls if window(key, 3) > a.slow_ms else a.calls
        samples = {key: [] for key in configs}
        for _ in range(a.runs):
            for key in configs:
                samples[key].append(window(key, calls[key]))
        # the refill shapes answer alike (and the guide's t is the query's on the guide rays, to the rays' rounding)
        same = {}
        for key, kind in (("a", 0), ("b", 0), ("c", 1)):
            got = []
            for refill in (0, 1):
                r.set_option(ptamd.PT_OPT_RAYS_REFILL, refill)
                configs[f"{'a_guide_rays' if key == 'a' else 'b_incoherent' if key == 'b' else 'c_occlusion'}_refill{refill}"][0]()
                r.synchronize()
                got.append((out_any if kind else out_hit[:dev[key].shape[0]]).cpu().numpy().tobytes())
            same[key] = got[0] == got[1]
        sc = {"triangles": int(i.size // 3), "wide_nodes": int(info[0]), "setup_s": round(setup_s, 1),
              "guide_rays_max_abs_difference_from_pt_guide_ray": check_guide_rays(cam, ga),
              "hits_b": int((hits_b["tri"] >= 0).sum()), "occluded_c": int(out_any.sum().item()),
              "refill_shapes_same_bytes": same, "workloads": {}}
        for key, (_, _, m) in configs.items():
            med = statistics.median(samples[key])
            sc["workloads"][key] = {"rays": m, "calls_per_window": calls[key], "ms": round(med, 5),
                                    "ms_spread": [round(min(samples[key]), 5), round(max(samples[key]), 5)],
                                    "grays_per_s": round(m / med / 1e6, 4)}
        wl = sc["workloads"]
        sc["query_over_guide"] = {f"refill{k}": round(wl[f"a_guide_rays_refill{k}"]["ms"] / wl["guide"]["ms"], 3) for k in (0, 1)}
        sc["refill1_over_refill0"] = {k: round(wl[f"{k}_refill1"]["ms"] / wl[f"{k}_refill0"]["ms"], 4)
                                      for k in ("a_guide_rays", "b_incoherent", "c_occlusion")}
        res["scenes"][name] = sc
        print(name, json.dumps(sc), flush=True)
        r.close()
        del dev, out_hit, out_any
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="sphere,cloud")
    ap.add_argument("--calls", type=int, default=200, help="back-to-back calls per window")
    ap.add_argument("--runs", type=int, default=7, help="windows per configuration; the median is reported")
    ap.add_argument("--slow-ms", type=float, default=5.0)
    ap.add_argument("--slow-calls", type=int, default=20)
    ap.add_argument("--threads", type=int, default=16, help="host threads of the BVH build")
    ap.add_argument("--counts", type=int, default=0, help="host node counts of this many rays per workload; no GPU")
    ap.add_argument("--out", default="", help="also write the JSON here")
    a = ap.parse_args()
    res = run_counts(a) if a.counts else run_timing(a)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
