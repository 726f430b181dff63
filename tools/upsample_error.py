#!/usr/bin/env python3
"""Whether rendering at half size and upsampling pays: at 1920x1080, on box.obj
and on the 20,480-triangle displaced sphere, the error over first-hit pixels
(the full guide's hit mask) against a 256-spp full-size render of

  full_8spp          the full size at 8 spp
  half_32spp_up      960x540 at 32 spp, upsampled (the same number of rays)
  half_8spp_up       960x540 at 8 spp, upsampled (a quarter of the rays)
  half_8spp_dn_up    the last with pt_denoise (default parameters) before the upsampling

and beside each the time of its steps: the render, the full-size guide, the
filter, the upsampling.  One JSON line.

The reference is rendered with another seed base (PT_OPT_SEED_BASE), so that no
candidate shares a sample with it.  Error: mean squared rgb difference in
float64 (tests/support.py mse).  Times: host clock around `--calls` back-to-back
calls and a synchronise, the median of `--runs` windows after a warm-up one; a
render window clears the frame and renders.  The guide's time is that of
pt_render_guide on the full-size context, the launch pt_upsample makes when the
camera has moved.

  python tools/upsample_error.py [--out profiles/upsample/error_1080p.json]
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

import ptamd    # noqa: E402
import scenes   # noqa: E402
import support  # noqa: E402

W, H, S = 1920, 1080, 2
REF_SPP = 256


def median_ms(r, fn, calls, runs):
    out = []
    for run in range(runs + 1):
        r.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        r.synchronize()
        if run:
            out.append((time.perf_counter() - t0) * 1e3 / calls)
    return round(statistics.median(out), 4), [round(min(out), 4), round(max(out), 4)]


def measure(name, mesh, cam, calls, runs):
    def context(w, h, seed_base=0):
        r = ptamd.Renderer(0)
        if seed_base:
            r.set_option(ptamd.PT_OPT_SEED_BASE, seed_base)
        r.upload_scene(*mesh)
        r.upload_lights(scenes.REFERENCE_LIGHT)
        r.set_camera(cam)
        r.set_params(4, 3)
        r.resize_and_clear(w, h)
        return r

    ref = context(W, H, seed_base=0x5eed)
    ref.render(0, REF_SPP)
    truth = ref.read_accum().reshape(H, W, 4)
    ref.render_guide()
    mask = ref.read_guide()[..., 3] < 1e30
    ref.close()

    full, half = context(W, H), context(W // S, H // S)

    def render(r, spp):
        def fn():
            r.resize_and_clear(r.width, r.height)
            r.render(0, spp)
        return fn

    t = {"render_full_8": median_ms(full, render(full, 8), calls, runs),
         "render_half_32": median_ms(half, render(half, 32), calls, runs),
         "render_half_8": median_ms(half, render(half, 8), calls, runs),
         "guide_full": median_ms(full, full.render_guide, calls, runs)}
    out = {"triangles": int(len(mesh[1]) // 3), "first_hit_pixels": int(mask.sum()), "rows": {}}

    render(full, 8)()
    out["rows"]["full_8spp"] = {"mse": support.mse(full.read_accum().reshape(H, W, 4), truth, mask),
                                "ms": {"render": t["render_full_8"][0]}}
    L = ptamd.lib()
    up = ptamd.UpsampleParams(S, 0.35, 0.25)
    render(half, 32)()
    image = half.upsample(up)
    t["upsample"] = median_ms(half, lambda: ptamd._check(L.pt_upsample(half._c, up, None, None), "pt_upsample"), calls, runs)
    out["rows"]["half_32spp_up"] = {"mse": support.mse(image, truth, mask),
                                    "ms": {"render": t["render_half_32"][0], "guide": t["guide_full"][0], "upsample": t["upsample"][0]}}
    render(half, 8)()
    out["rows"]["half_8spp_up"] = {"mse": support.mse(half.upsample(up), truth, mask),
                                   "ms": {"render": t["render_half_8"][0], "guide": t["guide_full"][0], "upsample": t["upsample"][0]}}
    half.denoise()   # the library-owned filtered image; its low-size guide is rendered here
    t["denoise"] = median_ms(half, lambda: ptamd._check(L.pt_denoise(half._c, None, None, None), "pt_denoise"), calls, runs)
    t["guide_half"] = median_ms(half, half.render_guide, calls, runs)
    buf = torch.zeros((H // S) * (W // S) * 4, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    dn = buf.data_ptr()
    half.denoise(None, None, dn)
    out["rows"]["half_8spp_dn_up"] = {"mse": support.mse(half.upsample(up, dn), truth, mask),
                                      "ms": {"render": t["render_half_8"][0], "guide": t["guide_full"][0],
                                             "guide_half": t["guide_half"][0], "denoise": t["denoise"][0],
                                             "upsample": t["upsample"][0]}}
    for row in out["rows"].values():
        row["mse"] = float(f"{row['mse']:.6g}")
        row["ms"]["total"] = round(sum(row["ms"].values()), 4)
        row["mse_over_full_8spp"] = round(row["mse"] / out["rows"]["full_8spp"]["mse"], 4)
    out["spreads_ms"] = {k: v[1] for k, v in t.items()}
    full.close()
    half.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20, help="back-to-back calls per window (at least 20)")
    ap.add_argument("--runs", type=int, default=5, help="windows per step; the median is reported")
    ap.add_argument("--out", default="", help="also write the JSON here")
    a = ap.parse_args()
    if a.calls < 20 or a.runs < 1:
        ap.error("--calls >= 20 and --runs >= 1")
    v, i, n, _, _ = ptamd.Scene.load_obj(scenes.BOX_OBJ).build_bvh().arrays()
    cases = {"box": ((v, i, n), scenes.DEFAULT_CAMERA),
             "sphere": (support.built(*scenes.displaced_sphere(subdiv=5)), scenes.camera((3, 2, 4)))}
    res = {"tool": "tools/upsample_error.py", "width": W, "height": H, "scale": S, "reference_spp": REF_SPP,
           "calls": a.calls, "runs": a.runs}
    for name, (mesh, cam) in cases.items():
        res[name] = measure(name, mesh, cam, a.calls, a.runs)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
