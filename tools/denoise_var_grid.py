#!/usr/bin/env python3
"""The search behind pt_denoise_var_default_params, and the
quality table beside it.

Frames: box.obj from the default camera and tests/scenes.py's
displaced_sphere(3) from (3, 2, 4), 96x96, rendered on the GPU with
PT_OPT_MOMENTS at 8 and at 32 spp, against a 256-spp frame of the same view.
The grid runs on the host filter (pt_denoise_var_host: the kernels' bits) over
sigma_lum x sigma_normal x sigma_depth x iterations; a point's score is the sum
over the four frames of (filtered MSE / raw MSE), rgb only.  Prints one JSON
line: the table (raw, pt_denoise at its defaults, pt_denoise_var at sigma_lum
1, 2, 4 and at the library's defaults), the best points and the score of the
library's defaults.

  python tools/denoise_var_grid.py [--out profiles/moments/grid.json]
"""
import argparse
import itertools
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "discovering-path-tracer_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import ptamd   # noqa: E402
import scenes  # noqa: E402

W = H = 96
SPPS = (8, 32)
REF_SPP = 256
SIGMA_LUM = (0.5, 0.75, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, 8.0)
SIGMA_NORMAL = (0.1, 0.2, 0.35, 0.5, 1.0)
SIGMA_DEPTH = (0.05, 0.25, 1.0)
ITERATIONS = (4, 5, 6)


def mse(a, b):
    d = a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)
    return float(np.mean(d * d))


def frames_of(name, scene, cam):
    v, i, n, _, _ = scene.build_bvh().arrays()
    r = ptamd.Renderer(0)
    r.set_option(ptamd.PT_OPT_MOMENTS, 1)
    r.upload_scene(v, i, n)
    r.upload_lights(scenes.REFERENCE_LIGHT)
    r.set_camera(cam)
    r.set_params(4, 3)
    r.resize_and_clear(W, H)
    r.render(0, REF_SPP)
    ref = r.read_accum().reshape(H, W, 4)
    r.render_guide()
    guide = r.read_guide()
    out = []
    for spp in SPPS:
        r.render(0, spp)
        raw = r.read_accum().reshape(H, W, 4)
        moments, n_s = r.read_moments()
        assert n_s == spp
        out.append({"name": f"{name}, {spp} spp", "raw": raw, "moments": moments, "n": spp, "guide": guide,
                    "ref": ref, "raw_mse": mse(raw, ref), "fixed_mse": mse(r.denoise(), ref)})
    r.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="", help="also write the JSON here")
    a = ap.parse_args()
    sv, si = scenes.displaced_sphere(subdiv=3)
    frames = frames_of("box.obj", ptamd.Scene.load_obj(scenes.BOX_OBJ), scenes.DEFAULT_CAMERA)
    frames += frames_of("displaced_sphere(3) from (3,2,4)", ptamd.Scene.from_arrays(sv, si), scenes.camera((3, 2, 4)))

    def ratios(params):
        return [mse(ptamd.denoise_var_host(f["raw"], f["moments"], f["n"], f["guide"], W, H, params), f["ref"]) /
                f["raw_mse"] for f in frames]

    dflt = ptamd.denoise_var_default_params()
    dflt = (dflt.iterations, dflt.sigma_lum, dflt.sigma_normal, dflt.sigma_depth)
    table = []
    for k, f in enumerate(frames):
        row = {"frame": f["name"], "raw_mse": f["raw_mse"], "pt_denoise_defaults_mse": f["fixed_mse"]}
        for sl in (1.0, 2.0, 4.0):
            row[f"sigma_lum_{sl:g}_mse"] = ratios((dflt[0], sl, dflt[2], dflt[3]))[k] * f["raw_mse"]
        row["pt_denoise_var_defaults_mse"] = ratios(dflt)[k] * f["raw_mse"]
        table.append(row)
    grid = []
    for it, sl, sn, sz in itertools.product(ITERATIONS, SIGMA_LUM, SIGMA_NORMAL, SIGMA_DEPTH):
        rs = ratios((it, sl, sn, sz))
        grid.append({"iterations": it, "sigma_lum": sl, "sigma_normal": sn, "sigma_depth": sz,
                     "score": sum(rs), "ratios": [round(x, 4) for x in rs]})
    grid.sort(key=lambda g: g["score"])
    # the score along sigma_lum at the other defaults
    along = [{"sigma_lum": g["sigma_lum"], "score": round(g["score"], 4), "ratios": g["ratios"]}
             for g in sorted(grid, key=lambda g: g["sigma_lum"])
             if (g["iterations"], g["sigma_normal"], g["sigma_depth"]) == (dflt[0], dflt[2], dflt[3])]
    drs = ratios(dflt)
    res = {"tool": "tools/denoise_var_grid.py", "width": W, "height": H, "spp": list(SPPS), "ref_spp": REF_SPP,
           "grid": {"sigma_lum": SIGMA_LUM, "sigma_normal": SIGMA_NORMAL, "sigma_depth": SIGMA_DEPTH,
                    "iterations": ITERATIONS, "points": len(grid)},
           "frames": [f["name"] for f in frames], "table": table, "best": grid[:10], "worst_score": grid[-1]["score"],
           "along_sigma_lum": along,
           "defaults": {"params": dflt, "score": sum(drs), "ratios": [round(x, 4) for x in drs]}}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
