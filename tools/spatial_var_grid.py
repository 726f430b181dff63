#!/usr/bin/env python3
"""The search behind pt_spatial_var_default_params, and the
quality table beside it.

Frames: box.obj from the default camera and tests/scenes.py's
displaced_sphere(3) from (3, 2, 4), 96x96, run through the temporal loop
(pt_temporal_advance) on the GPU at seed base 1000; per scene five cases: the
first frame at 1 spp, a second frame 60 degrees on at 1 and at 2 spp, and the
eighth frame of an orbit in 2 degree steps at 1 and at 2 spp.  The grid runs on
the host (pt_spatial_variance_host, then pt_denoise_var_plane_host at its
defaults: the kernels' bits) over below x radius x sigma_normal x sigma_depth;
a point's score is the sum over the ten frames of (filtered MSE / temporal
MSE), rgb over the first-hit pixels against a 256-spp frame of the same view
rendered at another seed base.  A point is "steady" when none of the four
orbit frames -- the state a running loop is in -- comes out worse than
pt_temporal_denoise leaves it; the library's defaults are the best steady
point.  Prints one JSON line: the table (the temporal colour,
pt_temporal_denoise, the estimate at radius 1, 2, 3 and at the library's
defaults), the best points, the best steady points and the score of the
library's defaults.

  python tools/spatial_var_grid.py [--out profiles/spatial_var/grid.json]
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
SEED_BASE, REF_SEED_BASE, REF_SPP = 1000, 1000 + (1 << 20), 256
BELOW = (2, 3, 4, 8)
RADIUS = (1, 2, 3)
SIGMA_NORMAL = (0.25, 0.5, 1.0)
SIGMA_DEPTH = (0.25, 0.5, 1.0)
F = np.float32


def mse(a, b, mask):
    d = a[..., :3].astype(np.float64)[mask] - b[..., :3].astype(np.float64)[mask]
    return float(np.mean(d * d))


def orbit(start, degrees):
    x, y, z = start
    a = np.deg2rad(degrees)
    return scenes.camera((x * np.cos(a) + z * np.sin(a), y, z * np.cos(a) - x * np.sin(a)))


def renderer(arrays, moments, seed_base):
    r = ptamd.Renderer(0)
    r.set_option(ptamd.PT_OPT_MOMENTS, moments)
    r.set_option(ptamd.PT_OPT_SEED_BASE, seed_base)
    r.upload_scene(*arrays)
    r.upload_lights(scenes.REFERENCE_LIGHT)
    r.set_params(4, 3)
    r.set_camera(scenes.DEFAULT_CAMERA)
    r.resize_and_clear(W, H)
    return r


def frames_of(name, scene, start):
    v, i, n, _, _ = scene.build_bvh().arrays()
    r, q = renderer((v, i, n), 1, SEED_BASE), renderer((v, i, n), 0, REF_SEED_BASE)
    refs = {}

    def capture(case, degrees, spp):
        if degrees not in refs:
            q.set_camera(orbit(start, degrees))
            q.render(0, REF_SPP)
            refs[degrees] = q.read_accum().reshape(H, W, 4).copy()
        c, m, l = r.read_temporal()
        guide = r.read_guide()
        var = (np.maximum(F(0), m[..., 1] - m[..., 0] * m[..., 0]) / np.maximum(l - F(1), F(1))).astype(F)   # out_var
        hit = guide[..., 3] < 1e30
        f = {"name": f"{name}, {case}, {spp} spp", "c": c, "m": m, "l": l, "v": var, "guide": guide, "hit": hit,
             "ref": refs[degrees], "short": int(np.count_nonzero(hit & (l < 2))), "first_hit": int(np.count_nonzero(hit)),
             "cache": {}}
        f["temporal_mse"] = mse(c, f["ref"], hit)
        f["plain_mse"] = mse(ptamd.denoise_var_plane_host(c, var, guide, W, H), f["ref"], hit)
        return f

    out = []
    r.temporal_advance(orbit(start, 0), 1)
    out.append(capture("first frame", 0, 1))
    for spp in (1, 2):
        r.temporal_reset()
        r.temporal_advance(orbit(start, 0), spp)
        r.temporal_advance(orbit(start, 60), spp)
        out.append(capture("60 degree jump", 60, spp))
    for spp in (1, 2):
        r.temporal_reset()
        for k in range(8):
            r.temporal_advance(orbit(start, 2 * k), spp)
        out.append(capture("eighth orbit frame", 14, spp))
    r.close()
    q.close()
    return out


def filtered_mse(f, params):
    """MSE of the filter fed with the estimate at params; frames whose plane
    comes out the same (no pixel below the threshold, say) are filtered once."""
    plane = ptamd.spatial_variance_host(f["m"], f["l"], f["v"], f["guide"], W, H, params)
    key = plane.tobytes()
    if key not in f["cache"]:
        f["cache"][key] = mse(ptamd.denoise_var_plane_host(f["c"], plane, f["guide"], W, H), f["ref"], f["hit"])
    return f["cache"][key]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="", help="also write the JSON here")
    a = ap.parse_args()
    sv, si = scenes.displaced_sphere(subdiv=3)
    frames = frames_of("box.obj", ptamd.Scene.load_obj(scenes.BOX_OBJ), (0.0, 0.0, 5.0))
    frames += frames_of("displaced_sphere(3) from (3,2,4)", ptamd.Scene.from_arrays(sv, si), (3.0, 2.0, 4.0))

    def ratios(params):
        return [filtered_mse(f, params) / f["temporal_mse"] for f in frames]

    dflt = ptamd.spatial_var_default_params()
    dflt = (dflt.below, dflt.radius, dflt.sigma_normal, dflt.sigma_depth)
    table = []
    for f in frames:
        row = {"frame": f["name"], "first_hit_pixels": f["first_hit"], "below_2": f["short"],
               "temporal_mse": f["temporal_mse"], "pt_temporal_denoise_mse": f["plain_mse"]}
        for rad in RADIUS:
            row[f"below_2_radius_{rad}_mse"] = filtered_mse(f, (2, rad, 1.0, 1.0))
        row["defaults_mse"] = filtered_mse(f, dflt)
        table.append(row)
    prs = [f["plain_mse"] / f["temporal_mse"] for f in frames]
    orbit_frames = [k for k, f in enumerate(frames) if "orbit" in f["name"]]
    grid = []
    for below, rad, sn, sz in itertools.product(BELOW, RADIUS, SIGMA_NORMAL, SIGMA_DEPTH):
        rs = ratios((below, rad, sn, sz))
        # steady: no orbit frame (the state a running loop is in) comes out worse than pt_temporal_denoise
        grid.append({"below": below, "radius": rad, "sigma_normal": sn, "sigma_depth": sz, "score": sum(rs),
                     "steady": all(rs[k] <= prs[k] for k in orbit_frames), "ratios": [round(x, 4) for x in rs]})
    grid.sort(key=lambda g: g["score"])
    drs = ratios(dflt)
    res = {"tool": "tools/spatial_var_grid.py", "width": W, "height": H, "seed_base": SEED_BASE, "ref_spp": REF_SPP,
           "ref_seed_base": REF_SEED_BASE,
           "grid": {"below": BELOW, "radius": RADIUS, "sigma_normal": SIGMA_NORMAL, "sigma_depth": SIGMA_DEPTH,
                    "points": len(grid)},
           "frames": [f["name"] for f in frames], "table": table, "best": grid[:10],
           "best_steady": [g for g in grid if g["steady"]][:10], "steady_points": sum(g["steady"] for g in grid),
           "all": grid,
           "worst_score": grid[-1]["score"],
           "pt_temporal_denoise": {"score": sum(prs), "ratios": [round(x, 4) for x in prs]},
           "defaults": {"params": dflt, "score": sum(drs), "ratios": [round(x, 4) for x in drs]}}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
