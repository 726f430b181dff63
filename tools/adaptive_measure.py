"""What adaptive sampling buys on the box at 1080p: adaptive renders whose threshold is
bisected until they spend the samples of uniform 8, 16 and 32 spp, against uniform renders, both judged by the
mean squared rgb error over lit pixels against 1024 spp at another seed base; wall times (host clock around
work that ends in a synchronise, median of 7); the fixed cost of a round whose list is empty.

  python tools/adaptive_measure.py [out.json]      (default profiles/adaptive/adaptive_1080p.json)"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "discovering-path-tracer_amd"), os.path.join(ROOT, "tests")]
import numpy as np
import ptamd, scenes
from support import mse, renderer, scene

W, H = 1920, 1080
r = renderer(scene("box"), scenes.DEFAULT_CAMERA, size=(W, H), options=[(ptamd.PT_OPT_MOMENTS, 1)])

def uniform(n):
    r.clear(); r.render(0, n); r.synchronize()
    return r.read_accum().reshape(H, W, 4).copy()

def timed(fn, reps=7):
    ts = []
    for _ in range(reps):
        r.synchronize(); t0 = time.perf_counter(); fn(); r.synchronize(); ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(min(ts)), float(max(ts))

def adaptive(params):
    r.adaptive_begin(params); r.adaptive_advance(10000)

# the truth: 1024 samples at another seed base, so that it shares no sample with what it judges
r.set_option(ptamd.PT_OPT_SEED_BASE, 1 << 20)
truth = uniform(1024)
r.set_option(ptamd.PT_OPT_SEED_BASE, 0)
lit = np.any(truth[..., :3] != 0, axis=-1)
out = {"frame": [W, H], "truth_spp": 1024, "truth_seed_base": 1 << 20, "lit_pixels": int(lit.sum()), "rows": []}
print("lit", int(lit.sum()), "of", W * H, flush=True)
# uniform renders at several counts: the error and the wall time
for n in (8, 16, 32, 64, 96, 128, 192):
    img = uniform(n)
    t = timed(lambda: (r.clear(), r.render(0, n)))
    row = {"uniform_spp": n, "mse": mse(img, truth, lit), "ms_median_min_max": t}
    out.setdefault("uniform", []).append(row)
    print(json.dumps(row), flush=True)
FINE = {8: (2, 64, 2), 16: (4, 128, 4), 32: (8, 256, 8)}         # 31 rounds
COARSE = {8: (2, 64, 16), 16: (4, 128, 31), 32: (8, 256, 62)}    # 4 rounds
for floor in (0.01, 0.5, 2.0, 8.0, 1e6):   # 1e6: the mean never reaches it, an absolute criterion
  for sname, SCHED in (("fine", FINE), ("coarse", COARSE)):
    for T, (lo, hi, step) in SCHED.items():
        target = T * W * H
        a, b = (1e-3, 1e3) if floor < 1e5 else (1e-9, 1e-3)   # bisection on log(threshold): samples fall as it rises
        best = None
        for _ in range(18):
            thr = float(np.sqrt(a * b))
            adaptive((lo, hi, step, thr, floor))
            s = r.adaptive_info()[2]
            if best is None or abs(s - target) < abs(best[1] - target):
                best = (thr, s)
            if s > target: a = thr
            else: b = thr
        thr, s = best
        P = (lo, hi, step, thr, floor)
        adaptive(P)
        rounds, _, s = r.adaptive_info()
        img = r.read_accum().reshape(H, W, 4).copy()
        counts, _ = r.adaptive_counts()
        t_ad = timed(lambda: adaptive(P))
        row = {"target_spp": T, "schedule": sname, "params": list(P), "samples": int(s), "samples_over_target": s / target,
               "rounds": rounds, "mse_adaptive": mse(img, truth, lit), "ms_adaptive_median_min_max": t_ad,
               "mean_count_live_tiles": float(counts[counts > lo].mean()) if np.any(counts > lo) else float(lo),
               "tiles_at_min": int(np.sum(counts == lo)), "tiles_at_max": int(np.sum(counts == hi)), "tiles": int(counts.size)}
        out["rows"].append(row)
        print(json.dumps(row), flush=True)
# the fixed cost of a round: every tile converges at once (a huge threshold), so each round is the rule,
# the list and a launch whose every workgroup leaves at once
P = (2, 402, 1, 1e30, 0.01)
r.adaptive_begin(P); r.synchronize()
ts = []
for _ in range(5):
    r.adaptive_begin(P); r.synchronize()
    t0 = time.perf_counter(); r.adaptive_advance(200); r.synchronize(); ts.append((time.perf_counter() - t0) * 1e3 / 200)
out["empty_round_ms_median_min_max"] = [float(np.median(ts)), float(min(ts)), float(max(ts))]
assert r.adaptive_info()[0] == 200 and int(r.adaptive_counts()[0].max()) == 2
print("empty round ms", out["empty_round_ms_median_min_max"], flush=True)
json.dump(out, open(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "adaptive", "adaptive_1080p.json"), "w"), indent=1)
