"""Adaptive rounds on the wavefront pipeline against the path-recursive rounds: the
displaced sphere of section 9's tables (displaced_sphere(5), 20,480 triangles) at 1920x1080 from (3, 2, 4).

For the default adaptive parameters and section 9d's coarse schedules (at the default threshold and floor):
the same adaptive render with PT_OPT_ADAPTIVE_WF 0 and 1 -- equal counts and equal bits of both images asserted
first, then the wall time of the whole render and of every round (a synchronise after each), the live tiles per
round, and the error against 1024 spp at another seed base.  Uniform renders on auto at several counts with
time and error, and from them the uniform render that takes the adaptive render's time.  The fixed cost of a
round whose list is empty, both ways.

Method: every shape runs once before it is timed; a host clock around work that ends in a synchronise; the
median of 7; the two configurations alternate within one run.

  python tools/adaptive_wf_measure.py [out.json]      (default profiles/adaptive_wf/adaptive_wf_1080p.json)"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "discovering-path-tracer_amd"), os.path.join(ROOT, "tests")]
import numpy as np
import ptamd, scenes
from support import built, mse, renderer

W, H = 1920, 1080
REPS = 7
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "adaptive_wf", "adaptive_wf_1080p.json")
v, i = scenes.displaced_sphere(5)
r = renderer(built(v, i), scenes.camera((3, 2, 4)), size=(W, H), options=[(ptamd.PT_OPT_MOMENTS, 1)])
out = {"scene": f"displaced_sphere(5), {i.size // 3} triangles, camera (3, 2, 4)", "frame": [W, H], "reps": REPS,
       "wide_nodes": r.wide_info()[0]}

def save():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    json.dump(out, open(OUT, "w"), indent=1)

def stat(ts):
    return [round(float(np.median(ts)), 4), round(float(min(ts)), 4), round(float(max(ts)), 4)]

def clock(fn):
    r.synchronize(); t0 = time.perf_counter(); fn(); r.synchronize()
    return (time.perf_counter() - t0) * 1e3

def uniform(n):
    r.clear(); r.render(0, n); r.synchronize()
    return r.read_accum().reshape(H, W, 4).copy()

# the truth: 1024 samples at another seed base, so that it shares no sample with what it judges
r.set_option(ptamd.PT_OPT_SEED_BASE, 1 << 20)
truth = uniform(1024)
r.set_option(ptamd.PT_OPT_SEED_BASE, 0)
lit = np.any(truth[..., :3] != 0, axis=-1)
out.update(truth_spp=1024, truth_seed_base=1 << 20, lit_pixels=int(lit.sum()))
print("lit", int(lit.sum()), "of", W * H, flush=True)

# ---- uniform renders on auto ----
out["uniform"] = []
for n in (4, 8, 16, 32, 64, 128, 256, 512, 768):
    img = uniform(n)   # also the warm-up of the shape
    kernel = r.last_kernel()
    ts = [clock(lambda: (r.clear(), r.render(0, n))) for _ in range(REPS)]
    row = {"spp": n, "kernel": kernel, "mse": mse(img, truth, lit), "ms_median_min_max": stat(ts)}
    out["uniform"].append(row)
    print(json.dumps(row), flush=True)
save()

def uniform_of_equal_time(ms):
    """(spp, mse) of the uniform render that takes `ms`, interpolated between the measured ones: the time
    linearly in spp, the error linearly in log-log."""
    u = out["uniform"]
    t = [x["ms_median_min_max"][0] for x in u]
    n = [float(x["spp"]) for x in u]
    spp = float(np.interp(ms, t, n))
    e = float(np.exp(np.interp(np.log(spp), np.log(n), np.log([x["mse"] for x in u]))))
    return round(spp, 2), e, bool(t[0] <= ms <= t[-1])

# ---- the same adaptive render, both ways ----
def adaptive(P, wf):
    r.set_option(ptamd.PT_OPT_ADAPTIVE_WF, wf)
    r.adaptive_begin(P); r.adaptive_advance(10000)

def adaptive_by_round(P, wf):
    """Wall time of every round with a synchronise after each, and the live tiles it listed."""
    r.set_option(ptamd.PT_OPT_ADAPTIVE_WF, wf)
    ts, live = [clock(lambda: r.adaptive_begin(P))], [int(len(r.adaptive_live()))]
    for _ in range(-(-(P[1] - P[0]) // P[2])):   # every round of the schedule, the empty ones at its end too
        ts.append(clock(lambda: r.adaptive_advance(1)))
        live.append(int(len(r.adaptive_live())))
    return ts, live

def result(P, wf):
    adaptive(P, wf); r.synchronize()
    counts, _ = r.adaptive_counts()
    return counts.copy(), r.read_accum().copy(), r.read_moments()[0].copy(), r.adaptive_info()

d = ptamd.adaptive_default_params()
SCHEDULES = {"default": (d.min_batches, d.max_batches, d.step), "coarse 8": (2, 64, 16), "coarse 16": (4, 128, 31),
             "coarse 32": (8, 256, 62)}
out["adaptive"] = []
for name, (lo, hi, step) in SCHEDULES.items():
    P = (lo, hi, step, d.threshold, d.lum_floor)
    c0, a0, m0, info0 = result(P, 0)   # also the warm-up of both
    c1, a1, m1, info1 = result(P, 1)
    assert np.array_equal(c0, c1), f"{name}: counts differ"
    assert np.array_equal(a0.view(np.uint32), a1.view(np.uint32)), f"{name}: accumulators differ"
    assert np.array_equal(m0.view(np.uint32), m1.view(np.uint32)), f"{name}: moments differ"
    assert info0 == info1
    total = {0: [], 1: []}
    rounds = {0: [], 1: []}
    live = None
    for _ in range(REPS):
        for wf in (0, 1):   # alternating
            total[wf].append(clock(lambda: adaptive(P, wf)))
    for _ in range(REPS):
        for wf in (0, 1):
            ts, lv = adaptive_by_round(P, wf)
            assert live is None or lv == live
            live = lv
            rounds[wf].append(ts)
    t0, t1 = stat(total[0]), stat(total[1])
    img = a1.reshape(H, W, 4)
    err = mse(img, truth, lit)
    row = {"schedule": name, "params": [lo, hi, step, float(d.threshold), float(d.lum_floor)], "equal_counts_and_bits": True,
           "rounds_done": info1[0], "samples": info1[2], "mean_spp": info1[2] / (W * H),
           "tiles": int(c1.size), "tiles_at_min": int(np.sum(c1 == lo)), "tiles_at_max": int(np.sum(c1 == hi)),
           "live_tiles_per_round": live, "mse_adaptive": err,
           "ms_total_option0_median_min_max": t0, "ms_total_option1_median_min_max": t1,
           "option1_over_option0": round(t1[0] / t0[0], 4),
           "ms_per_round_option0_median": [round(float(np.median(x)), 4) for x in zip(*rounds[0])],
           "ms_per_round_option1_median": [round(float(np.median(x)), 4) for x in zip(*rounds[1])]}
    for wf, t in ((0, t0), (1, t1)):
        spp, e, inside = uniform_of_equal_time(t[0])
        row[f"uniform_of_equal_time_option{wf}"] = {"spp": spp, "mse": e, "within_measured_range": inside,
                                                    "adaptive_mse_over_uniform_mse": err / e}
    out["adaptive"].append(row)
    print(json.dumps(row), flush=True)
    save()

# ---- the fixed cost of a round whose list is empty: every tile converges at once (a huge threshold) ----
P = (2, 402, 1, 1e30, 0.01)
for wf in (0, 1):
    r.set_option(ptamd.PT_OPT_ADAPTIVE_WF, wf)
    r.adaptive_begin(P); r.adaptive_advance(200); r.synchronize()
empty = {0: [], 1: []}
for _ in range(REPS):
    for wf in (0, 1):
        r.set_option(ptamd.PT_OPT_ADAPTIVE_WF, wf)
        r.adaptive_begin(P); r.synchronize()
        empty[wf].append(clock(lambda: r.adaptive_advance(200)) / 200)
        assert r.adaptive_info()[0] == 200 and int(r.adaptive_counts()[0].max()) == 2
out["empty_round_ms_option0_median_min_max"] = stat(empty[0])
out["empty_round_ms_option1_median_min_max"] = stat(empty[1])
print("empty round ms", stat(empty[0]), stat(empty[1]), flush=True)
save()
