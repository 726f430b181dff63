"""The launch plan (csrc/pt_plan.h plan_launch), one table for two readers.

Each row is what a context holds when a render starts -- the scene's facts, the
options set, the partition, the frame size, the batches, packed or not -- and
the plan (or the refusal) that render gets.  tests/test_plan.py gives every row
to tests/plan_check.cpp, a host program around plan_launch; tests/test_gpu_plan.py
runs the rows that name a real scene (`gpu`) through the library and compares
what the public API shows.  The expectations were read from the code of
render_impl as it stood before plan_launch was cut out of it, and the GPU rows
were checked against a build of that code.

Thresholds appear at the value and one below: 16384 / 32768 triangles, 2^20 and
2^23 paths (a tile holds 256 paths a batch), 3072 LDS records
(2 * nodes + 3 * triangles, 48 KB), kSweepAutoBoxes = 15 boxes, rank counts 2
and 8, kHitRankMask = 0x1fffffff triangles, PT_OPT_WF_GRID 100.
"""

# PT_OPT_<name> -> the pt_context field pt_set_option stores it in
OPT_FIELD = {
    "KERNEL": "opt_kernel", "SCENE_IN_LDS": "opt_scene_lds", "SAMPLE_LANES": "opt_sample_lanes",
    "ITEM_ORDER": "opt_item_order", "MIXED_LANES": "opt_mixed", "COUNT_TRACED": "opt_count",
    "SMALL_SWEEP": "opt_small_sweep", "SWEEP_HULL": "opt_sweep_hull", "EXIT_SKIP": "opt_exit_skip",
    "WIDE": "opt_wide", "WIDE_NODE": "opt_wide_node", "WF_FUSE": "opt_wf_fuse", "WF_TAIL": "opt_wf_tail",
    "WF_GRID": "opt_wf_grid", "WF_REFILL": "opt_wf_refill", "WF_STREAMS": "opt_wf_streams",
    "MOMENTS": "opt_moments",
}

PLAN_KEYS = ("spl", "lds", "wf", "cnt", "sweep", "sweep_hull", "wide", "mixed_eligible", "item_order", "exit_skip",
             "wide_qn", "wide_handback", "wf_fuse", "wf_tail", "wide_refill", "two_streams")

INF = float("inf")

# scene facts: triangles, collapsed nodes, every reference node (stats mode), sweep table (boxes, leaves,
# boxes with a hull code; 0 boxes = no table), wide nodes (0 = no wide table), one intensity per light,
# whether some stored normal is axis-pure
BOX = dict(tris=12, nodes=7, nodes_full=23, sweep=(7, 12, 6), n_wide=3, lights=(10.0,), exit_normals=1)


def scene(tris, nodes=None, n_wide=0, lights=(10.0,), exit_normals=0, sweep=(0, 0, 0), nodes_full=None):
    nodes = 2 * tris - 1 if nodes is None else nodes
    return dict(tris=tris, nodes=nodes, nodes_full=nodes if nodes_full is None else nodes_full, sweep=sweep,
                n_wide=n_wide, lights=tuple(lights), exit_normals=exit_normals)


FITS = scene(1000, 36)         # 2 * 36 + 3 * 1000 = 3072 records: the largest LDS scene
FITS_NOT = scene(1001, 35)     # 3073
TINY16 = dict(tris=16, nodes=31, nodes_full=31, n_wide=0, lights=(10.0,), exit_normals=0)   # + its sweep table
WIDE20K = scene(20480, n_wide=6000)   # displaced_sphere(5)

# the plan of the box's default frame (64x64, 8 batches, one rank), and of a large scene's on each kernel
P_BOX = dict(spl=4, lds=1, wf=0, cnt=0, sweep=1, sweep_hull=1, wide=0, mixed_eligible=1, item_order=0, exit_skip=1,
             wide_qn=0, wide_handback=0, wf_fuse=0, wf_tail=0, wide_refill=16, two_streams=0)
P_LDS = dict(P_BOX, sweep=0, sweep_hull=0, exit_skip=0)                     # an LDS scene without a table
P_REC = dict(P_LDS, lds=0, mixed_eligible=0, spl=8)                          # device memory, path-recursive
P_WF = dict(P_REC, wf=1, item_order=1)                                       # wavefront, exact walk
P_WIDE = dict(P_WF, wide=1, wide_qn=1, wf_fuse=1, wf_tail=400000)            # wavefront, culled wide walk

T_MOM_PACKED = "PT_OPT_MOMENTS: not with pt_render_packed or pt_dist_run"
T_MOM_RANKS = "PT_OPT_MOMENTS: not on a partition of more than one rank"
T_MOM_STATS = "PT_OPT_MOMENTS: not in stats mode"
T_MOM_COUNT = "PT_OPT_MOMENTS: not with PT_OPT_COUNT_TRACED"
T_LDS = "scene too large for the LDS variant"
T_STATS_WF = "stats mode runs the path-recursive kernel only"
UNSUPPORTED = -5

ROWS = []


def row(name, facts, expect, *, opts=None, stats=0, ranks=1, size=(64, 64), batches=8, packed=0, gpu=None):
    """expect: the plan (a dict over PLAN_KEYS) or a refusal's text.  gpu: None, or what the GPU test
    builds and sees -- {"scene": "box" | "sphere:<subdiv>", "mixed": pt_mixed_info()[0] after the render,
    "guide": the text pt_render_guide is refused with as well, None where it runs}."""
    assert name not in [r["name"] for r in ROWS]
    assert isinstance(expect, str) or set(expect) == set(PLAN_KEYS)
    ROWS.append(dict(name=name, facts=facts, expect=expect, opts=dict(opts or {}), stats=stats, ranks=ranks,
                     size=size, batches=batches, packed=packed, gpu=gpu))


def n_tiles(r):
    """Rank 0's tiles of an equal split: the frame's 16x16 blocks dealt round robin."""
    blocks = ((r["size"][0] + 15) // 16) * ((r["size"][1] + 15) // 16)
    return -(-blocks // r["ranks"])


G_BOX = {"scene": "box", "mixed": 0}

# ---- sample lanes: auto by rank count, capped by the batches; explicit lanes are not capped ----------------
row("box", BOX, P_BOX, gpu=G_BOX)
row("box_b4", BOX, P_BOX, batches=4)
row("box_b2", BOX, dict(P_BOX, spl=2), batches=2, gpu=G_BOX)
row("box_b1", BOX, dict(P_BOX, spl=1), batches=1, gpu=G_BOX)
P_SHARE = dict(P_BOX, item_order=1, mixed_eligible=0)
row("box_r2", BOX, dict(P_SHARE, spl=2), ranks=2, gpu=G_BOX)
row("box_r2_b1", BOX, dict(P_SHARE, spl=1), ranks=2, batches=1)
row("box_r7", BOX, dict(P_SHARE, spl=2), ranks=7)
row("box_r8", BOX, dict(P_SHARE, spl=4), ranks=8, gpu=G_BOX)
row("box_r8_b4", BOX, dict(P_SHARE, spl=4), ranks=8, batches=4)
row("box_r8_b2", BOX, dict(P_SHARE, spl=2), ranks=8, batches=2)
row("box_r8_b1", BOX, dict(P_SHARE, spl=1), ranks=8, batches=1)
row("large_b8", FITS_NOT, P_REC)
row("large_b4", FITS_NOT, dict(P_REC, spl=4), batches=4)
row("large_b1", FITS_NOT, dict(P_REC, spl=1), batches=1)
row("large_r8", FITS_NOT, dict(P_REC, item_order=1), ranks=8)
row("lanes8_b1", BOX, dict(P_BOX, spl=8), opts={"SAMPLE_LANES": 8}, batches=1)
row("lanes1", BOX, dict(P_BOX, spl=1), opts={"SAMPLE_LANES": 1})
row("lanes2_large", FITS_NOT, dict(P_REC, spl=2), opts={"SAMPLE_LANES": 2})

# ---- LDS: the 48 KB bound, the three option values, stats mode's node count ---------------------------------
row("lds_3072", FITS, P_LDS)
row("lds_3073", FITS_NOT, P_REC)
row("lds2_3072", FITS, P_LDS, opts={"SCENE_IN_LDS": 2})
row("lds2_3073", FITS_NOT, T_LDS, opts={"SCENE_IN_LDS": 2})
row("lds0_box", BOX, dict(P_BOX, lds=0, sweep=0, sweep_hull=0, mixed_eligible=0), opts={"SCENE_IN_LDS": 0})
row("stats_full_nodes", scene(1000, 36, nodes_full=37), dict(P_REC, exit_skip=0), stats=1)
row("sphere2", scene(320, 600, n_wide=100), P_LDS, gpu={"scene": "sphere:2", "mixed": 0})
# (pt_render_guide walks the wide table where there is one, and only otherwise asks the LDS rule)
row("sphere3_lds2", scene(1280, 2400, n_wide=648), T_LDS, opts={"SCENE_IN_LDS": 2},
    gpu={"scene": "sphere:3", "mixed": 0, "guide": None})
row("sphere3_lds2_wide0", scene(1280, 2400, n_wide=648), T_LDS, opts={"SCENE_IN_LDS": 2, "WIDE": 0},
    gpu={"scene": "sphere:3", "mixed": 0, "guide": T_LDS})

# ---- wavefront or path-recursive -------------------------------------------------------------------------------
M1 = (1024, 1024)        # 4096 tiles: 2^20 paths a batch
M1_LESS = (1008, 1040)   # 63 x 65 = 4095 tiles
M8 = (2048, 4096)        # 32768 tiles: 2^23 paths a batch
M8_LESS = (3472, 2416)   # 217 x 151 = 32767 tiles
P_WIDE1 = dict(P_WIDE, spl=1)
P_REC1 = dict(P_REC, spl=1)
row("wide_16383", scene(16383, n_wide=5000), P_REC1, size=M1, batches=1)
row("wide_16384", scene(16384, n_wide=5000), P_WIDE1, size=M1, batches=1)
row("wide_paths_below", WIDE20K, P_REC1, size=M1_LESS, batches=1)
row("wide_paths_at", WIDE20K, P_WIDE1, size=M1, batches=1, gpu={"scene": "sphere:5", "mixed": 0})
row("wide_paths_1008", WIDE20K, P_REC1, size=(1024, 1008), batches=1, gpu={"scene": "sphere:5", "mixed": 0})
row("wide_off", WIDE20K, P_REC1, opts={"WIDE": 0}, size=M1, batches=1, gpu={"scene": "sphere:5", "mixed": 0})
row("wide_batches", WIDE20K, dict(P_WIDE, spl=4), size=(512, 512), batches=4)
row("wide_share_below", WIDE20K, dict(P_REC1, item_order=1), size=M1, batches=1, ranks=2)
row("wide_share_at", WIDE20K, dict(P_WIDE, spl=2), size=M1, batches=2, ranks=2)
row("exact_32767", scene(32767), P_REC1, size=M8, batches=1)
row("exact_32768", scene(32768), dict(P_WF, spl=1), size=M8, batches=1)
row("exact_paths_below", scene(40000), P_REC1, size=M8_LESS, batches=1)
row("exact_paths_at", scene(40000), dict(P_WF, spl=1), size=M8, batches=1)
row("exact_1m_below", scene((1 << 20) - 1), P_REC1, size=M1, batches=1)
row("exact_1m_waives", scene(1 << 20), dict(P_WF, spl=1), size=M1, batches=1)
row("exact_1m_paths_below", scene(1 << 20), P_REC1, size=M1_LESS, batches=1)
row("no_wide_table", scene(20480), P_REC1, size=M1, batches=1)
row("kernel1", WIDE20K, P_REC1, opts={"KERNEL": 1}, size=M1, batches=1)
row("kernel3_box", BOX, dict(P_BOX, wf=1, sweep=0, sweep_hull=0, mixed_eligible=0, item_order=1),
    opts={"KERNEL": 3}, gpu=G_BOX)
row("kernel3_lds0_box", BOX, dict(P_WIDE, spl=4, exit_skip=1), opts={"KERNEL": 3, "SCENE_IN_LDS": 0})
row("lds_scene_many_paths", FITS, dict(P_LDS, spl=1), size=M8, batches=1)
row("stats_large", WIDE20K, dict(P_REC1), size=M1, batches=1, stats=1)
row("stats_kernel3", BOX, T_STATS_WF, opts={"KERNEL": 3}, stats=1, gpu=G_BOX)

# ---- counting, stats mode: no sweep, no mixed lanes, no exit skip in stats mode ----------------------------
row("count_box", BOX, dict(P_BOX, cnt=1, sweep=0, sweep_hull=0, mixed_eligible=0), opts={"COUNT_TRACED": 1})
row("stats_box", BOX, dict(P_BOX, sweep=0, sweep_hull=0, exit_skip=0), stats=1)
row("stats_count_box", BOX, dict(P_BOX, sweep=0, sweep_hull=0, exit_skip=0), opts={"COUNT_TRACED": 1}, stats=1)

# ---- the sweep walk ----------------------------------------------------------------------------------------------
P_T16 = dict(P_LDS, sweep=1, sweep_hull=1)
row("sweep_15", dict(TINY16, sweep=(15, 16, 2)), P_T16)
row("sweep_16", dict(TINY16, sweep=(16, 16, 2)), P_LDS)
row("sweep_16_on", dict(TINY16, sweep=(16, 16, 2)), P_T16, opts={"SMALL_SWEEP": 1})
row("sweep_15_on", dict(TINY16, sweep=(15, 16, 2)), P_T16, opts={"SMALL_SWEEP": 1})
row("sweep_15_off", dict(TINY16, sweep=(15, 16, 2)), P_LDS, opts={"SMALL_SWEEP": 0})
row("sweep_16_off", dict(TINY16, sweep=(16, 16, 2)), P_LDS, opts={"SMALL_SWEEP": 0})
row("sweep_no_table", dict(TINY16, sweep=(0, 0, 0)), P_LDS, opts={"SMALL_SWEEP": 1})
row("sweep_no_hull_codes", dict(TINY16, sweep=(15, 16, 2)), dict(P_T16, sweep_hull=0), opts={"SWEEP_HULL": 0})
row("sweep_no_hull_boxes", dict(TINY16, sweep=(15, 16, 0)), dict(P_T16, sweep_hull=0))

# ---- item order auto ---------------------------------------------------------------------------------------------
row("order_forced_1", BOX, dict(P_BOX, item_order=1), opts={"ITEM_ORDER": 1})
row("order_forced_0_wf", WIDE20K, dict(P_WIDE1, item_order=0), opts={"ITEM_ORDER": 0}, size=M1, batches=1)
row("order_forced_0_share", BOX, dict(P_SHARE, spl=2, item_order=0), opts={"ITEM_ORDER": 0}, ranks=2)

# ---- the wide walk's layout, fuse, tail and refill ------------------------------------------------------------
W = dict(size=M1, batches=1)
row("refill_grid_100", WIDE20K, P_WIDE1, opts={"WF_GRID": 100}, **W)
row("refill_grid_99", WIDE20K, dict(P_WIDE1, wide_refill=8), opts={"WF_GRID": 99}, **W)
row("refill_24", WIDE20K, dict(P_WIDE1, wide_refill=24), opts={"WF_GRID": 99, "WF_REFILL": 24}, **W)
row("refill_grid_99_box", BOX, dict(P_BOX, wide_refill=8), opts={"WF_GRID": 99})
row("fuse_no_lights", dict(WIDE20K, lights=()), dict(P_WIDE1, wf_fuse=0), **W)
row("fuse_rank_mask", scene(0x1fffffff, n_wide=5000), P_WIDE1, **W)
row("fuse_past_rank_mask", scene(0x20000000, n_wide=5000), dict(P_WIDE1, wf_fuse=0), **W)
row("fuse_off", WIDE20K, dict(P_WIDE1, wf_fuse=0), opts={"WF_FUSE": 0}, **W)
row("tail_0", WIDE20K, dict(P_WIDE1, wf_tail=0), opts={"WF_TAIL": 0}, **W)
row("tail_1000", WIDE20K, dict(P_WIDE1, wf_tail=1000), opts={"WF_TAIL": 1000}, **W)
row("handback", WIDE20K, dict(P_WIDE1, wide_handback=1), opts={"WIDE": 2}, **W)
row("node_128", WIDE20K, dict(P_WIDE1, wide_qn=0), opts={"WIDE_NODE": 128}, **W)
row("two_streams", WIDE20K, dict(P_WIDE1, two_streams=1), opts={"WF_STREAMS": 2}, **W)
row("two_streams_recursive", BOX, P_BOX, opts={"WF_STREAMS": 2})

# ---- the exit skip -------------------------------------------------------------------------------------------------
row("exit_off", BOX, dict(P_BOX, exit_skip=0), opts={"EXIT_SKIP": 0})
row("exit_no_normals", dict(BOX, exit_normals=0), dict(P_BOX, exit_skip=0))
row("exit_infinite_light", dict(BOX, lights=(INF,)), dict(P_BOX, exit_skip=0))
row("exit_second_light_infinite", dict(BOX, lights=(10.0, INF)), dict(P_BOX, exit_skip=0))
row("exit_no_lights", dict(BOX, lights=()), P_BOX)

# ---- mixed-lane eligibility -----------------------------------------------------------------------------------
row("mixed_off", BOX, dict(P_BOX, mixed_eligible=0), opts={"MIXED_LANES": 0})
row("mixed_static", BOX, P_BOX, opts={"MIXED_LANES": 50}, gpu={"scene": "box", "mixed": 1})
row("mixed_static_1_lane", BOX, dict(P_BOX, spl=1, mixed_eligible=0), opts={"MIXED_LANES": 50, "SAMPLE_LANES": 1})
row("mixed_static_kernel3", BOX, dict(P_BOX, wf=1, sweep=0, sweep_hull=0, mixed_eligible=0, item_order=1),
    opts={"MIXED_LANES": 50, "KERNEL": 3}, gpu=G_BOX)
row("mixed_static_share", BOX, dict(P_SHARE, spl=2), opts={"MIXED_LANES": 50}, ranks=2, gpu=G_BOX)
row("mixed_packed", BOX, dict(P_BOX, mixed_eligible=0), packed=1)

# ---- refusals: each alone, then in pairs (the first in render_impl's order is the one reported) ----------
MOM = {"MOMENTS": 1}
row("moments", BOX, P_BOX, opts=MOM)
row("moments_packed", BOX, T_MOM_PACKED, opts=MOM, packed=1)
row("moments_ranks", BOX, T_MOM_RANKS, opts=MOM, ranks=2)
row("moments_stats", BOX, T_MOM_STATS, opts=MOM, stats=1)
row("moments_count", BOX, T_MOM_COUNT, opts=dict(MOM, COUNT_TRACED=1))
row("moments_packed_ranks", BOX, T_MOM_PACKED, opts=MOM, packed=1, ranks=2)
row("moments_ranks_stats", BOX, T_MOM_RANKS, opts=MOM, ranks=2, stats=1)
row("moments_stats_count", BOX, T_MOM_STATS, opts=dict(MOM, COUNT_TRACED=1), stats=1)
row("moments_stats_kernel3", BOX, T_MOM_STATS, opts=dict(MOM, KERNEL=3), stats=1)
row("moments_count_lds", FITS_NOT, T_MOM_COUNT, opts=dict(MOM, COUNT_TRACED=1, SCENE_IN_LDS=2))
row("lds_stats_kernel3", FITS_NOT, T_LDS, opts={"SCENE_IN_LDS": 2, "KERNEL": 3}, stats=1)


# ==== kernel selection (csrc/pt_device.h plan_render, plan_wavefront) ==========================================
# What launch_render and launch_wavefront launch.  Most instantiations give bit-identical frames, so only these
# rows notice the wrong one.  The expectations are restatements of the two launchers' conditional ladders as they
# stood before the selection became a pure function over a table: they do not call the code under test.

K_MAX_SCENE_LDS = 48 * 1024     # pt_device.h kMaxSceneLds
PIX_PER_FILL = 8                # kernels/render.h kPixPerFill
GROUP4_TRIS = 500000            # kernels/wf_trace.h kWfGroup4Tris

# The 17 render_kernel instantiations the ladder of launch_render could reach, as
# (STATS, LDS, CNT, SWEEP, MOMENTS, EXIT): counted from its four arms --
# moments 6 (three sweep walks, LDS, device memory with and without the exit skip), the sweep walks 3,
# counting 3 (LDS, device memory with and without the exit skip), the rest 5 (stats and plain on LDS, stats,
# plain and plain with the exit skip on device memory).
RENDER_VARIANTS = {
    (0, 1, 0, 1, 1, 0), (0, 1, 0, 2, 1, 0), (0, 1, 0, 3, 1, 0), (0, 1, 0, 0, 1, 0), (0, 0, 0, 0, 1, 0), (0, 0, 0, 0, 1, 1),
    (0, 1, 0, 1, 0, 0), (0, 1, 0, 2, 0, 0), (0, 1, 0, 3, 0, 0),
    (0, 1, 1, 0, 0, 0), (0, 0, 1, 0, 0, 0), (0, 0, 1, 0, 0, 1),
    (1, 1, 0, 0, 0, 0), (0, 1, 0, 0, 0, 0), (1, 0, 0, 0, 0, 0), (0, 0, 0, 0, 0, 0), (0, 0, 0, 0, 0, 1),
}
# ... and launch_wavefront's: wf_trace_kernel<LDS, G, CNT> 8, wf_trace_wide_kernel by (qn, cnt) 4,
# wf_shade_kernel<EXIT> 2, wf_tail_kernel<CNT, QN, EXIT> 8
WF_TRACE_VARIANTS = {(l, g, c) for l in (0, 1) for g in (2, 4) for c in (0, 1)}
WF_WIDE_VARIANTS = {(q, c) for q in (0, 1) for c in (0, 1)}
WF_SHADE_VARIANTS = {(0,), (1,)}
WF_TAIL_VARIANTS = {(c, q, e) for c in (0, 1) for q in (0, 1) for e in (0, 1)}

# a launch's words: the launcher's flags and the RenderParams members the selection reads
RENDER_BASE = dict(stats=0, lds=0, cnt=0, sweep=0, moments=0, exit_skip=0, pack_out=0, items=0, spl=4, n_tiles=4,
                   n_batches=8, n_items=3, n_culled=5, n_unpack=4000, sweep_boxes=7, sweep_leaves=12, n_nodes=7,
                   n_tris=12)
WF_BASE = dict(lds=0, wide=0, wide_qn=0, cnt=0, exit_skip=0, moments=0, wf_tail=0, n_tris=12, spl=4, n_tiles=4,
               n_batches=8, items=0, n_items=3, n_culled=5, cap=1 << 20, n_nodes=7, wide_ovf_lanes=256)


def parent_launch_render(r):
    """launch_render's ladder: "refused" (hipErrorInvalidValue), "nothing" (success before any decision), or
    ("run", grid, dynamic LDS bytes, the instantiation)."""
    stats, lds_scene, cnt, spl = r["stats"], r["lds"], r["cnt"], r["spl"]
    if cnt and stats:
        return "refused"
    if spl not in (1, 2, 4, 8):
        return "refused"
    grid = r["n_tiles"] * spl
    if grid <= 0 or r["n_batches"] == 0:
        return "nothing"
    if r["pack_out"] and stats:
        return "refused"
    if r["pack_out"]:
        px = r["n_unpack"] * (256 // spl)
        grid = r["n_items"] + (px + 256 * PIX_PER_FILL - 1) // (256 * PIX_PER_FILL)
    elif r["items"]:
        px = r["n_culled"] * (256 // spl)
        grid = r["n_items"] + (px + 256 * PIX_PER_FILL - 1) // (256 * PIX_PER_FILL)
    if grid > 0x7fffffff:
        return "refused"
    sweep = bool(r["sweep"]) and lds_scene and not stats and not cnt
    if sweep and (r["sweep_boxes"] < 1 or r["sweep_boxes"] > 64 or r["sweep_leaves"] < 1 or r["sweep_leaves"] > 32):
        return "refused"
    lds = 3 * r["sweep_leaves"] * 16 if sweep else (2 * r["n_nodes"] + 3 * r["n_tris"]) * 16 if lds_scene else 0
    if lds > K_MAX_SCENE_LDS:
        return "refused"
    if r["moments"] and (stats or cnt or r["pack_out"]):
        return "refused"
    cube, hull = r["sweep"] == 3, r["sweep"] >= 2   # p.sweep_cube, p.sweep_hull
    ex = r["exit_skip"] and not stats
    if r["moments"]:
        if sweep:
            k = (0, 1, 0, 3, 1, 0) if cube else (0, 1, 0, 2, 1, 0) if hull else (0, 1, 0, 1, 1, 0)
        elif lds_scene:
            k = (0, 1, 0, 0, 1, 0)
        else:
            k = (0, 0, 0, 0, 1, 1) if ex else (0, 0, 0, 0, 1, 0)
    elif sweep:
        k = (0, 1, 0, 3, 0, 0) if cube else (0, 1, 0, 2, 0, 0) if hull else (0, 1, 0, 1, 0, 0)
    elif cnt:
        if lds_scene:
            k = (0, 1, 1, 0, 0, 0)
        else:
            k = (0, 0, 1, 0, 0, 1) if ex else (0, 0, 1, 0, 0, 0)
    elif lds_scene:
        k = (1, 1, 0, 0, 0, 0) if stats else (0, 1, 0, 0, 0, 0)
    elif stats:
        k = (1, 0, 0, 0, 0, 0)
    else:
        k = (0, 0, 0, 0, 0, 1) if ex else (0, 0, 0, 0, 0, 0)
    return ("run", grid, lds, k)


def parent_launch_wavefront(r):
    """launch_wavefront's decisions in its order: "refused", "nothing", ("fill_only", fill grid) for a launch
    without a live item, ("fill_refused", fill grid) for one refused after the culled items' fill was launched, or
    ("run", fill grid, pixels, the trace kernel's LDS bytes, ("trace" | "wide", variant), shade variant, tail
    variant or None)."""
    lds_scene, cnt, spl = r["lds"], r["cnt"], r["spl"]
    if r["moments"] and cnt:
        return "refused"
    if spl not in (1, 2, 4, 8):
        return "refused"
    if r["n_batches"] == 0:
        return "nothing"
    per = 256 // spl
    items = r["n_items"] if r["items"] else r["n_tiles"] * spl
    fill = 0
    if r["items"] and r["n_culled"] > 0:
        fill = (r["n_culled"] * per + 256 * PIX_PER_FILL - 1) // (256 * PIX_PER_FILL)
    if items <= 0:
        return ("fill_only", fill)
    px = items * per
    if px > r["cap"] or r["cap"] > 0x7fffffff:
        return ("fill_refused", fill)
    lds = (2 * r["n_nodes"] + 3 * r["n_tris"]) * 16 if lds_scene else 0
    if lds > K_MAX_SCENE_LDS:
        return ("fill_refused", fill)
    g = 2 if r["n_tris"] < GROUP4_TRIS else 4
    trace = ("trace", (1 if lds_scene else 0, g, 1 if cnt else 0))
    wide = bool(r["wide"]) and not lds_scene
    if wide:
        trace = ("wide", (1 if r["wide_qn"] else 0, 1 if cnt else 0))
    ex = 1 if r["exit_skip"] else 0
    tail = wide and r["wf_tail"] > 0
    if r["wf_tail"] > 0 and not tail:
        return ("fill_refused", fill)
    if wide and r["wide_ovf_lanes"] < 256:
        return ("fill_refused", fill)
    tail_v = (1 if cnt else 0, 1 if r["wide_qn"] else 0, ex) if tail else None
    return ("run", fill, px, 0 if wide else lds, trace, (ex,), tail_v)


def _cross(base, **axes):
    rows = [dict(base)]
    for k, values in axes.items():
        rows = [dict(r, **{k: v}) for r in rows for v in values]
    return rows


B = (0, 1)
# every flag the ladder reads, sweep as 0 off / 1 a general table / 2 a hull table / 3 the cube table: 512 rows
RENDER_CROSS = _cross(RENDER_BASE, stats=B, lds=B, cnt=B, sweep=(0, 1, 2, 3), moments=B, exit_skip=B, pack_out=B,
                      items=B)
SWEEP_ON = dict(RENDER_BASE, lds=1, sweep=2)
LDS_ON = dict(RENDER_BASE, lds=1)
RENDER_EDGES = (
    # the sweep table's sizes, both sides of both ends; they bind only where the sweep walk runs
    [dict(SWEEP_ON, sweep_boxes=n) for n in (0, 1, 64, 65)] + [dict(SWEEP_ON, sweep_leaves=n) for n in (0, 1, 32, 33)] +
    [dict(SWEEP_ON, cnt=1, sweep_boxes=65), dict(SWEEP_ON, stats=1, sweep_leaves=0), dict(SWEEP_ON, lds=0, sweep_boxes=0)] +
    # sample lanes; no batch, no tile
    [dict(RENDER_BASE, spl=s) for s in (0, 1, 2, 3, 4, 5, 8, 16)] +
    [dict(RENDER_BASE, n_batches=n) for n in (0, 1)] + [dict(RENDER_BASE, n_tiles=n) for n in (0, 1)] +
    # ... where only the refusals checked before "nothing to render" still refuse
    [dict(RENDER_BASE, n_batches=0, cnt=1, stats=1), dict(RENDER_BASE, n_batches=0, moments=1, stats=1),
     dict(RENDER_BASE, n_batches=0, spl=3), dict(RENDER_BASE, n_batches=0, lds=1, n_tris=2000)] +
    # 48 KB of LDS: 3072 records of 16 B fit, 3073 do not (and a sweep table's 32 leaves always fit)
    [dict(LDS_ON, n_nodes=36, n_tris=1000), dict(LDS_ON, n_nodes=35, n_tris=1001),
     dict(RENDER_BASE, n_nodes=35, n_tris=1001), dict(SWEEP_ON, n_nodes=35, n_tris=1001)] +
    # a grid of 2^31 - 1 workgroups and one more: whole tiles, a compact list, a packed launch
    [dict(RENDER_BASE, spl=1, n_tiles=0x7fffffff), dict(RENDER_BASE, spl=2, n_tiles=1 << 30),
     dict(RENDER_BASE, items=1, n_items=0x7fffffff, n_culled=0), dict(RENDER_BASE, items=1, n_items=0x7fffffff, n_culled=1),
     dict(RENDER_BASE, pack_out=1, n_items=0x7fffffff, n_unpack=0), dict(RENDER_BASE, pack_out=1, n_items=0x7fffffff, n_unpack=1)] +
    # a compact launch that lists nothing launches nothing; the trailing workgroups round up
    [dict(RENDER_BASE, items=1, n_items=0, n_culled=0), dict(RENDER_BASE, items=1, n_items=0, n_culled=32),
     dict(RENDER_BASE, items=1, n_items=0, n_culled=33), dict(RENDER_BASE, pack_out=1, n_items=2, n_unpack=33, spl=1)]
)
RENDER_ROWS = RENDER_CROSS + RENDER_EDGES

# every flag the ladder reads, on both sides of kWfGroup4Tris (scenes of that size never fit in LDS: those rows are
# refused for it) and for a scene that fits
WF_CROSS = _cross(WF_BASE, lds=B, wide=B, wide_qn=B, cnt=B, exit_skip=B, moments=B, wf_tail=(0, 1000),
                  n_tris=(12, GROUP4_TRIS - 1, GROUP4_TRIS))
WF_WIDE = dict(WF_BASE, wide=1, wide_qn=1, wf_tail=1000)
WF_EDGES = (
    [dict(WF_BASE, spl=s) for s in (0, 1, 2, 3, 4, 8, 16)] + [dict(WF_BASE, n_batches=0), dict(WF_BASE, n_batches=0, spl=3),
     dict(WF_BASE, n_batches=0, moments=1, cnt=1), dict(WF_BASE, n_batches=0, wf_tail=5)] +
    # no live item: the fill alone, whatever the later checks would say
    [dict(WF_BASE, n_tiles=0), dict(WF_BASE, items=1, n_items=0), dict(WF_BASE, items=1, n_items=0, n_culled=0),
     dict(WF_BASE, items=1, n_items=0, wf_tail=5), dict(WF_BASE, items=1, n_items=0, n_culled=33, spl=1)] +
    # the buffers hold the launch's pixels, and at most 2^31 - 1 paths
    [dict(WF_BASE, cap=16 * 64), dict(WF_BASE, cap=16 * 64 - 1), dict(WF_BASE, items=1, cap=3 * 64 - 1),
     dict(WF_BASE, cap=0x7fffffff), dict(WF_BASE, cap=1 << 31)] +
    [dict(WF_BASE, lds=1, n_nodes=36, n_tris=1000), dict(WF_BASE, lds=1, n_nodes=35, n_tris=1001),
     dict(WF_BASE, n_nodes=35, n_tris=1001), dict(WF_WIDE, lds=1, wf_tail=0, n_nodes=35, n_tris=1001)] +
    # the tail kernel needs the wide walk; the wide walk needs an overflow area per lane of a workgroup
    [dict(WF_BASE, wf_tail=1), dict(WF_WIDE, wf_tail=1), dict(WF_WIDE, lds=1), dict(WF_WIDE, wide_ovf_lanes=255),
     dict(WF_WIDE, wide_ovf_lanes=256), dict(WF_BASE, wide_ovf_lanes=0), dict(WF_WIDE, lds=1, wf_tail=0, wide_ovf_lanes=0)] +
    [dict(WF_WIDE, items=1), dict(WF_WIDE, items=1, n_culled=0)]
)
WF_ROWS = WF_CROSS + WF_EDGES
