"""The launch plan on the CPU: every row of tests/plan_cases.py through
tests/plan_check.cpp, a host program around plan_launch (csrc/pt_plan.h) and
around the kernel selection of launch_render and launch_wavefront
(csrc/pt_device.h plan_render, plan_wavefront).

The plan decides which kernel a frame runs on and with how many lanes; apart
from this table those decisions show only on a GPU (tests/test_gpu_plan.py runs
the table's cheap rows there)."""
import os
import re
import subprocess

import pytest

import native
import plan_cases
from plan_cases import ROWS


def _harness():
    return native.build("plan_check", [os.path.join(native.TESTS, "plan_check.cpp")],
                        ["-O1"] + native.COMMON[:2] + ["-I", native.CSRC])


def line_of(r):
    """The row as plan_check reads it."""
    f = r["facts"]
    boxes, leaves, hull = f["sweep"]
    w = dict(n_tris=f["tris"], n_nodes=f["nodes"], n_nodes_full=f["nodes_full"], n_wide=f["n_wide"],
             has_sweep=int(boxes > 0), sweep_boxes=boxes, sweep_leaves=leaves, sweep_hull=hull,
             exit_normals=f["exit_normals"], stats_mode=r["stats"], nranks=r["ranks"], rank=0, width=r["size"][0],
             height=r["size"][1], n_tiles=plan_cases.n_tiles(r), n_batches=r["batches"], packed=r["packed"])
    for k, v in r["opts"].items():
        w[plan_cases.OPT_FIELD[k]] = v
    words = [f"{k}={v}" for k, v in w.items()]
    if f["lights"]:
        words.append("lights=" + ",".join(repr(float(x)) for x in f["lights"]))
    return " ".join(words)


@pytest.fixture(scope="module")
def plans():
    out = subprocess.run([_harness()], input="\n".join(line_of(r) for r in ROWS) + "\n", capture_output=True,
                         text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    assert len(lines) == len(ROWS)
    return {r["name"]: ln for r, ln in zip(ROWS, lines)}


@pytest.mark.parametrize("r", ROWS, ids=[r["name"] for r in ROWS])
def test_row(plans, r):
    got, want = plans[r["name"]], r["expect"]
    if isinstance(want, str):
        first = int(want.startswith("PT_OPT_MOMENTS"))   # refused before the render touches anything
        assert got == f"refuse_code={plan_cases.UNSUPPORTED} first={first} refuse={want}"
        return
    assert not got.startswith("refuse"), got
    plan = {k: int(v) for k, v in re.findall(r"(\w+)=(-?\d+)", got)}
    assert plan == want, {k: (plan.get(k), want[k]) for k in want if plan.get(k) != want[k]}


def test_table_holds_both_sides_of_every_threshold():
    """The rows the thresholds need are there (by the facts, not by name)."""
    def has(pred):
        return any(pred(r) for r in ROWS)

    paths = lambda r: plan_cases.n_tiles(r) * 256 * r["batches"]
    for t in (16383, 16384):
        assert has(lambda r: r["facts"]["tris"] == t and r["facts"]["n_wide"] > 0 and paths(r) >= 1 << 20)
    for t in (32767, 32768):
        assert has(lambda r: r["facts"]["tris"] == t and r["facts"]["n_wide"] == 0 and paths(r) >= 1 << 23)
    for p in ((1 << 20) - 256, 1 << 20):
        assert has(lambda r: paths(r) == p and r["facts"]["n_wide"] > 0 and r["facts"]["tris"] >= 16384)
        assert has(lambda r: paths(r) == p and r["facts"]["n_wide"] == 0 and r["facts"]["tris"] == 1 << 20)
    for p in ((1 << 23) - 256, 1 << 23):
        assert has(lambda r: paths(r) == p and r["facts"]["n_wide"] == 0 and 32768 <= r["facts"]["tris"] < 1 << 20)
    for rec in (3072, 3073):
        assert has(lambda r: 2 * r["facts"]["nodes"] + 3 * r["facts"]["tris"] == rec and not r["opts"])
    for ranks in (1, 2, 7, 8):
        assert has(lambda r: r["ranks"] == ranks and "SAMPLE_LANES" not in r["opts"])
    for b in (1, 2, 4, 8):
        assert has(lambda r: r["ranks"] == 8 and r["batches"] == b)
    for boxes in (15, 16):
        for o in (None, 0, 1):
            assert has(lambda r: r["facts"]["sweep"][0] == boxes and r["opts"].get("SMALL_SWEEP") == o)
    for g in (99, 100):
        assert has(lambda r: r["opts"].get("WF_GRID") == g and "WF_REFILL" not in r["opts"])
    for t in (0x1fffffff, 0x20000000):
        assert has(lambda r: r["facts"]["tris"] == t)
    texts = {r["expect"] for r in ROWS if isinstance(r["expect"], str)}
    assert texts == {plan_cases.T_MOM_PACKED, plan_cases.T_MOM_RANKS, plan_cases.T_MOM_STATS, plan_cases.T_MOM_COUNT,
                     plan_cases.T_LDS, plan_cases.T_STATS_WF}


# ---- kernel selection: what launch_render and launch_wavefront launch ---------------------------------------

def _words(kind, r, **more):
    return kind + " " + " ".join(f"{k}={v}" for k, v in dict(r, **more).items())


def _variant(text):
    return tuple(int(x) for x in text.split(","))


@pytest.fixture(scope="module")
def selection():
    """plan_check's answers to every selection row, and the lists of instantiations it was built with."""
    lines = (["lists"] + [_words("render", r, pix_per_fill=plan_cases.PIX_PER_FILL) for r in plan_cases.RENDER_ROWS] +
             [_words("wavefront", r, pix_per_fill=plan_cases.PIX_PER_FILL, group4_tris=plan_cases.GROUP4_TRIS)
              for r in plan_cases.WF_ROWS])
    out = subprocess.run([_harness()], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    got = out.stdout.splitlines()
    assert len(got) == len(lines)
    n = len(plan_cases.RENDER_ROWS)
    return dict(lists=got[0], render=got[1:1 + n], wavefront=got[1 + n:])


def test_render_selection(selection):
    """plan_render against launch_render's ladder, row by row; every launch runs a listed instantiation."""
    assert len(plan_cases.RENDER_CROSS) == 512
    reached = set()
    for r, got in zip(plan_cases.RENDER_ROWS, selection["render"]):
        want = plan_cases.parent_launch_render(r)
        if isinstance(want, str):
            assert got == want, (r, got)
            continue
        _, grid, lds, k = want
        assert k in plan_cases.RENDER_VARIANTS, (r, k)
        assert got == f"run grid={grid} lds={lds} v={','.join(map(str, k))} listed", (r, got)
        reached.add(k)
    assert len(plan_cases.RENDER_VARIANTS) == 17 and reached == plan_cases.RENDER_VARIANTS


def test_wavefront_selection(selection):
    """plan_wavefront against launch_wavefront's ladder, row by row."""
    reached = dict(trace=set(), wide=set(), shade=set(), tail=set())
    for r, got in zip(plan_cases.WF_ROWS, selection["wavefront"]):
        want = plan_cases.parent_launch_wavefront(r)
        if isinstance(want, str):
            assert got == want, (r, got)
            continue
        if want[0] != "run":
            assert got == f"{want[0]} fill={want[1]}", (r, got)
            continue
        _, fill, px, lds, (family, trace), shade, tail = want
        text = f"run fill={fill} px={px} lds={lds} {family}={','.join(map(str, trace))} listed shade={shade[0]} listed"
        if tail is not None:
            text += f" tail={','.join(map(str, tail))} listed"
            reached["tail"].add(tail)
        assert got == text, (r, got)
        reached[family].add(trace)
        reached["shade"].add(shade)
    # (a scene of kWfGroup4Tris triangles never fits in LDS: the ladder named wf_trace_kernel<true, 4, *>, and the
    # lists keep them, but no launch reaches them)
    assert reached["trace"] == {v for v in plan_cases.WF_TRACE_VARIANTS if v[:2] != (1, 4)}
    assert reached["wide"] == plan_cases.WF_WIDE_VARIANTS
    assert reached["shade"] == plan_cases.WF_SHADE_VARIANTS
    assert reached["tail"] == plan_cases.WF_TAIL_VARIANTS


def test_variant_lists_are_the_ladders(selection):
    """The lists pt_device.hip builds its kernel tables from hold exactly the instantiations the ladders named
    (that they hold exactly what the picks can return is pt_device.h's static_assert)."""
    words = selection["lists"].split()
    lists, name = {}, None
    for w in words:
        if "," in w or w.isdigit():
            lists[name].append(_variant(w))
        else:
            name = w
            lists[name] = []
    want = dict(render=plan_cases.RENDER_VARIANTS, trace=plan_cases.WF_TRACE_VARIANTS, wide=plan_cases.WF_WIDE_VARIANTS,
                shade=plan_cases.WF_SHADE_VARIANTS, tail=plan_cases.WF_TAIL_VARIANTS)
    assert set(lists) == set(want)
    for name, variants in want.items():
        assert len(lists[name]) == len(variants) and set(lists[name]) == variants, name
