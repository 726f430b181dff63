// adaptive_wf_plan_check — adaptive rounds on the wavefront pipeline
// (PT_OPT_ADAPTIVE_WF) on the host, for tests/test_adaptive_wf.py: plan_adaptive
// (csrc/pt_plan.h) over contexts x the option x PT_OPT_KERNEL, with the wide
// walk's settings held against plan_launch's for a wavefront launch and the
// option-0 rows against the values of before; plan_wavefront_adaptive
// (csrc/pt_device.h): grids, chunk sizes, refusals; and wf_adaptive_path, the
// path numbering the two kernels share.  Prints one line per row, then
// "ok: N rows", exit status 0; or what failed and 1.
#include <stdio.h>
#include <string.h>

#include <functional>
#include <string>
#include <vector>

#include "pt_plan.h"

// pt_context.h's fail() refers to it; nothing here calls it
int pt_fail_internal(int code, const std::string&) { return code; }

namespace {

float4 g_table;       // stands for a device array: only tested against null
float2 g_moments;
int g_items;
pt_group* const kGroup = reinterpret_cast<pt_group*>(&g_table);

int fails = 0, rows = 0;

void check(bool ok, const char* name) {
  ++rows;
  if (!ok) {
    fprintf(stderr, "FAILED: %s\n", name);
    ++fails;
  }
}

// box.obj as the library sees it: 12 triangles, a cube table of 7 boxes, axis-pure normals, one finite light
void box(pt_context* c) {
  c->n_tris = 12;
  c->n_nodes = 23;
  c->n_nodes_full = 23;
  c->d_sweep = &g_table;
  c->sweep_boxes = 7;
  c->sweep_leaves = 12;
  c->sweep_hull = 6;
  c->sweep_cube = true;
  c->n_wide = 5;
  c->exit_normals = true;
  c->n_lights = 1;
  c->lights_host.resize(1);
  for (int k = 0; k < 3; ++k) c->lights_host[0].intensity[k] = 10.0f;
  c->opt_moments = 1;
  c->width = 72;
  c->height = 40;
}
// a scene too large for LDS, without a sweep table, with a wide tree
void big(pt_context* c) {
  box(c);
  c->n_tris = 100000;
  c->n_nodes = 199999;
  c->n_nodes_full = 199999;
  c->n_wide = 40000;
  c->d_sweep = nullptr;
  c->sweep_boxes = c->sweep_leaves = c->sweep_hull = 0;
  c->sweep_cube = false;
}

typedef std::function<void(pt_context*)> Setup;
const pt_adaptive_params A = {2, 9, 3, 0.25f, 0.01f};

// What the rounds of before ran (tests/adaptive_plan_check.cpp's rows): the path-recursive instantiation.
struct Before {
  int lds, sweep, exit, spl0, spl;
};

// One context under the option and PT_OPT_KERNEL.  wf: the plan's flag; with it the LDS staging, the exit skip
// and every wide-walk setting are plan_launch's for the same context asked for the wavefront pipeline; without
// it the plan is the one of before.  kernel 3 with the option off is refused, as before.
void plan_row(const char* name, const Setup& set, int adaptive_wf, int kernel, const Before& b) {
  pt_context c;
  set(&c);
  c.opt_adaptive_wf = adaptive_wf;
  c.opt_kernel = kernel;
  const AdaptivePlan p = plan_adaptive(c, A);
  char what[256];
  snprintf(what, sizeof what, "%s, option %d, kernel %d", name, adaptive_wf, kernel);
  if (kernel == 3 && !adaptive_wf) {
    printf("%s: refuse_code=%d refuse=%s\n", what, p.refuse_code, p.refuse ? p.refuse : "(none)");
    check(p.refuse_code == PT_ERR_UNSUPPORTED && p.refuse && strstr(p.refuse, "PT_OPT_KERNEL 3"), what);
    return;
  }
  const bool wf = adaptive_wf && kernel != 1;
  bool ok = !p.refuse && p.refuse_code == PT_OK && p.wf == wf && p.rounds == 3u;
  if (!wf) {
    ok = ok && (int)p.lds == b.lds && p.sweep == b.sweep && (int)p.v.lds == b.lds && p.v.sweep == b.sweep &&
         (int)p.v.exit == b.exit && p.spl0 == b.spl0 && p.spl == b.spl && !p.wide && !p.wide_qn && !p.wide_handback &&
         !p.wf_fuse && !p.wf_tail;
  } else {
    pt_context c3;
    set(&c3);
    c3.opt_kernel = 3;
    const LaunchPlan l = plan_launch(c3, 0, A.min_batches, false);
    ok = ok && l.wf && !l.refuse && p.lds == l.lds && p.sweep == 0 && p.exit_skip == l.exit_skip && p.wide == l.wide &&
         p.wide_qn == l.wide_qn && p.wide_handback == l.wide_handback && p.wf_fuse == l.wf_fuse &&
         p.wf_tail == l.wf_tail && p.wide_refill == l.wide_refill && ptd::spl_valid(p.spl0) && ptd::spl_valid(p.spl);
  }
  printf("%s: wf=%d lds=%d sweep=%d exit_skip=%d wide=%d qn=%d handback=%d fuse=%d tail=%d refill=%d spl0=%d spl=%d\n", what,
         (int)p.wf, (int)p.lds, p.sweep, p.exit_skip, (int)p.wide, p.wide_qn, p.wide_handback, p.wf_fuse, p.wf_tail,
         p.wide_refill, p.spl0, p.spl);
  check(ok, what);
}

void refusal_row(const char* name, const Setup& set, pt_adaptive_params a, int code, const char* text) {
  pt_context c;
  box(&c);
  c.opt_adaptive_wf = 1;
  set(&c);
  const AdaptivePlan p = plan_adaptive(c, a);
  printf("%s: refuse_code=%d refuse=%s\n", name, p.refuse_code, p.refuse ? p.refuse : "(none)");
  check(p.refuse_code == code && p.refuse && strstr(p.refuse, text), name);
}

// ---- plan_wavefront_adaptive ----
ptd::RenderParams round_params(int blocks, uint32_t nb) {
  ptd::RenderParams p{};
  p.spl = 4;
  p.nranks = 1;
  p.blocks_total = blocks;
  p.n_batches = nb;
  p.moments = &g_moments;
  p.n_nodes = 23;
  p.n_tris = 12;
  return p;
}

void launch_row(const char* name, const ptd::RenderParams& p, long long cap, bool lds, ptd::Launch what, uint32_t chunk,
                long long gen_grid) {
  const ptd::WfAdaptiveLaunch l = ptd::plan_wavefront_adaptive(p, cap, lds, 1 << 16);
  printf("%s: what=%d px=%lld chunk=%u gen_grid=%lld fold_grid=%lld lds=%zu wide=%d tail=%d\n", name, (int)l.what, l.px,
         l.chunk, l.gen_grid, l.fold_grid, l.lds_trace, (int)l.k.wide, (int)l.k.tail);
  bool ok = l.what == what;
  if (what == ptd::Launch::Run)
    ok = ok && l.px == (long long)p.blocks_total * 256 && l.chunk == chunk && l.gen_grid == gen_grid &&
         l.fold_grid == p.blocks_total && l.px * l.chunk <= cap && l.chunk >= 1 && l.chunk <= p.n_batches &&
         l.lds_trace == (lds && !l.k.wide ? ptd::scene_lds_bytes(p) : 0);
  check(ok, name);
}

// ---- the path numbering ----
// Every (block, tid) of a chunk of nb batches over n_entries entries: the path is (e * 256 + q) * nb + s with
// e = block / nb the same for the whole workgroup, q < 256, s < nb, and the map covers [0, entries * 256 * nb)
// once, a pixel's samples adjacent and in order.
bool numbering(uint32_t nb, uint32_t n_entries) {
  std::vector<unsigned char> seen((size_t)n_entries * 256 * nb, 0);
  for (uint32_t block = 0; block < n_entries * nb; ++block)
    for (uint32_t tid = 0; tid < 256; ++tid) {
      const ptd::WfAdaptivePath a = ptd::wf_adaptive_path(block, tid, nb);
      if (a.entry != block / nb || a.q >= 256u || a.s >= nb) return false;
      if (a.g != ptd::wf_adaptive_index(a.entry, (int)a.q, a.s, nb)) return false;
      if (a.g != (long long)block * 256 + tid) return false;
      if (a.g < 0 || a.g >= (long long)seen.size() || seen[(size_t)a.g]++) return false;
    }
  return true;
}

}  // namespace

int main() {
  // ---- plan_adaptive: contexts x the option x PT_OPT_KERNEL ----
  struct Ctx {
    const char* name;
    Setup set;
    Before before;
  };
  const Ctx contexts[] = {
      {"box", box, {1, 3, 0, 2, 2}},
      {"box from device memory", [](pt_context* c) { box(c); c->opt_scene_lds = 0; }, {0, 0, 1, 2, 2}},
      {"box from device memory, threaded walk", [](pt_context* c) { box(c); c->opt_scene_lds = 0; c->opt_wide = 0; },
       {0, 0, 1, 2, 2}},
      {"large scene", big, {0, 0, 1, 2, 2}},
      {"large scene, no exit skip", [](pt_context* c) { big(c); c->opt_exit_skip = 0; }, {0, 0, 0, 2, 2}},
      {"large scene, hand-back", [](pt_context* c) { big(c); c->opt_wide = 2; }, {0, 0, 1, 2, 2}},
      {"large scene, 128-B nodes", [](pt_context* c) { big(c); c->opt_wide_node = 128; }, {0, 0, 1, 2, 2}},
      {"large scene, no fused shadow walks", [](pt_context* c) { big(c); c->opt_wf_fuse = 0; }, {0, 0, 1, 2, 2}},
      {"large scene, tail never", [](pt_context* c) { big(c); c->opt_wf_tail = 0; }, {0, 0, 1, 2, 2}},
      {"large scene, tail always", [](pt_context* c) { big(c); c->opt_wf_tail = 0x7fffffff; }, {0, 0, 1, 2, 2}},
      {"large scene, refill 4", [](pt_context* c) { big(c); c->opt_wf_refill = 4; }, {0, 0, 1, 2, 2}},
      {"large scene, a split grid", [](pt_context* c) { big(c); c->opt_wf_grid = 50; }, {0, 0, 1, 2, 2}},
      {"large scene, two streams asked for", [](pt_context* c) { big(c); c->opt_wf_streams = 2; }, {0, 0, 1, 2, 2}},
      {"large scene without a wide tree", [](pt_context* c) { big(c); c->n_wide = 0; }, {0, 0, 1, 2, 2}},
  };
  for (const Ctx& x : contexts)
    for (int o = 0; o < 2; ++o)
      for (int k : {0, 1, 3}) plan_row(x.name, x.set, o, k, x.before);
  {   // what the rows above rely on: the wide walk is in force on the large scene and not on the LDS-staged box
    pt_context c;
    big(&c);
    c.opt_adaptive_wf = 1;
    const AdaptivePlan p = plan_adaptive(c, A);
    check(p.wf && p.wide && !p.lds && p.wide_qn == 1 && p.wf_fuse == 1 && p.wf_tail > 0 && p.wide_refill == 16,
          "large scene: the culled wide walk, 64-B nodes, fused, tail auto, refill 16");
    pt_context d;
    box(&d);
    d.opt_adaptive_wf = 1;
    const AdaptivePlan q = plan_adaptive(d, A);
    check(q.wf && q.lds && !q.wide && q.sweep == 0, "box: the wavefront pipeline from LDS, no sweep, no wide walk");
    d.opt_scene_lds = 0;
    const AdaptivePlan r = plan_adaptive(d, A);
    check(r.wf && !r.lds && r.wide, "box from device memory: the wide walk");
  }
  // ---- the refusals hold with the option on, in their order ----
  const int U = PT_ERR_UNSUPPORTED, I = PT_ERR_INVALID;
  refusal_row("refused: a multi-device context", [](pt_context* c) { c->group = kGroup; }, A, U, "multi-device");
  refusal_row("refused: a partition", [](pt_context* c) { c->nranks = 2; }, A, U, "more than one rank");
  refusal_row("refused: stats mode", [](pt_context* c) { c->stats_mode = true; }, A, U, "stats mode");
  refusal_row("refused: counting", [](pt_context* c) { c->opt_count = 1; }, A, U, "PT_OPT_COUNT_TRACED");
  refusal_row("refused: no moments", [](pt_context* c) { c->opt_moments = 0; }, A, I, "PT_OPT_MOMENTS 1");
  refusal_row("refused: LDS asked for a scene that cannot fit", [](pt_context* c) { big(c); c->opt_scene_lds = 2; }, A, U,
              "too large for the LDS");
  refusal_row("refused: bad parameters come first", [](pt_context* c) { c->group = kGroup; c->opt_kernel = 3; },
              {1, 9, 3, 0.25f, 0.01f}, I, "pt_adaptive_params");
  refusal_row("order: a multi-device context before a partition", [](pt_context* c) { c->group = kGroup; c->nranks = 2; },
              A, U, "multi-device");
  refusal_row("order: a partition before stats mode", [](pt_context* c) { c->nranks = 2; c->stats_mode = true; }, A, U,
              "more than one rank");
  refusal_row("order: stats mode before counting", [](pt_context* c) { c->stats_mode = true; c->opt_count = 1; }, A, U,
              "stats mode");
  refusal_row("order: counting before the moments", [](pt_context* c) { c->opt_count = 1; c->opt_moments = 0; }, A, U,
              "PT_OPT_COUNT_TRACED");
  refusal_row("order, option off: counting before PT_OPT_KERNEL 3",
              [](pt_context* c) { c->opt_adaptive_wf = 0; c->opt_count = 1; c->opt_kernel = 3; }, A, U, "PT_OPT_COUNT_TRACED");
  refusal_row("order, option off: PT_OPT_KERNEL 3 before the moments",
              [](pt_context* c) { c->opt_adaptive_wf = 0; c->opt_kernel = 3; c->opt_moments = 0; }, A, U, "PT_OPT_KERNEL 3");

  // ---- plan_wavefront_adaptive: 15 tiles (72x40), a step of 3 ----
  using ptd::Launch;
  const long long px = 15 * 256;
  const ptd::RenderParams r3 = round_params(15, 3);
  launch_row("cap = px: one batch per chunk", r3, px, true, Launch::Run, 1, 15);
  launch_row("cap = 2 px: chunks of 2 + 1", r3, 2 * px, true, Launch::Run, 2, 30);
  launch_row("cap = 3 px: the round in one chunk", r3, 3 * px, false, Launch::Run, 3, 45);
  launch_row("cap = px - 1: refused", r3, px - 1, true, Launch::Refused, 0, 0);
  launch_row("cap = 2^31 - 1: the round in one chunk", r3, 0x7fffffffll, true, Launch::Run, 3, 45);
  launch_row("cap = 2^31: refused", r3, 0x80000000ll, true, Launch::Refused, 0, 0);
  {
    ptd::RenderParams p = round_params(8160, 65536);   // 1920x1080, the longest round
    launch_row("1080p, 65536 batches, cap 2^27", p, 1ll << 27, false, Launch::Run, 64, 8160ll * 64);
    launch_row("1080p, 65536 batches, cap 2^31 - 1", p, 0x7fffffffll, false, Launch::Run, 1028, 8160ll * 1028);
    p.n_batches = 65537;
    launch_row("more than 65536 batches: refused", p, 1ll << 27, false, Launch::Refused, 0, 0);
  }
  launch_row("no batches: nothing", round_params(15, 0), px, true, Launch::Nothing, 0, 0);
  launch_row("no tiles: nothing", round_params(0, 3), px, true, Launch::Nothing, 0, 0);
  {
    ptd::RenderParams p = r3;
    p.moments = nullptr;
    launch_row("refused: no moments image", p, px, true, Launch::Refused, 0, 0);
    p = r3;
    p.items = &g_items;
    launch_row("refused: an item list", p, px, true, Launch::Refused, 0, 0);
    p = r3;
    p.pack_out = &g_table;
    launch_row("refused: a packed output", p, px, true, Launch::Refused, 0, 0);
    p = r3;
    p.nranks = 2;
    launch_row("refused: a partition", p, px, true, Launch::Refused, 0, 0);
    p = r3;
    p.spl = 3;
    launch_row("refused: 3 sample lanes", p, px, true, Launch::Refused, 0, 0);
    p = r3;
    p.wf_tail = 400000;
    launch_row("refused: a tail without the wide walk (pick_wavefront)", p, px, true, Launch::Refused, 0, 0);
    p.wide = &g_table;
    launch_row("refused: a tail on an LDS-staged scene (pick_wavefront)", p, px, true, Launch::Refused, 0, 0);
    launch_row("refused: the wide walk without overflow areas", p, px, false, Launch::Refused, 0, 0);
    p.wide_ovf_lanes = 256;
    launch_row("the wide walk with a tail", p, px, false, Launch::Run, 1, 15);
    const ptd::WfAdaptiveLaunch l = ptd::plan_wavefront_adaptive(p, px, false, 1 << 16);
    check(l.k.wide && l.k.tail && ptd::variant_index(ptd::kWfWideVariants, l.k.wide_trace) >= 0 &&
              ptd::variant_index(ptd::kWfTailVariants, l.k.tail_v) >= 0 && !l.k.wide_trace.cnt && !l.k.tail_v.cnt &&
              ptd::variant_index(ptd::kWfShadeVariants, l.k.shade) >= 0,
          "the wide walk's kernels are listed ones, without counters");
    p = round_params(15, 3);
    p.n_nodes = 199999;
    p.n_tris = 100000;
    launch_row("refused: LDS staging of a scene that cannot fit", p, px, true, Launch::Refused, 0, 0);
    launch_row("the same scene from device memory, threaded walk", p, px, false, Launch::Run, 1, 15);
  }

  // ---- the path numbering ----
  check(numbering(1, 3), "numbering: 1 batch");
  check(numbering(2, 3), "numbering: 2 batches (a chunk shorter than the round of 3)");
  check(numbering(3, 15), "numbering: 3 batches over 15 entries");
  check(numbering(9, 2), "numbering: 9 batches");
  check(numbering(257, 2), "numbering: 257 batches");
  {
    const uint32_t nb = 3, e = 7;
    const ptd::WfAdaptivePath first = ptd::wf_adaptive_path(e * nb, 0, nb), last = ptd::wf_adaptive_path(e * nb + nb - 1, 255, nb);
    check(first.entry == e && first.q == 0 && first.s == 0 && first.g == (long long)e * 256 * nb,
          "the first path of an entry");
    check(last.entry == e && last.q == 255 && last.s == nb - 1 && last.g == (long long)(e + 1) * 256 * nb - 1,
          "the last path of an entry");
    // past 2^31: the last thread of the largest grid, at the longest round
    const uint32_t big_nb = 65536, block = 0x7fffffffu;
    const ptd::WfAdaptivePath a = ptd::wf_adaptive_path(block, 255, big_nb);
    check(a.g == 0x7fffffffll * 256 + 255 && a.g > (1ll << 31) && a.entry == block / big_nb && a.q == 255 &&
              a.s == big_nb - 1 && a.g == ptd::wf_adaptive_index(a.entry, (int)a.q, a.s, big_nb),
          "a path past 2^31");
    const ptd::WfAdaptivePath b = ptd::wf_adaptive_path(8388608u, 17, 1);   // g = 2^31 + 17 at one batch
    check(b.g == (1ll << 31) + 17 && b.entry == 8388608u && b.q == 17 && b.s == 0 &&
              b.g == ptd::wf_adaptive_index(b.entry, (int)b.q, b.s, 1),
          "a path just past 2^31 at one batch");
  }
  if (fails) return 1;
  printf("ok: %d rows\n", rows);
  return 0;
}
