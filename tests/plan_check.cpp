// plan_check — plan_launch (csrc/pt_plan.h) and the kernel selection
// (csrc/pt_device.h plan_render, plan_wavefront) on the host, for
// tests/test_plan.py.
//
// Each line of stdin describes one render as `key=value` words: fields of a
// default pt_context by name (n_tris=12 opt_kernel=3 ...), has_sweep=1 for a
// scene with a sweep table, lights=10,inf for one intensity per light, and
// plan_launch's own arguments n_tiles, n_batches, packed.  Each line of stdout
// is that render's plan as `key=value` words, or `refuse_code=... first=...
// refuse=<text to the end of the line>`.
//
// A line that begins with the word `render` or `wavefront` is a launch of
// launch_render / launch_wavefront instead: its words are the launcher's flags
// and the RenderParams members the selection reads (a pointer member is set
// when its word is non-zero; `sweep` is 0 no table, 1 a general one, 2 one with
// hull faces, 3 the cube table), and the answer is `refused`, `nothing`, or
// what would be launched, each variant as its template arguments and `listed`
// when it is one of the instantiations pt_device.h lists.  The line `lists`
// prints those lists.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <iostream>
#include <map>
#include <sstream>
#include <string>

#include "pt_plan.h"

// pt_context.h's fail() refers to it; nothing here calls it
int pt_fail_internal(int code, const std::string&) { return code; }

static float4 g_table;   // stands for a sweep table: the plan asks only whether there is one

static bool set_field(pt_context* c, const std::string& k, long long v) {
#define F(name) if (k == #name) { c->name = (decltype(c->name))v; return true; }
  F(n_tris) F(n_nodes) F(n_nodes_full) F(n_wide) F(sweep_boxes) F(sweep_leaves) F(sweep_hull) F(exit_normals)
  F(stats_mode) F(nranks) F(rank) F(width) F(height)
  F(opt_kernel) F(opt_scene_lds) F(opt_sample_lanes) F(opt_item_order) F(opt_mixed) F(opt_count)
  F(opt_small_sweep) F(opt_sweep_hull) F(opt_exit_skip) F(opt_wide) F(opt_wide_node) F(opt_wf_fuse)
  F(opt_wf_tail) F(opt_wf_grid) F(opt_wf_refill) F(opt_wf_streams) F(opt_moments)
#undef F
  return false;
}

// ---- the kernel selection --------------------------------------------------------------------------------
struct Words {
  std::map<std::string, long long> kv;
  long long operator()(const char* k) const {
    const auto it = kv.find(k);
    if (it == kv.end()) { fprintf(stderr, "plan_check: word %s missing\n", k); exit(2); }
    return it->second;
  }
};

static int g_int;
static float2 g_moments;
static const char* listed(int index) { return index >= 0 ? "listed" : "unlisted"; }

// the members both launchers read
static ptd::RenderParams params_of(const Words& w) {
  ptd::RenderParams p{};
  p.spl = (int)w("spl");
  p.n_tiles = (int)w("n_tiles");
  p.n_batches = (uint32_t)w("n_batches");
  p.items = w("items") ? &g_int : nullptr;
  p.n_items = (int)w("n_items");
  p.n_culled_items = (int)w("n_culled");
  p.n_nodes = (int)w("n_nodes");
  p.n_tris = (int)w("n_tris");
  p.moments = w("moments") ? &g_moments : nullptr;
  p.exit_skip = (int)w("exit_skip");
  return p;
}

static void render_line(const Words& w) {
  ptd::RenderParams p = params_of(w);
  p.sweep = w("sweep") ? &g_table : nullptr;
  p.sweep_hull = w("sweep") >= 2;
  p.sweep_cube = w("sweep") == 3;
  p.sweep_boxes = (int)w("sweep_boxes");
  p.sweep_leaves = (int)w("sweep_leaves");
  p.pack_out = w("pack_out") ? &g_table : nullptr;
  p.n_unpack = (int)w("n_unpack");
  const ptd::RenderLaunch l = ptd::plan_render(p, w("stats") != 0, w("lds") != 0, w("cnt") != 0, (int)w("pix_per_fill"));
  if (l.what != ptd::Launch::Run) {
    puts(l.what == ptd::Launch::Nothing ? "nothing" : "refused");
    return;
  }
  printf("run grid=%lld lds=%zu v=%d,%d,%d,%d,%d,%d %s\n", l.grid, l.lds, (int)l.v.stats, (int)l.v.lds, (int)l.v.cnt,
         l.v.sweep, (int)l.v.moments, (int)l.v.exit, listed(ptd::variant_index(ptd::kRenderVariants, l.v)));
}

static void wavefront_line(const Words& w) {
  ptd::RenderParams p = params_of(w);
  p.wide = w("wide") ? &g_table : nullptr;
  p.wide_qn = (int)w("wide_qn");
  p.wide_ovf_lanes = w("wide_ovf_lanes");
  p.wf_tail = (int)w("wf_tail");
  const ptd::WfLaunch l =
      ptd::plan_wavefront(p, w("cap"), w("lds") != 0, w("cnt") != 0, (int)w("pix_per_fill"), (int)w("group4_tris"));
  switch (l.stop) {
    case ptd::WfStop::Refused: puts("refused"); return;
    case ptd::WfStop::Nothing: puts("nothing"); return;
    case ptd::WfStop::FillOnly: printf("fill_only fill=%lld\n", l.fill_grid); return;
    case ptd::WfStop::FillRefused: printf("fill_refused fill=%lld\n", l.fill_grid); return;
    case ptd::WfStop::Run: break;
  }
  printf("run fill=%lld px=%lld lds=%zu ", l.fill_grid, l.px, l.lds_trace);
  if (l.k.wide)
    printf("wide=%d,%d %s ", (int)l.k.wide_trace.qn, (int)l.k.wide_trace.cnt,
           listed(ptd::variant_index(ptd::kWfWideVariants, l.k.wide_trace)));
  else
    printf("trace=%d,%d,%d %s ", (int)l.k.trace.lds, l.k.trace.group, (int)l.k.trace.cnt,
           listed(ptd::variant_index(ptd::kWfTraceVariants, l.k.trace)));
  printf("shade=%d %s", (int)l.k.shade.exit, listed(ptd::variant_index(ptd::kWfShadeVariants, l.k.shade)));
  if (l.k.tail)
    printf(" tail=%d,%d,%d %s", (int)l.k.tail_v.cnt, (int)l.k.tail_v.qn, (int)l.k.tail_v.exit,
           listed(ptd::variant_index(ptd::kWfTailVariants, l.k.tail_v)));
  putchar('\n');
}

static void lists_line() {
  printf("render");
  for (const ptd::RenderVariant& v : ptd::kRenderVariants)
    printf(" %d,%d,%d,%d,%d,%d", (int)v.stats, (int)v.lds, (int)v.cnt, v.sweep, (int)v.moments, (int)v.exit);
  printf(" trace");
  for (const ptd::WfTraceVariant& v : ptd::kWfTraceVariants) printf(" %d,%d,%d", (int)v.lds, v.group, (int)v.cnt);
  printf(" wide");
  for (const ptd::WfWideVariant& v : ptd::kWfWideVariants) printf(" %d,%d", (int)v.qn, (int)v.cnt);
  printf(" shade");
  for (const ptd::WfShadeVariant& v : ptd::kWfShadeVariants) printf(" %d", (int)v.exit);
  printf(" tail");
  for (const ptd::WfTailVariant& v : ptd::kWfTailVariants) printf(" %d,%d,%d", (int)v.cnt, (int)v.qn, (int)v.exit);
  putchar('\n');
}

// true: the line was one of the selection's
static bool selection_line(const std::string& line) {
  std::istringstream words(line);
  std::string kind, w;
  words >> kind;
  if (kind == "lists") {
    lists_line();
    return true;
  }
  if (kind != "render" && kind != "wavefront") return false;
  Words kv;
  while (words >> w) {
    const size_t eq = w.find('=');
    if (eq == std::string::npos) { fprintf(stderr, "plan_check: no '=' in %s\n", w.c_str()); exit(2); }
    kv.kv[w.substr(0, eq)] = atoll(w.c_str() + eq + 1);
  }
  if (kind == "render")
    render_line(kv);
  else
    wavefront_line(kv);
  return true;
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    if (selection_line(line)) continue;
    pt_context c;
    long long n_tiles = 0, n_batches = 0, packed = 0;
    std::istringstream words(line);
    std::string w;
    while (words >> w) {
      const size_t eq = w.find('=');
      if (eq == std::string::npos) { fprintf(stderr, "plan_check: no '=' in %s\n", w.c_str()); return 2; }
      const std::string k = w.substr(0, eq), v = w.substr(eq + 1);
      if (k == "lights") {
        std::istringstream list(v);
        std::string x;
        while (std::getline(list, x, ',')) {
          pt_area_light l{};
          l.intensity[0] = l.intensity[1] = 1.0f;
          l.intensity[2] = strtof(x.c_str(), nullptr);
          c.lights_host.push_back(l);
        }
        c.n_lights = (int)c.lights_host.size();
      } else if (k == "has_sweep") {
        c.d_sweep = atoi(v.c_str()) ? &g_table : nullptr;
      } else if (k == "n_tiles") {
        n_tiles = atoll(v.c_str());
      } else if (k == "n_batches") {
        n_batches = atoll(v.c_str());
      } else if (k == "packed") {
        packed = atoll(v.c_str());
      } else if (!set_field(&c, k, atoll(v.c_str()))) {
        fprintf(stderr, "plan_check: unknown key %s\n", k.c_str());
        return 2;
      }
    }
    const LaunchPlan p = plan_launch(c, n_tiles, (uint32_t)n_batches, packed != 0);
    if (p.refuse) {
      printf("refuse_code=%d first=%d refuse=%s\n", p.refuse_code, (int)p.refuse_first, p.refuse);
      continue;
    }
    printf("spl=%d lds=%d wf=%d cnt=%d sweep=%d sweep_hull=%d wide=%d mixed_eligible=%d item_order=%d exit_skip=%d "
           "wide_qn=%d wide_handback=%d wf_fuse=%d wf_tail=%d wide_refill=%d two_streams=%d\n",
           p.spl, (int)p.lds, (int)p.wf, (int)p.cnt, (int)p.sweep, (int)p.sweep_hull, (int)p.wide,
           (int)p.mixed_eligible, p.item_order, p.exit_skip, p.wide_qn, p.wide_handback, p.wf_fuse, p.wf_tail,
           p.wide_refill, (int)p.two_streams);
  }
  return 0;
}
