// plan_check — plan_launch (csrc/pt_plan.h) on the host, for tests/test_plan.py.
//
// Each line of stdin describes one render as `key=value` words: fields of a
// default pt_context by name (n_tris=12 opt_kernel=3 ...), has_sweep=1 for a
// scene with a sweep table, lights=10,inf for one intensity per light, and
// plan_launch's own arguments n_tiles, n_batches, packed.  Each line of stdout
// is that render's plan as `key=value` words, or `refuse_code=... first=...
// refuse=<text to the end of the line>`.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <iostream>
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

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
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
