// Test infrastructure: a stand-alone program that table-tests plan_radiance (csrc/pt_device.h), the pure choice
// of a radiance query chunk's kernels, grids and LDS bytes.  No HIP call, no library.  Built by tests/native.py
// (tests/test_radiance.py), plainly and under the sanitizers; prints one line per case and
// "radiance_plan_check ok".
#include <stdio.h>

#include "pt_device.h"

using namespace ptd;

static int failures = 0;
#define EXPECT(cond)                                             \
  do {                                                           \
    if (!(cond)) {                                               \
      printf("FAILED line %d: %s\n", __LINE__, #cond);           \
      ++failures;                                                \
    }                                                            \
  } while (0)

static RenderParams scene(int n_tris, int n_nodes) {
  RenderParams p{};
  p.n_tris = n_tris;
  p.n_nodes = n_nodes;
  p.spl = 1;
  return p;
}

int main() {
  const int kGroup4 = 4096;
  int cases = 0;
  // refusals and no-ops, whatever the kernel family
  for (int wf = 0; wf < 2; ++wf) {
    RenderParams p = scene(12, 23);
    EXPECT(plan_radiance(p, wf, false, 10, 0, 1 << 20, kGroup4).what == Launch::Refused);
    EXPECT(plan_radiance(p, wf, false, 10, 65537, 1 << 20, kGroup4).what == Launch::Refused);
    EXPECT(plan_radiance(p, wf, false, -1, 1, 1 << 20, kGroup4).what == Launch::Refused);
    EXPECT(plan_radiance(p, wf, false, 0, 1, 1 << 20, kGroup4).what == Launch::Nothing);
    // the chunk's paths stay below 2^31 - 255
    EXPECT(plan_radiance(p, wf, false, kRadianceMaxPaths / 65536 + 1, 65536, 0x7fffffffll, kGroup4).what == Launch::Refused);
    EXPECT(plan_radiance(p, wf, false, kRadianceMaxPaths + 1, 1, 0x7fffffffll, kGroup4).what == Launch::Refused);
    cases += 6;
    printf("wf=%d refusals ok\n", wf);
  }
  // grids: one workgroup per 256 paths, one fold lane per query
  const long long nq[] = {1, 63, 64, 65, 255, 256, 257, 4097, 2073600};
  const uint32_t ns[] = {1, 2, 5, 64, 65536};
  for (long long n : nq)
    for (uint32_t s : ns) {
      if (n > kRadianceMaxPaths / (long long)s) continue;
      RenderParams p = scene(12, 23);
      const RadianceLaunch l = plan_radiance(p, false, true, n, s, 0, kGroup4);
      EXPECT(l.what == Launch::Run && !l.wf);
      EXPECT(l.paths == n * s && l.grid == (n * s + 255) / 256 && l.fold_grid == (n + 255) / 256);
      EXPECT(l.grid * 256 >= l.paths && (l.grid - 1) * 256 < l.paths);
      EXPECT(l.lds == scene_lds_bytes(p));
      ++cases;
      printf("n=%lld S=%u grid=%lld fold=%lld lds=%zu\n", n, s, l.grid, l.fold_grid, l.lds);
    }
  // the path-recursive instantiation: render_adaptive_kernel's pick, every listed variant met and no other
  unsigned met = 0;
  for (int lds = 0; lds < 2; ++lds)
    for (int table = 0; table < 4; ++table)
      for (int ex = 0; ex < 2; ++ex) {
        RenderParams p = scene(12, 23);
        p.exit_skip = ex;
        if (table) {
          static const float4 dummy[1] = {};
          p.sweep = dummy;
          p.sweep_boxes = 7;
          p.sweep_leaves = 12;
          p.sweep_hull = table >= 2;
          p.sweep_cube = table == 3;
        }
        const RadianceLaunch l = plan_radiance(p, false, lds != 0, 100, 3, 0, kGroup4);
        EXPECT(l.what == Launch::Run);
        const RadianceVariant want = {lds != 0, lds ? table : 0, ex && !lds};
        EXPECT(l.v == want);
        const int idx = variant_index(kAdaptiveVariants, l.v);
        EXPECT(idx >= 0);
        if (idx >= 0) met |= 1u << idx;
        EXPECT(l.lds == (l.v.sweep ? sweep_lds_bytes(p) : lds ? scene_lds_bytes(p) : 0));
        ++cases;
        printf("lds=%d table=%d exit=%d -> <%d, %d, %d> lds=%zu\n", lds, table, ex, l.v.lds, l.v.sweep, l.v.exit, l.lds);
      }
  EXPECT(met == (1u << (sizeof kAdaptiveVariants / sizeof kAdaptiveVariants[0])) - 1u);
  {   // a sweep table out of range, a scene too large for LDS
    RenderParams p = scene(12, 23);
    static const float4 dummy[1] = {};
    p.sweep = dummy;
    p.sweep_boxes = 65;
    p.sweep_leaves = 12;
    EXPECT(plan_radiance(p, false, true, 10, 1, 0, kGroup4).what == Launch::Refused);
    p.sweep_boxes = 7;
    p.sweep_leaves = 33;
    EXPECT(plan_radiance(p, false, true, 10, 1, 0, kGroup4).what == Launch::Refused);
    RenderParams big = scene(2000, 3999);
    EXPECT(scene_lds_bytes(big) > kMaxSceneLds);
    EXPECT(plan_radiance(big, false, true, 10, 1, 0, kGroup4).what == Launch::Refused);
    EXPECT(plan_radiance(big, true, true, 10, 1, 1 << 20, kGroup4).what == Launch::Refused);
    EXPECT(plan_radiance(big, false, false, 10, 1, 0, kGroup4).what == Launch::Run);
    cases += 5;
  }
  // the wavefront pipeline: the buffers bound the chunk; the wide walk needs its overflow areas; the kernels
  // are pick_wavefront's without counters or moments
  for (int wide = 0; wide < 2; ++wide)
    for (int qn = 0; qn < 2; ++qn)
      for (int ex = 0; ex < 2; ++ex)
        for (int tail = 0; tail < 2; ++tail) {
          RenderParams p = scene(20480, 40959);
          static const float4 dummy[1] = {};
          p.exit_skip = ex;
          if (wide) {
            p.wide = dummy;
            p.wide_qn = qn;
            p.wide_ovf_lanes = 1 << 16;
            p.wf_tail = tail ? 400000 : 0;
          }
          const RadianceLaunch l = plan_radiance(p, true, false, 1000, 5, 5000, kGroup4);
          EXPECT(l.what == Launch::Run && l.wf && l.paths == 5000 && l.grid == 20 && l.fold_grid == 4 && l.lds == 0);
          EXPECT(l.k.wide == (wide != 0) && l.k.tail == (wide && tail) && l.k.shade.exit == (ex != 0));
          EXPECT(!l.k.trace.cnt && !l.k.wide_trace.cnt && !l.k.tail_v.cnt);
          if (wide) EXPECT(l.k.wide_trace.qn == (qn != 0));
          if (!wide) EXPECT(l.k.trace.group == 4 && !l.k.trace.lds);
          EXPECT(plan_radiance(p, true, false, 1000, 5, 4999, kGroup4).what == Launch::Refused);
          if (wide) {
            p.wide_ovf_lanes = 255;
            EXPECT(plan_radiance(p, true, false, 1000, 5, 5000, kGroup4).what == Launch::Refused);
          }
          ++cases;
          printf("wf wide=%d qn=%d exit=%d tail=%d ok\n", wide, qn, ex, tail);
        }
  {   // an LDS-staged scene on the wavefront pipeline: the threaded trace kernel stages it, groups of two
    RenderParams p = scene(12, 23);
    const RadianceLaunch l = plan_radiance(p, true, true, 257, 5, 1 << 20, kGroup4);
    EXPECT(l.what == Launch::Run && l.k.trace.lds && l.k.trace.group == 2 && l.lds == scene_lds_bytes(p) && !l.k.wide);
    ++cases;
  }
  if (failures) {
    printf("radiance_plan_check: %d failures\n", failures);
    return 1;
  }
  printf("radiance_plan_check ok: %d cases\n", cases);
  return 0;
}
