// pt_api.cpp — the core of the C-ABI shim (include/pathtracer.h); pt_context.h
// has the context and names the files that hold the rest of the shim.
//
// Replaces the Vulkan resource/dispatch seam of src/Vulkan/VulkanRayTracer.cpp:
// staging buffers + vkCmdCopyBuffer become hipMemcpyAsync, the descriptor set
// becomes a RenderParams struct passed by value, vkCmdPushConstants +
// vkCmdDispatch become one kernel launch, and the per-batch fence wait becomes
// an explicit pt_synchronize / pt_read_accum.  Scene preparation that the
// device layout needs (threading the BVH, building triangle records) happens
// here once per upload.
#include <limits.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "pt_context.h"
#include "pt_cull.h"
#include "pt_denoise.h"
#include "pt_isect.h"
#include "pt_math.h"
#include "pt_plan.h"
#include "scene/small_sweep.h"
#include "scene/threaded_bvh.h"
#include "scene/wide_bvh.h"

namespace {

thread_local std::string g_err;   // pt_last_error(): its one definition (pt_fail_internal sets it)

// The threaded arrays of the exact walk (scene/threaded_bvh.h) as float4 pairs.
std::vector<float4> as_float4(const std::vector<float>& f) {
  std::vector<float4> v(f.size() / 4);
  if (!v.empty()) memcpy(v.data(), f.data(), v.size() * sizeof(float4));
  return v;
}

}  // namespace

// Pixels of columns [g0, g0+n) (or rows) whose NDC origin (the kernel's
// ndc = 2*p/res - 1) lies in [lo, hi].
static int pixels_in(int g0, int n, int res, float lo, float hi) {
  int k = 0;
  for (int i = 0; i < n; ++i) {
    const float v = (2.0f * (float)(g0 + i) / (float)res) - 1.0f;
    k += (v >= lo && v <= hi) ? 1 : 0;
  }
  return k;
}

// Live items are listed heaviest first (longest-processing-time order: the
// hardware dispatches workgroups in list order, so the long ones start early
// and the short ones fill the tail).  Weight = pixels inside the root box's
// rectangle (cull[0]: full paths, ~9 rays per sample on box.obj) x 8 + pixels
// inside a light rectangle (pre-pass only).  Output does not depend on the
// order; every consumer (launch, pack, unpack table) uses this one list.
// Every rank's share of the slotted partition (pt_device.h Part): the period's
// slots ordered by (k + 1/2) / slots[rank] for each rank's k-th slot (ties by
// rank), so every rank's slots are spread evenly over the period.
static std::vector<ptd::Part> parts_of_slots(const std::vector<int>& slots) {
  std::vector<std::pair<double, int>> seq;
  for (int i = 0; i < (int)slots.size(); ++i)
    for (int k = 0; k < slots[i]; ++k) seq.push_back({(k + 0.5) / slots[i], i});
  std::stable_sort(seq.begin(), seq.end());
  std::vector<ptd::Part> parts(slots.size(), ptd::Part{});
  for (auto& pt : parts) pt.m = (int)seq.size();
  for (int v = 0; v < (int)seq.size(); ++v) {
    ptd::Part& pt = parts[seq[v].second];
    pt.pos[pt.cnt++] = v;
  }
  return parts;
}
// Computed once per partition change (one sort of the period for all ranks)
// -- not per launch: at 8 ranks the per-call derivation cost ~10 us of host
// time per render launch.
static void ensure_parts(pt_context* c) {
  if (c->parts_valid && c->parts.size() == c->slots.size()) return;
  c->parts = parts_of_slots(c->slots);
  c->parts_valid = true;
  c->parts_synced = false;
}
const ptd::Part& part_of(pt_context* c, int r) {
  ensure_parts(c);
  return c->parts[r];
}

// Upload every rank's slot positions when the partition changed; the device
// copy of rank r's starts at d_parts + r * kMaxSlots.
static int upload_ints(const std::vector<int>& h, int** d, size_t* cap) {
  if (h.size() > *cap) {
    dev_free(*d);
    *cap = 0;
    PT_HIP(hipMalloc((void**)d, h.size() * sizeof(int)));
    *cap = h.size();
  }
  if (!h.empty()) PT_HIP(hipMemcpy(*d, h.data(), h.size() * sizeof(int), hipMemcpyHostToDevice));
  return PT_OK;
}
static int sync_parts(pt_context* c) {
  ensure_parts(c);
  if (c->parts_synced && c->d_parts) return PT_OK;
  std::vector<int> all((size_t)c->nranks * ptd::kMaxSlots, 0);
  for (int r = 0; r < c->nranks; ++r) {
    const ptd::Part& pt = c->parts[r];
    for (int i = 0; i < pt.cnt; ++i) all[(size_t)r * ptd::kMaxSlots + i] = pt.pos[i];
  }
  if (all == c->parts_key && c->d_parts) {
    c->parts_synced = true;
    return PT_OK;
  }
  { const int rc_ = quiesce(c); if (rc_) return rc_; }
  const int rc = upload_ints(all, &c->d_parts, &c->parts_cap);
  if (rc) return rc;
  c->parts_key = all;
  c->parts_synced = true;
  return PT_OK;
}

// The items (owned tile x sample-lane part) the render kernel would launch,
// split by the same float test its workgroups apply (render_kernel wg_live):
// those whose pixel rectangle can touch a cull rectangle go to the render
// kernel, the rest to fill_culled_kernel.  A culled workgroup still costs a
// workgroup launch (a fully culled 1080p frame took 0.10 ms at 4 sample
// lanes), so only live ones are launched.
void item_lists(const ptd::RenderParams& p, const ptd::Part& part, std::vector<int>* live,
                std::vector<int>* culled) {
  const int W = p.width, H = p.height, spl = p.spl, rows = 16 / spl;
  const int tiles = ptd::part_count(part, p.blocks_total);
  live->clear();
  culled->clear();
  std::vector<std::pair<int, int>> weighted;   // (-weight, item)
  for (int li = 0; li < tiles; ++li) {
    const int b = ptd::part_tile(part, li);
    int bx, by;
    ptd::tile_block(b, p.blocks_x, &bx, &by);
    const int gx0 = bx * 16;
    const float wx0 = (2.0f * (float)gx0 / (float)W) - 1.0f, wx1 = (2.0f * (float)(gx0 + 15) / (float)W) - 1.0f;
    int cols[ptd::kMaxCullRects] = {};
    for (int r = 0; r < p.n_cull; ++r) cols[r] = pixels_in(gx0, 16, W, p.cull[r][0], p.cull[r][1]);
    for (int part = 0; part < spl; ++part) {
      const int gy0 = by * 16 + part * rows;
      const float wy0 = (2.0f * (float)gy0 / (float)H) - 1.0f;
      const float wy1 = (2.0f * (float)(gy0 + rows - 1) / (float)H) - 1.0f;
      bool any = p.n_cull < 0;   // no culling: every item is live
      for (int r = 0; r < p.n_cull && !any; ++r)
        any = wx1 >= p.cull[r][0] && wx0 <= p.cull[r][1] && wy1 >= p.cull[r][2] && wy0 <= p.cull[r][3];
      if (!any) {
        culled->push_back(li * spl + part);
        continue;
      }
      int w = 0;
      for (int r = 0; r < p.n_cull; ++r)
        if (cols[r]) w += (r == 0 ? 8 : 1) * cols[r] * pixels_in(gy0, rows, H, p.cull[r][2], p.cull[r][3]);
      weighted.push_back({-w, li * spl + part});
    }
  }
  if (p.item_order)
    std::stable_sort(weighted.begin(), weighted.end(),
                   [](const std::pair<int, int>& a, const std::pair<int, int>& b) { return a.first < b.first; });
  live->reserve(weighted.size());
  for (const auto& e : weighted) live->push_back(e.second);
}

// Mixed sample lanes (PT_OPT_MIXED_LANES): the first `budget` live tiles
// whose every part is live, in list order, become whole-tile items at one lane
// per pixel; every other live part keeps p.spl lanes and follows them.  The
// whole tiles are the cheapest per sample (8 samples per lane, no colour
// hand-off) but the longest workgroups, so they start first and at most one
// round of them runs; the short parts then fill the launch's drain.
static void mixed_origins(const ptd::RenderParams& p, const ptd::Part& part, const std::vector<int>& live,
                          long long budget, std::vector<int>* org) {
  const int spl = p.spl, rows = 16 / spl;
  const int tiles = ptd::part_count(part, p.blocks_total);
  std::vector<int> parts_live(tiles, 0);
  for (int it : live) parts_live[it / spl]++;
  std::vector<char> whole(tiles, 0);
  long long k = 0;
  const int lg = __builtin_ctz((unsigned)spl);
  for (int it : live) {
    const int li = it / spl;
    if (k >= budget) break;
    if (whole[li] || parts_live[li] != spl) continue;
    whole[li] = 1;
    ++k;
    int bx, by;
    ptd::tile_block(ptd::part_tile(part, li), p.blocks_x, &bx, &by);
    org->push_back(bx * 16);   // log2(1) = 0 in the lane-count bits
    org->push_back(by * 16);
  }
  for (int it : live) {
    const int li = it / spl;
    if (whole[li]) continue;
    int bx, by;
    ptd::tile_block(ptd::part_tile(part, li), p.blocks_x, &bx, &by);
    org->push_back((bx * 16) | (lg << ptd::kMixShift));
    org->push_back(by * 16 + (it % spl) * rows);
  }
}

// Per-sample cost of 1, 2, 4 and 8 lanes per pixel relative to one lane:
// the box 1080p 8-spp frame with frames in flight (no drain), 0.2037 /
// 0.2121 / 0.2385 / 0.2775 ms per frame (profiles/r06b).
static const double kLaneInfl[4] = {1.0, 0.2121 / 0.2037, 0.2385 / 0.2037, 0.2775 / 0.2037};

// The measured schedule of mixed lanes.  cost[k], k = y / 4 * blocks_x +
// x / 16: the live work of the frame's 16x4 part k at one lane per pixel
// (render_kernel's cost feedback: every wave's duration added to the part
// its pixels lie in, divided by the lane factor it ran at).  A workgroup at s
// lanes lasts about the costliest part it covers * kLaneInfl[s] / s.
// Whole-live tiles run as 16x8 halves at kWholeLanes = 2 lanes -- the least
// work per sample whose workgroups fit inside a frame: at one lane the
// costliest tiles outlast the whole frame at two -- and the live parts of
// tiles with culled parts at p.spl lanes.  Every item goes longest first
// (longest-processing-time list scheduling on the measured costs), so the
// launch ends on its lightest items.  Box 1080p 8 spp, one context
// (profiles/r06h, r06i): 0.2214 ms per frame against 0.2416 at 4 lanes in
// the same order and 0.2349 for the best static mix (whole tiles at one lane
// for half the resident workgroups); whole tiles at one lane as well lost
// (0.2620: they outlast the frame), and so did splitting the last 5-35 % of
// the work into 4-lane parts for a finer drain (+1 to +5 %).  Any item order
// and lane count gives the same image.
struct MixItem {
  int x, y;
  double dur;
};
constexpr int kWholeLanes = 2;
static void measured_origins(const ptd::RenderParams& p, const ptd::Part& part, const std::vector<int>& live,
                             const std::vector<double>& cost, std::vector<int>* org) {
  const int spl = p.spl, rows = 16 / spl, lg_base = __builtin_ctz((unsigned)spl);
  const int lanes = std::min(kWholeLanes, spl), lg_whole = __builtin_ctz((unsigned)lanes), hrows = 16 / lanes;
  const int tiles = ptd::part_count(part, p.blocks_total);
  std::vector<int> parts_live(tiles, 0);
  for (int it : live) parts_live[it / spl]++;
  auto part_cost = [&](int x, int y) {   // pixel (x, y)'s 16x4 part
    const size_t k = (size_t)(y >> 2) * p.blocks_x + (x >> 4);
    return k < cost.size() ? std::max(1.0, cost[k]) : 1.0;
  };
  auto span_cost = [&](int x, int y, int nrows) {   // the costliest 16x4 part of rows [y, y + nrows)
    double c = 0;
    for (int yy = y; yy < y + std::max(nrows, 4); yy += 4) c = std::max(c, part_cost(x, yy));
    return c;
  };
  std::vector<char> seen(tiles, 0);
  std::vector<MixItem> items;
  for (int it : live) {
    const int li = it / spl;
    int bx, by;
    ptd::tile_block(ptd::part_tile(part, li), p.blocks_x, &bx, &by);
    const int x = bx * 16, y = by * 16;
    if (parts_live[li] == spl) {   // a whole-live tile: its halves, once
      if (seen[li]) continue;
      seen[li] = 1;
      for (int h = 0; h < lanes; ++h)
        items.push_back({x | (lg_whole << ptd::kMixShift), y + h * hrows,
                         span_cost(x, y + h * hrows, hrows) * kLaneInfl[lg_whole] / lanes});
      continue;
    }
    const int yp = y + (it % spl) * rows;
    items.push_back({x | (lg_base << ptd::kMixShift), yp, span_cost(x, yp, rows) * kLaneInfl[lg_base] / spl});
  }
  std::stable_sort(items.begin(), items.end(), [](const MixItem& a, const MixItem& b) { return a.dur > b.dur; });
  for (const MixItem& m : items) {
    org->push_back(m.x);
    org->push_back(m.y);
  }
  if (const char* dump = getenv("PT_MIX_DUMP")) {   // diagnostics: the chosen schedule and its predicted durations
    if (FILE* f = fopen(dump, "w")) {
      fprintf(f, "# items %zu\n", items.size());
      for (const MixItem& m : items)
        fprintf(f, "I %d %d %d %.1f\n", m.x & ((1 << ptd::kMixShift) - 1), m.y, m.x >> ptd::kMixShift, m.dur);
      fclose(f);
    }
  }
}

// Cost feedback of the measured mixed-lane schedule (PT_OPT_MIXED_LANES -1).
// The schedule belongs to the frame's inputs (the cost key: size, batches,
// lanes, camera, params, scene and lights, culling).  Once the key has held
// for a render, one launch records its blocks' costs (render_kernel adds
// every wave's duration on the GPU wall clock to its block), copied back
// asynchronously behind an event; a later render whose event has completed
// folds them in, divided by the lane factor each block ran at, and after
// kCostFrames such launches the schedule is built from them
// (measured_origins).  The host never waits: a render whose copy has not
// landed keeps the static schedule.
constexpr int kCostFrames = 2;
static int mix_feedback(pt_context* c, const ptd::RenderParams& p, uint32_t n_batches) {
  std::vector<float>& key = c->cost_scratch;
  key.assign({(float)p.width, (float)p.height, (float)n_batches, (float)(p.first_batch == 0), (float)p.spl,
              (float)c->params.max_depth, (float)c->params.sss_bounces, (float)c->scene_serial, (float)p.n_cull,
              (float)c->opt_item_order});
  key.insert(key.end(), c->cam, c->cam + 16);
  for (int r = 0; r < p.n_cull; ++r) key.insert(key.end(), p.cull[r], p.cull[r] + 4);
  const size_t nb = (size_t)p.blocks_total;
  const size_t np4 = (size_t)p.blocks_x * (size_t)((p.height + 15) / 16) * 4;   // 16x4 parts
  if (key != c->cost_key) {
    c->cost_key = key;
    c->cost_stable = 0;
    c->cost_frames = 0;
    c->cost_ready = false;
    c->cost_measure = false;
    c->cost_stale = c->cost_pending;   // a copy in flight belongs to the old inputs
    c->block_cost.assign(np4, 0.0);
  }
  if (c->cost_pending && hipEventQuery(c->cost_ev) == hipSuccess) {
    c->cost_pending = false;
    if (!c->cost_stale && c->cost_lanes.size() == nb) {
      for (size_t k = 0; k < np4; ++k) {   // part k lies in block (k / blocks_x / 4, k % blocks_x)
        const size_t b = (k / (size_t)p.blocks_x / 4) * (size_t)p.blocks_x + k % (size_t)p.blocks_x;
        const int s = c->cost_lanes[b];
        if (s > 0) c->block_cost[k] += (double)c->h_cost[k] / kLaneInfl[__builtin_ctz((unsigned)s)];
      }
      if (++c->cost_frames >= kCostFrames) {
        for (double& x : c->block_cost) x /= c->cost_frames;
        c->cost_ready = true;
        c->cost_gen++;
      }
    }
    c->cost_stale = false;
  }
  c->cost_stable++;
  c->cost_measure = false;
  if (!c->cost_ready && !c->cost_pending && c->cost_stable >= 2) {
    if (c->cost_n < np4) {
      dev_free(c->d_cost);
      if (c->h_cost) (void)hipHostFree(c->h_cost);
      c->h_cost = nullptr;
      c->cost_n = 0;
      PT_HIP(hipMalloc((void**)&c->d_cost, np4 * sizeof(unsigned)));
      PT_HIP(hipHostMalloc((void**)&c->h_cost, np4 * sizeof(unsigned), hipHostMallocDefault));
      c->cost_n = np4;
    }
    if (!c->cost_ev) PT_HIP(hipEventCreateWithFlags(&c->cost_ev, hipEventDisableTiming));
    c->cost_measure = true;
  }
  return PT_OK;
}

// How a launch mixes lane counts (cull_and_items): PT_OPT_MIXED_LANES k > 0, a
// static budget of whole tiles (mixed_origins); -1, uniform lanes until the
// part costs are measured, then the measured schedule (measured_origins).
struct MixPlan {
  long long budget = 0;                       // whole tiles of the static schedule
  const std::vector<double>* cost = nullptr;  // measured part costs, or null
  int gen = 0;                                // measured schedule generation (cache key)
};

static int compact_items(pt_context* c, ptd::RenderParams* p, const MixPlan* mix = nullptr) {
  const long long mix_budget = mix ? (mix->cost ? -1 - mix->gen : mix->budget) : 0;
  const ptd::Part& pt = part_of(c, p->rank);
  // every slot position of this rank's share: two slot sets with the same
  // period, count and first position still deal different tiles
  std::vector<float>& key = c->items_scratch;
  key.assign({(float)p->width, (float)p->height, (float)pt.m, (float)pt.cnt, (float)p->rank, (float)p->spl,
              (float)p->n_cull, (float)p->item_order, (float)mix_budget});
  for (int k = 0; k < pt.cnt; ++k) key.push_back((float)pt.pos[k]);
  for (int r = 0; r < p->n_cull; ++r) key.insert(key.end(), p->cull[r], p->cull[r] + 4);
  if (key.size() != c->items_key.size() || memcmp(key.data(), c->items_key.data(), key.size() * 4) != 0) {
    std::vector<int> live, culled;
    item_lists(*p, pt, &live, &culled);
    { const int rc_ = quiesce(c); if (rc_) return rc_; }   // the previous list may still be in use
    // live items, culled items, then (8-B aligned) each culled item's first
    // pixel {x, y} for the fill (fill_culled: no tile arithmetic per pixel)
    c->h_items = live;
    c->h_items.insert(c->h_items.end(), culled.begin(), culled.end());
    if (c->h_items.size() & 1) c->h_items.push_back(0);
    const int rows = 16 / p->spl;
    auto origins = [&](const std::vector<int>& list) {
      for (int it : list) {
        int bx, by;
        ptd::tile_block(ptd::part_tile(pt, it / p->spl), p->blocks_x, &bx, &by);
        c->h_items.push_back(bx * 16);
        c->h_items.push_back(by * 16 + (it % p->spl) * rows);
      }
    };
    c->culled_org_off = c->h_items.size();
    origins(culled);
    c->live_org_off = c->h_items.size();
    int n_launch = (int)live.size();
    if (mix && (mix->cost || (p->spl > 1 && mix->budget > 0))) {
      std::vector<int> org;
      if (mix->cost)
        measured_origins(*p, pt, live, *mix->cost, &org);
      else
        mixed_origins(*p, pt, live, mix->budget, &org);
      c->h_items.insert(c->h_items.end(), org.begin(), org.end());
      n_launch = (int)(org.size() / 2);
    } else {
      origins(live);
    }
    const int ru = upload_ints(c->h_items, &c->d_items, &c->items_cap);
    if (ru) return ru;
    c->n_live_items = n_launch;
    c->n_culled_items = (int)culled.size();
    c->items_mixed = mix && (mix->cost || (p->spl > 1 && mix->budget > 0));
    // the lane count each block's workgroups run at (cost feedback)
    c->block_lanes.assign((size_t)p->blocks_total, 0);
    for (size_t k = 0; k + 1 < c->h_items.size() - c->live_org_off; k += 2) {
      const int ox = c->h_items[c->live_org_off + k], oy = c->h_items[c->live_org_off + k + 1];
      c->block_lanes[(size_t)(oy >> 4) * p->blocks_x + ((ox & ((1 << ptd::kMixShift) - 1)) >> 4)] =
          c->items_mixed ? 1 << (ox >> ptd::kMixShift) : p->spl;
    }
    c->items_key = key;
  }
  p->items = c->d_items;
  p->n_items = c->n_live_items;
  p->mix = c->items_mixed ? 1 : 0;
  p->culled_org = (const int2*)(c->d_items + c->culled_org_off);
  p->items_org = (const int2*)(c->d_items + c->live_org_off);
  p->n_culled_items = c->n_culled_items;
  return PT_OK;
}

// The frame parameters an item layout depends on, into *key (its capacity is
// kept between launches: no allocation per launch).
void frame_key(const pt_context* c, const ptd::RenderParams& p, std::vector<float>* key) {
  key->assign({(float)p.width, (float)p.height, (float)p.nranks, (float)p.rank, (float)p.spl, (float)p.n_cull,
               (float)p.blocks_x, (float)p.blocks_total, (float)p.item_order});
  for (int r = 0; r < p.n_cull; ++r) key->insert(key->end(), p.cull[r], p.cull[r] + 4);
  for (int sl : c->slots) key->push_back((float)sl);   // every rank's share (the assembly table)
}

// The root's assembly table for frames rendered with params p: per rank its
// live items {rank, x0, y0, slot} and its culled items {rank, x0, y0, -1},
// (x0, y0) the item's first pixel.
int unpack_table(pt_context* c, const ptd::RenderParams& p, const std::vector<float>& key) {
  if (key == c->unpack_key) return PT_OK;
  std::vector<int> table, live, culled;
  for (int r = 0; r < p.nranks; ++r) {
    const ptd::Part pt = part_of(c, r);
    item_lists(p, pt, &live, &culled);
    // {rank, x0, y0, slot} (unpack_pixel)
    auto add = [&](int item, int slot) {
      int bx, by;
      ptd::tile_block(ptd::part_tile(pt, item / p.spl), p.blocks_x, &bx, &by);
      table.insert(table.end(), {r, bx * 16, by * 16 + (item % p.spl) * (16 / p.spl), slot});
    };
    for (size_t i = 0; i < live.size(); ++i) add(live[i], (int)i);
    for (int it : culled) add(it, -1);
  }
  std::vector<int> live_only;
  for (size_t k = 0; k + 3 < table.size(); k += 4)
    if (table[k + 3] >= 0) live_only.insert(live_only.end(), table.begin() + k, table.begin() + k + 4);
  { const int rc_ = quiesce(c); if (rc_) return rc_; }
  const int rc = upload_ints(table, &c->d_unpack, &c->unpack_cap);
  if (rc) return rc;
  const int rl = upload_ints(live_only, &c->d_unpack_live, &c->unpack_live_cap);
  if (rl) return rl;
  c->n_unpack = (int)(table.size() / 4);
  c->n_unpack_live = (int)(live_only.size() / 4);
  c->unpack_key = key;
  return PT_OK;
}
// Wavefront buffers for `paths` paths in one allocation.  Up to 2^27 paths
// (416 B each: 56 GB of the 288-GB HBM) are kept per launch, so config 4's
// 4K x 16 spp frame (133M paths) runs as one chunk: every ray round has 8x
// the rays of a 2^24 chunk, and each round's drain (its longest walk) is paid
// 65 times per frame instead of 520 -- 767 -> 560 ms (2^26: 591).  More
// batches run in chunks of that size; an allocation that fails halves it.
constexpr long long kWfMaxPaths = 1ll << 27;
static int wf_reserve(pt_context* c, long long pixels, uint32_t batches, long long* chunk_paths) {
  const long long limit = c->opt_wf_paths > 0 ? c->opt_wf_paths : kWfMaxPaths;
  long long want = std::max(pixels, std::min(pixels * (long long)batches, limit));
  if (c->wf_fail > 0) want = std::max(pixels, std::min(want, c->wf_fail / 2));   // an earlier allocation failed
  if (want > 0x7fffffffll) return fail(PT_ERR_UNSUPPORTED, "frame too large for the wavefront kernel");
  *chunk_paths = want;
  if (want <= c->wf.cap) return PT_OK;
  { const int rc_ = quiesce(c); if (rc_) return rc_; }
  dev_free(c->wf_block);
  c->wf = ptd::WfBuffers{};
  char* base = nullptr;
  size_t n = 0, b_state = 0, b_col = 0, b_rays = 0, b_ids = 0, b_hits = 0;
  for (;;) {
    n = (size_t)want;
    b_state = n * ptd::kWfStateF4 * 16, b_col = n * 16, b_rays = n * 32, b_ids = n * 4, b_hits = n * 8;
    const hipError_t e = hipMalloc((void**)&base, 2 * b_state + b_col + 2 * (b_rays + b_ids) + b_hits + 64);
    if (e == hipSuccess) break;
    (void)hipGetLastError();
    if (e != hipErrorOutOfMemory || want <= pixels) PT_HIP(e);
    c->wf_fail = want;
    want = std::max(pixels, want / 2);   // less memory than that: smaller chunks
  }
  *chunk_paths = want;
  c->wf_block = base;
  char* q = base;
  c->wf.state[0] = (float4*)q; q += b_state;
  c->wf.state[1] = (float4*)q; q += b_state;
  c->wf.colors = (float4*)q;   q += b_col;
  c->wf.rays[0] = (float4*)q;  q += b_rays;
  c->wf.rays[1] = (float4*)q;  q += b_rays;
  c->wf.hits = (float2*)q;     q += b_hits;
  c->wf.ids[0] = (int*)q;      q += b_ids;
  c->wf.ids[1] = (int*)q;      q += b_ids;
  c->wf.counters = (int*)q;
  c->wf.cap = want;
  return PT_OK;
}

// The camera block and the frame main() derives from it (:447-448, :457),
// computed on the host with pt_math.h.
void camera_params(const float cam[16], ptd::RenderParams* p) {
  const ptdn::CamBasis b = ptdn::cam_basis(cam);
  for (int i = 0; i < 3; ++i) {
    p->cam_pos[i] = cam[i];
    p->cam_dir[i] = cam[4 + i];
    p->cam_up[i] = cam[8 + i];
  }
  p->fov = cam[12];
  p->cam_right[0] = b.right.x; p->cam_right[1] = b.right.y; p->cam_right[2] = b.right.z;
  p->cam_upv[0] = b.up.x; p->cam_upv[1] = b.up.y; p->cam_upv[2] = b.up.z;
  p->tan_fov = b.tan_fov;
}

// The culled wide walk's arrays for a launch, its per-lane stack overflow
// areas (re)allocated first when the grid or the scene's stack bound outgrew
// them.
int wide_params(pt_context* c, ptd::RenderParams* p) {
  const long long lanes = ptd::wide_trace_lanes();
  if (lanes <= 0) return fail(PT_ERR_HIP, "wide walk: occupancy query failed");
  const int stack = c->wide_stack;
  if (lanes > c->wide_ovf_lanes || stack > c->wide_ovf_stack) {   // every lane of the grid gets its area
    { const int rc_ = quiesce(c); if (rc_) return rc_; }
    dev_free(c->d_wide_ovf);
    c->wide_ovf_lanes = 0;
    // two sets: the two halves of a chunk trace concurrently (launch_wavefront)
    PT_HIP(hipMalloc((void**)&c->d_wide_ovf, 2 * (size_t)lanes * (size_t)stack * sizeof(int2)));
    c->wide_ovf_lanes = lanes;
    c->wide_ovf_stack = stack;
  }
  // closest hits come back as leaf ranks
  p->wide_qn = wide_layout_qn(*c);
  p->wide = p->wide_qn ? c->d_wide_q : c->d_wide;
  p->wide_leafbox = c->d_wide_leafbox;
  p->wide_tris = c->d_wide_tris;
  p->wide_rank_of = c->d_wide_rank_of;
  p->hit_tris = c->d_wide_tris;
  p->wide_ovf = c->d_wide_ovf;
  p->wide_ovf_lanes = c->wide_ovf_lanes;
  p->wide_stack = stack;
  return PT_OK;
}

// ---- a render, step by step (render_impl below puts them in order) ------------------------------

// The launch-timing ring (PT_OPT_LAUNCH_TIMING): an event pair around every
// k-th render launch, render_impl's and relaunch's alike.
struct LaunchTimer {
  int slot = 0;
  bool timed = false;
};
static int timing_begin(pt_context* c, LaunchTimer* t) {
  t->slot = c->ring_n % pt_context::kRing;
  t->timed = c->opt_timing > 0 && c->launch_n % c->opt_timing == 0;
  if (t->timed) PT_HIP(hipEventRecord(c->ring[t->slot][0], c->stream));
  return PT_OK;
}
static int timing_end(pt_context* c, const LaunchTimer& t) {
  if (t.timed) {
    PT_HIP(hipEventRecord(c->ring[t.slot][1], c->stream));
    c->ring_launch[t.slot] = c->launch_n;
    c->last_slot = t.slot;
    c->ring_n++;
    c->timed = true;
  }
  c->launch_n++;
  return PT_OK;
}

// One path-recursive launch of prepared parameters, timed as render_impl
// times its launches.
int relaunch(pt_context* c, const ptd::RenderParams& p, bool lds, bool cnt) {
  LaunchTimer timer;
  { const int rc = timing_begin(c, &timer); if (rc) return rc; }
  PT_HIP(ptd::launch_render(p, false, lds, c->stream, cnt));
  return timing_end(c, timer);
}

static int render_ready(const pt_context* c) {
  if (!c) return fail(PT_ERR_INVALID, "null context");
  if (!c->has_scene) return fail(PT_ERR_INVALID, "no scene uploaded");
  if (!c->has_camera) return fail(PT_ERR_INVALID, "no camera set");
  if (!c->d_accum) return fail(PT_ERR_INVALID, "no accumulation buffer");
  return PT_OK;
}

// PT_OPT_MOMENTS: the launches of a render fold the luminance moments too; the image counts as valid
// (batches 0..n-1, in order) when this render starts at 0 or continues at n.  What the option refuses
// (a packed render, a partition, stats mode, counting) the plan has refused already.
struct Moments {
  bool fold = false, cont = false;
};
static int moments_open(pt_context* c, uint32_t first_batch, uint32_t n_batches, bool packed, Moments* m) {
  if (!c->opt_moments) {
    if (n_batches > 0 && !packed) c->moments_valid = false;   // the accumulator moves on without them
    return PT_OK;
  }
  if (n_batches == 0) return PT_OK;
  const size_t n = (size_t)c->width * c->height;
  if (!c->d_moments || c->moments_cap < n) {
    c->moments_valid = false;
    PT_HIP(hipSetDevice(c->device));
    const int rg = grow_dev(c, &c->d_moments, &c->moments_cap, n);
    if (rg) return rg;
    PT_HIP(hipMemsetAsync(c->d_moments, 0, n * sizeof(float2), c->stream));
  }
  m->fold = true;
  m->cont = first_batch == 0 || (c->moments_valid && first_batch == c->moments_n);
  c->moments_valid = false;   // until the launch is enqueued
  return PT_OK;
}
static void moments_close(pt_context* c, const Moments& m, uint32_t first_batch, uint32_t n_batches) {
  if (!m.fold) return;
  c->moments_valid = m.cont;
  c->moments_n = m.cont ? first_batch + n_batches : 0;
}

// The scene, frame and camera fields of a launch's parameters: all that the guide's launch takes
// (pt_render_guide).  full_nodes: every reference node (stats mode).
void frame_params(const pt_context* c, bool full_nodes, ptd::RenderParams* p) {
  p->nodes = full_nodes ? c->d_nodes_full : c->d_nodes;
  p->n_nodes = full_nodes ? c->n_nodes_full : c->n_nodes;
  p->tris = c->d_tris;
  p->hit_tris = c->d_tris;
  p->n_tris = c->n_tris;
  p->width = c->width;
  p->height = c->height;
  camera_params(c->cam, p);
  p->blocks_x = (c->width + 15) / 16;
  p->blocks_total = p->blocks_x * ((c->height + 15) / 16);
}

// ... and what a render adds: lights and buffers, the batches, what the plan chose, this rank's partition
// (uploaded here when it changed).
static int render_params(pt_context* c, const LaunchPlan& plan, uint32_t first_batch, uint32_t n_batches, bool packed,
                         ptd::RenderParams* p) {
  p->wf_grid = c->opt_wf_grid;
  p->wide_refill = plan.wide_refill;
  p->lights = c->d_lights_dev;
  p->accum = c->d_accum;
  p->stats = c->d_stats;
  p->n_lights = c->n_lights;
  p->first_batch = first_batch;
  p->n_batches = n_batches;
  p->seed_base = c->opt_seed_base + c->seed_extra;   // PT_OPT_SEED_BASE (mod 2^32)
  p->max_depth = c->params.max_depth;
  p->sss_bounces = c->params.sss_bounces;
  p->exit_skip = plan.exit_skip;
  memcpy(p->root_lo, c->root_lo, sizeof p->root_lo);
  memcpy(p->root_hi, c->root_hi, sizeof p->root_hi);
  p->nranks = c->nranks;
  p->rank = c->rank;
  const ptd::Part& hpart = part_of(c, c->rank);
  {
    const int rc = sync_parts(c);
    if (rc) return rc;
  }
  p->part_m = hpart.m;
  p->part_cnt = hpart.cnt;
  p->part_pos = c->d_parts + (size_t)c->rank * ptd::kMaxSlots;
  p->n_tiles = ptd::part_count(hpart, p->blocks_total);
  p->fresh = packed ? 1 : c->opt_fresh;
  p->spl = plan.spl;
  if (plan.sweep) {
    p->sweep = c->opt_sweep_hull ? c->d_sweep : c->d_sweep_plain;
    p->sweep_hull = plan.sweep_hull;
    p->sweep_boxes = c->sweep_boxes;
    p->sweep_leaves = c->sweep_leaves;
    if (plan.sweep_cube) {   // the straight-line walk's table: the root box is root_lo / root_hi above
      p->sweep_cube = 1;
      memcpy(p->cube_under, c->cube_under, sizeof p->cube_under);
      p->cube_all = c->cube_all;
    }
  }
  p->item_order = plan.item_order;
  return PT_OK;
}

// The cull rectangles of the frame (stats mode derives none), loose and tight.
static void cull_rectangles(const pt_context* c, ptd::RenderParams* p) {
  p->n_cull = -1;
  if (c->opt_cull && !c->stats_mode)
    p->n_cull = ptd::cull_rects(c->cam, c->width, c->height, c->root_lo, c->root_hi, c->lights_host.data(),
                                c->n_lights, &p->cull[0][0], ptd::kMaxCullRects);
  // the tight rectangles (PT_OPT_CULL_TIGHT): the kernel's per-sample skip; every host-side use of the
  // rectangles (items, fills, partitions) keeps the loose ones.  Off (-1, "never skip") unless both derive
  p->n_cull_tight = -1;
  p->cull_u0 = ptd::kCullTightU0;
  if (p->n_cull >= 0 && c->opt_cull_tight) {
    p->n_cull_tight = ptd::cull_rects(c->cam, c->width, c->height, c->root_lo, c->root_hi, c->lights_host.data(),
                                      c->n_lights, &p->cull_tight[0][0], ptd::kMaxCullRects, ptd::kCullTightR);
    if (p->n_cull_tight != p->n_cull) p->n_cull_tight = -1;
  }
  p->n_foot = 0;
  p->n_sure = 0;
  p->foot = nullptr;
}

// The footprint table of the frame (PT_OPT_CULL_FOOTPRINT) into table[2][kMaxCullRects][kFootprintFloats]: the
// footprints, one per tight rectangle, then the lights' sure regions.  Returns how many footprints are in
// force, or 0: the rectangles decide; *n_sure: the lights that have a region in the table (0: none has a
// non-empty one), *sure_regions: the non-empty ones.  The counting pass keeps the rectangles unless the
// option is 1.
constexpr size_t kFootTable = 2 * (size_t)ptd::kMaxCullRects * ptd::kFootprintFloats;
static_assert(ptd::kMaxCullObjects == ptd::kMaxCullRects, "pt_cull.h's bound is pt_device.h's");
static int cull_footprint_table(const pt_context* c, const ptd::RenderParams& p, float* table, int* n_sure,
                                int* sure_regions) {
  *n_sure = *sure_regions = 0;
  const bool counting = c->opt_count != 0 && !c->stats_mode;
  if (p.n_cull_tight < 1 || c->opt_cull_foot == 0 || (c->opt_cull_foot < 0 && counting)) return 0;
  const int n = ptd::cull_footprints(c->cam, c->width, c->height, c->root_lo, c->root_hi, c->lights_host.data(),
                                     c->n_lights, table, ptd::kMaxCullRects, ptd::kCullTightR);
  if (n != p.n_cull_tight) return 0;
  const int ns = ptd::cull_sure(c->cam, c->width, c->height, c->root_lo, c->root_hi, c->lights_host.data(), c->n_lights,
                                table + ptd::kMaxCullRects * ptd::kFootprintFloats, ptd::kMaxCullRects, ptd::kCullTightR);
  if (ns > 0) {
    *n_sure = c->n_lights;
    *sure_regions = ns;
  }
  return n;
}

// ... and into the context's table in device memory, which the kernels read (RenderParams::foot): uploaded
// when it differs from what the table holds, after the launches that may still read it.
static int cull_footprints(pt_context* c, ptd::RenderParams* p) {
  static_assert(sizeof(c->foot_up) == kFootTable * sizeof(float), "pt_context::foot_up");
  float table[kFootTable] = {};
  int n_sure = 0, regions = 0;
  const int n = cull_footprint_table(c, *p, table, &n_sure, &regions);
  if (n == 0) return PT_OK;
  if (!c->d_foot || memcmp(table, c->foot_up, sizeof(table)) != 0) {
    { const int rc_ = quiesce(c); if (rc_) return rc_; }
    PT_HIP(hipSetDevice(c->device));
    if (!c->d_foot) PT_HIP(hipMalloc((void**)&c->d_foot, sizeof(table)));
    PT_HIP(hipMemcpy(c->d_foot, table, sizeof(table), hipMemcpyHostToDevice));
    memcpy(c->foot_up, table, sizeof(table));
  }
  p->n_foot = n;
  p->n_sure = n_sure;
  p->foot = c->d_foot;
  return PT_OK;
}

// The cull rectangles and the item lists of the frame; mixed lanes where the plan admits them and the
// frame has rectangles.  (Stats mode derives no rectangles, so its launches never mix lanes.)
static int cull_and_items(pt_context* c, const LaunchPlan& plan, uint32_t n_batches, ptd::RenderParams* p) {
  c->last_mix = 0;
  cull_rectangles(c, p);
  if (p->n_cull < 0) return PT_OK;
  { const int rc = cull_footprints(c, p); if (rc) return rc; }
  MixPlan mix;
  const bool mixed = plan.mixed_eligible;
  if (mixed) {
    const size_t lds_b = plan.sweep ? ptd::sweep_lds_bytes(*p) : ptd::scene_lds_bytes(*p);
    if (c->render_slots < 0 || c->render_slots_lds != lds_b || c->render_slots_sweep != plan.sweep) {
      c->render_slots_sweep = plan.sweep;
      c->render_slots = ptd::render_slots(lds_b, plan.sweep);
      c->render_slots_lds = lds_b;
    }
    // auto: every item at PT_OPT_SAMPLE_LANES until the block costs are
    // measured -- the measuring launches then run a uniform schedule, whose
    // workgroups nearly all run at full occupancy (a mixed one measured its
    // drain's parts at low occupancy, too short: profiles/r06g)
    mix.budget = c->opt_mixed > 0 ? std::max(1ll, c->render_slots * c->opt_mixed / 100) : 0;
    if (c->opt_mixed < 0) {
      const int rm = mix_feedback(c, *p, n_batches);
      if (rm) return rm;
      if (c->cost_ready) {
        mix.cost = &c->block_cost;
        mix.gen = c->cost_gen;
      }
    }
  }
  const int rc = compact_items(c, p, mixed ? &mix : nullptr);
  if (rc) return rc;
  c->last_mix = !mixed || !c->items_mixed ? 0 : mix.cost ? 2 : 1;
  if (mixed && c->opt_mixed < 0 && c->cost_measure) {
    // this launch measures its blocks' costs (mix_feedback)
    PT_HIP(hipMemsetAsync(c->d_cost, 0, (size_t)p->blocks_total * 4 * sizeof(unsigned), c->stream));
    p->cost_out = c->d_cost;
    c->cost_lanes = c->block_lanes;
  }
  return PT_OK;
}

// Culled items written once (culled_state): a launch whose culled items
// already hold (0,0,0,1) in this buffer under this item layout -- a fold of
// (0,0,0,1) samples into (0,0,0,1) is (0,0,0,1), whatever the batch --
// skips their fill workgroups (23 MB of writes per box 1080p frame).
// culled_before says whether the launch fills culled items of the accumulation
// buffer at all and skips the fill where it can; culled_after records what
// they hold once the launch is enqueued.
struct Culled {
  bool launch = false, skipped = false;
};
static bool culled_hold(const pt_context* c) {
  return c->culled_state == 2 && c->culled_buf == c->d_accum && c->culled_key == c->items_key;
}
static Culled culled_before(pt_context* c, ptd::RenderParams* p, bool packed, uint32_t n_batches) {
  Culled cu;
  cu.launch = p->n_cull >= 0 && p->items && !packed && !c->stats_mode && n_batches > 0;
  if (cu.launch && culled_hold(c)) {
    p->n_culled_items = 0;
    cu.skipped = true;
  }
  return cu;
}
static void culled_after(pt_context* c, const Culled& cu, bool packed, bool fresh, uint32_t first_batch,
                         uint32_t n_batches) {
  if (cu.launch && !cu.skipped) {
    const bool exact = (fresh && first_batch == 0) || culled_hold(c) ||
                       (first_batch == 0 && c->culled_state == 1 && c->culled_buf == c->d_accum);
    c->culled_state = exact ? 2 : 0;
    c->culled_key = c->items_key;
    c->culled_buf = c->d_accum;
  } else if (!cu.launch && !packed && n_batches > 0) {
    c->culled_state = 0;   // every pixel rendered (no culling, stats mode): not tracked
  }
}

// pt_render_packed's optional assembly of a gathered frame by the launch's trailing workgroups.
static int assembly_params(pt_context* c, const Assembly& as, ptd::RenderParams* p) {
  if (!as.src) return PT_OK;
  const int rc = unpack_table(c, *p, c->key_scratch);
  if (rc) return rc;
  p->unpack_src = (const float4*)as.src;
  p->unpack_frame = (float4*)as.frame;
  p->unpack_table = c->d_unpack;
  p->n_unpack = c->n_unpack;
  p->unpack_slot_f4 = (long long)(as.slot_floats / 4);
  return PT_OK;
}

// The wavefront pipeline's launch: its path buffers, the wide walk's arrays where the plan walks them,
// the second stream on first use.
static int launch_wf(pt_context* c, const LaunchPlan& plan, uint32_t n_batches, ptd::RenderParams* p) {
  const long long tiles = p->n_tiles;
  const long long items = p->items ? p->n_items : tiles * p->spl;
  long long chunk_paths = 0;
  const int rc = wf_reserve(c, items * (256 / p->spl), n_batches, &chunk_paths);
  if (rc) return rc;
  ptd::WfBuffers b = c->wf;
  b.cap = chunk_paths;   // paths per chunk (the allocation may be larger)
  if (plan.wide) {
    const int rw = wide_params(c, p);
    if (rw) return rw;
    p->wide_handback = plan.wide_handback;
    p->wf_fuse = plan.wf_fuse;
    p->wf_tail = plan.wf_tail;
  }
  if (plan.two_streams && !c->wf_stream2) {
    PT_HIP(hipStreamCreateWithFlags(&c->wf_stream2, hipStreamNonBlocking));
    PT_HIP(hipEventCreateWithFlags(&c->wf_fork, hipEventDisableTiming));
    PT_HIP(hipEventCreateWithFlags(&c->wf_join, hipEventDisableTiming));
  }
  PT_HIP(ptd::launch_wavefront(*p, b, plan.lds, c->stream, plan.cnt, plan.two_streams ? c->wf_stream2 : nullptr,
                               c->wf_fork, c->wf_join));
  return PT_OK;
}

// The path-recursive launch, the read-back of a measuring launch's costs (mix_feedback), and the
// parameters pt_dist_run relaunches.
static int launch_recursive(pt_context* c, const LaunchPlan& plan, const ptd::RenderParams& p, Launched* launched) {
  PT_HIP(ptd::launch_render(p, c->stats_mode, plan.lds, c->stream, plan.cnt));
  if (p.cost_out) {
    PT_HIP(hipMemcpyAsync(c->h_cost, c->d_cost, (size_t)p.blocks_total * 4 * sizeof(unsigned), hipMemcpyDeviceToHost,
                          c->stream));
    PT_HIP(hipEventRecord(c->cost_ev, c->stream));
    c->cost_pending = true;
    c->cost_measure = false;
  }
  if (launched && p.pack_out && !c->stats_mode) {
    launched->p = p;
    launched->lds = plan.lds;
    launched->cnt = plan.cnt;
    launched->valid = true;
  }
  return PT_OK;
}

// pt_render_packed on the wavefront pipeline, whose kernels render into the
// accumulation buffer: assemble the previous frame in a launch of its own,
// render a fresh frame from batch 0 as pt_render would (p is that render's too:
// a packed frame is fresh, and neither mixes lanes), then pack it.
static int render_packed_wavefront(pt_context* c, const LaunchPlan& plan, ptd::RenderParams p, uint32_t n_batches,
                                   float4* pack_out, const Assembly& as) {
  // (the calls below rebuild c->key_scratch: keep this frame's key)
  const std::vector<float> frame_k = c->key_scratch;
  if (as.src) {
    const int rc = pt_items_unpack_all(c, as.src, as.slot_floats, as.frame);
    if (rc) return rc;
  }
  if (n_batches > 0) c->moments_valid = false;   // the accumulator moves on without them
  LaunchTimer timer;   // the pair opens after the assembly
  { const int rc = timing_begin(c, &timer); if (rc) return rc; }
  const Culled culled = culled_before(c, &p, false, n_batches);
  { const int rc = order_shared(c); if (rc) return rc; }
  { const int rc = launch_wf(c, plan, n_batches, &p); if (rc) return rc; }
  { const int rc = mark_shared(c); if (rc) return rc; }
  { const int rc = timing_end(c, timer); if (rc) return rc; }
  culled_after(c, culled, false, true, 0, n_batches);
  c->packed_key = frame_k;
  const int rp = pt_items_pack(c, pack_out);
  if (rp) return rp;
  return mark_shared(c);   // the pack read the accumulation buffer
}

// pt_render / pt_render_packed (pack_out != null: fresh frame, live items
// written to pack_out in the pt_items_pack layout).
int render_impl(pt_context* c, uint32_t first_batch, uint32_t n_batches, float4* pack_out, const Assembly& as,
                Launched* launched) {
  { const int rc = render_ready(c); if (rc) return rc; }
  adaptive_forget(c);   // an ordinary render ends an adaptive one
  const bool packed = pack_out != nullptr;
  ptd::RenderParams p{};   // what is not set below is 0 or null: no wide walk, item list, packed output, assembly
  frame_params(c, c->stats_mode, &p);
  const LaunchPlan plan =
      plan_launch(*c, ptd::part_count(part_of(c, c->rank), p.blocks_total), n_batches, packed);
  if (plan.refuse_first) return fail(plan.refuse_code, plan.refuse);
  Moments moments;
  { const int rc = moments_open(c, first_batch, n_batches, packed, &moments); if (rc) return rc; }
  p.moments = moments.fold ? c->d_moments : nullptr;
  { const int rc = render_params(c, plan, first_batch, n_batches, packed, &p); if (rc) return rc; }
  PT_HIP(hipSetDevice(c->device));
  LaunchTimer timer;
  { const int rc = timing_begin(c, &timer); if (rc) return rc; }
  if (plan.refuse) return fail(plan.refuse_code, plan.refuse);
  { const int rc = cull_and_items(c, plan, n_batches, &p); if (rc) return rc; }
  c->last = p;   // the item exchange (pt_items_*) follows the last rendered frame
  const Culled culled = culled_before(c, &p, packed, n_batches);
  c->last_kernel = plan.wf ? 3 : 1;
  c->last_valid = true;
  if (packed && as.frame == (void*)c->d_accum) c->culled_state = 0;   // the assembly writes this buffer
  if (packed) {
    frame_key(c, p, &c->key_scratch);
    if (as.src && c->key_scratch != c->packed_key)
      return fail(PT_ERR_INVALID, "pt_render_packed: the frame to assemble has another item layout (size, partition, lanes, culling)");
    if (plan.wf) return render_packed_wavefront(c, plan, p, n_batches, pack_out, as);
    { const int rc = assembly_params(c, as, &p); if (rc) return rc; }
    if (!p.items) p.n_items = p.n_tiles * p.spl;
    c->packed_key = c->key_scratch;
    p.pack_out = pack_out;
  }
  // every launch but the path-recursive render_packed writes the context's
  // accumulation buffer or wavefront buffers
  const bool shared = !packed || plan.wf || c->stats_mode;
  if (shared) {
    const int ro = order_shared(c);
    if (ro) return ro;
  }
  // a launch from batch 0 starts every pixel's moments at +0; the kernels write the live pixels only
  if (moments.fold && first_batch == 0)
    PT_HIP(hipMemsetAsync(c->d_moments, 0, (size_t)c->width * c->height * sizeof(float2), c->stream));
  {
    const int rc = plan.wf ? launch_wf(c, plan, n_batches, &p) : launch_recursive(c, plan, p, launched);
    if (rc) return rc;
  }
  if (shared) {
    const int rm = mark_shared(c);
    if (rm) return rm;
  } else if (!c->in_dist) {
    const int ru = note_use(c);   // render_packed reads the scene and item tables
    if (ru) return ru;
  }
  { const int rc = timing_end(c, timer); if (rc) return rc; }
  moments_close(c, moments, first_batch, n_batches);
  culled_after(c, culled, packed, c->opt_fresh != 0, first_batch, n_batches);
  return PT_OK;
}

// The parameters of an adaptive round's launch (pt_adaptive.cpp): render_impl's scene, frame, camera and
// option fields under the adaptive plan, the cull rectangles, and neither item list nor packed output; the
// batches are the live list's.
int adaptive_render_params(pt_context* c, const AdaptivePlan& ap, int spl, ptd::RenderParams* p) {
  { const int rc = render_ready(c); if (rc) return rc; }
  if (c->n_lights < 1) return fail(PT_ERR_INVALID, "no lights uploaded");
  frame_params(c, false, p);
  LaunchPlan plan;
  plan.spl = spl;
  plan.lds = ap.lds;
  plan.exit_skip = ap.exit_skip;
  plan.sweep = ap.sweep != 0;
  plan.sweep_hull = ap.sweep >= 2;
  plan.sweep_cube = ap.sweep == 3;
  plan.wide_refill = ap.wide_refill;
  { const int rc = render_params(c, plan, 0, 0, false, p); if (rc) return rc; }
  p->moments = c->d_moments;
  cull_rectangles(c, p);
  return cull_footprints(c, p);
}

int adaptive_launch_wavefront(pt_context* c, const AdaptivePlan& ap, uint32_t reserve_batches, ptd::RenderParams* p) {
  long long chunk_paths = 0;
  const int rc = wf_reserve(c, (long long)p->blocks_total * 256, reserve_batches, &chunk_paths);
  if (rc) return rc;
  ptd::WfBuffers b = c->wf;
  b.cap = chunk_paths;   // paths per chunk (the allocation may be larger)
  if (ap.wide) {
    const int rw = wide_params(c, p);
    if (rw) return rw;
    p->wide_handback = ap.wide_handback;
    p->wf_fuse = ap.wf_fuse;
    p->wf_tail = ap.wf_tail;
  }
  PT_HIP(ptd::launch_wavefront_adaptive(*p, b, ap.lds, c->d_ad_list, c->d_ad_live, c->stream));
  return PT_OK;
}

int radiance_wf_buffers(pt_context* c, long long paths, ptd::WfBuffers* b) {
  long long chunk_paths = 0;
  const int rc = wf_reserve(c, paths, 1, &chunk_paths);   // one "batch" of `paths` "pixels": no less than asked for
  if (rc) return rc;
  *b = c->wf;
  b->cap = chunk_paths;
  return PT_OK;
}

// The device arrays of the uploaded scene: pt_upload_scene replaces them,
// pt_destroy frees them.
static void scene_release(pt_context* c) {
  dev_free(c->d_nodes);
  dev_free(c->d_nodes_full);
  dev_free(c->d_sweep);
  dev_free(c->d_sweep_plain);
  c->sweep_boxes = c->sweep_leaves = c->sweep_hull = 0;
  c->sweep_cube = false;
  dev_free(c->d_wide);
  dev_free(c->d_wide_q);
  dev_free(c->d_wide_leafbox);
  dev_free(c->d_wide_tris);
  dev_free(c->d_wide_rank_of);
  dev_free(c->d_tris);
  // the wide walk's overflow area is sized by the scene's stack bound: a
  // deeper tree needs a new one (it is reallocated at the next wide launch)
  dev_free(c->d_wide_ovf);
  c->wide_ovf_lanes = 0;
  c->wide_ovf_stack = 0;
  c->n_wide = 0;
}

int pt_fail_internal(int code, const std::string& msg) {
  g_err = msg;
  return code;
}
void pt_note_accum_written(pt_context* c, bool finite) {
  if (!c) return;
  c->culled_state = finite ? 1 : 0;
  c->culled_buf = c->d_accum;
}

extern "C" {

int pt_abi_version(void) { return PT_ABI_VERSION; }
const char* pt_last_error(void) { return g_err.c_str(); }

int pt_create(int device_ordinal, pt_context** out) {
  if (!out) return fail(PT_ERR_INVALID, "out is null");
  *out = nullptr;
  int n = 0;
  PT_HIP(hipGetDeviceCount(&n));
  if (device_ordinal < 0 || device_ordinal >= n)
    return fail(PT_ERR_INVALID, "device ordinal " + std::to_string(device_ordinal) + " out of range (" +
                                    std::to_string(n) + " devices)");
  PT_HIP(hipSetDevice(device_ordinal));
  hipDeviceProp_t prop;
  PT_HIP(hipGetDeviceProperties(&prop, device_ordinal));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(PT_ERR_UNSUPPORTED, std::string("built for gfx950, device is ") + prop.gcnArchName);
  pt_context* c = new pt_context();
  c->device = device_ordinal;
  hipError_t e = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipMalloc((void**)&c->d_stats, ptd::kStatsWords * sizeof(unsigned long long));
  if (e == hipSuccess) e = hipMemset(c->d_stats, 0, ptd::kStatsWords * sizeof(unsigned long long));
  for (int i = 0; i < pt_context::kRing && e == hipSuccess; ++i) {
    e = hipEventCreate(&c->ring[i][0]);
    if (e == hipSuccess) e = hipEventCreate(&c->ring[i][1]);
  }
  if (e == hipSuccess) e = hipEventCreateWithFlags(&c->shared_ev, hipEventDisableTiming);
  if (e != hipSuccess) {
    pt_destroy(c);
    return fail(PT_ERR_HIP, std::string("context setup: ") + hipGetErrorString(e));
  }
  c->stream = c->own_stream;
  *out = c;
  return PT_OK;
}

int pt_create_multi(const int* device_ordinals, int n, pt_context** out) {
  if (!out || !device_ordinals) return fail(PT_ERR_INVALID, "null argument");
  *out = nullptr;
  pt_group* g = nullptr;
  const int rc = ptg::make(device_ordinals, n, &g);
  if (rc) return rc;
  pt_context* c = new pt_context();
  c->device = device_ordinals[0];
  c->group = g;
  *out = c;
  return PT_OK;
}

int pt_group_info(pt_context* c, int* n_devices, int* devices, int max_devices, int* peer_stores) {
  if (!c) return fail(PT_ERR_INVALID, "null context");
  if (!c->group) {
    if (n_devices) *n_devices = 1;
    if (devices && max_devices > 0) devices[0] = c->device;
    if (peer_stores) *peer_stores = 0;
    return PT_OK;
  }
  return ptg::members(c->group, n_devices, devices, max_devices, peer_stores);
}

int pt_group_check(pt_context* c, int* state, float* ms_peer, float* ms_staged) {
  if (!c) return fail(PT_ERR_INVALID, "null context");
  if (!c->group) {
    if (state) *state = -1;
    if (ms_peer) *ms_peer = 0.0f;
    if (ms_staged) *ms_staged = 0.0f;
    return PT_OK;
  }
  return ptg::check_info(c->group, state, ms_peer, ms_staged);
}

int pt_destroy(pt_context* c) {
  if (!c) return PT_OK;
  if (c->group) {   // a multi-device context: its members and buffers
    (void)ptg::destroy(c->group);
    delete c;
    return PT_OK;
  }
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->wf_stream2) (void)hipStreamSynchronize(c->wf_stream2);
  if (c->dist) (void)pt_dist_finalize(c);
  (void)quiesce(c);
  for (auto& u : c->uses) (void)hipEventDestroy(u.ev);
  c->uses.clear();
  scene_release(c);
  dev_free(c->d_lights);
  dev_free(c->d_lights_dev);
  if (c->own_accum) dev_free(c->d_accum);
  dev_free(c->d_stats);
  dev_free(c->d_items);
  dev_free(c->d_foot);
  dev_free(c->d_cost);
  if (c->h_cost) (void)hipHostFree(c->h_cost);
  if (c->cost_ev) (void)hipEventDestroy(c->cost_ev);
  dev_free(c->d_pack_items);
  dev_free(c->d_unpack);
  dev_free(c->d_unpack_live);
  dev_free(c->wf_block);
  dev_free(c->d_moments);
  post_release(c);
  adaptive_release(c);
  display_release(c);
  rays_release(c);
  upsample_release(c);
  radiance_release(c);
  for (auto& r : c->rb) {
    dev_free(r.dev);
    if (r.host) (void)hipHostFree(r.host);
    if (r.snap) (void)hipEventDestroy(r.snap);
    if (r.done) (void)hipEventDestroy(r.done);
  }
  if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
  if (c->shared_ev) (void)hipEventDestroy(c->shared_ev);
  dev_free(c->d_parts);
  for (int i = 0; i < pt_context::kRing; ++i)
    for (int j = 0; j < 2; ++j)
      if (c->ring[i][j]) (void)hipEventDestroy(c->ring[i][j]);
  if (c->wf_stream2) (void)hipStreamDestroy(c->wf_stream2);
  if (c->wf_fork) (void)hipEventDestroy(c->wf_fork);
  if (c->wf_join) (void)hipEventDestroy(c->wf_join);
  if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
  delete c;
  return PT_OK;
}

int pt_set_stream(pt_context* c, void* s) {
  if (c && c->group) return ptg::set_stream(c->group, s);
  if (!c) return fail(PT_ERR_INVALID, "null context");
  c->stream = s ? (hipStream_t)s : c->own_stream;
  return PT_OK;
}

int pt_synchronize(pt_context* c) {
  if (c && c->group) return ptg::synchronize(c->group);
  if (!c) return fail(PT_ERR_INVALID, "null context");
  PT_HIP(hipSetDevice(c->device));
  PT_HIP(hipStreamSynchronize(c->stream));
  return c->dist ? dist_synchronize(c) : PT_OK;   // the native step loop's streams
}

int pt_upload_scene(pt_context* c, const float* vertices, size_t n_vertex_floats, const uint32_t* indices,
                    size_t n_indices, const pt_bvh_node* nodes, size_t n_nodes, const float* uvs,
                    size_t n_uv_floats, const uint32_t* mat_indices, size_t n_mat, uint32_t flags) {
  if (c && c->group) return ptg::upload_scene(c->group, vertices, n_vertex_floats, indices, n_indices, nodes, n_nodes, uvs, n_uv_floats, mat_indices, n_mat, flags);
  if (!c) return fail(PT_ERR_INVALID, "null context");
  if (!vertices || !indices || !nodes) return fail(PT_ERR_INVALID, "null scene array");
  if (n_vertex_floats % 3 || n_indices % 3 || n_indices == 0)
    return fail(PT_ERR_SCENE, "vertex/index array sizes must be non-zero multiples of 3");
  if (n_nodes != 2 * (n_indices / 3) - 1)
    return fail(PT_ERR_SCENE, "expected 2T-1 = " + std::to_string(2 * (n_indices / 3) - 1) + " nodes, got " +
                                  std::to_string(n_nodes));
  if ((n_uv_floats && !uvs) || (n_mat && !mat_indices)) return fail(PT_ERR_INVALID, "null uv/material array");
  if (n_indices / 3 > 0x7fffffffull) return fail(PT_ERR_UNSUPPORTED, "too many triangles");
  const size_t nv = n_vertex_floats / 3;
  for (size_t i = 0; i < n_indices; ++i)
    if (indices[i] >= nv) return fail(PT_ERR_SCENE, "vertex index out of range at " + std::to_string(i));
  std::vector<float> threaded_f, collapsed_f;
  const std::string not_tree =
      pt::thread_bvh((const float*)nodes, n_nodes, (flags & PT_NODES_INT_BITS) != 0, n_indices / 3, &threaded_f);
  if (!not_tree.empty()) return fail(PT_ERR_SCENE, not_tree);
  pt::collapse_implied(threaded_f, &collapsed_f);
  std::vector<float4> threaded = as_float4(threaded_f), collapsed = as_float4(collapsed_f);
  // tiny scenes: the sweep table of the LDS render kernel (PT_OPT_SMALL_SWEEP)
  pt::SmallSweep sweep;
  // (a node array with an unreachable node has fewer leaves than triangles: no table)
  const bool has_sweep = pt::build_small_sweep(collapsed_f.data(), collapsed_f.size() / 8, &sweep) &&
                         (size_t)sweep.n_leaves == n_indices / 3;
  pt::WideBVH wide;
  const std::string wide_reason =
      pt::build_wide_bvh((const float*)nodes, n_nodes, (flags & PT_NODES_INT_BITS) != 0, vertices, n_vertex_floats,
                         indices, n_indices / 3, &wide, c->opt_wide_build);
  float lo[3] = {threaded[0].x, threaded[0].y, threaded[0].z};   // node 0 is the root
  // the exit skip (PT_OPT_EXIT_SKIP) can fire only on an axis-pure stored normal: look for one with the
  // ops of setup_tris_kernel (a cross product with two zero components first: normalize keeps a zero)
  bool exit_normals = false;
  for (size_t t = 0; t < n_indices / 3 && !exit_normals; ++t) {
    const float* a = vertices + 3 * (size_t)indices[3 * t];
    const float* b = vertices + 3 * (size_t)indices[3 * t + 1];
    const float* d = vertices + 3 * (size_t)indices[3 * t + 2];
    const ptm::v3 v0 = ptm::mk(a[0], a[1], a[2]);
    const ptm::v3 cr = ptm::cross(ptm::sub(ptm::mk(b[0], b[1], b[2]), v0), ptm::sub(ptm::mk(d[0], d[1], d[2]), v0));
    if ((cr.x == 0.0f) + (cr.y == 0.0f) + (cr.z == 0.0f) >= 2) exit_normals = ptd::exit_normal(ptm::normalize(cr));
  }
  float hi[3] = {threaded[1].x, threaded[1].y, threaded[1].z};
  PT_HIP(hipSetDevice(c->device));
  { const int rc_ = quiesce(c); if (rc_) return rc_; }
  scene_release(c);
  c->has_scene = false;
  c->guide_valid = false;
  temporal_forget(c);
  display_forget(c);
  upsample_forget(c);
  adaptive_forget(c);
  const int T = (int)(n_indices / 3);
  struct Staging {   // vertex/index copies live only until the triangle records are built
    float* v = nullptr;
    uint32_t* i = nullptr;
    ~Staging() { if (v) (void)hipFree(v); if (i) (void)hipFree(i); }
  } st;
  // one zero node of padding past the end: the traversal loads node k+1
  // speculatively, also when k is the last node
  collapsed.push_back(make_float4(0, 0, 0, 0));
  collapsed.push_back(make_float4(0, 0, 0, 0));
  threaded.push_back(make_float4(0, 0, 0, 0));
  threaded.push_back(make_float4(0, 0, 0, 0));
  PT_HIP(hipMalloc((void**)&c->d_nodes, collapsed.size() * sizeof(float4)));
  PT_HIP(hipMalloc((void**)&c->d_nodes_full, threaded.size() * sizeof(float4)));
  PT_HIP(hipMalloc((void**)&c->d_tris, (size_t)T * 3 * sizeof(float4)));
  PT_HIP(hipMalloc((void**)&st.v, n_vertex_floats * sizeof(float) + 16));
  PT_HIP(hipMalloc((void**)&st.i, n_indices * sizeof(uint32_t)));
  PT_HIP(hipMemcpyAsync(c->d_nodes, collapsed.data(), collapsed.size() * sizeof(float4), hipMemcpyHostToDevice, c->stream));
  PT_HIP(hipMemcpyAsync(c->d_nodes_full, threaded.data(), threaded.size() * sizeof(float4), hipMemcpyHostToDevice, c->stream));
  PT_HIP(hipMemcpyAsync(st.v, vertices, n_vertex_floats * sizeof(float), hipMemcpyHostToDevice, c->stream));
  PT_HIP(hipMemcpyAsync(st.i, indices, n_indices * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
  PT_HIP(ptd::launch_setup_tris(st.v, st.i, T, c->d_tris, c->stream));
  // (both live until the copies have run: synchronized below)
  const std::vector<float> sweep_table = sweep.pack(), sweep_plain = sweep.pack(false);
  if (has_sweep) {
    PT_HIP(hipMalloc((void**)&c->d_sweep, sweep_table.size() * sizeof(float)));
    PT_HIP(hipMemcpyAsync(c->d_sweep, sweep_table.data(), sweep_table.size() * sizeof(float), hipMemcpyHostToDevice,
                          c->stream));
    PT_HIP(hipMalloc((void**)&c->d_sweep_plain, sweep_plain.size() * sizeof(float)));
    PT_HIP(hipMemcpyAsync(c->d_sweep_plain, sweep_plain.data(), sweep_plain.size() * sizeof(float),
                          hipMemcpyHostToDevice, c->stream));
  }
  std::vector<int> rank_of_host(wide_reason.empty() ? (size_t)T : 0);
  if (wide_reason.empty()) {
    PT_HIP(hipMalloc((void**)&c->d_wide, wide.nodes.size() * sizeof(float)));
    PT_HIP(hipMalloc((void**)&c->d_wide_q, wide.qnodes.size() * sizeof(float)));
    PT_HIP(hipMalloc((void**)&c->d_wide_leafbox, wide.leaf_box.size() * sizeof(float)));
    PT_HIP(hipMemcpyAsync(c->d_wide_q, wide.qnodes.data(), wide.qnodes.size() * sizeof(float), hipMemcpyHostToDevice,
                          c->stream));
    PT_HIP(hipMemcpyAsync(c->d_wide_leafbox, wide.leaf_box.data(), wide.leaf_box.size() * sizeof(float),
                          hipMemcpyHostToDevice, c->stream));
    PT_HIP(hipMalloc((void**)&c->d_wide_rank_of, (size_t)T * sizeof(int)));
    PT_HIP(hipMalloc((void**)&c->d_wide_tris, (size_t)T * 3 * sizeof(float4)));
    PT_HIP(hipMemcpyAsync(c->d_wide, wide.nodes.data(), wide.nodes.size() * sizeof(float), hipMemcpyHostToDevice,
                          c->stream));
    PT_HIP(hipMemcpyAsync(c->d_wide_rank_of, wide.rank_tri.data(), (size_t)T * sizeof(int), hipMemcpyHostToDevice,
                          c->stream));
    PT_HIP(ptd::launch_gather_tris(c->d_tris, c->d_wide_rank_of, T, c->d_wide_tris, c->stream));
    // then the same buffer becomes slot -> rank (the kernels' only use of it)
    for (int r = 0; r < T; ++r) rank_of_host[wide.rank_tri[r]] = r;
    PT_HIP(hipMemcpyAsync(c->d_wide_rank_of, rank_of_host.data(), (size_t)T * sizeof(int), hipMemcpyHostToDevice,
                          c->stream));
  }
  PT_HIP(hipStreamSynchronize(c->stream));
  c->n_wide = wide_reason.empty() ? wide.n_nodes : 0;
  c->wide_stack = wide.stack_cap;
  c->wide_reason = wide_reason;
  c->n_nodes = (int)(collapsed.size() / 2) - 1;
  c->n_nodes_full = (int)(threaded.size() / 2) - 1;
  c->n_tris = T;
  c->sweep_boxes = has_sweep ? sweep.n_boxes : 0;
  c->sweep_leaves = has_sweep ? sweep.n_leaves : 0;
  c->sweep_hull = has_sweep ? sweep.n_hull : 0;
  // the cube table's walk reads the root box from root_lo / root_hi: only where box 0 of the table is that, bitwise
  c->sweep_cube = has_sweep && sweep.cube && memcmp(&sweep.boxes[0], lo, sizeof lo) == 0 &&
                  memcmp(&sweep.boxes[4], hi, sizeof hi) == 0;
  memcpy(c->cube_under, sweep.cube_under, sizeof c->cube_under);
  c->cube_all = sweep.cube_all;
  memcpy(c->root_lo, lo, sizeof lo);
  memcpy(c->root_hi, hi, sizeof hi);
  c->exit_normals = exit_normals;
  c->has_scene = true;
  c->scene_serial++;
  return PT_OK;
}

int pt_upload_lights(pt_context* c, const pt_area_light* lights, size_t n) {
  if (c && c->group) return ptg::upload_lights(c->group, lights, n);
  if (!c) return fail(PT_ERR_INVALID, "null context");
  if (n && !lights) return fail(PT_ERR_INVALID, "null lights");
  if (n > 1024) return fail(PT_ERR_UNSUPPORTED, "more than 1024 lights");
  PT_HIP(hipSetDevice(c->device));
  { const int rc_ = quiesce(c); if (rc_) return rc_; }
  dev_free(c->d_lights);
  dev_free(c->d_lights_dev);
  c->n_lights = 0;
  c->lights_host.clear();
  temporal_forget(c);
  adaptive_forget(c);
  if (n) {
    PT_HIP(hipMalloc((void**)&c->d_lights, n * sizeof(ptd::LightRec)));
    PT_HIP(hipMalloc((void**)&c->d_lights_dev, n * sizeof(ptd::LightDev)));
    PT_HIP(hipMemcpyAsync(c->d_lights, lights, n * sizeof(ptd::LightRec), hipMemcpyHostToDevice, c->stream));
    PT_HIP(ptd::launch_setup_lights(c->d_lights, (int)n, c->d_lights_dev, c->stream));
    PT_HIP(hipStreamSynchronize(c->stream));
  }
  c->n_lights = (int)n;
  c->lights_host.assign(lights, lights + n);
  c->scene_serial++;
  return PT_OK;
}

int pt_set_camera(pt_context* c, const float ubo[16]) {
  if (c && c->group) return ptg::set_camera(c->group, ubo);
  if (!c || !ubo) return fail(PT_ERR_INVALID, "null argument");
  if (!c->has_camera || memcmp(c->cam, ubo, sizeof c->cam) != 0) c->guide_valid = false;
  memcpy(c->cam, ubo, sizeof c->cam);
  c->has_camera = true;
  return PT_OK;
}

int pt_set_params(pt_context* c, const pt_params* p) {
  if (c && c->group) return ptg::set_params(c->group, p);
  if (!c || !p) return fail(PT_ERR_INVALID, "null argument");
  if (p->max_depth < 0 || p->max_depth > 64 || p->sss_bounces < 0 || p->sss_bounces > 64)
    return fail(PT_ERR_INVALID, "max_depth and sss_bounces must be in [0,64]");
  c->params = *p;
  temporal_forget(c);
  adaptive_forget(c);
  return PT_OK;
}

int pt_set_partition(pt_context* c, int nranks, int rank) {
  PT_SINGLE(c, "pt_set_partition");
  if (!c) return fail(PT_ERR_INVALID, "null context");
  if (nranks < 1 || rank < 0 || rank >= nranks) return fail(PT_ERR_INVALID, "bad partition");
  c->nranks = nranks;
  c->rank = rank;
  c->slots.assign((size_t)nranks, 1);
  c->parts_valid = false;
  c->items_key.clear();   // the cached item lists follow the partition
  return PT_OK;
}

int pt_set_partition_slots(pt_context* c, int nranks, int rank, const int* slots) {
  PT_SINGLE(c, "pt_set_partition_slots");
  if (!c || !slots) return fail(PT_ERR_INVALID, "null argument");
  if (nranks < 1 || rank < 0 || rank >= nranks) return fail(PT_ERR_INVALID, "bad partition");
  long long m = 0;
  for (int r = 0; r < nranks; ++r) {
    if (slots[r] < 1 || slots[r] > ptd::kMaxSlots) return fail(PT_ERR_INVALID, "partition slots must be 1..64 per rank");
    m += slots[r];
  }
  if (m > 4096) return fail(PT_ERR_INVALID, "more than 4096 partition slots");
  c->nranks = nranks;
  c->rank = rank;
  c->slots.assign(slots, slots + nranks);
  c->parts_valid = false;
  c->items_key.clear();
  return PT_OK;
}

// The moments image back to "no batches": zeros, on the context's stream.
static int moments_zero(pt_context* c) {
  adaptive_forget(c);   // a cleared or newly bound image holds no adaptive render
  c->moments_valid = false;
  c->moments_n = 0;
  const size_t n = (size_t)c->width * c->height;
  if (c->d_moments && n > 0 && c->moments_cap >= n) PT_HIP(hipMemsetAsync(c->d_moments, 0, n * sizeof(float2), c->stream));
  return PT_OK;
}

int pt_clear_accum(pt_context* c) {
  if (c && c->group) return ptg::clear_accum(c->group);
  if (!c) return fail(PT_ERR_INVALID, "null context");
  if (!c->d_accum) return fail(PT_ERR_INVALID, "no accumulation buffer");
  PT_HIP(hipSetDevice(c->device));
  const int ro = order_shared(c);
  if (ro) return ro;
  {
    const int rc = sync_parts(c);
    if (rc) return rc;
  }
  PT_HIP(ptd::launch_clear(c->d_accum, c->width, c->height, part_of(c, c->rank),
                           c->d_parts + (size_t)c->rank * ptd::kMaxSlots, c->stream));
  c->culled_state = 1;
  c->culled_buf = c->d_accum;
  {
    const int rz = moments_zero(c);
    if (rz) return rz;
  }
  return mark_shared(c);
}

int pt_resize_and_clear(pt_context* c, int w, int h) {
  if (c && c->group) return ptg::resize_and_clear(c->group, w, h);
  if (!c) return fail(PT_ERR_INVALID, "null context");
  if (w <= 0 || h <= 0 || (long long)w * h > (1ll << 31)) return fail(PT_ERR_INVALID, "bad resolution");
  PT_HIP(hipSetDevice(c->device));
  if (c->width != w || c->height != h) c->guide_valid = false;
  if (!(c->own_accum && c->width == w && c->height == h)) {
    { const int rc_ = quiesce(c); if (rc_) return rc_; }
    if (c->own_accum) dev_free(c->d_accum);
    c->d_accum = nullptr;
    c->own_accum = false;
    temporal_forget(c);   // another size or another buffer
    display_forget(c);
    PT_HIP(hipMalloc((void**)&c->d_accum, (size_t)w * h * sizeof(float4)));
    c->own_accum = true;
    c->width = w;
    c->height = h;
  }
  return pt_clear_accum(c);
}

int pt_bind_accum(pt_context* c, void* ptr, int w, int h) {
  if (c && c->group) return ptg::bind_accum(c->group, ptr, w, h);
  if (!c || !ptr) return fail(PT_ERR_INVALID, "null argument");
  if (w <= 0 || h <= 0) return fail(PT_ERR_INVALID, "bad resolution");
  if (((uintptr_t)ptr) & 15) return fail(PT_ERR_INVALID, "accumulation buffer must be 16-B aligned");
  PT_HIP(hipSetDevice(c->device));
  { const int rc_ = quiesce(c); if (rc_) return rc_; }
  if (c->own_accum) dev_free(c->d_accum);
  if (c->d_accum != (float4*)ptr || c->own_accum || c->width != w || c->height != h) {
    temporal_forget(c);
    display_forget(c);
  }
  c->d_accum = (float4*)ptr;
  c->own_accum = false;
  if (c->width != w || c->height != h) c->guide_valid = false;
  c->width = w;
  c->height = h;
  c->culled_state = 0;   // the caller's buffer: its content is not known
  return moments_zero(c);
}

void* pt_accum_device_ptr(pt_context* c) {
  if (c && c->group) return ptg::accum_device_ptr(c->group);
  return c ? (void*)c->d_accum : nullptr;
}

int pt_read_accum(pt_context* c, float* rgba, size_t n) {
  if (c && c->group) return ptg::read_accum(c->group, rgba, n);
  if (!c || !rgba) return fail(PT_ERR_INVALID, "null argument");
  if (!c->d_accum) return fail(PT_ERR_INVALID, "no accumulation buffer");
  return read_image(c, c->d_accum, c->width, c->height, 4, rgba, n);
}

int pt_render(pt_context* c, uint32_t first_batch, uint32_t n_batches) {
  if (c && c->group) return ptg::render(c->group, first_batch, n_batches);
  return render_impl(c, first_batch, n_batches, nullptr);
}

// The gather step of a tile split (bench.py N>1): a fresh frame rendered from
// batch 0 whose live items go straight into the pt_items_pack layout -- one
// launch instead of render + culled fill + pack, and no accumulation-buffer
// traffic.  The accumulation buffer is neither read nor written.
int pt_render_packed(pt_context* c, uint32_t n_batches, void* packed, const void* gathered, size_t slot_floats,
                     void* frame) {
  PT_SINGLE(c, "pt_render_packed");
  if (!c || !packed) return fail(PT_ERR_INVALID, "null argument");
  if (((uintptr_t)packed) & 15) return fail(PT_ERR_INVALID, "packed buffer must be 16-B aligned");
  if (c->stats_mode) return fail(PT_ERR_UNSUPPORTED, "stats mode renders into the accumulation buffer");
  if (c->opt_moments) return fail(PT_ERR_UNSUPPORTED, "PT_OPT_MOMENTS: not with pt_render_packed");
  Assembly as;
  if (gathered) {
    if (!frame) return fail(PT_ERR_INVALID, "gathered slots without a frame");
    if ((((uintptr_t)gathered) & 15) || (((uintptr_t)frame) & 15) || (slot_floats & 3))
      return fail(PT_ERR_INVALID, "buffers must be 16-B aligned, slots whole float4s");
    as.src = gathered;
    as.slot_floats = slot_floats;
    as.frame = frame;
  }
  return render_impl(c, 0, n_batches, (float4*)packed, as);
}

int pt_dispatch(pt_context* c, uint32_t sample_batch) { return pt_render(c, sample_batch, 1); }

// ---- progressive loop + asynchronous readback -----------
// The reference's mainLoop (VulkanRayTracer.cpp:717-865) resets sampleBatch to
// 0 whenever any camera field changes (:739-754; batch 0 weights the old image
// by 0), dispatches one 1-spp batch, waits on two fences and copies the image
// out, up to 1024 batches (:719, :857).  Here a camera change resets the
// counter the same way, pending batches go out as one fused launch, and a
// readback snapshots the image on the render stream (device-to-device) and
// copies it to pinned host memory on a second stream, so rendering goes on
// while the previous frame travels over PCIe.
int pt_progressive_camera(pt_context* c, const float ubo[16], int* reset) {
  if (c && c->group) return ptg::progressive_camera(c->group, ubo, reset);
  if (!c || !ubo) return fail(PT_ERR_INVALID, "null argument");
  const bool changed = !c->prog_has_cam || memcmp(ubo, c->prog_cam, sizeof c->prog_cam) != 0;
  if (changed) {
    memcpy(c->prog_cam, ubo, sizeof c->prog_cam);
    c->prog_has_cam = true;
    c->prog_batch = 0;
    const int rc = pt_set_camera(c, ubo);
    if (rc) return rc;
  }
  if (reset) *reset = changed ? 1 : 0;
  return PT_OK;
}

int pt_progressive_advance(pt_context* c, uint32_t max_new, uint32_t limit, uint32_t* first, uint32_t* count) {
  if (c && c->group) return ptg::progressive_advance(c->group, max_new, limit, first, count);
  if (!c) return fail(PT_ERR_INVALID, "null context");
  if (!c->prog_has_cam) return fail(PT_ERR_INVALID, "no camera (pt_progressive_camera)");
  const uint32_t room = limit > c->prog_batch ? limit - c->prog_batch : 0u;
  const uint32_t n = max_new < room ? max_new : room;
  if (first) *first = c->prog_batch;
  if (count) *count = n;
  if (n == 0) return PT_OK;
  const int rc = pt_render(c, c->prog_batch, n);
  if (rc) return rc;
  c->prog_batch += n;
  return PT_OK;
}

int pt_readback_begin(pt_context* c, int* ticket) {
  if (c && c->group) return ptg::readback_begin(c->group, ticket);
  if (!c || !ticket) return fail(PT_ERR_INVALID, "null argument");
  if (!c->d_accum) return fail(PT_ERR_INVALID, "no accumulation buffer");
  PT_HIP(hipSetDevice(c->device));
  if (!c->copy_stream) PT_HIP(hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
  // the free slot, else the older one (its unread result is dropped)
  int slot = c->rb[0].ticket == 0 ? 0 : c->rb[1].ticket == 0 ? 1 : (c->rb[0].ticket < c->rb[1].ticket ? 0 : 1);
  pt_context::Readback& r = c->rb[slot];
  if (r.ticket) PT_HIP(hipEventSynchronize(r.done));
  const size_t bytes = (size_t)c->width * c->height * sizeof(float4);
  if (r.bytes != bytes) {
    dev_free(r.dev);
    if (r.host) (void)hipHostFree(r.host);
    r.host = nullptr;
    r.bytes = 0;
    PT_HIP(hipMalloc((void**)&r.dev, bytes));
    PT_HIP(hipHostMalloc(&r.host, bytes, hipHostMallocDefault));
    r.bytes = bytes;
  }
  if (!r.snap) PT_HIP(hipEventCreateWithFlags(&r.snap, hipEventDisableTiming));
  if (!r.done) PT_HIP(hipEventCreateWithFlags(&r.done, hipEventDisableTiming));
  {
    const int ro = order_shared(c);
    if (ro) return ro;
  }
  PT_HIP(hipMemcpyAsync(r.dev, c->d_accum, bytes, hipMemcpyDeviceToDevice, c->stream));
  {
    const int ru = note_use(c);
    if (ru) return ru;
  }
  PT_HIP(hipEventRecord(r.snap, c->stream));
  PT_HIP(hipStreamWaitEvent(c->copy_stream, r.snap, 0));
  PT_HIP(hipMemcpyAsync(r.host, r.dev, bytes, hipMemcpyDeviceToHost, c->copy_stream));
  PT_HIP(hipEventRecord(r.done, c->copy_stream));
  r.w = c->width;
  r.h = c->height;
  r.ticket = c->rb_next_ticket++;
  *ticket = r.ticket;
  return PT_OK;
}

int pt_readback_end(pt_context* c, int ticket, float* rgba, size_t n) {
  if (c && c->group) return ptg::readback_end(c->group, ticket, rgba, n);
  if (!c || !rgba) return fail(PT_ERR_INVALID, "null argument");
  for (auto& r : c->rb) {
    if (r.ticket != ticket || ticket == 0) continue;
    const size_t need = (size_t)r.w * r.h * 4;
    if (n < need) return fail(PT_ERR_INVALID, "output buffer too small: need " + std::to_string(need) + " floats");
    PT_HIP(hipSetDevice(c->device));
    PT_HIP(hipEventSynchronize(r.done));
    memcpy(rgba, r.host, need * sizeof(float));
    r.ticket = 0;
    return PT_OK;
  }
  return fail(PT_ERR_INVALID, "unknown or already collected readback ticket " + std::to_string(ticket));
}

int pt_last_kernel(pt_context* c, int* kernel) {
  if (c && c->group) return ptg::last_kernel(c->group, kernel);
  if (!c || !kernel) return fail(PT_ERR_INVALID, "null argument");
  *kernel = c->last_kernel;
  return PT_OK;
}

// The options that are a range check and a store: value in [lo, hi] goes into
// the field, anything else is refused with the message.
struct IntOption {
  int key;
  int pt_context::* field;
  int lo, hi;
  const char* message;
};
static const IntOption kIntOptions[] = {
    {PT_OPT_KERNEL, &pt_context::opt_kernel, 0, 3, "PT_OPT_KERNEL takes 0, 1 or 3"},   // (2: refused below)
    {PT_OPT_WIDE, &pt_context::opt_wide, 0, 2, "PT_OPT_WIDE takes 0, 1 or 2"},
    {PT_OPT_WF_FUSE, &pt_context::opt_wf_fuse, 0, 1, "PT_OPT_WF_FUSE takes 0 or 1"},
    {PT_OPT_WF_TAIL, &pt_context::opt_wf_tail, -1, INT_MAX, "PT_OPT_WF_TAIL takes -1 (auto) or a ray count >= 0"},
    {PT_OPT_WF_REFILL, &pt_context::opt_wf_refill, 0, 64, "PT_OPT_WF_REFILL takes 0 (auto) to 64 idle lanes"},
    {PT_OPT_WF_GRID, &pt_context::opt_wf_grid, 1, 100, "PT_OPT_WF_GRID takes 1 to 100 (percent)"},
    {PT_OPT_WF_STREAMS, &pt_context::opt_wf_streams, 1, 2, "PT_OPT_WF_STREAMS takes 1 or 2"},
    {PT_OPT_WIDE_BUILD, &pt_context::opt_wide_build, 0, 1, "PT_OPT_WIDE_BUILD takes 0 or 1"},
    {PT_OPT_COUNT_TRACED, &pt_context::opt_count, 0, 1, "PT_OPT_COUNT_TRACED takes 0 or 1"},
    {PT_OPT_PRIMARY_CULL, &pt_context::opt_cull, 0, 1, "PT_OPT_PRIMARY_CULL takes 0 or 1"},
    {PT_OPT_WF_PATHS, &pt_context::opt_wf_paths, 0, INT_MAX, "PT_OPT_WF_PATHS takes 0 or a path count"},
    {PT_OPT_LAUNCH_TIMING, &pt_context::opt_timing, 0, INT_MAX,
     "PT_OPT_LAUNCH_TIMING takes 0 (off) or k >= 1 (every k-th launch)"},
    {PT_OPT_MIXED_LANES, &pt_context::opt_mixed, -1, 1000, "PT_OPT_MIXED_LANES takes -1 (auto), 0 (off) or 1-1000"},
    {PT_OPT_ITEM_ORDER, &pt_context::opt_item_order, -1, 1, "PT_OPT_ITEM_ORDER takes -1 (auto), 0 or 1"},
    {PT_OPT_FRESH_BATCH0, &pt_context::opt_fresh, 0, 1, "PT_OPT_FRESH_BATCH0 takes 0 or 1"},
    {PT_OPT_SCENE_IN_LDS, &pt_context::opt_scene_lds, 0, 2, "PT_OPT_SCENE_IN_LDS takes 0, 1 or 2"},
    {PT_OPT_DENOISE_LDS, &pt_context::opt_denoise_lds, 0, 1, "PT_OPT_DENOISE_LDS takes 0 or 1"},
    {PT_OPT_SMALL_SWEEP, &pt_context::opt_small_sweep, -1, 1, "PT_OPT_SMALL_SWEEP takes -1 (auto), 0 or 1"},
    {PT_OPT_CULL_TIGHT, &pt_context::opt_cull_tight, 0, 1, "PT_OPT_CULL_TIGHT takes 0 or 1"},
    {PT_OPT_SWEEP_HULL, &pt_context::opt_sweep_hull, 0, 1, "PT_OPT_SWEEP_HULL takes 0 or 1"},
    {PT_OPT_EXIT_SKIP, &pt_context::opt_exit_skip, 0, 1, "PT_OPT_EXIT_SKIP takes 0 or 1"},
    {PT_OPT_SWEEP_CUBE, &pt_context::opt_sweep_cube, 0, 1, "PT_OPT_SWEEP_CUBE takes 0 or 1"},
    {PT_OPT_ADAPTIVE_WF, &pt_context::opt_adaptive_wf, 0, 1, "PT_OPT_ADAPTIVE_WF takes 0 or 1"},
    {PT_OPT_RAYS_REFILL, &pt_context::opt_rays_refill, 0, 1, "PT_OPT_RAYS_REFILL takes 0 or 1"},
    {PT_OPT_CULL_FOOTPRINT, &pt_context::opt_cull_foot, -1, 1, "PT_OPT_CULL_FOOTPRINT takes -1 (auto), 0 or 1"},
    {PT_OPT_RADIANCE_CHUNK, &pt_context::opt_radiance_chunk, 0, INT_MAX, "PT_OPT_RADIANCE_CHUNK takes 0 (auto) or a path count"},
};

int pt_set_option(pt_context* c, int key, int value) {
  if (c && c->group && key == PT_OPT_MOMENTS && value != 0)
    return fail(PT_ERR_UNSUPPORTED, "PT_OPT_MOMENTS: not on a multi-device context (pt_create_multi)");
  if (c && c->group && key == PT_OPT_MOMENTS) return PT_OK;
  if (c && c->group) return ptg::set_option(c->group, key, value);
  if (!c) return fail(PT_ERR_INVALID, "null context");
  switch (key) {   // the options that are more than a row of the table
    case PT_OPT_KERNEL:
      if (value == 2) return fail(PT_ERR_UNSUPPORTED, "PT_OPT_KERNEL 2 (lane state machine) was removed: slower on every scene");
      break;
    case PT_OPT_WIDE_NODE:
      if (value == 80) return fail(PT_ERR_UNSUPPORTED, "PT_OPT_WIDE_NODE 80 (8-wide nodes) was removed: slower on every scene");
      if (value != 64 && value != 128) return fail(PT_ERR_INVALID, "PT_OPT_WIDE_NODE takes 64 or 128");
      c->opt_wide_node = value;
      return PT_OK;
    case PT_OPT_PAIRS:
      if (value == 1) return fail(PT_ERR_UNSUPPORTED, "PT_OPT_PAIRS 1 (child-pair records) was removed: slower on every scene");
      if (value != 0) return fail(PT_ERR_INVALID, "PT_OPT_PAIRS takes 0");
      return PT_OK;
    case PT_OPT_SM_BATCH:
      return fail(PT_ERR_UNSUPPORTED, "PT_OPT_SM_BATCH: the lane state-machine kernel was removed");
    case PT_OPT_SAMPLE_LANES:
      if (value != 0 && value != 1 && value != 2 && value != 4 && value != 8)
        return fail(PT_ERR_INVALID, "PT_OPT_SAMPLE_LANES takes 0 (auto), 1, 2, 4 or 8");
      c->opt_sample_lanes = value;
      return PT_OK;
    case PT_OPT_MOMENTS:
      if (value != 0 && value != 1) return fail(PT_ERR_INVALID, "PT_OPT_MOMENTS takes 0 or 1");
      if (value != c->opt_moments) c->moments_valid = false;
      c->opt_moments = value;
      return PT_OK;
    case PT_OPT_SEED_BASE:
      if (value < 0) return fail(PT_ERR_INVALID, "PT_OPT_SEED_BASE takes 0 to 2^31-1");
      c->opt_seed_base = (uint32_t)value;
      return PT_OK;
    case PT_OPT_GROUP_EXCHANGE:
    case PT_OPT_GROUP_CHECK:
      return fail(PT_ERR_UNSUPPORTED, "option " + std::to_string(key) + ": multi-device contexts only (pt_create_multi)");
    default:
      break;
  }
  for (const IntOption& o : kIntOptions) {
    if (o.key != key) continue;
    if (value < o.lo || value > o.hi) return fail(PT_ERR_INVALID, o.message);
    c->*o.field = value;
    return PT_OK;
  }
  return fail(PT_ERR_INVALID, "unknown option " + std::to_string(key));
}

int pt_tiles_owned(pt_context* c, int* n_tiles) {
  PT_SINGLE(c, "pt_tiles_owned");
  if (!c || !n_tiles) return fail(PT_ERR_INVALID, "null argument");
  if (!c->d_accum) return fail(PT_ERR_INVALID, "no accumulation buffer");
  *n_tiles = ptd::owned_tiles(c->width, c->height, part_of(c, c->rank));
  return PT_OK;
}

int pt_tiles_pack(pt_context* c, void* dst) {
  PT_SINGLE(c, "pt_tiles_pack");
  if (!c || !dst) return fail(PT_ERR_INVALID, "null argument");
  if (!c->d_accum) return fail(PT_ERR_INVALID, "no accumulation buffer");
  PT_HIP(hipSetDevice(c->device));
  const int ro = order_shared(c);
  if (ro) return ro;
  {
    const int rc = sync_parts(c);
    if (rc) return rc;
  }
  PT_HIP(ptd::launch_tiles(true, c->d_accum, (float4*)dst, c->width, c->height, part_of(c, c->rank),
                           c->d_parts + (size_t)c->rank * ptd::kMaxSlots, c->stream));
  return mark_shared(c);
}

int pt_tiles_unpack(pt_context* c, const void* src, int src_rank, void* frame) {
  PT_SINGLE(c, "pt_tiles_unpack");
  if (!c || !src || !frame) return fail(PT_ERR_INVALID, "null argument");
  if (!c->d_accum) return fail(PT_ERR_INVALID, "no accumulation buffer (it sets the frame size)");
  if (src_rank < 0 || src_rank >= c->nranks) return fail(PT_ERR_INVALID, "src_rank out of range");
  if ((((uintptr_t)src) & 15) || (((uintptr_t)frame) & 15)) return fail(PT_ERR_INVALID, "buffers must be 16-B aligned");
  PT_HIP(hipSetDevice(c->device));
  {
    const int rc = sync_parts(c);
    if (rc) return rc;
  }
  PT_HIP(ptd::launch_tiles(false, (float4*)frame, (float4*)src, c->width, c->height, part_of(c, src_rank),
                           c->d_parts + (size_t)src_rank * ptd::kMaxSlots, c->stream));
  if (frame == (void*)c->d_accum) c->culled_state = 0;
  return note_use(c);
}

// ---- sparse tile exchange (live items only) --------------------------------

int pt_items_live(pt_context* c, int rank, int* n_items, int* item_pixels) {
  PT_SINGLE(c, "pt_items_live");
  if (!c || !n_items || !item_pixels) return fail(PT_ERR_INVALID, "null argument");
  if (!c->last_valid) return fail(PT_ERR_INVALID, "no path-recursive pt_render yet");
  if (rank < 0 || rank >= c->last.nranks || rank >= (int)c->slots.size()) return fail(PT_ERR_INVALID, "rank out of range");
  std::vector<int> live, culled;
  item_lists(c->last, part_of(c, rank), &live, &culled);
  *n_items = (int)live.size();
  *item_pixels = 256 / c->last.spl;
  return PT_OK;
}

int pt_items_pack(pt_context* c, void* dst) {
  PT_SINGLE(c, "pt_items_pack");
  if (!c || !dst) return fail(PT_ERR_INVALID, "null argument");
  if (!c->last_valid || !c->d_accum) return fail(PT_ERR_INVALID, "no path-recursive pt_render yet");
  PT_HIP(hipSetDevice(c->device));
  frame_key(c, c->last, &c->key_scratch);
  const std::vector<float>& key = c->key_scratch;
  if (key != c->pack_key) {
    std::vector<int> live, culled;
    item_lists(c->last, part_of(c, c->last.rank), &live, &culled);
    { const int rc_ = quiesce(c); if (rc_) return rc_; }
    const int rc = upload_ints(live, &c->d_pack_items, &c->pack_cap);
    if (rc) return rc;
    c->n_pack_items = (int)live.size();
    c->pack_key = key;
  }
  const int ro = order_shared(c);
  if (ro) return ro;
  PT_HIP(ptd::launch_items_pack(c->last, c->d_accum, (float4*)dst, c->d_pack_items, c->n_pack_items, c->stream));
  return mark_shared(c);
}

int pt_items_unpack_all(pt_context* c, const void* src, size_t slot_floats, void* frame) {
  PT_SINGLE(c, "pt_items_unpack_all");
  if (!c || !src || !frame) return fail(PT_ERR_INVALID, "null argument");
  if (!c->last_valid) return fail(PT_ERR_INVALID, "no path-recursive pt_render yet");
  if (c->last.first_batch != 0)
    return fail(PT_ERR_INVALID, "sparse exchange needs a frame rendered from batch 0 (culled pixels are rebuilt)");
  if ((((uintptr_t)src) & 15) || (((uintptr_t)frame) & 15) || (slot_floats & 3))
    return fail(PT_ERR_INVALID, "buffers must be 16-B aligned, slots whole float4s");
  PT_HIP(hipSetDevice(c->device));
  frame_key(c, c->last, &c->key_scratch);
  const int rc = unpack_table(c, c->last, c->key_scratch);
  if (rc) return rc;
  PT_HIP(ptd::launch_items_unpack(c->last, (float4*)frame, (const float4*)src, slot_floats / 4, c->d_unpack,
                                  c->n_unpack, c->stream));
  if (frame == (void*)c->d_accum) c->culled_state = 0;
  return note_use(c);
}

int pt_set_stats_mode(pt_context* c, int enabled) {
  if (c && c->group) return ptg::set_stats_mode(c->group, enabled);
  if (!c) return fail(PT_ERR_INVALID, "null context");
  c->stats_mode = enabled != 0;
  return PT_OK;
}

int pt_get_stats(pt_context* c, pt_stats* out) {
  if (c && c->group) return ptg::get_stats(c->group, out);
  if (!c || !out) return fail(PT_ERR_INVALID, "null argument");
  unsigned long long h[4];
  PT_HIP(hipSetDevice(c->device));
  PT_HIP(hipMemcpyAsync(h, c->d_stats, sizeof h, hipMemcpyDeviceToHost, c->stream));
  PT_HIP(hipStreamSynchronize(c->stream));
  out->rays = h[0];
  out->nodes = h[1];
  out->leaf_tests = h[2];
  out->samples = h[3];
  return PT_OK;
}

int pt_wide_info(pt_context* c, int info[2]) {
  if (c && c->group) return ptg::wide_info(c->group, info);
  if (!c || !info) return fail(PT_ERR_INVALID, "null argument");
  info[0] = c->n_wide;
  info[1] = c->n_wide ? c->wide_stack : 0;
  if (!c->n_wide) g_err = c->wide_reason;
  return PT_OK;
}

int pt_sweep_info(pt_context* c, int* boxes, int* leaves) {
  if (c && c->group) return ptg::sweep_info(c->group, boxes, leaves);
  if (!c || !boxes || !leaves) return fail(PT_ERR_INVALID, "null argument");
  const bool on = sweep_in_force(c);
  *boxes = on ? c->sweep_boxes : 0;
  *leaves = on ? c->sweep_leaves : 0;
  return PT_OK;
}

int pt_cull_info(pt_context* c, int info[3]) {
  if (c && c->group) return ptg::cull_info(c->group, info);
  if (!c || !info) return fail(PT_ERR_INVALID, "null argument");
  ptd::RenderParams p{};
  cull_rectangles(c, &p);
  float table[kFootTable];
  int n_sure = 0;
  info[0] = p.n_cull_tight > 0 ? p.n_cull_tight : 0;
  info[1] = cull_footprint_table(c, p, table, &n_sure, &info[2]);
  return PT_OK;
}

int pt_sweep_walk(pt_context* c, int* walk) {
  if (c && c->group) return ptg::sweep_walk(c->group, walk);
  if (!c || !walk) return fail(PT_ERR_INVALID, "null argument");
  *walk = sweep_in_force(c) ? sweep_walk_kind(*c) : 0;
  return PT_OK;
}

int pt_mixed_info(pt_context* c, int info[3]) {
  if (!c || !info) return fail(PT_ERR_INVALID, "null argument");
  info[0] = info[1] = info[2] = 0;
  if (c->group) return PT_OK;
  info[0] = c->last_mix;
  info[1] = c->last_mix ? c->n_live_items : 0;
  info[2] = c->cost_frames;
  return PT_OK;
}

int pt_get_traced(pt_context* c, pt_traced* out) {
  if (c && c->group) return ptg::get_traced(c->group, out);
  if (!c || !out) return fail(PT_ERR_INVALID, "null argument");
  unsigned long long h[ptd::kStatsWords];
  PT_HIP(hipSetDevice(c->device));
  PT_HIP(hipMemcpyAsync(h, c->d_stats, sizeof h, hipMemcpyDeviceToHost, c->stream));
  PT_HIP(hipStreamSynchronize(c->stream));
  out->closest_walks = h[4];
  out->shadow_walks = h[5];
  out->nodes = h[6];
  out->tri_tests = h[7];
  out->primaries = h[8];
  return PT_OK;
}

int pt_reset_stats(pt_context* c) {
  if (c && c->group) return ptg::reset_stats(c->group);
  if (!c) return fail(PT_ERR_INVALID, "null context");
  PT_HIP(hipSetDevice(c->device));
  PT_HIP(hipMemsetAsync(c->d_stats, 0, ptd::kStatsWords * sizeof(unsigned long long), c->stream));
  return note_use(c);
}

int pt_last_launch_ms(pt_context* c, float* ms) {
  if (c && c->group) return ptg::last_launch_ms(c->group, ms);
  if (!c || !ms) return fail(PT_ERR_INVALID, "null argument");
  if (!c->timed) return fail(PT_ERR_INVALID, "no launch recorded");
  PT_HIP(hipSetDevice(c->device));
  PT_HIP(hipEventSynchronize(c->ring[c->last_slot][1]));
  PT_HIP(hipEventElapsedTime(ms, c->ring[c->last_slot][0], c->ring[c->last_slot][1]));
  return PT_OK;
}

int pt_launch_times_ms(pt_context* c, float* out, size_t max_n, size_t* n_out) {
  if (c && c->group) return ptg::launch_times_ms(c->group, out, max_n, n_out);
  if (!c || !n_out) return fail(PT_ERR_INVALID, "null argument");
  const int have = c->ring_n < pt_context::kRing ? c->ring_n : pt_context::kRing;
  const int first = c->ring_n - have;
  size_t n = 0;
  PT_HIP(hipSetDevice(c->device));
  for (int k = first; k < c->ring_n && n < max_n; ++k) {
    const int slot = k % pt_context::kRing;
    PT_HIP(hipEventSynchronize(c->ring[slot][1]));
    if (out) PT_HIP(hipEventElapsedTime(&out[n], c->ring[slot][0], c->ring[slot][1]));
    ++n;
  }
  *n_out = n;
  return PT_OK;
}

// Launches may overlap (frames alternating between streams): the device time
// from the first launch's start to the last end, i.e. the busy span a
// throughput figure divides by.
int pt_launch_span_ms(pt_context* c, float* ms, size_t* n_out) {
  if (c && c->group) return ptg::launch_span_ms(c->group, ms, n_out);
  if (!c || !ms || !n_out) return fail(PT_ERR_INVALID, "null argument");
  if (c->ring_n == 0) return fail(PT_ERR_INVALID, "no launch recorded since pt_reset_launch_times");
  if (c->ring_n > pt_context::kRing) return fail(PT_ERR_UNSUPPORTED, "more launches than the event ring holds");
  PT_HIP(hipSetDevice(c->device));
  float span = 0.0f;
  for (int k = 0; k < c->ring_n; ++k) {
    float t = 0.0f;
    PT_HIP(hipEventSynchronize(c->ring[k][1]));
    PT_HIP(hipEventElapsedTime(&t, c->ring[0][0], c->ring[k][1]));
    span = t > span ? t : span;
  }
  *ms = span;
  *n_out = (size_t)(c->ring_launch[c->ring_n - 1] - c->ring_launch[0] + 1);   // launches the span covers
  return PT_OK;
}

int pt_reset_launch_times(pt_context* c) {
  if (c && c->group) return ptg::reset_launch_times(c->group);
  if (!c) return fail(PT_ERR_INVALID, "null context");
  c->ring_n = 0;
  c->launch_n = 0;
  return PT_OK;
}

int pt_selftest_math(int device, int fn, const float* x, float* y, size_t n) {
  if (!x || !y) return fail(PT_ERR_INVALID, "null argument");
  if (n == 0) return PT_OK;
  PT_HIP(hipSetDevice(device));
  float *dx = nullptr, *dy = nullptr;
  PT_HIP(hipMalloc((void**)&dx, n * sizeof(float)));
  hipError_t e = hipMalloc((void**)&dy, n * sizeof(float));
  if (e == hipSuccess) e = hipMemcpy(dx, x, n * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = ptd::launch_math(fn, dx, dy, n, nullptr);
  if (e == hipSuccess) e = hipMemcpy(y, dy, n * sizeof(float), hipMemcpyDeviceToHost);
  (void)hipFree(dx);
  if (dy) (void)hipFree(dy);
  if (e != hipSuccess) return fail(PT_ERR_HIP, std::string("pt_selftest_math: ") + hipGetErrorString(e));
  return PT_OK;
}

int pt_selftest_exhaustive(int device, int fn, unsigned long long* mismatches, uint32_t* first_bad) {
  if (!mismatches || !first_bad) return fail(PT_ERR_INVALID, "null argument");
  if (fn < 0 || fn > 7) return fail(PT_ERR_INVALID, "fn must be 0..7");
  PT_HIP(hipSetDevice(device));
  unsigned long long* d_bad = nullptr;
  PT_HIP(hipMalloc((void**)&d_bad, 16));
  hipError_t e = hipMemset(d_bad, 0, 8);
  if (e == hipSuccess) e = hipMemset((char*)d_bad + 8, 0xff, 4);
  if (e == hipSuccess) e = ptd::launch_exhaustive(fn, d_bad, (uint32_t*)((char*)d_bad + 8), nullptr);
  if (e == hipSuccess) e = hipMemcpy(mismatches, d_bad, 8, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(first_bad, (char*)d_bad + 8, 4, hipMemcpyDeviceToHost);
  (void)hipFree(d_bad);
  if (e != hipSuccess) return fail(PT_ERR_HIP, std::string("pt_selftest_exhaustive: ") + hipGetErrorString(e));
  return PT_OK;
}

int pt_partition_items(int w, int h, int spl, int nranks, int rank, const int* slots, const float* cull_rects,
                       int n_cull, int item_order, int* live, size_t* n_live, int* culled, size_t* n_culled,
                       int* pixel_of) {
  if (!n_live || !n_culled) return fail(PT_ERR_INVALID, "null argument");
  if (w <= 0 || h <= 0) return fail(PT_ERR_INVALID, "bad resolution");
  if (spl != 1 && spl != 2 && spl != 4 && spl != 8) return fail(PT_ERR_INVALID, "sample lanes must be 1, 2, 4 or 8");
  if (nranks < 1 || rank < 0 || rank >= nranks) return fail(PT_ERR_INVALID, "bad partition");
  if (n_cull > ptd::kMaxCullRects || (n_cull > 0 && !cull_rects)) return fail(PT_ERR_INVALID, "bad cull rectangles");
  std::vector<int> sl((size_t)nranks, 1);
  if (slots) {
    long long m = 0;
    for (int r = 0; r < nranks; ++r) {
      if (slots[r] < 1 || slots[r] > ptd::kMaxSlots) return fail(PT_ERR_INVALID, "partition slots must be 1..64");
      sl[r] = slots[r];
      m += slots[r];
    }
    if (m > 4096) return fail(PT_ERR_INVALID, "more than 4096 partition slots");
  }
  ptd::RenderParams p{};
  p.width = w;
  p.height = h;
  p.spl = spl;
  p.blocks_x = (w + 15) / 16;
  p.blocks_total = p.blocks_x * ((h + 15) / 16);
  p.n_cull = n_cull < 0 ? -1 : n_cull;
  for (int r = 0; r < n_cull; ++r)
    for (int k = 0; k < 4; ++k) p.cull[r][k] = cull_rects[4 * r + k];
  p.item_order = item_order;
  const ptd::Part pt = parts_of_slots(sl)[(size_t)rank];
  std::vector<int> lv, cu;
  item_lists(p, pt, &lv, &cu);
  if ((live && *n_live < lv.size()) || (culled && *n_culled < cu.size()))
    return fail(PT_ERR_INVALID, "item buffers too small");
  if (live) std::copy(lv.begin(), lv.end(), live);
  if (culled) std::copy(cu.begin(), cu.end(), culled);
  if (pixel_of) {   // the kernels' item -> pixel map (tile_pixel), live items first
    const int per = 256 / spl;
    size_t o = 0;
    for (const std::vector<int>* v : {&lv, &cu})
      for (int item : *v) {
        const int tile = ptd::part_tile(pt, item / spl), part = item % spl;
        int bx, by;
        ptd::tile_block(tile, p.blocks_x, &bx, &by);
        for (int q = 0; q < per; ++q, ++o) {
          const int px = bx * 16 + q % 16, py = by * 16 + part * (16 / spl) + q / 16;
          pixel_of[o] = (tile < p.blocks_total && px < w && py < h) ? py * w + px : -1;
        }
      }
  }
  *n_live = lv.size();
  *n_culled = cu.size();
  return PT_OK;
}

}  // extern "C"
