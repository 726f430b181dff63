// pt_device.hip — the CDNA4 path-tracing kernels: one translation unit.  The
// device code lies in csrc/kernels/*.h by subsystem, included below in
// dependency order; this file holds the host launchers and, per kernel
// family, the table of its instantiations (chosen by pt_device.h's pure
// plan_render / plan_wavefront).
//
// One thread per pixel, one 64-lane wave per 8x8 pixel tile, four waves per
// 256-thread workgroup covering a 16x16 block (the reference's workgroup
// footprint, raytrace_comp.comp:43).  Each thread runs n_batches consecutive
// samples of its pixel and folds them into the running mean in registers, so
// the accumulation buffer is read and written once per launch instead of once
// per sample; the op sequence per sample is identical to n separate 1-spp
// dispatches (raytrace_comp.comp:467-469).
//
// Traversal (raytrace_comp.comp:159-204) is the reference's exhaustive DFS,
// executed stack-free over the threaded layout documented in pt_device.h: the
// node visit sequence, the AABB tests and the strict '<' tie-break are the
// reference's, so hits are bit-identical.  Two exact shortcuts:
//   * shadow rays only need "is there a hit closer than the light"
//     (:359, :398) — any accepted triangle with t < 1e30 and !(t >= limit)
//     settles it, so traversal stops there;
//   * the light pre-pass (:319-320) traces exactly the depth-0 ray (:333), so
//     that closest hit is computed once and used for both.
// In stats mode neither shortcut is taken and every reference traceRay call
// is counted with its exhaustive node/leaf counts.
//
// Numerics: every float op is the reference's, in its order, via pt_math.h;
// the file is compiled with -ffp-contract=off and correctly rounded div/sqrt.
#include <algorithm>

#include "pt_device.h"
#include "pt_camera_ray.h"
#include "pt_cull.h"
#include "pt_denoise.h"
#include "pt_isect.h"
#include "wide_walk.h"
#include "sweep_walk.h"
#include "pt_math.h"

#pragma clang fp contract(off)

namespace ptd {
using namespace ptm;

namespace {

#include "kernels/walks.h"
#include "kernels/shading.h"
#include "kernels/render.h"
#include "kernels/small.h"
#include "kernels/wf_state.h"
#include "kernels/wf_trace.h"
#include "kernels/wf_wide.h"
#include "kernels/wf_shade.h"
#include "kernels/wf_adaptive.h"
#include "kernels/guide.h"
#include "kernels/adaptive.h"
#include "kernels/rays.h"
#include "kernels/radiance.h"

}  // namespace

hipError_t launch_math(int fn, const float* x, float* y, size_t n, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  math_kernel<<<(unsigned)((n + 255) / 256), 256, 0, stream>>>(fn, x, y, n);
  return hipGetLastError();
}

hipError_t launch_exhaustive(int fn, unsigned long long* bad, uint32_t* first_bad, hipStream_t stream) {
  exhaustive_kernel<<<8192, 256, 0, stream>>>(fn, bad, first_bad);
  return hipGetLastError();
}

hipError_t launch_setup_tris(const float* d_vertices, const uint32_t* d_indices, int n_tris, float4* d_tris,
                             hipStream_t stream) {
  if (n_tris <= 0) return hipSuccess;
  setup_tris_kernel<<<(n_tris + 255) / 256, 256, 0, stream>>>(d_vertices, d_indices, n_tris, d_tris);
  return hipGetLastError();
}

hipError_t launch_gather_tris(const float4* tris, const int* tri_of, int n, float4* dst, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  gather_tris_kernel<<<(unsigned)((3ll * n + 255) / 256), 256, 0, stream>>>(tris, tri_of, n, dst);
  return hipGetLastError();
}

hipError_t launch_setup_lights(const LightRec* d_in, int n, LightDev* d_out, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  setup_lights_kernel<<<(n + 63) / 64, 64, 0, stream>>>(d_in, n, d_out);
  return hipGetLastError();
}

int owned_tiles(int width, int height, const Part& part) {
  return part_count(part, ((width + 15) / 16) * ((height + 15) / 16));
}

hipError_t launch_tiles(bool pack, float4* frame, float4* packed, int width, int height, const Part& part,
                        const int* d_pos, hipStream_t stream) {
  const int n = owned_tiles(width, height, part);
  if (n <= 0) return hipSuccess;
  const int bx = (width + 15) / 16;
  if (pack)
    tiles_kernel<true><<<n, 256, 0, stream>>>(frame, packed, width, height, bx, part.m, part.cnt, d_pos);
  else
    tiles_kernel<false><<<n, 256, 0, stream>>>(frame, packed, width, height, bx, part.m, part.cnt, d_pos);
  return hipGetLastError();
}

hipError_t launch_items_pack(const RenderParams& p, const float4* frame, float4* packed, const int* items, int n,
                             hipStream_t stream) {
  const long long px = (long long)n * (256 / p.spl);
  if (px == 0) return hipSuccess;
  items_pack_kernel<<<(unsigned)((px + 255) / 256), 256, 0, stream>>>(p, frame, packed, items, n);
  return hipGetLastError();
}

hipError_t launch_items_unpack(const RenderParams& p, float4* frame, const float4* src, size_t slot_f4,
                               const int* table, int n, hipStream_t stream) {
  const long long px = (long long)n * (256 / p.spl);
  if (px == 0) return hipSuccess;
  items_unpack_kernel<<<(unsigned)((px + 255) / 256), 256, 0, stream>>>(p, frame, src, slot_f4, table, n);
  return hipGetLastError();
}

hipError_t launch_clear(float4* accum, int width, int height, const Part& part, const int* d_pos, hipStream_t stream) {
  const size_t n = (size_t)width * (size_t)height;
  if (n == 0) return hipSuccess;
  clear_kernel<<<(unsigned)((n + 255) / 256), 256, 0, stream>>>(accum, width, height, part.m, part.cnt, d_pos);
  return hipGetLastError();
}

namespace {

// One table per kernel family: the instantiations pt_device.h lists, by their variant.
template <class V, class K>
struct KernelEntry {
  V v;
  K kern;
};
template <class V, class K, size_t N>
K find_kernel(const KernelEntry<V, K> (&table)[N], const V& v) {   // nullptr: no such instantiation
  for (const KernelEntry<V, K>& e : table)
    if (e.v == v) return e.kern;
  return nullptr;
}
typedef void (*RenderKernel)(RenderParams);
typedef void (*WfKernel)(RenderParams, WfBuffers, int);
#define PT_ROW(S, L, C, W, M, E) {{S, L, C, W, M, E}, render_kernel<S, L, C, W, M, E>},
const KernelEntry<RenderVariant, RenderKernel> kRenderKernels[] = {PT_RENDER_VARIANTS(PT_ROW)};
#undef PT_ROW

// Workgroups of `kern` resident on this device at once at `lds` bytes of dynamic LDS: CUs x blocks per CU,
// a kernel that reports no resident block counting as min_per_cu.
template <class K>
hipError_t resident_blocks(K kern, size_t lds, int min_per_cu, long long* blocks) {
  int dev = 0, cus = 0, per_cu = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  if (e == hipSuccess) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, 256, lds);
  *blocks = (long long)cus * std::max(per_cu, min_per_cu);
  return e;
}

}  // namespace

hipError_t launch_render(const RenderParams& p, bool stats, bool lds_scene, hipStream_t stream, bool cnt) {
  const RenderLaunch l = plan_render(p, stats, lds_scene, cnt, kPixPerFill);
  if (l.what == Launch::Nothing) return hipSuccess;
  const RenderKernel kern = l.what == Launch::Run ? find_kernel(kRenderKernels, l.v) : nullptr;
  if (!kern) return hipErrorInvalidValue;
  if (l.grid > 0) hipLaunchKernelGGL(kern, dim3((unsigned)l.grid), dim3(256), l.lds, stream, p);
  return hipGetLastError();
}

hipError_t launch_guide(const RenderParams& p, float4* guide, bool lds_scene, hipStream_t stream) {
  const int n_tiles = p.blocks_total;
  if (n_tiles <= 0) return hipSuccess;
  void (*kern)(RenderParams, float4*, int);
  if (p.wide) {   // the culled wide walk; every lane needs its overflow stack area
    if (p.wide_ovf_lanes < 256) return hipErrorInvalidValue;
    const unsigned grid = (unsigned)std::min<long long>(n_tiles, p.wide_ovf_lanes / 256);
    kern = p.wide_qn ? guide_kernel<2, true> : guide_kernel<2, false>;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, stream, p, guide, n_tiles);
    return hipGetLastError();
  }
  const size_t lds = lds_scene ? scene_lds_bytes(p) : 0;
  if (lds > kMaxSceneLds) return hipErrorInvalidValue;
  kern = lds_scene ? guide_kernel<1, false> : guide_kernel<0, false>;
  hipLaunchKernelGGL(kern, dim3((unsigned)n_tiles), dim3(256), lds, stream, p, guide, n_tiles);
  return hipGetLastError();
}

namespace {
// ... and the wavefront pipeline's four families (after the guide kernels: the order of the code object)
#define PT_ROW(Q, C) {{Q, C}, wf_trace_wide_kernel<C, Q ? 1 : 0>},
const KernelEntry<WfWideVariant, WfKernel> kWfWideKernels[] = {PT_WF_WIDE_VARIANTS(PT_ROW)};
#undef PT_ROW
#define PT_ROW(L, G, C) {{L, G, C}, wf_trace_kernel<L, G, C>},
const KernelEntry<WfTraceVariant, WfKernel> kWfTraceKernels[] = {PT_WF_TRACE_VARIANTS(PT_ROW)};
#undef PT_ROW
#define PT_ROW(E) {{E}, wf_shade_kernel<E>},
const KernelEntry<WfShadeVariant, WfKernel> kWfShadeKernels[] = {PT_WF_SHADE_VARIANTS(PT_ROW)};
#undef PT_ROW
#define PT_ROW(C, Q, E) {{C, Q, E}, wf_tail_kernel<C, Q, E>},
const KernelEntry<WfTailVariant, WfKernel> kWfTailKernels[] = {PT_WF_TAIL_VARIANTS(PT_ROW)};
#undef PT_ROW
}  // namespace

long long render_slots(size_t lds_bytes, bool sweep) {
  // of the plain LDS kernel, or -- for any sweep table -- of the hull table's walk
  const RenderKernel kern = find_kernel(kRenderKernels, RenderVariant{false, true, false, sweep ? 2 : 0, false, false});
  long long blocks = 0;
  return kern && resident_blocks(kern, lds_bytes, 0, &blocks) == hipSuccess ? blocks : 0;
}

long long wide_trace_lanes() {
  long long most = 0, blocks = 0;
  for (const auto& e : kWfWideKernels) {
    if (resident_blocks(e.kern, 0, 1, &blocks) != hipSuccess) return 0;
    most = std::max(most, blocks);
  }
  return most * 256;
}

namespace {
// The kernels of a wavefront launch's ray rounds and their persistent grids: the trace kernel (the culled
// wide walk, PT_OPT_WIDE, or the threaded one), the shading kernel, the tail kernel where planned
// (PT_OPT_WF_TAIL); the exit skip picks the shading and tail kernels' EXIT instantiations (generation never
// reaches a bounce).
struct WfKernels {
  WfKernel trace = nullptr, shade = nullptr, tail = nullptr;
  unsigned grid_t = 0, grid_s = 0, grid_x = 0;
};
hipError_t wf_kernels(const WfPick& pick, size_t lds_t, const RenderParams& p0, WfKernels* k) {
  k->trace = pick.wide ? find_kernel(kWfWideKernels, pick.wide_trace) : find_kernel(kWfTraceKernels, pick.trace);
  k->shade = find_kernel(kWfShadeKernels, pick.shade);
  k->tail = pick.tail ? find_kernel(kWfTailKernels, pick.tail_v) : nullptr;
  if (!k->trace || !k->shade || (pick.tail && !k->tail)) return hipErrorInvalidValue;
  long long blocks_t = 0, blocks_s = 0, blocks_x = 0;
  hipError_t e = resident_blocks(k->trace, lds_t, 1, &blocks_t);
  if (e == hipSuccess) e = resident_blocks(k->shade, 0, 1, &blocks_s);
  if (e == hipSuccess && pick.tail) e = resident_blocks(k->tail, 0, 1, &blocks_x);
  if (e != hipSuccess) return e;
  k->grid_t = (unsigned)blocks_t;
  k->grid_x = (unsigned)blocks_x;
  // PT_OPT_WF_GRID: a smaller persistent grid gives each lane more rays per
  // round (a shorter drain relative to the round) when other frames' launches
  // fill the rest of the GPU
  if (p0.wf_grid > 0 && p0.wf_grid < 100)
    k->grid_t = std::max(1u, (unsigned)((unsigned long long)k->grid_t * p0.wf_grid / 100));
  if (pick.wide) {   // every lane needs its overflow stack area
    k->grid_t = std::min<unsigned>(k->grid_t, (unsigned)(p0.wide_ovf_lanes / 256));
    k->grid_x = std::min<unsigned>(k->grid_x, (unsigned)(p0.wide_ovf_lanes / 256));
  }
  k->grid_s = (unsigned)blocks_s;
  return hipSuccess;
}
}  // namespace

hipError_t launch_wavefront(const RenderParams& p0, const WfBuffers& b, bool lds_scene, hipStream_t stream, bool cnt,
                            hipStream_t stream2, hipEvent_t ev_fork, hipEvent_t ev_join) {
  const WfLaunch l = plan_wavefront(p0, b.cap, lds_scene, cnt, kPixPerFill, kWfGroup4Tris);
  if (l.stop == WfStop::Refused) return hipErrorInvalidValue;
  if (l.stop == WfStop::Nothing) return hipSuccess;
  if (l.fill_grid > 0) fill_culled_kernel<<<(unsigned)l.fill_grid, 256, 0, stream>>>(p0);
  if (l.stop == WfStop::FillOnly) return hipGetLastError();
  if (l.stop == WfStop::FillRefused) return hipErrorInvalidValue;
  const long long px = l.px;
  WfKernels k;
  hipError_t e = wf_kernels(l.k, l.lds_trace, p0, &k);
  if (e != hipSuccess) return e;
  const bool tail = l.k.tail;
  const WfKernel trace = k.trace, shade = k.shade, tailk = k.tail;
  const size_t lds_t = l.lds_trace;
  const unsigned grid_t = k.grid_t, grid_s = k.grid_s, grid_x = k.grid_x;
  const uint32_t chunk = (uint32_t)std::min<long long>((long long)p0.n_batches, b.cap / px);
  const int iters = wf_max_rays(p0);
  // Two halves of the chunk's pixels on two streams (PT_OPT_WF_STREAMS):
  // each trace launch ends in a tail where most lanes are out of rays
  // (lane census: ~50 % of lane-steps idle), which the other half's trace
  // and shading fill.  The halves share the path state (disjoint ranges)
  // and get their own lists, counters and stack overflow areas.
  const bool split = stream2 && px >= 2 * 4096;
  const int H = split ? 2 : 1;
  for (uint32_t b0 = 0; b0 < p0.n_batches; b0 += chunk) {
    RenderParams p = p0;
    p.first_batch = p0.first_batch + b0;
    p.n_batches = std::min(chunk, p0.n_batches - b0);
    RenderParams ph[2] = {p, p};
    WfBuffers bh[2] = {b, b};
    hipStream_t sh[2] = {stream, split ? stream2 : stream};
    long long px0[2] = {0, 0}, pxn[2] = {px, 0};
    if (split) {
      pxn[0] = (px / 2 + 255) / 256 * 256;
      pxn[1] = px - pxn[0];
      px0[1] = pxn[0];
      const long long sb = pxn[0] * p.n_batches;   // half 1's paths and list slots start here
      for (int k = 0; k < 2; ++k) {
        bh[1].rays[k] = b.rays[k] + sb;   // slot s of half 1: rays[sb + s], rays[cap + sb + s]
        bh[1].ids[k] = b.ids[k] + sb;
        bh[1].state[k] = b.state[k] + sb;
      }
      bh[1].hits = b.hits + sb;
      bh[1].counters = b.counters + 4;
      ph[1].wide_ovf = p.wide_ovf ? p.wide_ovf + (size_t)p.wide_ovf_lanes * (size_t)p.wide_stack : nullptr;
      e = hipEventRecord(ev_fork, stream);
      if (e == hipSuccess) e = hipStreamWaitEvent(stream2, ev_fork, 0);
      if (e != hipSuccess) return e;
    }
    for (int h = 0; h < H; ++h) {
      const long long n = pxn[h] * p.n_batches;
      e = hipMemsetAsync(bh[h].counters, 0, 3 * sizeof(int), sh[h]);
      if (e != hipSuccess) return e;
      if (cnt)
        wf_gen_kernel<true><<<(unsigned)((n + 255) / 256), 256, 0, sh[h]>>>(ph[h], bh[h], n, px0[h] * p.n_batches);
      else
        wf_gen_kernel<false><<<(unsigned)((n + 255) / 256), 256, 0, sh[h]>>>(ph[h], bh[h], n, px0[h] * p.n_batches);
    }
    int cur = 0;
    for (int it = 0; it < iters; ++it) {
      for (int h = 0; h < H; ++h) hipLaunchKernelGGL(trace, dim3(grid_t), dim3(256), lds_t, sh[h], ph[h], bh[h], cur);
      if (tail)
        for (int h = 0; h < H; ++h) hipLaunchKernelGGL(tailk, dim3(grid_x), dim3(256), 0, sh[h], ph[h], bh[h], cur);
      for (int h = 0; h < H; ++h) hipLaunchKernelGGL(shade, dim3(grid_s), dim3(256), 0, sh[h], ph[h], bh[h], cur);
      cur ^= 1;
    }
    for (int h = 0; h < H; ++h)
      if (p.moments)
        wf_fold_kernel<true><<<(unsigned)((pxn[h] + 255) / 256), 256, 0, sh[h]>>>(ph[h], bh[h], pxn[h], px0[h]);
      else
        wf_fold_kernel<false><<<(unsigned)((pxn[h] + 255) / 256), 256, 0, sh[h]>>>(ph[h], bh[h], pxn[h], px0[h]);
    if (split) {
      e = hipEventRecord(ev_join, stream2);
      if (e == hipSuccess) e = hipStreamWaitEvent(stream, ev_join, 0);
      if (e != hipSuccess) return e;
    }
  }
  return hipGetLastError();
}

namespace {
// ... and the adaptive round's (last: the kernels before it keep their places in the code object)
typedef void (*AdaptiveKernel)(RenderParams, const int4*, const int*);
#define PT_ROW(L, W, E) {{L, W, E}, render_adaptive_kernel<L, W, E>},
const KernelEntry<AdaptiveVariant, AdaptiveKernel> kAdaptiveKernels[] = {PT_ADAPTIVE_VARIANTS(PT_ROW)};
#undef PT_ROW
}  // namespace

hipError_t launch_render_adaptive(const RenderParams& p, bool lds_scene, const int4* list, const int* n_live,
                                  hipStream_t stream) {
  const AdaptiveLaunch l = plan_render_adaptive(p, lds_scene);
  if (l.what == Launch::Nothing) return hipSuccess;
  const AdaptiveKernel kern = l.what == Launch::Run ? find_kernel(kAdaptiveKernels, l.v) : nullptr;
  if (!kern || !list || !n_live) return hipErrorInvalidValue;
  hipLaunchKernelGGL(kern, dim3((unsigned)l.grid), dim3(256), l.lds, stream, p, list, n_live);
  return hipGetLastError();
}

namespace {
// ... and the wavefront adaptive round's generation and fold (last again: kernels/wf_adaptive.h says why)
typedef void (*WfAdaptiveKernel)(RenderParams, WfBuffers, const int4*, const int*);
const WfAdaptiveKernel kWfGenAdaptive = wf_gen_adaptive_kernel<1>, kWfFoldAdaptive = wf_fold_adaptive_kernel<1>;
}  // namespace

// An adaptive round on the wavefront pipeline: launch_wavefront's chunk loop on one stream, with the live
// list in place of item lists and no culled-item fill (the fold writes every listed tile's pixels).
//
// The invariant that lets the host number the round: every tile starts at min_batches, a tile is live in a
// round only if it was live in every earlier one, and a live tile advances by min(step, max - n) -- so all
// live entries of one round hold the same {first_batch, n_batches}, which the host knows without reading
// the list.  They travel in p0 and advance per chunk as launch_wavefront's do; the list supplies origins only.
// The second stream (PT_OPT_WF_STREAMS 2) is not used: the host cannot halve a live pixel count it does not know.
// A round whose list is empty still enqueues everything; every workgroup finds nothing to do.
hipError_t launch_wavefront_adaptive(const RenderParams& p0, const WfBuffers& b, bool lds_scene, const int4* list,
                                     const int* n_live, hipStream_t stream) {
  const WfAdaptiveLaunch l = plan_wavefront_adaptive(p0, b.cap, lds_scene, kWfGroup4Tris);
  if (l.what == Launch::Nothing) return hipSuccess;
  if (l.what != Launch::Run || !list || !n_live) return hipErrorInvalidValue;
  WfKernels k;
  hipError_t e = wf_kernels(l.k, l.lds_trace, p0, &k);
  if (e != hipSuccess) return e;
  const int iters = wf_max_rays(p0);
  for (uint32_t b0 = 0; b0 < p0.n_batches; b0 += l.chunk) {
    RenderParams p = p0;
    p.first_batch = p0.first_batch + b0;
    p.n_batches = std::min(l.chunk, p0.n_batches - b0);
    e = hipMemsetAsync(b.counters, 0, 3 * sizeof(int), stream);
    if (e != hipSuccess) return e;
    const unsigned gen_grid = (unsigned)((long long)p.blocks_total * p.n_batches);
    hipLaunchKernelGGL(kWfGenAdaptive, dim3(gen_grid), dim3(256), 0, stream, p, b, list, n_live);
    int cur = 0;
    for (int it = 0; it < iters; ++it) {
      hipLaunchKernelGGL(k.trace, dim3(k.grid_t), dim3(256), l.lds_trace, stream, p, b, cur);
      if (l.k.tail) hipLaunchKernelGGL(k.tail, dim3(k.grid_x), dim3(256), 0, stream, p, b, cur);
      hipLaunchKernelGGL(k.shade, dim3(k.grid_s), dim3(256), 0, stream, p, b, cur);
      cur ^= 1;
    }
    hipLaunchKernelGGL(kWfFoldAdaptive, dim3((unsigned)l.fold_grid), dim3(256), 0, stream, p, b, list, n_live);
  }
  return hipGetLastError();
}

namespace {
// ... and the ray queries' (last once more: kernels/rays.h)
typedef void (*RaysExactKernel)(RenderParams, const float4*, void*, long long, int, const uint32_t*);
typedef void (*RaysWideKernel)(RenderParams, const float4*, void*, uint32_t, uint32_t*, const int*);
#define PT_ROW(K, L) {{K, L}, rays_exact_kernel<K, L>},
const KernelEntry<RaysExactVariant, RaysExactKernel> kRaysExactKernels[] = {PT_RAYS_EXACT_VARIANTS(PT_ROW)};
#undef PT_ROW
#define PT_ROW(K, Q, R) {{K, Q, R}, rays_wide_kernel<K, Q, R>},
const KernelEntry<RaysWideVariant, RaysWideKernel> kRaysWideKernels[] = {PT_RAYS_WIDE_VARIANTS(PT_ROW)};
#undef PT_ROW
}  // namespace

hipError_t launch_rays_slots(const int* rank_of, int n, int* slot_of, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  rays_slot_kernel<<<(unsigned)((n + 255) / 256), 256, 0, stream>>>(rank_of, n, slot_of);
  return hipGetLastError();
}

hipError_t launch_rays(const RenderParams& p, int kind, const void* rays, size_t n, void* out, uint32_t* counters,
                       const int* slot_of, bool lds_scene, bool refill, hipStream_t stream) {
  if (n > (size_t)kRaysMax) return hipErrorInvalidValue;
  long long wide_blocks = 0;
  RaysWideKernel wide = nullptr;
  if (p.wide) {   // the wide kernel the plan will pick, for its residency
    wide = find_kernel(kRaysWideKernels, RaysWideVariant{kind, p.wide_qn != 0, refill});
    if (!wide || !counters || !slot_of) return hipErrorInvalidValue;
    const hipError_t e = resident_blocks(wide, 0, 1, &wide_blocks);
    if (e != hipSuccess) return e;
  }
  const RaysLaunch l = plan_rays(p, kind, (long long)n, lds_scene, refill, wide_blocks);
  if (l.what == Launch::Nothing) return hipSuccess;
  const RaysExactKernel exact = l.what == Launch::Run ? find_kernel(kRaysExactKernels, l.exact_v) : nullptr;
  if (!exact) return hipErrorInvalidValue;
  if (l.wide) {
    const hipError_t e = hipMemsetAsync(counters, 0, 2 * sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(wide, dim3((unsigned)l.grid_wide), dim3(256), 0, stream, p, (const float4*)rays, out,
                       (uint32_t)n, counters, slot_of);
  }
  hipLaunchKernelGGL(exact, dim3((unsigned)l.grid_exact), dim3(256), l.lds, stream, p, (const float4*)rays, out,
                     (long long)n, l.wide ? 1 : 0, (const uint32_t*)counters);
  return hipGetLastError();
}

namespace {
// ... and the radiance queries' (last: kernels/radiance.h)
typedef void (*RadianceKernel)(RenderParams, const float4*, float4*, long long, int, uint32_t, uint32_t);
#define PT_ROW(L, W, E) {{L, W, E}, radiance_kernel<L, W, E>},
const KernelEntry<RadianceVariant, RadianceKernel> kRadianceKernels[] = {PT_RADIANCE_VARIANTS(PT_ROW)};
#undef PT_ROW
typedef void (*WfGenRaysKernel)(RenderParams, WfBuffers, const float4*, long long, int, uint32_t, uint32_t);
typedef void (*RadianceFoldKernel)(const float4*, float4*, long long, int, uint32_t);
typedef void (*CameraRaysKernel)(RenderParams, uint32_t, const int*, long long, float4*);
const WfGenRaysKernel kWfGenRays = wf_gen_rays_kernel<1>;
const RadianceFoldKernel kRadianceFold = radiance_fold_kernel<1>;
const CameraRaysKernel kCameraRays = camera_rays_kernel<1>;
}  // namespace

hipError_t launch_radiance(const RenderParams& p, bool lds_scene, const void* rays, long long q0, long long n_queries,
                           uint32_t n_samples, uint32_t seed_stride, float4* colors, void* out, hipStream_t stream) {
  const RadianceLaunch l = plan_radiance(p, false, lds_scene, n_queries, n_samples, 0, kWfGroup4Tris);
  if (l.what == Launch::Nothing) return hipSuccess;
  const RadianceKernel kern = l.what == Launch::Run ? find_kernel(kRadianceKernels, l.v) : nullptr;
  if (!kern || !rays || !colors || !out || q0 < 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(kern, dim3((unsigned)l.grid), dim3(256), l.lds, stream, p, (const float4*)rays, colors, q0,
                     (int)l.paths, n_samples, seed_stride);
  hipLaunchKernelGGL(kRadianceFold, dim3((unsigned)l.fold_grid), dim3(256), 0, stream, (const float4*)colors,
                     (float4*)out, q0, (int)n_queries, n_samples);
  return hipGetLastError();
}

// A chunk of queries on the wavefront pipeline: launch_wavefront's rounds on one stream behind the queries'
// generation, with the queries' fold in place of the pixels'.  No item lists, no fill, no second stream.
hipError_t launch_wavefront_rays(const RenderParams& p, const WfBuffers& b, bool lds_scene, const void* rays,
                                 long long q0, long long n_queries, uint32_t n_samples, uint32_t seed_stride, void* out,
                                 hipStream_t stream) {
  const RadianceLaunch l = plan_radiance(p, true, lds_scene, n_queries, n_samples, b.cap, kWfGroup4Tris);
  if (l.what == Launch::Nothing) return hipSuccess;
  if (l.what != Launch::Run || !rays || !out || q0 < 0) return hipErrorInvalidValue;
  WfKernels k;
  hipError_t e = wf_kernels(l.k, l.lds, p, &k);
  if (e != hipSuccess) return e;
  e = hipMemsetAsync(b.counters, 0, 3 * sizeof(int), stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kWfGenRays, dim3((unsigned)l.grid), dim3(256), 0, stream, p, b, (const float4*)rays, q0,
                     (int)l.paths, n_samples, seed_stride);
  const int iters = wf_max_rays(p);
  int cur = 0;
  for (int it = 0; it < iters; ++it) {
    hipLaunchKernelGGL(k.trace, dim3(k.grid_t), dim3(256), l.lds, stream, p, b, cur);
    if (l.k.tail) hipLaunchKernelGGL(k.tail, dim3(k.grid_x), dim3(256), 0, stream, p, b, cur);
    hipLaunchKernelGGL(k.shade, dim3(k.grid_s), dim3(256), 0, stream, p, b, cur);
    cur ^= 1;
  }
  hipLaunchKernelGGL(kRadianceFold, dim3((unsigned)l.fold_grid), dim3(256), 0, stream, (const float4*)b.colors,
                     (float4*)out, q0, (int)n_queries, n_samples);
  return hipGetLastError();
}

hipError_t launch_camera_rays(const RenderParams& p, uint32_t batch, const int* pixels, long long n, void* rays,
                              hipStream_t stream) {
  if (n == 0) return hipSuccess;
  if (n < 0 || n > kRaysMax || !rays || p.width <= 0 || p.height <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(kCameraRays, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, p, batch, pixels, n,
                     (float4*)rays);
  return hipGetLastError();
}

#ifdef PT_WG_TRACE
hipError_t wg_trace_read(unsigned long long* dst, int n) {
  if (n > kWgTraceCap) n = kWgTraceCap;
  const hipError_t e = hipDeviceSynchronize();
  if (e != hipSuccess) return e;
  return hipMemcpyFromSymbol(dst, HIP_SYMBOL(g_wg_trace), (size_t)n * 32, 0, hipMemcpyDeviceToHost);
}
#endif

}  // namespace ptd

#ifdef PT_WG_TRACE
extern "C" int pt_probe_wg_trace(unsigned long long* dst, int n) { return (int)ptd::wg_trace_read(dst, n); }
#endif
