// kernels/wf_shade.h — the wavefront pipeline's shading, tail and fold kernels
// (wf_shade_kernel, wf_tail_kernel, wf_fold_kernel) and fill_culled_kernel.
// A fragment: csrc/pt_device.hip includes it after kernels/wf_wide.h (the tail
// kernel runs its walk and flush), inside namespace ptd's anonymous namespace.

// Shading of every path in list `cur` (path_step on the returned hit);
// paths that need another ray go to list cur^1, finished ones store colour.
//
// With the wide walk a workgroup appends its next rays binned -- one atomic
// per workgroup, a counting sort in LDS -- by the phase the path waits in
// (closest-hit and shadow rays apart, and the next shading pass runs one case
// of path_step per wave instead of several).  A ray's result does not depend
// on where it sits in the list, so the image is unchanged.  Measured at 1080p
// 8 spp with the wide walk (single-lane refill, null queries inline): sphere
// 70.7 -> 65.0 ms, 10M cloud 181.5 -> 158.0 ms by phase; binned by ray kind
// and direction octant instead 65.7 / 158.3; by phase and octant 65.7 /
// 159.1.  (With the exhaustive walks and refill groups of round 2's first
// half, kind and octant had measured sphere -0.5 %, 10M cloud +3.5 %; the
// exhaustive walk keeps the unsorted lists.)
// A null shadow query (trav_null: its answer cannot change
// the image) is answered by the shading kernel itself, with the wide walk --
// path_step runs on with "unoccluded" -- instead of taking a list slot, a refill and a lane of
// the next traversal launch (where it started finished and left its lane
// idle until the wave's next refill) and a second shading pass.  The path's
// arithmetic and draws are the same; it only reaches its next real ray a
// round earlier.  1080p 8 spp, wide walk: sphere 75.1 -> 70.6 ms, 10M cloud
// 206 -> 181 ms; with the exhaustive threaded walk (PT_OPT_WIDE 0) the 10M
// cloud measured 2799 -> 2980 ms (paths drift out of phase), so it keeps the
// null rays in its lists.
#ifndef PT_WF_SHADE_MIN_BLOCKS
#define PT_WF_SHADE_MIN_BLOCKS 4
#endif
constexpr int kWfBins = 16;
template <bool EXIT = false>
__global__ __launch_bounds__(256, PT_WF_SHADE_MIN_BLOCKS) void wf_shade_kernel(RenderParams P, WfBuffers B, int cur) {
  if (blockIdx.x == 0 && threadIdx.x == 0) B.counters[2] = 0;   // the next traversal's cursor
  const int count = B.counters[cur];
  if (count < P.wf_tail) return;   // PT_OPT_WF_TAIL: wf_tail_kernel has finished these paths
  CamFrame F = {};   // camera frame: used by PH_BEGIN only
  __shared__ int bin_cnt[kWfBins], bin_base[kWfBins], wg_base;
  __shared__ int cand_buf[4][kCand][64];   // exact walks of handed-back rays
  int* cand = &cand_buf[threadIdx.x >> 6][0][threadIdx.x & 63];
  for (int base = (int)blockIdx.x * 256; base < count; base += (int)gridDim.x * 256) {
    const int i = base + (int)threadIdx.x;
    bool need = false;
    int p = -1;
    Trav T;
    PathSt S;
    if (i < count) {
      p = B.ids[cur][i];
      float4 r0, r1;
      wf_load_ray(B.rays[cur], B.cap, i, &r0, &r1);
      const float2 h = B.hits[i];
      T.o = mk(r0.x, r0.y, r0.z);
      T.d = mk(r1.x, r1.y, r1.z);
      wf_load_state(B, cur, i, T.o, T.d, &S);
      T.shadow = __float_as_int(r1.w) & kRayKindMask;
      T.lim = h.x;
      T.res = __float_as_int(h.y);
      int fused = 0;   // PT_OPT_WF_FUSE: 1 the path's next shadow ray was walked unoccluded, 2 occluded
      if (T.shadow == 0 && T.res >= 0 && (T.res & kHitFused)) {
        fused = (T.res & kHitOccluded) ? 2 : 1;
        T.res &= kHitRankMask;
      }
      T.nc = 0;
      T.cn = T.cl = 0u;
      Ctr c = {0u, 0u, 0u, 0u, 0u};
      if (T.shadow == 0 && T.res == kNeedExactClosest) {   // handed back by wf_trace_wide_kernel
        const Hit e = trace_closest<false, false, true, false>(P, T.o, T.d, c, cand);
        T.lim = e.t;
        T.res = e.tri >= 0 ? P.wide_rank_of[e.tri] : e.tri;   // a slot; hit_tris is by rank
      } else if (T.shadow == 1 && T.res == kNeedExactShadow) {
        T.res = occluded<false, false>(P, T.o, T.d, T.lim, c) ? 1 : 0;
      }
      v3 col;
      need = path_step<false, EXIT>(P, F, S, T, c, &col);
      if (fused) {
        // the shading just derived the shadow ray the trace kernel walked
        // (same hit, same draws, same ops): take its answer
        if (need && T.shadow != 0) {
          T.res = T.shadow == 2 ? 0 : fused - 1;
          need = path_step<false, EXIT>(P, F, S, T, c, &col);
        } else {   // cannot happen; fail loudly rather than shade wrongly
          need = false;
          col = mk(__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""));
        }
      }
      while (P.wide && need && T.shadow == 2) {   // a null shadow query (trav_null): unoccluded, answered here
        T.res = 0;
        need = path_step<false, EXIT>(P, F, S, T, c, &col);
      }
      if (!need) B.colors[p] = make_float4(col.x, col.y, col.z, 1.0f);
    }
    if (P.wide) {   // uniform: every thread of the workgroup runs each iteration
      const int tid = (int)threadIdx.x;
      if (tid < kWfBins) bin_cnt[tid] = 0;
      __syncthreads();
      const int bin = need ? (S.phase & 7) : 0;   // the phase the path waits in
      const int rank = need ? atomicAdd(&bin_cnt[bin], 1) : 0;
      __syncthreads();
      if (tid == 0) {
        int acc = 0;
        for (int k = 0; k < kWfBins; ++k) {
          bin_base[k] = acc;
          acc += bin_cnt[k];
        }
        wg_base = acc ? atomicAdd(&B.counters[cur ^ 1], acc) : 0;
      }
      __syncthreads();
      if (need) {
        const int slot = wg_base + bin_base[bin] + rank;
        wf_push(B, cur ^ 1, slot, p, T, fuse_bits(P, S, T), S.rng);
        wf_store_state(B, cur ^ 1, slot, S);
      }
      __syncthreads();   // the bins are reused by the next iteration
    } else {
      const int slot = wave_slot(&B.counters[cur ^ 1], need);
      if (need) {
        wf_push(B, cur ^ 1, slot, p, T, fuse_bits(P, S, T), S.rng);
        wf_store_state(B, cur ^ 1, slot, S);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// PT_OPT_WF_TAIL: the last paths of a chunk in one launch.  Every ray round
// of the pipeline ends when its longest walk ends, and a path needs a round
// per ray it traces (up to 33 at MAX_DEPTH 4, 65 at 8).  Late rounds hold few
// rays -- on a 1/8 tile share only a few per traversal lane from the start --
// so each costs about one long walk's latency plus three launches while most
// of the GPU idles.  Once a round's list holds fewer than P.wf_tail rays, this
// kernel takes the whole list instead of the trace and shading kernels: each
// lane claims a waiting path (its list slot) and runs it to the end -- walk
// (the culled wide walk with the trace kernel's queued leaf tests and
// wave-wide flushes), then path_step, then the next ray's walk in the same
// lane -- and stores the path's colour; the lanes whose walks have ended
// shade together at the check every PT_WIDE_STEPS steps, as the trace kernel
// finishes its walks.  The path's state waits in its own list slot
// (wf_store_state / wf_load_state) while the lane walks, so the walk keeps
// the trace kernel's registers.  The rays, draws, float operations and their
// order per path are those of the rounds (path_step on each returned hit,
// null shadow queries answered unoccluded, rays the wide walk does not take
// walked exactly): the image is bit-identical; the trace and shading kernels
// of that round and every later round find nothing to do.  No fused shadow
// walks here: path_step derives each shadow ray itself.
#ifndef PT_WF_TAIL_MIN_BLOCKS
#define PT_WF_TAIL_MIN_BLOCKS 4
#endif
template <bool CNT, bool QN, bool EXIT = false>
__global__ __launch_bounds__(256, PT_WF_TAIL_MIN_BLOCKS) void wf_tail_kernel(RenderParams P, WfBuffers B, int cur) {
  const int count = B.counters[cur];
  if (count == 0 || count >= P.wf_tail) return;
  const int tid = (int)threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  __shared__ int2 stk[4][kWideLds][64];
  int2* lds = &stk[wave][0][lane];
  // leaf queue; an exact walk's candidates (the queue is empty then)
  __shared__ int cq[4][kWideQ > kCand ? kWideQ : kCand][64];
  int* cand = &cq[wave][0][lane];
  __shared__ unsigned long long fkeys[4][64];
  const long long os = (long long)gridDim.x * 256;
  int2* ovf = P.wide_ovf + ((long long)blockIdx.x * 256 + tid);
  const float4* __restrict__ rays = B.rays[cur];
  const CamFrame F = {};   // no path begins here
  int p = -1;              // list slot of the lane's path
  bool fin = false;        // the lane's walk is over (its queue may still hold candidates)
  bool more = true;
  WideRay R;
  R.cur = -1;
  R.sp = R.lo = 0;
  R.nc = 0;
  R.shadow = 0;
  R.lim = 0.0f;
  R.best = 0;
  Ctr c = {0u, 0u, 0u, 0u, 0u};
  // the reference's traversal of the lane's ray by the exact threaded walk
  // (a ray the wide walk does not take, wide_ray_ok, or a stack bound hit)
  auto exact_walk = [&]() {
    Ctr cx = {0u, 0u, 0u, 0u, 0u};
    if (!R.shadow) {
      const Hit e = trace_closest<false, false, true, false>(P, R.o, R.d, cx, cand);
      R.lim = e.t;
      R.best = e.tri >= 0 ? P.wide_rank_of[e.tri] : e.tri;   // a slot; hit_tris is by rank
    } else {
      R.best = occluded<false, false>(P, R.o, R.d, R.lim, cx) ? 1 : 0;
    }
    R.nc = 0;
    fin = true;
  };
  // the lane's next ray: kind 0 closest, 1 shadow, 2 null shadow query (its
  // answer cannot change the image: unoccluded, no walk)
  auto begin = [&](v3 o, v3 d, int kind, float lim) {
    wide_start(R, o, d, kind != 0, lim);
    fin = true;
    if (kind == 2) {
      R.best = 0;
      return;
    }
    if (CNT) {
      c.rays += kind == 0 ? 1u : 0u;
      c.srays += kind == 1 ? 1u : 0u;
    }
    if (!wide_ray_ok(R.o, R.d, R.inv)) {
      exact_walk();
      return;
    }
    fin = false;
  };
  for (;;) {
    // lanes whose walk is over shade together: path_step on the answer, then
    // the path's next ray starts in the lane, or its colour is stored
    while (p >= 0 && fin && R.nc == 0) {
      Trav T;
      T.o = R.o;
      T.d = R.d;
      T.shadow = R.shadow;
      T.lim = R.lim;
      T.res = R.best;
      T.nc = 0;
      T.cn = T.cl = 0u;
      PathSt S;
      wf_load_state(B, cur, p, R.o, R.d, &S);   // PH_SSS: the walk ray is S.so / S.sd
      v3 col;
      bool need = path_step<false, EXIT>(P, F, S, T, c, &col);
      while (need && T.shadow == 2) {   // null shadow queries (trav_null)
        T.res = 0;
        need = path_step<false, EXIT>(P, F, S, T, c, &col);
      }
      if (need) {
        wf_store_state(B, cur, p, S);
        begin(T.o, T.d, T.shadow, T.lim);
      } else {
        B.colors[B.ids[cur][p]] = make_float4(col.x, col.y, col.z, 1.0f);
        p = -1;
        fin = false;
      }
    }
    const unsigned long long idle = __ballot(p < 0);
    const int ng = (int)__popcll(idle);
    if (more && ng >= PT_WIDE_REFILL) {
      int base = 0;
      if (lane == 0) base = atomicAdd(&B.counters[2], ng);
      base = __shfl(base, 0);
      if (base + ng >= count) more = false;
      if (p < 0) {
        const int slot = base + (int)__popcll(idle & ((1ull << lane) - 1ull));
        if (slot < count) {
          float4 r0, r1;
          wf_load_ray(rays, B.cap, slot, &r0, &r1);
          p = slot;
          // a closest ray's limit word may carry fuse bits' RNG state: unused
          // here (wide_start ignores a closest ray's limit)
          begin(mk(r0.x, r0.y, r0.z), mk(r1.x, r1.y, r1.z), __float_as_int(r1.w) & kRayKindMask, r0.w);
        }
      }
    }
    if (!more && __ballot(p >= 0) == 0ull) break;
    if (__ballot(p >= 0 && fin && R.nc == 0)) continue;   // shade first (a walk answered at its start)
    for (int it = 0; it < PT_WIDE_STEPS; ++it) {
      bool exact = false;
      if (p >= 0 && !fin)
        fin = wide_step<CNT, true, QN>(R, P.wide, P.wide_tris, lds, 64, ovf, os, P.wide_stack, &exact, &c.nodes,
                                       &c.leaves, cand, P.wide_leafbox);
      if (exact) exact_walk();   // the builder's stack bound rules this out; stay exact anyway
      const unsigned long long waiting = __ballot(p >= 0 && fin && R.nc > 0);
      if (__ballot(p >= 0 && R.nc > kWideQ - 4) || (int)__popcll(waiting) >= PT_WIDE_FLUSH_T ||
          (waiting && __ballot(p >= 0 && !fin) == 0ull)) {
        if (wide_flush_wave<CNT, QN>(R, p >= 0, P.wide_tris, cand, fkeys[wave], lane, &c.leaves, P.wide_leafbox)) {
          fin = true;   // occluded
          R.sp = 0;
          R.cur = -1;
        }
      }
      if (__ballot(p >= 0 && !(fin && R.nc == 0)) == 0ull) break;
    }
  }
  if (CNT) flush_traced(P, c, lane);
}

// Running mean (:467-469) of each pixel's samples, in batch order.
template <bool MOMENTS>
__global__ __launch_bounds__(256) void wf_fold_kernel(RenderParams P, WfBuffers B, long long n_pix, long long pp0) {
  const long long pp = pp0 + (long long)blockIdx.x * 256 + threadIdx.x;   // pixels [pp0, pp0 + n_pix)
  if (pp - pp0 >= n_pix) return;
  int px, py;
  if (!wf_pixel(P, pp, &px, &py)) return;
  float4* dst = P.accum + (size_t)py * (size_t)P.width + (size_t)px;
  float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (!(P.fresh && P.first_batch == 0)) {
    const float4 a = *dst;
    acc[0] = a.x; acc[1] = a.y; acc[2] = a.z; acc[3] = a.w;
  }
  float mom1 = 0.0f, mom2 = 0.0f;   // MOMENTS: the luminance moments, the same step (render_kernel)
  float2* mdst = nullptr;
  if constexpr (MOMENTS) {
    mdst = P.moments + (size_t)py * (size_t)P.width + (size_t)px;
    if (P.first_batch != 0) {
      const float2 m = *mdst;
      mom1 = m.x;
      mom2 = m.y;
    }
  }
  const float4* col = B.colors + (size_t)pp * P.n_batches;
  for (uint32_t s = 0; s < P.n_batches; ++s) {
    const float4 c = col[s];
    const uint32_t batch = P.first_batch + s;
    const float fb = (float)batch, fb1 = (float)(batch + 1u);
    acc[0] = (acc[0] * fb + c.x) / fb1;
    acc[1] = (acc[1] * fb + c.y) / fb1;
    acc[2] = (acc[2] * fb + c.z) / fb1;
    acc[3] = (acc[3] * fb + 1.0f) / fb1;
    if constexpr (MOMENTS) {
      const float L = ptdn::lum(c.x, c.y, c.z);
      mom1 = (mom1 * fb + L) / fb1;
      mom2 = (mom2 * fb + L * L) / fb1;
    }
  }
  if constexpr (MOMENTS) *mdst = make_float2(mom1, mom2);
  *dst = make_float4(acc[0], acc[1], acc[2], acc[3]);
}

__global__ __launch_bounds__(256) void fill_culled_kernel(RenderParams P) {
  fill_culled(P, P.culled_org, P.n_culled_items, (int)blockIdx.x);
}
