// kernels/wf_wide.h — the wavefront pipeline's traversal kernel over the
// culled wide walk (wf_trace_wide_kernel), with the fused shadow ray and the
// wave-wide candidate flush that the tail kernel shares.
// A fragment: csrc/pt_device.hip includes it after kernels/wf_trace.h (whose
// count_start it uses), inside namespace ptd's anonymous namespace.

// ---------------------------------------------------------------------------
// Culled wide walk (wide_walk.h) for scenes in device memory: 4-wide nodes of
// the reference's own boxes, nearest child first, children culled once no
// triangle in them can beat (or tie) the best hit -- the same answer as the
// exhaustive DFS, far fewer node fetches (CPU harness, 1M-triangle cloud,
// camera rays: 42 wide nodes and 4.3 triangle tests per ray against 1022
// nodes and 31 leaf tests).  Per lane: the ray, the node to expand, and a
// stack of pending (node, cull threshold) entries -- the top kWideLds in LDS
// ([entry][lane], conflict-free), older ones in a per-lane global overflow
// area (P.wide_ovf, strided by lane so neighbouring lanes' spills coalesce).
// Rays the walk does not take (zero / subnormal direction components) return
// kNeedExact* and wf_shade_kernel walks them exactly (trace_closest /
// occluded).
// ---------------------------------------------------------------------------
// Refill group of the wide walk: single lanes (G = 1).  Lane census of the
// wide walk with G = 4 on the 10M cloud: 56 % of lane-steps idle while the
// list still held rays -- a lane could refill only once its whole aligned
// group of four was idle.  G = 1 vs the earlier choice (2 below 500K
// triangles, 4 above): sphere 78.0 -> 75.1 ms, 10M cloud 237 -> 206 ms;
// the refill threshold is P.wide_refill (PT_OPT_WF_REFILL; PT_WIDE_REFILL for
// the tail kernel).
// refill threshold of the wide walk: 16 idle lanes.  Before the finished
// walks were batched at the refill check (wf_trace_wide_kernel), 24 measured
// best (sphere -0.9 %, 10M cloud -0.35 % against 32; 16 then +3 %); with
// them batched, 16 against 24: sphere -2 %, 10M cloud -1.5 % (DESIGN item
// 36); 12: +0.2 % / +4 %, 8: +7 % / +31 %.
#ifndef PT_WIDE_REFILL
#define PT_WIDE_REFILL 16
#endif
// steps between the wide walk's refill checks: 12 (with the wave-wide flush,
// item 39): 10M cloud -1.7 %, sphere -0.1 % against 8; 16: -0.5 % / +0.6 %
#ifndef PT_WIDE_STEPS
#define PT_WIDE_STEPS 12
#endif
// finished walks waiting on their leaf queue that make the wave flush
#ifndef PT_WIDE_FLUSH_T
#define PT_WIDE_FLUSH_T 1
#endif
#ifndef PT_WIDE_MIN_BLOCKS
// 6: the LDS stack and leaf queue (96 B per lane) fit 6 workgroups per CU;
// 79 VGPRs, no spills.  8 workgroups with a 6-entry stack ring (80 B per lane,
// 64 VGPRs, 60 B spilled): sphere +6.5 %, 10M cloud +5.4 %; with 7: +1 %.
#define PT_WIDE_MIN_BLOCKS 6
#endif
// PT_OPT_WF_FUSE: the shadow ray pathTrace traces right after closest hit
// (t, rank) of ray (o, d), from the path's RNG state `rng` -- light 0's
// sample, direction, diffuse term and distance with the ops of path_step's
// PH_DIRECT / PH_SSS_SHADOW (:345-366, :383-402; the hit point o + d t is
// S.hp / S.cp, the normal the record's).  0: none (a primary ray's light
// pre-pass, :311-328, ends the path); 1: answered without a walk (its answer
// cannot change the image, shadow_needed); 2: walk (so, sd) up to lim.
__device__ __forceinline__ int fused_shadow_ray(const RenderParams& P, v3 o, v3 d, float t, int rank, bool primary,
                                                uint32_t rng, v3* so, v3* sd, float* lim) {
  if (primary) {
    for (int i = 0; i < P.n_lights; ++i) {
      float tl;
      if (intersect_area_light(o, d, load_light(P, i), &tl) && t > tl) return 0;   // lit: T.res >= 0 here
    }
  }
  const float OFFSET = 0.001f;
  const v3 hp = add(o, muls(d, t));
  const v3 hn = tri_normal(P, rank);
  const LightDev L = load_light(P, 0);
  const LightSample s = sample_light(L, hp, hn, &rng);
  if (!shadow_needed(L, s.diff)) return 1;
  *so = add(hp, muls(hn, OFFSET));
  *sd = s.dir;
  *lim = s.dist - OFFSET;
  return 2;
}
constexpr int kFuseWalk = 16;   // lane state: walking the fused shadow ray

// The wave's queued leaf candidates tested one per lane.
// wide_flush runs a lane's queue in its own lane, so a flush takes as many
// loop trips as the longest queue while the others idle: a probe of the trace
// kernel (tools/flush_probe.py) measured 67 candidates per flush on the
// displaced sphere and 38 on the 10M cloud, against a longest queue of 5.8 /
// 4.7 -- 18 % / 13 % of the flush loop's lane slots in use.  Here the
// candidates are numbered across the wave (a prefix sum of the queue
// lengths), and lane j of each window of 64 tests candidate j: it finds the
// owner by a binary search over the prefix sums, reads the rank from the
// owner's queue column, the owner's ray by lane shuffles, and runs the same
// triangle test and accept rules.  The owner's answer is a lexicographic
// minimum of (t, rank) -- an LDS atomic min of (t bits << 32 | rank), t > 0
// (tri_test accepts t > 1e-6), so its bits order as its value -- merged with
// the owner's best by wide_cand's own rule; a shadow ray is occluded if any
// of its candidates is an accepted hit below its limit.  Neither answer
// depends on the order the candidates are tested in (ties go to the lower
// rank, the reference's visit order): the same hits as wide_flush.  Call with
// every lane of the wave active; keys: the wave's 64 LDS words; returns true
// for a shadow ray found occluded.
// Inclusive prefix sum over the wave's 64 lanes (every lane active) by DPP
// row shifts within each row of 16 and row broadcasts across rows: six VALU
// steps, where __shfl_up made six dependent LDS-crossbar round trips.
__device__ __forceinline__ int wave_incl_sum(int v) {
  v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false);   // row_shr:1
  v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false);   // row_shr:2
  v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false);   // row_shr:4
  v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false);   // row_shr:8
  v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);   // row_bcast:15 into rows 1, 3
  v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);   // row_bcast:31 into rows 2, 3
  return v;
}
template <bool CNT, bool QN>
__device__ __forceinline__ bool wide_flush_wave(WideRay& R, bool mine, const float4* __restrict__ tris, const int* cand,
                                                unsigned long long* keys, int lane, uint32_t* cl,
                                                const float4* __restrict__ leaf_box) {
  const int n = mine ? R.nc : 0;
  const int incl = wave_incl_sum(n);   // inclusive prefix sum of the queue lengths
  const int total = __builtin_amdgcn_readlane(incl, 63);
  const int off = incl - n;
  keys[lane] = ~0ull;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const int* qbase = cand - lane;   // the wave's queue: [k][lane]
  for (int base = 0; base < total; base += 64) {
    const int target = base + lane;
    int L = 0;   // the owner: lanes whose inclusive sum is <= target
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
      const int v = __shfl(incl, L + s - 1);
      if (v <= target) L += s;
    }
    L = min(L, 63);
    const int offL = __shfl(off, L);
    const v3 o = mk(__shfl(R.o.x, L), __shfl(R.o.y, L), __shfl(R.o.z, L));
    const v3 d = mk(__shfl(R.d.x, L), __shfl(R.d.y, L), __shfl(R.d.z, L));
    const float lim = __shfl(R.lim, L);
    const int shadow = __shfl(R.shadow, L);
    if (target < total) {
      const int r = wide_qrank(qbase[(target - offL) * 64 + L]);
      const float4* T = tris + 3 * (size_t)r;
      const float4 A = T[0], B = T[1], C = T[2];
      if (CNT) ++*cl;
      float t;
      // shadow: :359 / :398; closest: a hit that can still win (t == lim may
      // tie with a lower rank)
      if (tri_test(o, d, A, B, C, &t) && t < 1e30f && (shadow ? !(t >= lim) : t <= lim)) {
        bool ok = true;
        if (QN) ok = slab(o, mk(rcp_(d.x), rcp_(d.y), rcp_(d.z)), leaf_box[2 * (size_t)r], leaf_box[2 * (size_t)r + 1]);
        if (ok) atomicMin(&keys[L], shadow ? 0ull : ((unsigned long long)__float_as_uint(t) << 32) | (uint32_t)r);
      }
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  if (n == 0) return false;
  R.nc = 0;
  const unsigned long long k = keys[lane];
  if (k == ~0ull) return false;
  if (R.shadow) {
    R.best = 1;
    return true;
  }
  const float tm = __uint_as_float((uint32_t)(k >> 32));
  const int rm = (int)(uint32_t)k;
  if (tm < R.lim || (tm == R.lim && R.best >= 0 && rm < R.best)) {   // wide_cand's rule
    R.lim = tm;
    R.best = rm;
  }
  return false;
}

// LAYOUT: 0 128-B 4-wide nodes, 1 64-B 4-wide nodes (QN)
template <bool CNT = false, int LAYOUT = 1>
__global__ __launch_bounds__(256, PT_WIDE_MIN_BLOCKS) void wf_trace_wide_kernel(RenderParams P, WfBuffers B,
                                                                                int cur) {
  constexpr bool QN = LAYOUT >= 1;
  const int tid = (int)threadIdx.x;
  if (blockIdx.x == 0 && tid == 0) B.counters[cur ^ 1] = 0;   // filled by the shading that follows
  const int count = B.counters[cur];
  if (count == 0 || count < P.wf_tail) return;   // PT_OPT_WF_TAIL: wf_tail_kernel finishes the list
  const int wave = tid >> 6, lane = tid & 63;
  __shared__ int2 stk[4][kWideLds][64];
  int2* lds = &stk[wave][0][lane];
  __shared__ int cq[4][kWideQ][64];   // the lanes' leaf queues (wide_walk.h)
  int* cand = &cq[wave][0][lane];
  __shared__ unsigned long long fkeys[4][64];
  bool fin = false;
  const long long os = (long long)gridDim.x * 256;
  int2* ovf = P.wide_ovf + ((long long)blockIdx.x * 256 + tid);
  const float4* __restrict__ rays = B.rays[cur];
  int p = -1;   // list slot this lane traces
  bool more = true;
  WideRay R;
  R.cur = -1;
  R.sp = R.lo = 0;
  R.nc = 0;
  // PT_OPT_WF_FUSE: fz = the ray's kRayFuse / kRayPrimary bits, or kFuseWalk
  // while the lane walks the fused shadow ray; aux = the path's RNG state,
  // then the closest hit's t; cr = its rank
  int fz = 0, cr = 0;
  uint32_t aux = 0u;
  Ctr c = {0u, 0u, 0u, 0u, 0u};
  // A lane whose walk is over (fin, queue empty): its answer goes to the
  // hit list -- or, after a closest hit whose first-light shadow ray the
  // trace kernel walks (PT_OPT_WF_FUSE), that ray starts in the lane.
  auto finish = [&]() {
    float t = R.lim;
    int res = R.best;   // occluded, or the hit's rank (hit_tris = wide_tris; the record the flush just tested)
    bool done = true;
    if (fz & kFuseWalk) {   // the fused shadow ray's answer joins its closest hit
      t = __uint_as_float(aux);
      res = cr | kHitFused | (R.best ? kHitOccluded : 0);
    } else if ((fz & kRayFuse) && R.best >= 0) {
      v3 so, sd;
      float lim;
      const int k = fused_shadow_ray(P, R.o, R.d, R.lim, R.best, (fz & kRayPrimary) != 0, aux, &so, &sd, &lim);
      if (k == 1) {
        res = R.best | kHitFused;   // unoccluded without a walk
      } else if (k == 2) {
        cr = R.best;
        aux = __float_as_uint(R.lim);
        wide_start(R, so, sd, true, lim);
        if (wide_ray_ok(R.o, R.d, R.inv)) {   // walk it in this lane now
          fz = kFuseWalk;
          fin = false;
          done = false;
          if (CNT) ++c.srays;
        } else {   // the shading's next round hands it to the exact walk
          t = __uint_as_float(aux);
          res = cr;
        }
      }
    }
    if (done) {
      B.hits[p] = make_float2(t, __int_as_float(res));
      p = -1;
      fin = false;
      fz = 0;
    }
  };
  for (;;) {
    // The lanes whose walks ended since the last check finish here together,
    // not in the step their walk ended in (where the wave ran the finishing
    // code -- the fused shadow ray's light sample, normalisations and start --
    // for one or two lanes at a time)
    if (p >= 0 && fin && R.nc == 0) finish();
    // every idle lane refills on its own (no refill groups: see above)
    const unsigned long long idle = __ballot(p < 0);
    const int need = (int)__popcll(idle);
    if (more && need >= P.wide_refill) {
      int base = 0;
      if (lane == 0) base = atomicAdd(&B.counters[2], need);
      base = __shfl(base, 0);
      if (base + need >= count) more = false;
      if ((idle >> lane) & 1ull) {
        const int slot = base + (int)__popcll(idle & ((1ull << lane) - 1ull));
        if (slot < count) {
          float4 r0, r1;
          wf_load_ray(rays, B.cap, slot, &r0, &r1);
          const int kbits = __float_as_int(r1.w);
          const int kind = kbits & kRayKindMask;   // 0 closest, 1 shadow, 2 null shadow (trav_null)
          if (CNT) count_start(r1, c);
          wide_start(R, mk(r0.x, r0.y, r0.z), mk(r1.x, r1.y, r1.z), kind != 0, r0.w);
          fz = kbits & (kRayFuse | kRayPrimary);
          aux = __float_as_uint(r0.w);
          if (kind == 2) {
            B.hits[slot] = make_float2(R.lim, __int_as_float(0));
          } else if (!wide_ray_ok(R.o, R.d, R.inv) || (P.wide_handback && (slot & 1))) {
            B.hits[slot] = make_float2(R.lim, __int_as_float(kind ? kNeedExactShadow : kNeedExactClosest));
          } else {
            p = slot;
          }
        }
      }
    }
    if (!more && __ballot(p >= 0) == 0ull) break;
    for (int it = 0; it < PT_WIDE_STEPS; ++it) {
      bool exact = false;
      // fin: the walk has no node left (its queue may still hold candidates)
      if (p >= 0 && !fin)
        fin = wide_step<CNT, true, QN>(R, P.wide, P.wide_tris, lds, 64, ovf, os, P.wide_stack, &exact, &c.nodes,
                                       &c.leaves, cand, P.wide_leafbox);
      if (exact) {
        R.nc = 0;
        // a fused shadow ray the walk cannot take goes to the shading's next round
        B.hits[p] = (fz & kFuseWalk) ? make_float2(__uint_as_float(aux), __int_as_float(cr))
                                     : make_float2(R.lim, __int_as_float(R.shadow ? kNeedExactShadow
                                                                                  : kNeedExactClosest));
        p = -1;
        fin = false;
        fz = 0;
      }
      // wave-uniform flush: a queue that cannot take another node's four
      // leaves, or PT_WIDE_FLUSH_T finished walks waiting on their queue,
      // or nothing left walking
      const unsigned long long waiting = __ballot(p >= 0 && fin && R.nc > 0);
#ifdef PT_WIDE_PROBE_FLUSH
      if (lane == 0) atomicAdd(&P.stats[7], 1ull);
      if (lane == 0) atomicAdd(&P.stats[8], (unsigned long long)__popcll(__ballot(p >= 0 && !fin)));
#endif
#ifdef PT_WIDE_PROBE   // lane-state census per step (traced counters 0-4: walking, idle with rays left
                     // in the list, idle in the drain, steps, waiting on the leaf queue)
      {
        const unsigned long long walking = __ballot(p >= 0 && !fin), idle_l = __ballot(p < 0);
        if (lane == 0) {
          atomicAdd(&P.stats[4], (unsigned long long)__popcll(walking));
          atomicAdd(&P.stats[more ? 5 : 6], (unsigned long long)__popcll(idle_l));
          atomicAdd(&P.stats[7], 1ull);
          atomicAdd(&P.stats[8], (unsigned long long)__popcll(waiting));
        }
      }
#endif
      if (__ballot(p >= 0 && R.nc > kWideQ - 4) || (int)__popcll(waiting) >= PT_WIDE_FLUSH_T ||
          (waiting && __ballot(p >= 0 && !fin) == 0ull)) {
#ifdef PT_WIDE_PROBE_FLUSH   // flush loop use: [4] flushes, [5] sum of candidates, [6] sum of the largest queue, [7] steps
        {
          int mx = p >= 0 ? R.nc : 0, sm = mx;
#pragma unroll
          for (int o = 32; o >= 1; o >>= 1) {
            mx = max(mx, __shfl_xor(mx, o));
            sm += __shfl_xor(sm, o);
          }
          if (lane == 0) {
            atomicAdd(&P.stats[4], 1ull);
            atomicAdd(&P.stats[5], (unsigned long long)sm);
            atomicAdd(&P.stats[6], (unsigned long long)mx);
          }
        }
#endif
        if (wide_flush_wave<CNT, QN>(R, p >= 0, P.wide_tris, cand, fkeys[wave], lane, &c.leaves, P.wide_leafbox)) {
          fin = true;   // occluded
          R.sp = 0;
          R.cur = -1;
        }
      }
      // every lane idle or done: back to the refill check (where the done ones finish)
      if (__ballot(p >= 0 && !(fin && R.nc == 0)) == 0ull) break;
    }
  }
  if (CNT) flush_traced(P, c, lane);
}
