// kernels/rays.h — batched ray queries (pt_trace_rays): the caller's own rays
// through the walks the renderer uses, closest hit or occlusion.
// A fragment: csrc/pt_device.hip includes it last (the kernels before it keep
// their places in the code object), inside namespace ptd's anonymous namespace.
//
// A ray is 2 float4 {o.xyz, d.x} {d.yz, limit, reserved} (pt_ray), a closest
// hit 2 float4 {t, tri bits, u, v} {n.xyz, 0} (pt_hit), an occlusion answer one
// word.  No kernel here counts anything (stats mode, PT_OPT_COUNT_TRACED): the
// walks run their uncounted instantiations.
//
// Scenes with a wide tree: rays_wide_kernel walks the culled wide walk and
// marks the answer of a ray it does not take -- one wide_ray_ok refuses, one
// the walk hands back (*exact), and with PT_OPT_WIDE 2 every odd ray -- with
// kNeedExactClosest in pt_hit::tri or kNeedExactShadow in the occlusion word,
// values no answer has.  rays_exact_kernel then runs once more over the batch
// and walks the marked rays only; the wide kernel counts its marks in
// counters[1], and a batch without one costs that second launch a load.
// (Walking such a ray in the wide kernel's own lane would put trace_closest's
// node loop and candidate queue beside the wide walk's state in a kernel held
// to PT_WIDE_MIN_BLOCKS workgroups per CU; the marked launch keeps the wide
// kernel's registers the wide walk's alone.)

// rank -> triangle slot, the inverse of RenderParams::wide_rank_of (a permutation
// of 0..n-1, built by the host from the wide tree it made).
__global__ __launch_bounds__(256) void rays_slot_kernel(const int* __restrict__ rank_of, int n,
                                                        int* __restrict__ slot_of) {
  const int s = (int)(blockIdx.x * 256 + threadIdx.x);
  if (s < n) slot_of[rank_of[s]] = s;
}

struct RayIn {
  v3 o, d;
  float limit;
};
__device__ __forceinline__ RayIn rays_load(const float4* __restrict__ rays, size_t i) {
  const float4 r0 = rays[2 * i], r1 = rays[2 * i + 1];
  RayIn r;
  r.o = mk(r0.x, r0.y, r0.z);
  r.d = mk(r0.w, r1.x, r1.y);
  r.limit = r1.z;
  return r;
}

// The closest hit of ray (o, d): t, the triangle's index and its record (null: a miss).
__device__ __forceinline__ void rays_store_hit(float4* __restrict__ out, size_t i, v3 o, v3 d, float t, int tri,
                                               const float4* rec) {
  float4 h0 = make_float4(1e30f, __int_as_float(-1), 0.0f, 0.0f), h1 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (rec) {
    const float4 A = rec[0], B = rec[1], C = rec[2];
    float u, v;
    tri_uv(o, d, A, B, C, &u, &v);
    h0 = make_float4(t, __int_as_float(tri), u, v);
    h1 = make_float4(C.y, C.z, C.w, 0.0f);
  }
  out[2 * i] = h0;
  out[2 * i + 1] = h1;
}

template <int KIND>
__device__ __forceinline__ void rays_mark(void* __restrict__ out, size_t i) {
  if (KIND == kRaysAny)
    ((uint32_t*)out)[i] = (uint32_t)kNeedExactShadow;
  else
    ((float4*)out)[2 * i] = make_float4(1e30f, __int_as_float(kNeedExactClosest), 0.0f, 0.0f);
}
template <int KIND>
__device__ __forceinline__ bool rays_marked(const void* __restrict__ out, size_t i) {
  return KIND == kRaysAny ? ((const uint32_t*)out)[i] == (uint32_t)kNeedExactShadow
                          : ((const int*)out)[8 * i + 1] == kNeedExactClosest;
}

// The exact threaded walk, one ray per lane: a wave takes 64 consecutive rays
// (two 16-B loads a lane), the workgroups stride over the batch.  LDS: the
// scene staged per workgroup (PT_OPT_SCENE_IN_LDS).  marked: only the rays the
// wide kernel marked, and nothing at all when it counted none.
template <int KIND, bool LDS>
__global__ __launch_bounds__(256) void rays_exact_kernel(RenderParams P, const float4* __restrict__ rays,
                                                         void* __restrict__ out, long long n, int marked,
                                                         const uint32_t* __restrict__ counters) {
  const int tid = (int)threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  if (marked && counters[1] == 0u) return;   // the same word for every thread of the grid
  __shared__ int cq[4][kCand][64];
  int* cand = &cq[wave][0][lane];
  if (LDS) {
    extern __shared__ float4 lds_scene[];
    const int nn = 2 * P.n_nodes, nt = 3 * P.n_tris;
    for (int i = tid; i < nn; i += 256) lds_scene[i] = P.nodes[i];
    for (int i = tid; i < nt; i += 256) lds_scene[nn + i] = P.tris[i];
    __syncthreads();
    P.nodes = lds_scene;
    P.tris = lds_scene + nn;
  }
  Ctr c = {0u, 0u, 0u, 0u, 0u};
  const long long stride = (long long)gridDim.x * 256;
  for (long long i = (long long)blockIdx.x * 256 + tid; i < n; i += stride) {
    if (marked && !rays_marked<KIND>(out, (size_t)i)) continue;
    const RayIn r = rays_load(rays, (size_t)i);
    if (KIND == kRaysAny) {
      ((uint32_t*)out)[i] = occluded<false, false>(P, r.o, r.d, r.limit, c) ? 1u : 0u;
    } else {
      const Hit h = LDS ? trace_closest<false, false, false>(P, r.o, r.d, c, cand)
                        : trace_closest<false, false, true>(P, r.o, r.d, c, cand);
      rays_store_hit((float4*)out, (size_t)i, r.o, r.d, h.t, h.tri, h.tri >= 0 ? P.tris + 3 * (size_t)h.tri : nullptr);
    }
  }
}

// The culled wide walk's answer of a finished ray: its rank becomes the triangle's index.
template <int KIND>
__device__ __forceinline__ void rays_wide_answer(const RenderParams& P, void* __restrict__ out, size_t i,
                                                 const WideRay& R, const int* __restrict__ slot_of) {
  if (KIND == kRaysAny) {
    ((uint32_t*)out)[i] = R.best ? 1u : 0u;
  } else {
    const bool hit = R.best >= 0;
    rays_store_hit((float4*)out, i, R.o, R.d, R.lim, hit ? slot_of[R.best] : -1,
                   hit ? P.wide_tris + 3 * (size_t)R.best : nullptr);
  }
}

// The culled wide walk (wide_walk.h) over the batch, for scenes that have a wide tree.  Every lane owns a
// stack overflow area, so the grid is bounded by P.wide_ovf_lanes (launch_rays) and strides over the rays.
// REFILL false, the plain shape (guide_kernel<2, QN>'s): a lane walks a ray to its end with its own
// wide_step / wide_flush, then takes the ray a grid stride on.
// REFILL true, the persistent shape (wf_trace_wide_kernel's): the lanes of a wave refill singly from the
// ray counter counters[0] (cleared on the stream before the launch) once P.wide_refill of them are idle,
// PT_WIDE_STEPS steps run between checks, and the leaf queues are tested across the wave (wide_flush_wave).
// Both test the same candidates under the same accept rules: the same bits.
template <int KIND, bool QN, bool REFILL>
__global__ __launch_bounds__(256, PT_WIDE_MIN_BLOCKS) void rays_wide_kernel(RenderParams P,
                                                                            const float4* __restrict__ rays,
                                                                            void* __restrict__ out, uint32_t n,
                                                                            uint32_t* __restrict__ counters,
                                                                            const int* __restrict__ slot_of) {
  const int tid = (int)threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  __shared__ int2 stk[4][kWideLds][64];
  int2* lds = &stk[wave][0][lane];
  __shared__ int cq[4][kWideQ][64];
  int* cand = &cq[wave][0][lane];
  const long long os = (long long)gridDim.x * 256;
  int2* ovf = P.wide_ovf + ((long long)blockIdx.x * 256 + tid);
  Ctr c = {0u, 0u, 0u, 0u, 0u};
  uint32_t marks = 0u;   // rays this lane left to the exact kernel
  if (!REFILL) {
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + tid; i < n; i += (unsigned long long)os) {
      const RayIn r = rays_load(rays, (size_t)i);
      WideRay R;
      wide_start(R, r.o, r.d, KIND == kRaysAny, r.limit);
      bool exact = !wide_ray_ok(R.o, R.d, R.inv) || (P.wide_handback && (i & 1ull));
      while (!exact) {
        const bool fin = wide_step<false, true, QN>(R, P.wide, P.wide_tris, lds, 64, ovf, os, P.wide_stack, &exact,
                                                    &c.nodes, &c.leaves, cand, P.wide_leafbox);
        if (exact) break;   // the builder's stack bound rules this out; stay exact anyway
        bool occ = false;
        if (fin || R.nc > kWideQ - 4) occ = wide_flush<false, QN>(R, P.wide_tris, cand, &c.leaves, P.wide_leafbox);
        if (fin || occ) break;
      }
      if (exact) {
        rays_mark<KIND>(out, (size_t)i);
        ++marks;
      } else {
        rays_wide_answer<KIND>(P, out, (size_t)i, R, slot_of);
      }
    }
  } else {
    __shared__ unsigned long long fkeys[4][64];
    bool fin = false, more = true;
    int p = -1;   // the ray this lane walks (n < 2^31)
    WideRay R;
    R.cur = -1;
    R.sp = R.lo = 0;
    R.nc = 0;
    R.shadow = KIND == kRaysAny ? 1 : 0;
    for (;;) {
      // the lanes whose walks ended since the last check answer here together
      if (p >= 0 && fin && R.nc == 0) {
        rays_wide_answer<KIND>(P, out, (size_t)p, R, slot_of);
        p = -1;
        fin = false;
      }
      const unsigned long long idle = __ballot(p < 0);
      const int need = (int)__popcll(idle);
      if (more && need >= P.wide_refill) {
        uint32_t base = 0u;
        if (lane == 0) base = atomicAdd(&counters[0], (uint32_t)need);
        base = (uint32_t)__shfl((int)base, 0);
        if (base + (uint32_t)need >= n) more = false;   // (base <= n + the grid's lanes: no wrap)
        if ((idle >> lane) & 1ull) {
          const uint32_t slot = base + (uint32_t)__popcll(idle & ((1ull << lane) - 1ull));
          if (slot < n) {
            const RayIn r = rays_load(rays, (size_t)slot);
            wide_start(R, r.o, r.d, KIND == kRaysAny, r.limit);
            if (!wide_ray_ok(R.o, R.d, R.inv) || (P.wide_handback && (slot & 1u))) {
              rays_mark<KIND>(out, (size_t)slot);
              ++marks;
            } else {
              p = (int)slot;
            }
          }
        }
      }
      if (!more && __ballot(p >= 0) == 0ull) break;
      for (int it = 0; it < PT_WIDE_STEPS; ++it) {
        bool exact = false;
        // fin: the walk has no node left (its queue may still hold candidates)
        if (p >= 0 && !fin)
          fin = wide_step<false, true, QN>(R, P.wide, P.wide_tris, lds, 64, ovf, os, P.wide_stack, &exact, &c.nodes,
                                           &c.leaves, cand, P.wide_leafbox);
        if (exact) {
          R.nc = 0;
          rays_mark<KIND>(out, (size_t)p);
          ++marks;
          p = -1;
          fin = false;
        }
        // wave-uniform flush, wf_trace_wide_kernel's rule: a queue that cannot take another node's four
        // leaves, a finished walk waiting on its queue, or nothing left walking
        const unsigned long long waiting = __ballot(p >= 0 && fin && R.nc > 0);
        if (__ballot(p >= 0 && R.nc > kWideQ - 4) || (int)__popcll(waiting) >= PT_WIDE_FLUSH_T ||
            (waiting && __ballot(p >= 0 && !fin) == 0ull)) {
          if (wide_flush_wave<false, QN>(R, p >= 0, P.wide_tris, cand, fkeys[wave], lane, &c.leaves, P.wide_leafbox)) {
            fin = true;   // occluded
            R.sp = 0;
            R.cur = -1;
          }
        }
        // every lane idle or done: back to the refill check (where the done ones answer)
        if (__ballot(p >= 0 && !(fin && R.nc == 0)) == 0ull) break;
      }
    }
  }
  // one add a wave (every lane is here: both loops end wave-uniformly or reconverge)
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) marks += (uint32_t)__shfl_xor((int)marks, o);
  if (lane == 0 && marks) atomicAdd(&counters[1], marks);
}
