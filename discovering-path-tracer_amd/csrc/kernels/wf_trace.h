// kernels/wf_trace.h — the wavefront pipeline's generation kernel and its
// persistent traversal kernel over the threaded walk (wf_gen_kernel,
// wf_trace_kernel).
// A fragment: csrc/pt_device.hip includes it after kernels/wf_state.h, inside
// namespace ptd's anonymous namespace.

// Ray generation + shading up to the primary trace (path_step from PH_BEGIN).
// Four blocks per CU: left to itself the compiler takes 129 VGPRs behind the
// wave-uniform rcp_ guards (119 with the per-lane ones) and drops to three
// waves per SIMD; held at 128 it spills nothing.
template <bool CNT>
__global__ __launch_bounds__(256, 4) void wf_gen_kernel(RenderParams P, WfBuffers B, long long n, long long g0) {
  const long long g = g0 + (long long)blockIdx.x * 256 + threadIdx.x;   // paths [g0, g0 + n)
  bool need = false, gen = false;
  Trav T;
  PathSt S;
  if (g - g0 < n) {
    const long long pp = g / (long long)P.n_batches;
    CamFrame F;
    if (wf_pixel(P, pp, &F.px, &F.py)) {
      F.W = P.width;
      F.H = P.height;
      load_camera(P, &F.cpos, &F.cdir, &F.right, &F.up);
      F.ndcX0 = (2.0f * (float)F.px / (float)F.W) - 1.0f;
      F.ndcY0 = (2.0f * (float)F.py / (float)F.H) - 1.0f;
      F.aspect = (float)F.W / (float)F.H;
      F.tanFov = P.tan_fov;
      v3 col = mk(0.0f, 0.0f, 0.0f);
      S.s = (uint32_t)(g - pp * (long long)P.n_batches);
      // render_kernel's per-sample skip (PT_OPT_CULL_TIGHT): outside the tight
      // rectangles a sample whose two radius draws are at least P.cull_u0
      // reaches nothing and is (0,0,0)
      bool reach = pixel_live(P, F.ndcX0, F.ndcY0);
      const int skip = reach ? pixel_skip(P, F.ndcX0, F.ndcY0) : kSkipBlack;   // l >= 0: a sure region, the light's intensity
      if (reach && skip != kSkipNever) {
        const uint32_t batch = (P.first_batch + P.seed_base) + S.s;   // the seed's batch (PT_OPT_SEED_BASE)
        uint32_t rng = (batch * (uint32_t)F.H + (uint32_t)F.py) * (uint32_t)F.W + (uint32_t)F.px;
        const float u1a = fmax_(1e-38f, rng_next(&rng));
        rng_next(&rng);
        const float u1j = fmax_(1e-38f, rng_next(&rng));
        reach = u1a < P.cull_u0 || u1j < P.cull_u0;
        if (!reach) {
          const float4 c4 = skip_colour(P, skip);
          col = mk(c4.x, c4.y, c4.z);
        }
      }
      if (reach) {
        gen = true;
        S.phase = PH_BEGIN;
        Ctr c = {0u, 0u, 0u, 0u, 0u};
        need = path_step<false>(P, F, S, T, c, &col);
      }
      if (!need) B.colors[g] = make_float4(col.x, col.y, col.z, 1.0f);
    }
  }
  // list slots: one atomic per workgroup instead of one per wave -- the
  // generation is otherwise short, and every wave of the launch adding to the
  // same counter queued on that one address
  __shared__ int wave_n[4], wave_base[4];
  const unsigned long long m = __ballot(need);
  const int w = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
  if (lane == 0) wave_n[w] = (int)__popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) {
    const int tot = wave_n[0] + wave_n[1] + wave_n[2] + wave_n[3];
    const int base = tot ? atomicAdd(&B.counters[0], tot) : 0;
    wave_base[0] = base;
    wave_base[1] = base + wave_n[0];
    wave_base[2] = base + wave_n[0] + wave_n[1];
    wave_base[3] = base + wave_n[0] + wave_n[1] + wave_n[2];
  }
  __syncthreads();
  const int slot =
      wave_base[w] + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
  if (need) {
    wf_push(B, 0, slot, (int)g, T, fuse_bits(P, S, T), S.rng);
    wf_store_state(B, 0, slot, S);
  }
  if (CNT) {
    const unsigned long long mg = __ballot(gen);
    if (__lane_id() == 0 && mg) atomicAdd(&P.stats[8], (unsigned long long)__popcll(mg));
  }
}

// Traversal state of one lane of the persistent traversal kernel: the ray,
// the walk position and the node at it (loaded one step ahead, as in
// trace_closest).
struct WfLane {
  v3 o, d, inv;
  float4 a, b;   // node k
  int k, nc, res, shadow;
  float lim;
};

// CNT: a ray handed to the traversal kernel -- closest (kind 0) or shadow
// (kind 1) walk; a null shadow query (kind 2, trav_null) is no walk.
__device__ __forceinline__ void count_start(float4 r1, Ctr& c) {
  const int kind = __float_as_int(r1.w) & kRayKindMask;
  c.rays += kind == 0 ? 1u : 0u;
  c.srays += kind == 1 ? 1u : 0u;
}

__device__ __forceinline__ void wf_lane_start(const RenderParams& P, float4 r0, float4 r1, float4 root_a,
                                              float4 root_b, WfLane& L) {
  L.o = mk(r0.x, r0.y, r0.z);
  L.d = mk(r1.x, r1.y, r1.z);
  L.inv = mk(rcp_(L.d.x), rcp_(L.d.y), rcp_(L.d.z));
  const int kind = __float_as_int(r1.w);   // 0 closest, 1 shadow, 2 null shadow (trav_null)
  L.shadow = kind ? 1 : 0;
  L.lim = L.shadow ? r0.w : 1e30f;
  L.res = L.shadow ? 0 : -1;
  L.k = kind == 2 ? P.n_nodes : 0;
  L.nc = 0;
  L.a = root_a;
  L.b = root_b;
}

// One node of trace_closest / occluded (same visit order and tests); true
// when the ray is finished (L.lim / L.res hold the result).
template <bool CNT = false>
__device__ __forceinline__ bool wf_lane_step(const RenderParams& P, WfLane& L, int* cand, Ctr& c) {
  if (L.k >= P.n_nodes) {
    if (!L.shadow)
      test_candidates(P, L.o, L.d, cand, L.nc, &L.lim, &L.res);
    else if (L.nc > 0)
      L.res = test_shadow_candidates(P, L.o, L.d, L.lim, cand, L.nc) ? 1 : L.res;
    return true;
  }
  if (CNT) c.nodes++;
  const int raw = __float_as_int(L.a.w);
  const bool h = slab(L.o, L.inv, L.a, L.b) || (raw < 0);
  const int tri = __float_as_int(L.b.w);
  const bool leaf_hit = h && tri >= 0;
  if (CNT) c.leaves += leaf_hit ? 1u : 0u;
  // closest-hit and shadow rays alike queue the leaf; the kernel's wave-wide flush tests it
  cand[L.nc * 64] = tri;
  L.nc += leaf_hit ? 1 : 0;
  const int next = (h && tri < 0) ? L.k + 1 : (raw & 0x7fffffff);
  L.a = P.nodes[2 * next];
  L.b = P.nodes[2 * next + 1];
  L.k = next;
  return false;
}

// Persistent traversal over list `cur`: lanes pull list slots (one atomic per
// wave) and refill once at least PT_WF_REFILL lanes are idle.
//
// Closest-hit candidates are tested wave-wide -- as soon as
// one lane's queue is full, every lane with queued candidates tests them in
// the same loop -- instead of by each full lane alone while the other lanes
// of the wave wait (round-1 counters on the sphere: ~10 of 64 lanes active
// per VALU instruction in wf_trace_kernel).  Same candidates, same visit
// order, same strict '<': the same hit.  1080p8 displaced sphere 378 -> 289
// ms, 1M cloud +0.5 %.
// Shadow rays queue their hit leaves as well instead of
// testing each at once in a branch the other lanes wait on; the wave-wide
// flush tests them in visit order and ends the walk at the first occluder.
// The answer ("some accepted triangle has !(t >= limit)") is the same; the
// walk may visit a few nodes past that occluder before the flush finds it.
// Sphere 288 -> 242 ms, 1M cloud 636 -> 602.  (With it, the counting mode's
// triangle tests and nodes of shadow walks are the queued ones.)
#ifndef PT_WF_STEPS
#define PT_WF_STEPS 8
#endif

#ifndef PT_WF_REFILL
#define PT_WF_REFILL 32   // 1080p8: sphere -3.3 %, 1M cloud -2.0 % vs 16 (with the shadow queue); 48: +1.3 % / -0.3 %
#endif
// Refill group: lanes refill in groups of G with consecutive list slots.  G
// is chosen per launch (launch_wavefront): 2 for scenes under kWfGroup4Tris
// triangles, 4 above.  Measured at 1080p 8 spp, G = 2 vs 4: displaced sphere
// (82K) -4.6 %, random clouds 100K +3.4 % and 1M (4 spp) +3 %: a coherent
// surface gains, a random cloud loses; the threshold puts the BASELINE
// configs (sphere; 10M cloud) on their better side.
constexpr int kWfGroup4Tris = 500000;
template <int G>
constexpr unsigned long long group_lead() {
  static_assert(G == 1 || G == 2 || G == 4 || G == 8 || G == 16, "refill group: power of two");
  return G == 1 ? ~0ull : G == 2 ? 0x5555555555555555ull : G == 4 ? 0x1111111111111111ull
                                    : G == 8 ? 0x0101010101010101ull : 0x0001000100010001ull;
}
#ifndef PT_WF_MIN_BLOCKS
#define PT_WF_MIN_BLOCKS 7   // 72 VGPRs (11 spilled): sphere -7 %, 1M cloud -0.6 % vs 6; 8 spills 30 (+50 %)
#endif
template <bool LDS, int G, bool CNT = false>
__global__ __launch_bounds__(256, PT_WF_MIN_BLOCKS) void wf_trace_kernel(RenderParams P, WfBuffers B, int cur) {
  const int tid = (int)threadIdx.x;
  if (blockIdx.x == 0 && tid == 0) B.counters[cur ^ 1] = 0;   // filled by the shading that follows
  const int count = B.counters[cur];
  if (count == 0) return;
  if (LDS) {
    extern __shared__ float4 lds_scene[];
    const int nn = 2 * P.n_nodes, nt = 3 * P.n_tris;
    for (int i = tid; i < nn; i += 256) lds_scene[i] = P.nodes[i];
    for (int i = tid; i < nt; i += 256) lds_scene[nn + i] = P.tris[i];
    __syncthreads();
    P.nodes = lds_scene;
    P.tris = lds_scene + nn;
    P.hit_tris = P.tris;   // no wide walk here: hits are slots
  }
  const int wave = tid >> 6, lane = tid & 63;
  __shared__ int cand_buf[4][kCand][64];
  int* cand = &cand_buf[wave][0][lane];
  const float4* __restrict__ rays = B.rays[cur];
  // every walk starts at node 0: held in scalar registers
  float4 root_a = P.nodes[0], root_b = P.nodes[1];
  root_a.x = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(root_a.x)));
  root_a.y = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(root_a.y)));
  root_a.z = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(root_a.z)));
  root_a.w = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(root_a.w)));
  root_b.x = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(root_b.x)));
  root_b.y = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(root_b.y)));
  root_b.z = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(root_b.z)));
  root_b.w = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(root_b.w)));
  int p = -1;   // list slot this lane traces
  bool more = true;
  WfLane L;
  Ctr c = {0u, 0u, 0u, 0u, 0u};
  for (;;) {
    const unsigned long long idle = __ballot(p < 0);
    // groups of G lanes refill together with consecutive list
    // slots (neighbouring paths: the same pixel's samples), so their walks
    // stay as coherent as the path-recursive kernel's sample lanes
    unsigned long long gm = idle;
#pragma unroll
    for (int sh = 1; sh < G; sh <<= 1) gm &= gm >> sh;
    gm &= group_lead<G>();
    const int ng = (int)__popcll(gm);
    if (more && ng * G >= PT_WF_REFILL) {
      int base = 0;
      if (lane == 0) base = atomicAdd(&B.counters[2], ng * G);
      base = __shfl(base, 0);
      if (base + ng * G >= count) more = false;
      const int lead = lane & ~(G - 1);
      if ((gm >> lead) & 1ull) {
        const int slot = base + (int)__popcll(gm & ((1ull << lead) - 1ull)) * G + (lane - lead);
        if (slot < count) {
          p = slot;
          float4 r0, r1;
          wf_load_ray(rays, B.cap, slot, &r0, &r1);
          wf_lane_start(P, r0, r1, root_a, root_b, L);
          if (CNT) count_start(r1, c);
        }
      }
    }
    if (!more && __ballot(p >= 0) == 0ull) break;
    for (int it = 0; it < PT_WF_STEPS; ++it) {
      if (p >= 0 && wf_lane_step<CNT>(P, L, cand, c)) {
        B.hits[p] = make_float2(L.lim, __int_as_float(L.res));
        p = -1;
      }
      if (__ballot(p >= 0 && L.nc == kCand)) {   // wave-uniform
        if (p >= 0 && L.nc > 0) {
          if (!L.shadow) {
            test_candidates(P, L.o, L.d, cand, L.nc, &L.lim, &L.res);
          } else if (test_shadow_candidates(P, L.o, L.d, L.lim, cand, L.nc)) {
            L.res = 1;
            L.k = P.n_nodes;   // occluded: the walk ends (its next step reports it)
          }
          L.nc = 0;
        }
      }
    }
  }
  if (CNT) flush_traced(P, c, lane);
}
