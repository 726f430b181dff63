// kernels/wf_state.h — the wavefront pipeline's per-path state: the Trav walk
// record, PathSt, camera_ray, the path_step state machine, the state and ray
// load / store by list slot, the list helpers and the per-pixel culling test.
// A fragment: csrc/pt_device.hip includes it after kernels/render.h and before
// the wavefront kernels, inside namespace ptd's anonymous namespace.

// ===========================================================================
// pathTrace (:300-418) as a state machine over one sample -- phases PRIMARY,
// DIRECT, SSS, SSS_SHADOW, BOUNCE -- holding at most one ray in flight: the
// shading half of the wavefront pipeline and of the tail kernel below.  The
// arithmetic, RNG draws and traversal order per ray are exactly those of
// path_trace(); only the interleaving across paths differs.  (A lane
// state-machine kernel built on it, each lane running its own pixel's
// samples, measured slower than the path-recursive kernel on every scene and
// was removed in round 4.)
// ===========================================================================
enum : int { PH_BEGIN = 0, PH_PRIMARY, PH_DIRECT, PH_SSS, PH_SSS_SHADOW, PH_BOUNCE };

struct Trav {
  v3 o, d, inv;
  int k;        // next node
  float lim;    // closest: best t so far; shadow: occlusion limit
  int res;      // closest: best triangle (-1 none); shadow: 1 once occluded
  int shadow;   // 0 closest-hit, 1 shadow query
  int nc;       // queued leaf candidates (closest)
  uint32_t cn, cl;   // node visits / leaf tests of this ray (stats)
};

struct PathSt {
  uint32_t s, rng;
  int phase, depth, li, k;
  v3 thr, rad, hp, hn, acc3, pend, sss_thr, so, sd, cp, sn;
  float travel;
};

__device__ __forceinline__ void trav_start(Trav& T, v3 o, v3 d, bool shadow, float limit) {
  T.o = o;
  T.d = d;
  T.inv = mk(rcp_(d.x), rcp_(d.y), rcp_(d.z));
  T.k = 0;
  T.shadow = shadow ? 1 : 0;
  T.lim = shadow ? limit : 1e30f;
  T.res = shadow ? 0 : -1;
  T.nc = 0;
  T.cn = 0u;
  T.cl = 0u;
}

// A shadow query whose answer cannot change the image (shadow_needed): it is
// still handed out as a ray, so the path keeps its place in the ray rounds
// (the wavefront lists stay phase-aligned, neighbouring paths coherent), but
// it starts finished, unoccluded: no node is visited.  Skipping it inside
// path_step instead measured +3 % on the displaced sphere (paths drift apart)
// with the exhaustive walks; with the culled wide walk the shading kernel
// answers it itself (wf_shade_kernel).
__device__ __forceinline__ void trav_null(const RenderParams& P, Trav& T) {
  T.k = P.n_nodes;
  T.shadow = 2;
}

// One node of the walk; returns true when the ray is finished.
template <bool STATS>
__device__ __forceinline__ bool trav_step(const RenderParams& P, Trav& T, int* cand) {
  if (T.k >= P.n_nodes) {
    if (!T.shadow) {
      float best = T.lim;
      int bt = T.res;
      test_candidates(P, T.o, T.d, cand, T.nc, &best, &bt);
      T.lim = best;
      T.res = bt;
      T.nc = 0;
    }
    return true;
  }
  const float4 a = P.nodes[2 * T.k];
  const float4 b = P.nodes[2 * T.k + 1];
  if (STATS) T.cn++;
  const int raw = __float_as_int(a.w);
  const bool h = raw < 0 ? true : slab(T.o, T.inv, a, b);
  const int tri = __float_as_int(b.w);
  if (h && tri >= 0) {
    if (STATS) T.cl++;
    if (T.shadow) {
      const float4* Tr = P.tris + 3 * tri;
      float t;
      if (tri_test(T.o, T.d, Tr[0], Tr[1], Tr[2], &t) && t < 1e30f && !(t >= T.lim)) {
        T.res = 1;
        if (!STATS) return true;
      }
    } else {
      cand[T.nc * 64] = tri;
      if (++T.nc == kCand) {
        float best = T.lim;
        int bt = T.res;
        test_candidates(P, T.o, T.d, cand, T.nc, &best, &bt);
        T.lim = best;
        T.res = bt;
        T.nc = 0;
      }
    }
  }
  T.k = (h && tri < 0) ? T.k + 1 : (raw & 0x7fffffff);
  return false;
}

// CamFrame and camera_ray, main()'s ray generation (:430-460) for one sample batch: pt_camera_ray.h, which the
// host compiles too (pt_camera_rays_host).

// pathTrace (:300-418) as a state machine over one sample: runs shading from
// the current phase until a ray must be traced (returns true, T set up; the
// caller traces it and calls again with T.lim/T.res holding the result) or
// the sample is complete (returns false, *out = its radiance).  Shared by the
// wavefront pipeline's generation, shading and tail kernels.
// EXIT: with the exit skip (the shading and tail kernels' instantiations that
// launch_wavefront picks when P.exit_skip is set; the others are the code of before).
template <bool STATS, bool EXIT = false>
__device__ bool path_step(const RenderParams& P, const CamFrame& F, PathSt& S, Trav& T, Ctr& c, v3* out) {
  const float OFFSET = 0.001f;
  const v3 albedo = mk(0.8f, 0.8f, 0.8f);
  const v3 sss_albedo = mk(1.0f, 0.2f, 0.1f);
  const float sss_radius = 1.0f;
  v3 color = mk(0.0f, 0.0f, 0.0f);
  for (;;) {
    bool finished = false;   // sample complete, `color` holds its radiance
    switch (S.phase) {
      case PH_BEGIN: {
        const uint32_t batch = (P.first_batch + P.seed_base) + S.s;   // the seed's batch (PT_OPT_SEED_BASE)
        const uint32_t seed = (batch * (uint32_t)F.H + (uint32_t)F.py) * (uint32_t)F.W + (uint32_t)F.px;
        v3 o, d;
        camera_ray(F, seed, &o, &d);
        S.rng = seed;                                                         // :307
        S.thr = mk(1.0f, 1.0f, 1.0f);
        S.rad = mk(0.0f, 0.0f, 0.0f);
        S.depth = 0;
        bool need = P.max_depth > 0;
        for (int i = 0; i < P.n_lights && !need; ++i) {
          float tl;
          need = intersect_area_light(o, d, load_light(P, i), &tl);
        }
        if (need) {
          trav_start(T, o, d, false, 0.0f);
          S.phase = PH_PRIMARY;
          return true;
        }
        finished = true;   // no light in view and max_depth 0: radiance 0
        break;
      }
      case PH_PRIMARY: {
        // light pre-pass (:311-328) on the same ray, then depth 0 (:333)
        bool lit = false;
        for (int i = 0; i < P.n_lights; ++i) {
          const LightDev L = load_light(P, i);
          float tl;
          if (intersect_area_light(T.o, T.d, L, &tl)) {
            if (STATS) { c.rays++; c.nodes += T.cn; c.leaves += T.cl; }
            if (T.res < 0 || T.lim > tl) {
              color = mk(L.inten[0], L.inten[1], L.inten[2]);
              lit = true;
              break;
            }
          }
        }
        if (lit) { finished = true; break; }
        if (P.max_depth == 0) { color = S.rad; finished = true; break; }
        if (STATS) { c.rays++; c.nodes += T.cn; c.leaves += T.cl; }
        S.phase = PH_BOUNCE;   // handled as the result of a closest-hit trace at depth S.depth
        continue;
      }
      case PH_BOUNCE: {
        if (S.depth > 0 && STATS) { c.rays++; c.nodes += T.cn; c.leaves += T.cl; }
        if (T.res < 0) {
          S.rad = add(S.rad, mul(S.thr, mk(0.0f, 0.0f, 0.0f)));   // background (:336)
          color = S.rad;
          finished = true;
          break;
        }
        S.hp = add(T.o, muls(T.d, T.lim));
        S.hn = tri_normal(P, T.res);
        S.acc3 = mk(0.0f, 0.0f, 0.0f);   // directLight
        S.li = 0;
        S.phase = PH_DIRECT;
        S.k = -1;                         // marks "no shadow ray returned yet"
        continue;
      }
      case PH_DIRECT: {
        if (S.k >= 0) {   // a shadow ray for light S.li has returned
          if (STATS) { c.rays++; c.nodes += T.cn; c.leaves += T.cl; }
          if (!T.res) S.acc3 = add(S.acc3, mul(albedo, S.pend));
          S.li++;
        }
        if (S.li < P.n_lights) {                                            // :345-366
          const LightDev L = load_light(P, S.li);
          const LightSample s = sample_light(L, S.hp, S.hn, &S.rng);
          S.pend = muls(muls(mk(L.inten[0], L.inten[1], L.inten[2]), s.diff), rcp_(fmax_(s.dist * s.dist, 0.01f)));
          S.k = 0;
          trav_start(T, add(S.hp, muls(S.hn, OFFSET)), s.dir, true, s.dist - OFFSET);
          if (!STATS && !shadow_needed(L, s.diff)) trav_null(P, T);
          return true;
        }
        S.rad = add(S.rad, mul(S.thr, S.acc3));
        // SSS walk (:371-408): the first direction is drawn even if no step runs
        S.sss_thr = mk(1.0f, 1.0f, 1.0f);
        S.so = sub(S.hp, muls(S.hn, OFFSET));
        S.sd = sample_sphere(&S.rng);
        S.k = 0;
        if (S.k < P.sss_bounces) {
          trav_start(T, S.so, S.sd, false, 0.0f);
          S.phase = PH_SSS;
          return true;
        }
        S.phase = -1;   // to the bounce
        break;
      }
      case PH_SSS: {
        if (STATS) { c.rays++; c.nodes += T.cn; c.leaves += T.cl; }
        if (T.res < 0) { S.phase = -1; break; }                           // :381 miss ends the walk
        S.travel = T.lim;
        S.cp = add(S.so, muls(S.sd, S.travel));
        S.sn = tri_normal(P, T.res);
        S.acc3 = mk(0.0f, 0.0f, 0.0f);   // sssLight
        S.li = 0;
        S.phase = PH_SSS_SHADOW;
        if (P.n_lights > 0) {
          const LightDev L = load_light(P, 0);
          const LightSample s = sample_light(L, S.cp, S.sn, &S.rng);
          S.pend = muls(mul(muls(sss_albedo, s.diff), mk(L.inten[0], L.inten[1], L.inten[2])), rcp_(fmax_(s.dist * s.dist, 0.01f)));
          trav_start(T, add(S.cp, muls(S.sn, OFFSET)), s.dir, true, s.dist - OFFSET);
          if (!STATS && !shadow_needed(L, s.diff)) trav_null(P, T);
          return true;
        }
        continue;
      }
      case PH_SSS_SHADOW: {
        if (S.li < P.n_lights) {   // the shadow ray for light S.li returned
          if (STATS) { c.rays++; c.nodes += T.cn; c.leaves += T.cl; }
          if (!T.res) S.acc3 = add(S.acc3, S.pend);
          S.li++;
        }
        if (S.li < P.n_lights) {
          const LightDev L = load_light(P, S.li);
          const LightSample s = sample_light(L, S.cp, S.sn, &S.rng);
          S.pend = muls(mul(muls(sss_albedo, s.diff), mk(L.inten[0], L.inten[1], L.inten[2])), rcp_(fmax_(s.dist * s.dist, 0.01f)));
          trav_start(T, add(S.cp, muls(S.sn, OFFSET)), s.dir, true, s.dist - OFFSET);
          if (!STATS && !shadow_needed(L, s.diff)) trav_null(P, T);
          return true;
        }
        S.rad = add(S.rad, muls(mul(mul(S.thr, S.sss_thr), S.acc3), 1.0f + sss_radius * 0.5f));
        S.sss_thr = mul(S.sss_thr, muls(sss_albedo, exp_(-S.travel / (sss_radius * 1.5f))));
        S.so = sub(S.cp, muls(S.sn, OFFSET));
        S.sd = sample_sphere(&S.rng);
        S.k++;
        if (S.k < P.sss_bounces) {
          trav_start(T, S.so, S.sd, false, 0.0f);
          S.phase = PH_SSS;
          return true;
        }
        S.phase = -1;
        break;
      }
      default:
        break;
    }
    if (!finished && S.phase == -1) {
      // indirect bounce (:411-414)
      const float r1 = rng_next(&S.rng);
      if constexpr (EXIT) {
        // the ray provably misses the root box (exit_skip): the path ends with the radiance it has
        if (exit_skipped(P, S.hn, add(S.hp, muls(S.hn, OFFSET)), r1)) {
          *out = S.rad;
          return false;
        }
      }
      const v3 bd = sample_hemisphere_r1(S.hn, r1, &S.rng);
      S.thr = mul(S.thr, muls(albedo, dot(S.hn, bd)));
      const v3 ro = add(S.hp, muls(S.hn, OFFSET));
      S.depth++;
      if (S.depth < P.max_depth) {
        trav_start(T, ro, bd, false, 0.0f);
        S.phase = PH_BOUNCE;
        return true;
      }
      color = S.rad;
      finished = true;
    }
    if (finished) {
      *out = color;
      return false;
    }
  }
}

// ===========================================================================
// Wavefront pipeline, for scenes too large for LDS.
//
// Measured on the 1080p displaced sphere (16.6M paths): the path-recursive
// kernel keeps 11 % of its lanes busy (VALUUtilization) with L2 hit rate 92 %
// and no memory stall — the wave waits for its longest walk.  Here every
// (pixel, sample) path lives in HBM (PathSt, 160 B) and the work is split by
// kind: a persistent traversal kernel whose lanes pull waiting paths from a
// list and refill as soon as their walk ends (uniform code, ~20 live VGPRs),
// and a shading kernel that consumes the hits with path_step() and appends
// the paths that need another ray to the next list.  Each path's arithmetic,
// RNG draws and traversal order are those of path_trace(); the colours are
// folded per pixel in batch order at the end, so the image is bit-identical.
// ===========================================================================
// A waiting path's state travels with its ray: list slot s holds both, each
// stored by component (chunk j of the state at state[list][j * cap + s]; the
// ray at rays[list][s] and rays[list][cap + s]).  A wave reads and writes
// consecutive slots, so every access instruction covers consecutive 16-B
// words.  (Indexed by path, the state of a list's sparse surviving paths
// cost 64 lines per instruction and a dependent load of the path id first;
// by path and by component it measured +2.5 % / +4 %.)
//
// Only the fields the phase the path waits in reads again are stored, in
// chunks of 4 words, a prefix per phase (the 160-B PathSt lives in registers
// only):
//   c0 {s, rng, phase, depth}       c1 {thr.xyz, rad.x}
//   c2 {rad.yz, li | sss_thr.z, k}  c3 {hp.xyz, hn.x}
//   c4 {hn.yz, acc3.xy | sss_thr.xy}
//   c5 {acc3.z, pend.xyz}           c6 {sss_thr.xyz, travel}
//   c7 {cp.xyz, sn.x}               c8 {sn.yz, -, -}
// PH_PRIMARY: c0 (thr = 1, rad = 0, depth = 0: PH_BEGIN's values); PH_BOUNCE:
// c0-c2; PH_SSS: c0-c4 with sss_thr in the li / acc3 words (li and acc3 are
// set again before they are read; the walk ray's origin and direction are
// S.so / S.sd bitwise, restored from the ray record); PH_DIRECT: c0-c5;
// PH_SSS_SHADOW: c0-c8.  With the fused shadow walks a path mostly waits in
// PH_BOUNCE / PH_SSS: 48 / 80 B stored and loaded instead of 160.
__device__ __forceinline__ int wf_state_chunks(int phase) {
  return phase == PH_PRIMARY ? 1 : phase == PH_BOUNCE ? 3 : phase == PH_SSS ? 5 : phase == PH_DIRECT ? 6 : 9;
}

__device__ __forceinline__ void wf_store_state(const WfBuffers& B, int list, long long slot, const PathSt& S) {
  float4* __restrict__ dst = B.state[list] + slot;
  const size_t cap = (size_t)B.cap;
  const bool sss = S.phase == PH_SSS;
  const int n = wf_state_chunks(S.phase);
  dst[0] = make_float4(__uint_as_float(S.s), __uint_as_float(S.rng), __int_as_float(S.phase), __int_as_float(S.depth));
  if (n > 1) {
    dst[cap] = make_float4(S.thr.x, S.thr.y, S.thr.z, S.rad.x);
    dst[2 * cap] = make_float4(S.rad.y, S.rad.z, sss ? S.sss_thr.z : __int_as_float(S.li), __int_as_float(S.k));
  }
  if (n > 3) {
    dst[3 * cap] = make_float4(S.hp.x, S.hp.y, S.hp.z, S.hn.x);
    dst[4 * cap] = sss ? make_float4(S.hn.y, S.hn.z, S.sss_thr.x, S.sss_thr.y)
                       : make_float4(S.hn.y, S.hn.z, S.acc3.x, S.acc3.y);
  }
  if (n > 5) dst[5 * cap] = make_float4(S.acc3.z, S.pend.x, S.pend.y, S.pend.z);
  if (n > 6) {
    dst[6 * cap] = make_float4(S.sss_thr.x, S.sss_thr.y, S.sss_thr.z, S.travel);
    dst[7 * cap] = make_float4(S.cp.x, S.cp.y, S.cp.z, S.sn.x);
    dst[8 * cap] = make_float4(S.sn.y, S.sn.z, 0.0f, 0.0f);
  }
}

// o, d: the path's waiting ray (PH_SSS: S.so, S.sd).  Every field is
// assigned (chunks a phase does not store read as 0), so the state stays in
// registers.
__device__ __forceinline__ void wf_load_state(const WfBuffers& B, int list, long long slot, v3 o, v3 d, PathSt* S) {
  const float4* __restrict__ src = B.state[list] + slot;
  const size_t cap = (size_t)B.cap;
  float4 c[kWfStateF4];
  c[0] = src[0];
  const int phase = __float_as_int(c[0].z);
  const int n = wf_state_chunks(phase);
#pragma unroll
  for (int j = 1; j < kWfStateF4; ++j) c[j] = j < n ? src[(size_t)j * cap] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  const bool prim = n == 1, sss = phase == PH_SSS;
  S->s = __float_as_uint(c[0].x);
  S->rng = __float_as_uint(c[0].y);
  S->phase = phase;
  S->depth = __float_as_int(c[0].w);
  S->thr = prim ? mk(1.0f, 1.0f, 1.0f) : mk(c[1].x, c[1].y, c[1].z);
  S->rad = prim ? mk(0.0f, 0.0f, 0.0f) : mk(c[1].w, c[2].x, c[2].y);
  S->li = __float_as_int(c[2].z);
  S->k = __float_as_int(c[2].w);
  S->hp = mk(c[3].x, c[3].y, c[3].z);
  S->hn = mk(c[3].w, c[4].x, c[4].y);
  S->acc3 = mk(c[4].z, c[4].w, c[5].x);
  S->pend = mk(c[5].y, c[5].z, c[5].w);
  S->sss_thr = sss ? mk(c[4].z, c[4].w, c[2].z) : mk(c[6].x, c[6].y, c[6].z);
  S->travel = c[6].w;
  S->so = o;
  S->sd = d;
  S->cp = mk(c[7].x, c[7].y, c[7].z);
  S->sn = mk(c[7].w, c[8].x, c[8].y);
}

// bits: kRayFuse / kRayPrimary (fuse_bits); the limit word of a fused
// closest ray (whose limit is always 1e30) carries the path's RNG state
__device__ __forceinline__ void wf_store_ray(float4* __restrict__ rays, long long cap, int slot, const Trav& T,
                                             int bits = 0, uint32_t rng = 0u) {
  rays[slot] = make_float4(T.o.x, T.o.y, T.o.z, bits ? __uint_as_float(rng) : T.lim);
  rays[(size_t)cap + (size_t)slot] = make_float4(T.d.x, T.d.y, T.d.z, __int_as_float(T.shadow | bits));
}

__device__ __forceinline__ void wf_load_ray(const float4* __restrict__ rays, long long cap, int slot, float4* r0,
                                            float4* r1) {
  *r0 = rays[slot];
  *r1 = rays[(size_t)cap + (size_t)slot];
}

// A list slot for every lane with pred set (-1 for the others): one atomic
// per wave, consecutive slots in lane order.
__device__ __forceinline__ int wave_slot(int* counter, bool pred) {
  const unsigned long long m = __ballot(pred);
  if (m == 0ull) return -1;
  const int lane = (int)__lane_id();
  const int leader = __ffsll((unsigned long long)m) - 1;
  int base = 0;
  if (lane == leader) base = atomicAdd(counter, (int)__popcll(m));
  base = __shfl(base, leader);
  return pred ? base + (int)__popcll(m & ((1ull << lane) - 1ull)) : -1;
}

// PT_OPT_WF_FUSE: which closest rays the trace kernel follows with the
// path's next shadow ray.  After the hit of a primary (unless the light
// pre-pass ends the path), bounce or SSS ray, pathTrace's next draws sample
// light 0 (PH_DIRECT :345-366, PH_SSS_SHADOW :383-402) from the state the
// path holds now, and the shadow ray depends only on the hit and those draws.
__device__ __forceinline__ int fuse_bits(const RenderParams& P, const PathSt& S, const Trav& T) {
  if (!P.wf_fuse || T.shadow != 0) return 0;
  if (S.phase == PH_PRIMARY) return P.max_depth > 0 ? kRayFuse | kRayPrimary : 0;
  return (S.phase == PH_BOUNCE || S.phase == PH_SSS) ? kRayFuse : 0;
}

__device__ __forceinline__ void wf_push(const WfBuffers& B, int list, int slot, int p, const Trav& T, int bits = 0,
                                        uint32_t rng = 0u) {
  B.ids[list][slot] = p;
  wf_store_ray(B.rays[list], B.cap, slot, T, bits, rng);
}

// Path g of a launch: pixel (item, q) = g / n_batches, sample g % n_batches
// (samples of a pixel adjacent, so the fold reads them contiguously).
__device__ __forceinline__ bool wf_pixel(const RenderParams& P, long long pp, int* px, int* py) {
  const int spl = P.spl, per = 256 / spl;
  const int idx = (int)(pp / per), q = (int)(pp % per);
  const int item = P.items ? P.items[idx] : idx;
  const int tile = rank_tile(P, item / spl), part = item % spl;
  int bx, by;
  tile_block(tile, P.blocks_x, &bx, &by);
  *px = bx * 16 + q % 16;
  *py = by * 16 + part * (16 / spl) + q / 16;
  return tile < P.blocks_total && *px < P.width && *py < P.height;
}

// render_kernel's per-pixel culling test, same float ops.
__device__ __forceinline__ bool pixel_live(const RenderParams& P, float ndcX0, float ndcY0) {
  if (P.n_cull < 0) return true;
  bool live = false;
#pragma unroll
  for (int r = 0; r < kMaxCullRects; ++r)
    live = live || (r < P.n_cull && ndcX0 >= P.cull[r][0] && ndcX0 <= P.cull[r][1] && ndcY0 >= P.cull[r][2] &&
                    ndcY0 <= P.cull[r][3]);
  return live;
}
