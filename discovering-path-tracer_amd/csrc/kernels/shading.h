// kernels/shading.h — lights and their sampling, the sphere and hemisphere
// draws, the exit skip on the kernel's values, the parked-state macros, and
// the two path-recursive shaders path_trace and path_trace_fused.
// A fragment: csrc/pt_device.hip includes it after kernels/walks.h, inside
// namespace ptd's anonymous namespace.

// Lights are read-only for the whole launch and indexed by a wave-uniform
// loop counter: reading them through the constant address space lets the
// compiler use scalar loads (scalar cache, one load per wave) instead of a
// per-lane vector load whose latency every shadow ray waited on.
__device__ __forceinline__ LightDev load_light(const RenderParams& P, int i) {
#if defined(__HIP_DEVICE_COMPILE__)
  typedef const __attribute__((address_space(4))) float* ConstF;
  const ConstF f = (ConstF)(P.lights + i);
  LightDev L;
  float* o = (float*)&L;
#pragma unroll
  for (int k = 0; k < (int)(sizeof(LightDev) / 4); ++k) o[k] = f[k];
  return L;
#else
  return P.lights[i];
#endif
}

// Whether a shadow ray's answer can change the image.  Its light term is
// I * diff * rcp(max(d2, 0.01)) (:352-363, :392-402).  When diff = max(dot, 0)
// is 0 and I is finite, every channel of the term is +-0, and adding +-0 to
// the running sum (direct / sssLight, which start at +0 and so are never -0)
// leaves it bitwise unchanged: occluded or not, the result is the same, so the
// fast kernels skip the walk.  (The RNG draws for the light sample are made
// before, as in the reference.)  Stats mode still walks every shadow ray.
__device__ __forceinline__ bool shadow_needed(const LightDev& L, float diff) {
  return diff != 0.0f || L.finite == 0.0f;
}

// sampleAreaLight (:255-268); the light's frame (:261-264) is precomputed per
// light by setup_lights_kernel with the same ops.
__device__ __forceinline__ v3 sample_area_light(const LightDev& L, uint32_t* rng) {
  const float u = rng_next(rng) * 2.0f - 1.0f;
  const float v = rng_next(rng) * 2.0f - 1.0f;
  const v3 right = mk(L.right[0], L.right[1], L.right[2]);
  const v3 up = mk(L.up[0], L.up[1], L.up[2]);
  const v3 pos = mk(L.pos[0], L.pos[1], L.pos[2]);
  return add(add(pos, muls(muls(muls(right, u), L.size[0]), 0.5f)), muls(muls(muls(up, v), L.size[1]), 0.5f));
}

// intersectAreaLight (:271-298)
__device__ __forceinline__ bool intersect_area_light(v3 o, v3 d, const LightDev& L, float* t) {
  const v3 n_raw = mk(L.nraw[0], L.nraw[1], L.nraw[2]);
  const v3 pos = mk(L.pos[0], L.pos[1], L.pos[2]);
  const float denom = dot(n_raw, d);
  if (fabs_(denom) < 0.0001f) return false;
  const float tt = dot(n_raw, sub(pos, o)) / denom;
  *t = tt;
  if (tt <= 0.0f) return false;
  const v3 hp = add(o, muls(d, tt));
  const v3 th = sub(hp, pos);
  const float u = dot(th, mk(L.right[0], L.right[1], L.right[2]));
  const float v = dot(th, mk(L.up[0], L.up[1], L.up[2]));
  return fabs_(u) <= L.half[0] && fabs_(v) <= L.half[1];
}

// One light's sample seen from the point p with the normal n (:350-357, :386-392): the direction to the
// sampled point, the diffuse term max(dot(n, dir), 0) and the distance.  Every light loop -- path_trace,
// path_trace_fused, path_step, fused_shadow_ray -- takes its sample here, so they are the same operations in
// the same order (the bit-exactness argument of DESIGN.md §4 rests on that).  The light terms that follow,
// I * diff * rcp(max(dist^2, 0.01)) direct and (sss_albedo * diff) * I * rcp(...) for an SSS step, stay written
// out at their sites: as helpers they changed the instruction streams of the kernels (profiles/kernels).
struct LightSample {
  v3 dir;
  float diff, dist;
};
__device__ __forceinline__ LightSample sample_light(const LightDev& L, v3 p, v3 n, uint32_t* rng) {
  const v3 lp = sample_area_light(L, rng);
  LightSample s;
  // normalize and length take sqrt_ of the same dot: one evaluation serves both (the guarded sqrt_ has a
  // ballot in it, which the compiler does not fold across the branch)
  const v3 d = sub(lp, p);
  const float len = sqrt_(dot(d, d));
  s.dir = muls(d, rcp_(len));
  s.diff = fmax_(dot(n, s.dir), 0.0f);
  s.dist = len;
  return s;
}

// The camera's position and frame (:430-432): the frame is computed once on the host with the same ops.
// (render_kernel loads the four itself: through this helper five of its instantiations changed.)
__device__ __forceinline__ void load_camera(const RenderParams& P, v3* cpos, v3* cdir, v3* right, v3* up) {
  *cpos = mk(P.cam_pos[0], P.cam_pos[1], P.cam_pos[2]);
  *cdir = mk(P.cam_dir[0], P.cam_dir[1], P.cam_dir[2]);
  *right = mk(P.cam_right[0], P.cam_right[1], P.cam_right[2]);
  *up = mk(P.cam_upv[0], P.cam_upv[1], P.cam_upv[2]);
}

// sampleSphere (:246-253)
__device__ __forceinline__ v3 sample_sphere(uint32_t* rng) {
  const float z = 2.0f * rng_next(rng) - 1.0f;
  const float th = (2.0f * 0x1.921fb6p+1f) * rng_next(rng);
  const float r = sqrt_(1.0f - z * z);
  float sn, cs;
  sincos_(th, &sn, &cs);
  return mk(r * cs, r * sn, z);
}

// sampleHemisphere (:229-243): pt_isect.h hemisphere_dir on its two draws
// (r1: the first, already made -- the exit skip reads it before the rest)
__device__ __forceinline__ v3 sample_hemisphere_r1(v3 n, float r1, uint32_t* rng) {
  const float r2 = rng_next(rng);
  return hemisphere_dir(n, r1, r2);
}
// The exit skip (pt_isect.h exit_skip) on the kernel's values.
__device__ __forceinline__ bool exit_skipped(const RenderParams& P, v3 hn, v3 ro, float r1) {
  return exit_skip(hn, ro, r1, mk(P.root_lo[0], P.root_lo[1], P.root_lo[2]), mk(P.root_hi[0], P.root_hi[1], P.root_hi[2]));
}

__device__ __forceinline__ v3 tri_normal(const RenderParams& P, int tri) {
  const float4 C = P.hit_tris[3 * tri + 2];
  return mk(C.y, C.z, C.w);
}

__device__ __forceinline__ void add_ctr(Ctr& a, const Ctr& b) {
  a.rays += b.rays;
  a.nodes += b.nodes;
  a.leaves += b.leaves;
  a.srays += b.srays;
  a.prim += b.prim;
}

// LDS-staged scenes park path state in LDS during walks and run 6 waves per
// SIMD (80 VGPRs, 2 spilled) instead of 5 (96): box 1080p8 -3.8 %.
// 7 waves spill 19 VGPRs and gain nothing; parking at 5 waves costs +1.7 %.
// Parking in the paired walks of device-memory scenes (25 instead of 35
// spilled VGPRs, at 5 waves/SIMD): sphere 5K tris -1.0 %, 20K cloud -2.0 %
// (neutral while the k+1 prefetch held 8 more registers).  4 waves without
// spills: +12 %.
// ... and with the sweep walk (PT_OPT_SMALL_SWEEP), measured on its own (box
// 1080p8, 200 frames, four runs each, profiles/sweep/ab_occupancy.log):
// parked at 5 / 6 / 7 blocks 0.1721-0.1724 / 0.1601-0.1625 / 0.1662-0.1734 ms,
// not parked 0.1706-0.1718 / 0.1636-0.1661 / 0.1675-0.1719: parked at 6
// blocks, as the threaded walk.
constexpr int kPark = 12;   // floats of path state parked in LDS around a walk
__device__ __forceinline__ void park3(float* pk, int i, v3 v) {
  pk[i * 64] = v.x;
  pk[(i + 1) * 64] = v.y;
  pk[(i + 2) * 64] = v.z;
}
__device__ __forceinline__ v3 unpark3(const float* pk, int i) {
  return mk(pk[i * 64], pk[(i + 1) * 64], pk[(i + 2) * 64]);
}
// PARK: the path state a walk does not read (throughput, radiance, hit
// point and normal) waits in this lane's LDS column during the walk, so the
// walk's registers peak lower.  The empty asm with a memory clobber keeps the
// compiler from forwarding the stored values past the walk.
#define PT_WALK2(PARK, stmt)                                                         \
  do {                                                                               \
    if (PARK) { park3(pk, 0, thr); park3(pk, 3, rad); __asm__ volatile("" ::: "memory"); } \
    stmt;                                                                            \
    if (PARK) { __asm__ volatile("" ::: "memory"); thr = unpark3(pk, 0); rad = unpark3(pk, 3); } \
  } while (0)
#define PT_WALK4(PARK, stmt)                                                         \
  do {                                                                               \
    if (PARK) {                                                                      \
      park3(pk, 0, thr); park3(pk, 3, rad); park3(pk, 6, hp); park3(pk, 9, hn);      \
      __asm__ volatile("" ::: "memory");                                             \
    }                                                                                \
    stmt;                                                                            \
    if (PARK) {                                                                      \
      __asm__ volatile("" ::: "memory");                                             \
      thr = unpark3(pk, 0); rad = unpark3(pk, 3); hp = unpark3(pk, 6); hn = unpark3(pk, 9); \
    }                                                                                \
  } while (0)

// pathTrace (:300-418)
// SWEEP: the walks are the box sweep's (no candidate queue: the parked state
// starts at cand); 2: of a table with hull faces (sweep_walk.h sweep_slab_hull);
// 3: of the cube table (sweep_cands_cube).
template <bool STATS, bool PF, bool CNT = false, int SWEEP = 0>
__device__ v3 path_trace(const RenderParams& P, v3 ro, v3 rd, uint32_t seed, Ctr& c, int* cand) {
  constexpr bool PARK = !STATS && !PF;
  float* pk = (float*)(cand + (SWEEP ? 0 : kCand) * 64);
  auto closest = [&](v3 o, v3 d, Ctr& cc) {
    if constexpr (SWEEP)
      return sweep_trace_closest<SWEEP>(P, o, d);
    else
      return trace_closest<STATS, PF, false, CNT>(P, o, d, cc, cand);
  };
  auto shadowed = [&](v3 o, v3 d, float limit) {
    if constexpr (SWEEP)
      return sweep_trace_occluded<SWEEP>(P, o, d, limit);
    else
      return occluded<STATS, PF, CNT>(P, o, d, limit, c);
  };
  const float OFFSET = 0.001f;
  v3 thr = mk(1.0f, 1.0f, 1.0f);
  v3 rad = mk(0.0f, 0.0f, 0.0f);
  v3 hp, hn;
  uint32_t rng = seed;                                  // :307 re-seed

  Hit h0;
  h0.t = 1e30f;
  h0.tri = -1;
  bool have_h0 = false;
  Ctr c0 = {0u, 0u, 0u, 0u, 0u};
  Ctr& cp0 = CNT ? c : c0;   // CNT: the one walk is counted once
  for (int i = 0; i < P.n_lights; ++i) {                // :311-328
    const LightDev L = load_light(P, i);
    float tl;
    if (intersect_area_light(ro, rd, L, &tl)) {
      if (!have_h0) {
        h0 = closest(ro, rd, cp0);
        have_h0 = true;
      }
      if (STATS) add_ctr(c, c0);
      if (h0.tri < 0 || h0.t > tl) return mk(L.inten[0], L.inten[1], L.inten[2]);
    }
  }

  for (int depth = 0; depth < P.max_depth; ++depth) {   // :331
    Hit h;
    if (depth == 0) {
      if (!have_h0) {
        h0 = closest(ro, rd, cp0);
        have_h0 = true;
      }
      if (STATS) add_ctr(c, c0);
      h = h0;
    } else {
      PT_WALK2(PARK, h = closest(ro, rd, c));
    }
    if (h.tri < 0) {
      rad = add(rad, mul(thr, mk(0.0f, 0.0f, 0.0f)));  // background (:336)
      break;
    }
    hp = add(ro, muls(rd, h.t));                        // :188
    hn = tri_normal(P, h.tri);                          // :189

    const v3 albedo = mk(0.8f, 0.8f, 0.8f);
    v3 direct = mk(0.0f, 0.0f, 0.0f);
    for (int i = 0; i < P.n_lights; ++i) {              // :345-366
      const LightDev L = load_light(P, i);
      const LightSample s = sample_light(L, hp, hn, &rng);
      bool vis = !STATS && !shadow_needed(L, s.diff);
      if (!vis) PT_WALK4(PARK, vis = !shadowed(add(hp, muls(hn, OFFSET)), s.dir, s.dist - OFFSET));
      if (vis) direct = add(direct, mul(albedo, muls(muls(mk(L.inten[0], L.inten[1], L.inten[2]), s.diff), rcp_(fmax_(s.dist * s.dist, 0.01f)))));
    }
    rad = add(rad, mul(thr, direct));

    const v3 sss_albedo = mk(1.0f, 0.2f, 0.1f);         // :371-408
    const float sss_radius = 1.0f;
    v3 sss_thr = mk(1.0f, 1.0f, 1.0f);
    v3 so = sub(hp, muls(hn, OFFSET));
    v3 sd = sample_sphere(&rng);
    for (int k = 0; k < P.sss_bounces; ++k) {
      Hit sh;
      PT_WALK4(PARK, sh = closest(so, sd, c));
      if (sh.tri < 0) break;
      const float travel = sh.t;
      const v3 cp = add(so, muls(sd, travel));
      const v3 sn = tri_normal(P, sh.tri);
      v3 sl = mk(0.0f, 0.0f, 0.0f);
      for (int i = 0; i < P.n_lights; ++i) {
        const LightDev L = load_light(P, i);
        const LightSample s = sample_light(L, cp, sn, &rng);
        bool vis = !STATS && !shadow_needed(L, s.diff);
        if (!vis) PT_WALK4(PARK, vis = !shadowed(add(cp, muls(sn, OFFSET)), s.dir, s.dist - OFFSET));
        if (vis) sl = add(sl, muls(mul(muls(sss_albedo, s.diff), mk(L.inten[0], L.inten[1], L.inten[2])), rcp_(fmax_(s.dist * s.dist, 0.01f))));
      }
      rad = add(rad, muls(mul(mul(thr, sss_thr), sl), 1.0f + sss_radius * 0.5f));
      // the last step's throughput is never read and its next direction
      // (:406-407) never traced: its two draws only advance the stream (the
      // same state as sample_sphere's)
      if (STATS || k + 1 < P.sss_bounces) {
        sss_thr = mul(sss_thr, muls(sss_albedo, exp_(div1p5_(-travel))));
        so = sub(cp, muls(sn, OFFSET));
        sd = sample_sphere(&rng);
      } else {
        rng_skip(&rng, 2);
      }
    }

    // the last bounce's direction (:411-414) is never traced and the stream
    // is not read again: the path ends here
    if (!STATS && depth + 1 >= P.max_depth) break;
    ro = add(hp, muls(hn, OFFSET));
    const float r1 = rng_next(&rng);
    // the bounce ray provably misses the root box (exit_skip): rad stays
    if (!STATS && P.exit_skip && exit_skipped(P, hn, ro, r1)) break;
    const v3 bd = sample_hemisphere_r1(hn, r1, &rng);   // :411-414
    thr = mul(thr, muls(albedo, dot(hn, bd)));
    rd = bd;
  }
  return rad;
}


// pathTrace (:300-418) for the fast kernels, with every shadow ray that has an
// independent closest-hit ray next to it walked as a pair (walk_pair): the
// last light's shadow ray of the direct term with the first SSS ray, and each
// SSS step's last shadow ray with the next SSS ray.  The RNG draws, the float
// operations and their order are path_trace's: a shadow result is only used
// after the pair returns, to finish the same sums in the same order.
// EXIT: the instantiation the host picks when P.exit_skip is set (this kernel's
// registers are tight: a branch on the flag costs the others 10-17 spilled VGPRs).
template <bool CNT = false, bool EXIT = false>
__device__ v3 path_trace_fused(const RenderParams& P, v3 ro, v3 rd, uint32_t seed, int* cand, Ctr& c) {
  float* pk = (float*)(cand + kCand * 64);
  const float OFFSET = 0.001f;
  v3 thr = mk(1.0f, 1.0f, 1.0f);
  v3 rad = mk(0.0f, 0.0f, 0.0f);
  v3 hp, hn;
  uint32_t rng = seed;                                  // :307 re-seed
  const int NL = P.n_lights;

  Hit h0;
  h0.t = 1e30f;
  h0.tri = -1;
  bool have_h0 = false;
  for (int i = 0; i < NL; ++i) {                        // :311-328
    const LightDev L = load_light(P, i);
    float tl;
    if (intersect_area_light(ro, rd, L, &tl)) {
      if (!have_h0) {
        h0 = trace_closest<false, false, true, CNT>(P, ro, rd, c, cand);
        have_h0 = true;
      }
      if (h0.tri < 0 || h0.t > tl) return mk(L.inten[0], L.inten[1], L.inten[2]);
    }
  }

  const v3 albedo = mk(0.8f, 0.8f, 0.8f);
  const v3 sss_albedo = mk(1.0f, 0.2f, 0.1f);           // :371-408
  const float sss_radius = 1.0f;
  for (int depth = 0; depth < P.max_depth; ++depth) {   // :331
    Hit h;
    if (depth == 0) {
      if (!have_h0) {
        h0 = trace_closest<false, false, true, CNT>(P, ro, rd, c, cand);
        have_h0 = true;
      }
      h = h0;
    } else {
      PT_WALK2(true, h = (trace_closest<false, false, true, CNT>(P, ro, rd, c, cand)));
    }
    if (h.tri < 0) {
      rad = add(rad, mul(thr, mk(0.0f, 0.0f, 0.0f)));  // background (:336)
      break;
    }
    hp = add(ro, muls(rd, h.t));                        // :188
    hn = tri_normal(P, h.tri);                          // :189

    // direct light (:345-366); the last light's shadow ray is deferred
    v3 direct = mk(0.0f, 0.0f, 0.0f);
    v3 s_o = hp, s_d = hp, s_c = hp;   // deferred shadow ray: origin, dir, contribution if visible
    float s_lim = 0.0f;
    bool s_need = false;   // the deferred shadow ray can change the image (shadow_needed)
    for (int i = 0; i < NL; ++i) {
      const LightDev L = load_light(P, i);
      const LightSample s = sample_light(L, hp, hn, &rng);
      const v3 contrib = mul(albedo, muls(muls(mk(L.inten[0], L.inten[1], L.inten[2]), s.diff), rcp_(fmax_(s.dist * s.dist, 0.01f))));
      if (i + 1 < NL) {
        if (!shadow_needed(L, s.diff) ||
            !occluded<false, false, CNT>(P, add(hp, muls(hn, OFFSET)), s.dir, s.dist - OFFSET, c))
          direct = add(direct, contrib);
      } else {
        s_need = shadow_needed(L, s.diff);
        s_o = add(hp, muls(hn, OFFSET));
        s_d = s.dir;
        s_lim = s.dist - OFFSET;
        s_c = contrib;
      }
    }
    v3 sss_thr = mk(1.0f, 1.0f, 1.0f);
    v3 so = sub(hp, muls(hn, OFFSET));
    v3 sd = sample_sphere(&rng);
    Hit sh;
    bool occ = false;
    PT_WALK4(true, walk_pair<CNT>(P, NL > 0 && s_need, s_o, s_d, s_lim, &occ, P.sss_bounces > 0, so, sd, cand, &sh, c));
    if (NL > 0 && !occ) direct = add(direct, s_c);
    rad = add(rad, mul(thr, direct));

    for (int k = 0; k < P.sss_bounces; ++k) {
      if (sh.tri < 0) break;
      const float travel = sh.t;
      const v3 cp = add(so, muls(sd, travel));
      const v3 sn = tri_normal(P, sh.tri);
      v3 sl = mk(0.0f, 0.0f, 0.0f);
      for (int i = 0; i < NL; ++i) {
        const LightDev L = load_light(P, i);
        const LightSample s = sample_light(L, cp, sn, &rng);
        const v3 term = muls(mul(muls(sss_albedo, s.diff), mk(L.inten[0], L.inten[1], L.inten[2])), rcp_(fmax_(s.dist * s.dist, 0.01f)));
        if (i + 1 < NL) {
          if (!shadow_needed(L, s.diff) ||
              !occluded<false, false, CNT>(P, add(cp, muls(sn, OFFSET)), s.dir, s.dist - OFFSET, c))
            sl = add(sl, term);
        } else {
          s_need = shadow_needed(L, s.diff);
          s_o = add(cp, muls(sn, OFFSET));
          s_d = s.dir;
          s_lim = s.dist - OFFSET;
          s_c = term;
        }
      }
      const v3 thr_k = mul(thr, sss_thr);
      sss_thr = mul(sss_thr, muls(sss_albedo, exp_(div1p5_(-travel))));
      so = sub(cp, muls(sn, OFFSET));
      sd = sample_sphere(&rng);
      PT_WALK4(true, walk_pair<CNT>(P, NL > 0 && s_need, s_o, s_d, s_lim, &occ, k + 1 < P.sss_bounces, so, sd, cand, &sh, c));
      if (NL > 0 && !occ) sl = add(sl, s_c);
      rad = add(rad, muls(mul(thr_k, sl), 1.0f + sss_radius * 0.5f));
    }

    const float r1 = rng_next(&rng);
    if constexpr (EXIT) {
      // the bounce ray provably misses the root box (exit_skip): rad stays
      if (depth + 1 >= P.max_depth || exit_skipped(P, hn, add(hp, muls(hn, OFFSET)), r1)) break;
    }
    const v3 bd = sample_hemisphere_r1(hn, r1, &rng);   // :411-414
    thr = mul(thr, muls(albedo, dot(hn, bd)));
    ro = add(hp, muls(hn, OFFSET));
    rd = bd;
  }
  return rad;
}
