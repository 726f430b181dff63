// kernels/walks.h — the per-lane counters, the threaded walks (trace_closest,
// occluded, walk_pair) with their leaf-candidate queue, and the glue between
// the render kernel and the sweep walk (CubeWords, sweep_trace_*).
// A fragment, not a stand-alone header: csrc/pt_device.hip includes it first,
// inside namespace ptd's anonymous namespace.

// Per-lane counters.  STATS (reference-exhaustive mode): rays = every
// reference traceRay, nodes/leaves = its exhaustive visits.  CNT (the fast
// kernels with counters, PT_OPT_COUNT_TRACED): rays = closest-hit walks and
// srays = shadow walks actually started, nodes = nodes actually visited,
// leaves = triangle tests actually run, prim = primary rays generated.
struct Ctr {
  uint32_t rays, nodes, leaves, srays, prim;
};

// This rank's li-th tile (pt_device.h Part; slot positions in device memory:
// a kernel argument array indexed at run time would be copied to scratch).
__device__ __forceinline__ int rank_tile(const RenderParams& P, int li) {
  return (li / P.part_cnt) * P.part_m + P.part_pos[li % P.part_cnt];
}

struct Hit {
  float t;
  int tri;   // -1 = miss
};

// Leaf candidates are queued per lane (in LDS, [slot][lane] so a wave's
// stores hit 64 distinct banks) and their triangles tested after the walk:
// in a wave whose lanes pass different leaves the triangle test then runs
// max-over-lanes times instead of once per leaf any lane passed.  Candidates
// are tested in visit order with the same strict '<', so the hit is the same.
#ifndef PT_KCAND
#define PT_KCAND 8
#endif
constexpr int kCand = PT_KCAND;

// The running mean's step (:467-469): (acc * b + c) / (b + 1).  Where b + 1
// is a power of two the quotient is a product with its exact reciprocal
// (bitwise the IEEE quotient: both round the same exact value), and a running
// value of 1 folding a colour of 1 stays 1 ((b + 1) / (b + 1), b + 1 < 2^24
// exact) -- the alpha channel of every live pixel.
// With one lane per pixel each lane folds its own sample (no colour hand-off
// through LDS).  The last SSS step's next direction and the last bounce's
// direction, never traced, are not computed (their draws still advance the
// stream).  Box 1080p8, driver command: the three together 0.2131 -> 0.2114 ms
// (profiles/r05b/ab_box.log).

// PF (prefetch): load node k+1 while node k is being tested — it is the next
// visit whenever k is a hit internal node or a leaf (the node arrays carry one
// node of padding so k+1 is always readable).  It was worth 12 % on a
// 1M-triangle scene in the first kernel; re-measured after the candidate queue,
// paired walks and null shadow rays it costs more than it hides: wavefront 1M
// cloud 400 -> 337 ms and 10M cloud 662 -> 616 ms without it, sphere 452 ->
// 423, recursive 5K sphere -2.5 %.  The wavefront and fused walks no longer
// carry it; only the reference-exhaustive stats walk from device memory
// (trace_closest, occluded, path_trace with PF) still prefetches.  An
// LDS-staged walk never used it.

__device__ __forceinline__ void test_candidates(const RenderParams& P, v3 o, v3 d, const int* cand, int nc,
                                                float* best, int* bt) {
  for (int i = 0; i < nc; ++i) {
    const int tri = cand[i * 64];
    const float4* T = P.tris + 3 * tri;
    float t;
    if (tri_test(o, d, T[0], T[1], T[2], &t) && t < *best) {
      *best = t;
      *bt = tri;
    }
  }
}

// Shadow-ray candidates (wf_trace_kernel): the queued triangles in visit
// order until the first one occluded() would stop at; true if any.
__device__ __forceinline__ bool test_shadow_candidates(const RenderParams& P, v3 o, v3 d, float limit,
                                                       const int* cand, int nc) {
  for (int i = 0; i < nc; ++i) {
    const int tri = cand[i * 64];
    const float4* T = P.tris + 3 * tri;
    float t;
    if (tri_test(o, d, T[0], T[1], T[2], &t) && t < 1e30f && !(t >= limit)) return true;
  }
  return false;
}

// FLUSH_OUT: the candidate queue is tested when the walk ends or the queue is
// full, by an outer loop around the node loop, instead of by a branch inside
// it.  Device-memory walks (path_trace_fused) gain 7 % (sphere 5K tris);
// LDS walks lose 1.6 % (box), so they keep the inner branch.
template <bool STATS, bool PF, bool FLUSH_OUT = false, bool CNT = false>
__device__ Hit trace_closest(const RenderParams& P, v3 o, v3 d, Ctr& c, int* cand) {
  const v3 inv = mk(rcp_(d.x), rcp_(d.y), rcp_(d.z));
  float best = 1e30f;
  int bt = -1;
  if (STATS || CNT) c.rays++;
  int k = 0, nc = 0;
  const int n = P.n_nodes;
  float4 a = P.nodes[0], b = P.nodes[1];
  while (k < n) {
   // FLUSH_OUT: walk until the walk ends or the queue is full, then test it
   while (k < n && (!FLUSH_OUT || nc < kCand)) {
    float4 na, nb;
    if (PF) {
      na = P.nodes[2 * k + 2];
      nb = P.nodes[2 * k + 3];
    }
    if (STATS || CNT) c.nodes++;
    const int raw = __float_as_int(a.w);
    // bit 31: bounds identical to the parent's, which this ray hit -> hit
    const bool h = slab(o, inv, a, b) || (raw < 0);   // branch-free: one LDS round trip per node
    const int tri = __float_as_int(b.w);
    // slot nc is free: write it unconditionally, keep it only for a hit leaf
    cand[nc * 64] = tri;
    const bool leaf_hit = h && tri >= 0;
    if (STATS || CNT) c.leaves += leaf_hit ? 1u : 0u;
    nc += leaf_hit ? 1 : 0;
    if (!FLUSH_OUT && nc == kCand) {
      test_candidates(P, o, d, cand, nc, &best, &bt);
      nc = 0;
    }
    const int next = (h && tri < 0) ? k + 1 : (raw & 0x7fffffff);
    if (PF && next == k + 1) {
      a = na;
      b = nb;
    } else {
      a = P.nodes[2 * next];
      b = P.nodes[2 * next + 1];
    }
    k = next;
   }
   if (FLUSH_OUT && nc == kCand) {
     test_candidates(P, o, d, cand, nc, &best, &bt);
     nc = 0;
   }
  }
  test_candidates(P, o, d, cand, nc, &best, &bt);
  Hit r;
  r.t = best;
  r.tri = bt;
  return r;
}

// Shadow query for "!hit || hit.t >= limit" (:359, :398): true iff some
// triangle the reference would accept (t < 1e30) has !(t >= limit).
// Triangles are tested as soon as their leaf is reached (no candidate queue):
// the early exit is worth more than the compaction for shadow rays (queueing
// 2/4/8 candidates measured 1-15 % slower on box.obj).
template <bool STATS, bool PF, bool CNT = false>
__device__ bool occluded(const RenderParams& P, v3 o, v3 d, float limit, Ctr& c) {
  const v3 inv = mk(rcp_(d.x), rcp_(d.y), rcp_(d.z));
  bool occ = false;
  if (STATS) c.rays++;
  if (CNT) c.srays++;
  int k = 0;
  const int n = P.n_nodes;
  float4 a = P.nodes[0], b = P.nodes[1];
  while (k < n) {
    float4 na, nb;
    if (PF) {
      na = P.nodes[2 * k + 2];
      nb = P.nodes[2 * k + 3];
    }
    if (STATS || CNT) c.nodes++;
    const int raw = __float_as_int(a.w);
    // bit 31: bounds identical to the parent's, which this ray hit -> hit
    const bool h = slab(o, inv, a, b) || (raw < 0);   // branch-free: one LDS round trip per node
    const int tri = __float_as_int(b.w);
    if (h && tri >= 0) {
      if (STATS || CNT) c.leaves++;
      const float4* T = P.tris + 3 * tri;
      float t;
      if (tri_test(o, d, T[0], T[1], T[2], &t) && t < 1e30f && !(t >= limit)) {
        occ = true;
        if (!STATS) return true;
      }
    }
    const int next = (h && tri < 0) ? k + 1 : (raw & 0x7fffffff);
    if (PF && next == k + 1) {
      a = na;
      b = nb;
    } else {
      a = P.nodes[2 * next];
      b = P.nodes[2 * next + 1];
    }
    k = next;
  }
  return occ;
}

// An occlusion query S and a closest-hit walk C, interleaved one node each per
// iteration: each walker visits exactly the node sequence of occluded() /
// trace_closest() above, with the same tests, candidate queue and strict '<',
// so both results are theirs bit for bit.  Interleaving only puts two
// independent node round trips in flight per lane -- the walks are bound by
// that latency (LDS or L2), not by issue.  has_s / has_c switch a walker off
// (it starts finished).  Fast kernels only: stats mode walks one ray at a time.
template <bool CNT = false>
__device__ __forceinline__ void walk_pair(const RenderParams& P, bool has_s, v3 so, v3 sd, float limit, bool* occ,
                                          bool has_c, v3 co, v3 cd, int* cand, Hit* hit, Ctr& c) {
  const int n = P.n_nodes;
  const v3 sinv = mk(rcp_(sd.x), rcp_(sd.y), rcp_(sd.z));
  const v3 cinv = mk(rcp_(cd.x), rcp_(cd.y), rcp_(cd.z));
  int ks = has_s ? 0 : n, kc = has_c ? 0 : n;
  if (CNT) {
    c.srays += has_s ? 1u : 0u;
    c.rays += has_c ? 1u : 0u;
  }
  bool oc = false;
  float best = 1e30f;
  int bt = -1, nc = 0;
  while (ks < n || kc < n) {
    // both loads first (a finished walker re-reads node 0, unused)
    const int ls = ks < n ? ks : 0, lc = kc < n ? kc : 0;
    const float4 sa = P.nodes[2 * ls], sb = P.nodes[2 * ls + 1];
    const float4 ca = P.nodes[2 * lc], cb = P.nodes[2 * lc + 1];
    if (ks < n) {
      const int raw = __float_as_int(sa.w);
      const bool h = slab(so, sinv, sa, sb) || (raw < 0);
      const int tri = __float_as_int(sb.w);
      int next = (h && tri < 0) ? ks + 1 : (raw & 0x7fffffff);
      if (CNT) c.nodes++;
      if (h && tri >= 0) {
        if (CNT) c.leaves++;
        const float4* T = P.tris + 3 * tri;
        float t;
        if (tri_test(so, sd, T[0], T[1], T[2], &t) && t < 1e30f && !(t >= limit)) {
          oc = true;
          next = n;
        }
      }
      ks = next;
    }
    if (kc < n) {
      const int raw = __float_as_int(ca.w);
      const bool h = slab(co, cinv, ca, cb) || (raw < 0);
      const int tri = __float_as_int(cb.w);
      cand[nc * 64] = tri;
      nc += (h && tri >= 0) ? 1 : 0;
      if (CNT) {
        c.nodes++;
        c.leaves += (h && tri >= 0) ? 1u : 0u;
      }
      if (nc == kCand) {
        test_candidates(P, co, cd, cand, nc, &best, &bt);
        nc = 0;
      }
      kc = (h && tri < 0) ? kc + 1 : (raw & 0x7fffffff);
    }
  }
  test_candidates(P, co, cd, cand, nc, &best, &bt);
  *occ = oc;
  hit->t = best;
  hit->tri = bt;
}

// The walks of a tiny scene as a box sweep (sweep_walk.h; PT_OPT_SMALL_SWEEP):
// P.tris holds the LDS-staged triangle records by leaf, and a hit's index is
// its leaf's (P.hit_tris is the same array).  A wave none of whose rays passes
// the root box has no candidates.  One kernel for every table (up to 64
// boxes, 32 leaves): the lanes hold a leaf mask only, no box mask.
// SWEEP: 1 a table without hull faces, 2 with some, 3 the cube table, whose
// walk reads the root box and the faces' under words from the parameters and
// nothing through P.sweep (sweep_cands_cube).
//
// The cube table's 13 words -- root_lo, root_hi, cube_under[], cube_all, one run
// of RenderParams -- are read from the kernel argument segment at each walk,
// issued ahead of the three rcp_ and waited on once, past them.  Left to the
// compiler they stay in 13 scalar registers for the whole kernel, which cost
// more in spilled scalars than the loads do (53 against 34; profiles/cube: the
// frame 0.128 against 0.120 ms), so the offset goes through an empty asm that
// keeps the loads where they are written.  Only for a kernel whose first
// argument is the RenderParams (render_kernel).
struct CubeWords {
  float lo[3], hi[3];
  uint32_t under[6], all;
};
static_assert(offsetof(RenderParams, root_lo) % 4 == 0 &&
                  offsetof(RenderParams, root_hi) == offsetof(RenderParams, root_lo) + 12 &&
                  offsetof(RenderParams, cube_under) == offsetof(RenderParams, root_lo) + 28 &&
                  offsetof(RenderParams, cube_all) == offsetof(RenderParams, root_lo) + 52,
              "sweep_cube_words reads root_lo .. cube_all as one run of words");
template <int SWEEP>
__device__ __forceinline__ CubeWords sweep_cube_words() {
  CubeWords w = {};
  if constexpr (SWEEP == 3) {
    typedef const __attribute__((address_space(4))) uint32_t* KernargWords;
    uint32_t at = (uint32_t)(offsetof(RenderParams, root_lo) / 4);
    __asm__ volatile("" : "+s"(at));
    const KernargWords k = (KernargWords)__builtin_amdgcn_kernarg_segment_ptr() + at;
    for (int i = 0; i < 3; ++i) w.lo[i] = u2f(k[i]), w.hi[i] = u2f(k[3 + i]);
    for (int i = 0; i < 6; ++i) w.under[i] = k[7 + i];   // (k[6] is seed_base)
    w.all = k[13];
  }
  return w;
}

template <int SWEEP>
__device__ uint32_t sweep_trace_cands(const RenderParams& P, const CubeWords& w, v3 o, v3 inv, bool* none) {
  if constexpr (SWEEP == 3) {
    return sweep_cands_cube(o, inv, w.lo, w.hi, w.under, w.all, none);
  } else {
    const SweepTable tb = {P.sweep, P.sweep_boxes, P.sweep_leaves};
    return sweep_cands<SWEEP == 2>(o, inv, tb, none);
  }
}

template <int SWEEP>
__device__ Hit sweep_trace_closest(const RenderParams& P, v3 o, v3 d) {
  const CubeWords w = sweep_cube_words<SWEEP>();
  const v3 inv = mk(rcp_(d.x), rcp_(d.y), rcp_(d.z));
  Hit r;
  r.t = 1e30f;
  r.tri = -1;
  bool none;
  const uint32_t lm = sweep_trace_cands<SWEEP>(P, w, o, inv, &none);
  if (none) return r;
  sweep_closest(o, d, lm, P.tris, &r.t, &r.tri);
  return r;
}

template <int SWEEP>
__device__ bool sweep_trace_occluded(const RenderParams& P, v3 o, v3 d, float limit) {
  const CubeWords w = sweep_cube_words<SWEEP>();
  const v3 inv = mk(rcp_(d.x), rcp_(d.y), rcp_(d.z));
  bool none;
  const uint32_t lm = sweep_trace_cands<SWEEP>(P, w, o, inv, &none);
  if (none) return false;
  return sweep_occluded(o, d, limit, lm, P.tris);
}
