// kernels/adaptive.h — render_adaptive_kernel, the path-recursive launch of an
// adaptive round (pt_adaptive_begin / pt_adaptive_advance): render_kernel's
// MOMENTS instantiations with the origin, the first batch and the batch count
// taken per workgroup from the round's live list instead of per launch.
// A fragment: csrc/pt_device.hip includes it after kernels/render.h, inside
// namespace ptd's anonymous namespace.
//
// A sibling of render_kernel, not a further instantiation: a seventh template
// argument would have put a list pointer and a count pointer into RenderParams
// and a test of them on every workgroup's way, in kernels whose code is to stay
// as it is (profiles/adaptive/resource_usage.md).  It reuses what carries the
// numbers -- path_trace / path_trace_fused, fold_one, fold_constant, store_lane,
// pixel_tight -- and restates render_kernel's frame around them without the
// parts an adaptive round never has: item lists, culled-item fill, mixed lanes,
// packed output, stats, counters, cost feedback.
//
// The launch holds tiles * spl workgroups whatever the list holds; workgroup i
// serves part i % spl of entry i / spl and leaves at once when the entry is past
// *n_live, which the round's compaction kernel wrote earlier on the same stream:
// no host synchronisation between rounds.  The entry's {first_batch, n_batches}
// replace P.first_batch / P.n_batches in the kernel's own copy of P before
// anything reads them, so the culled pixels' fold_constant, the fresh rule, the
// moments load, the seed and the fold weight all follow the entry.  They come
// from a load at a wave-uniform address (blockIdx.x), so they stay scalar.
template <bool LDS, int SWEEP, bool EXIT>
__global__ __launch_bounds__(256, SWEEP || LDS ? 6 : PT_RENDER_MIN_BLOCKS) void render_adaptive_kernel(
    RenderParams P, const int4* __restrict__ list, const int* __restrict__ n_live) {
  static_assert(!SWEEP || LDS, "the sweep walk is the LDS kernel's");
  static_assert(!EXIT || !LDS, "the LDS-staged kernels branch on P.exit_skip");
  const int tid = (int)threadIdx.x;
  const int spl = P.spl;
  const int lg = __builtin_ctz((unsigned)spl);
  const int entry = (int)blockIdx.x >> lg;
  if (entry >= *n_live) return;   // uniform per workgroup
  const int4 en = list[entry];
  const int gx0 = en.x;
  const int gy0 = en.y + ((int)blockIdx.x & (spl - 1)) * (16 / spl);
  P.first_batch = (uint32_t)en.z;
  P.n_batches = (uint32_t)en.w;
  const int wave = tid >> 6, lane = tid & 63;
  constexpr int kQueue = SWEEP ? 0 : kCand;   // the sweep walk queues nothing
  constexpr int kHand = 5;                    // floats handed off per sample: the colour, then L
  static_assert(kPark >= kHand, "the hand-off shares the parked state's area");
  __shared__ int cand_buf[4][kQueue + kPark][64];
  int* cand = &cand_buf[wave][0][lane];
  float* colw = (float*)&cand_buf[wave][kQueue][0];   // colour hand-off, [channel][lane]
  const int q = wave * (64 / spl) + lane / spl;       // pixel within the workgroup
  const int j = lane % spl;                           // sample slot
  const int px = gx0 + q % 16;
  const int py = gy0 + q / 16;
  const bool active = px < P.width && py < P.height;
  Ctr c = {0u, 0u, 0u, 0u, 0u};
  const int W = P.width, H = P.height;
  const float ndcX0 = (2.0f * (float)px / (float)W) - 1.0f;
  const float ndcY0 = (2.0f * (float)py / (float)H) - 1.0f;
  // primary-ray culling, as render_kernel
  bool live = true;
  bool wg_live = true;
  if (P.n_cull >= 0) {
    const float wx0 = (2.0f * (float)gx0 / (float)W) - 1.0f, wx1 = (2.0f * (float)(gx0 + 15) / (float)W) - 1.0f;
    const float wy0 = (2.0f * (float)gy0 / (float)H) - 1.0f;
    const float wy1 = (2.0f * (float)(gy0 + 16 / spl - 1) / (float)H) - 1.0f;
    live = false;
    wg_live = false;
#pragma unroll
    for (int r = 0; r < kMaxCullRects; ++r) {   // static indices: P stays in SGPRs/kernarg
      live = live || (r < P.n_cull && ndcX0 >= P.cull[r][0] && ndcX0 <= P.cull[r][1] && ndcY0 >= P.cull[r][2] &&
                      ndcY0 <= P.cull[r][3]);
      wg_live = wg_live || (r < P.n_cull && wx1 >= P.cull[r][0] && wx0 <= P.cull[r][1] && wy1 >= P.cull[r][2] &&
                            wy0 <= P.cull[r][3]);
    }
  }
  const bool tight = pixel_tight(P, ndcX0, ndcY0);
  const size_t pix = (size_t)py * (size_t)W + (size_t)px;
  // the running mean so far; an entry from batch 0 of a fresh launch starts from +0 without reading it
  float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (active && !(P.fresh && P.first_batch == 0)) {
    const float* a = (const float*)&P.accum[pix];
#pragma unroll
    for (int ch = 0; ch < 4; ++ch)
      if (ch % spl == j) acc[ch] = a[ch];
  }
  if (!live && active) fold_constant(P, acc, spl, j);   // the entry's batches of (0,0,0,1)
  // the pixel's moments, on its first lane: an entry from batch 0 starts from +0
  float mom1 = 0.0f, mom2 = 0.0f;
  if (active && live && j == 0 && P.first_batch != 0) {
    const float2 m = P.moments[pix];
    mom1 = m.x;
    mom2 = m.y;
  }
  if (!wg_live) {   // uniform per workgroup
    if (active) store_lane(P.accum + pix, acc, spl, j);
    return;
  }
  if (SWEEP) {
    extern __shared__ float4 lds_scene[];
    const SweepTable tb = {P.sweep, P.sweep_boxes, P.sweep_leaves};
    const int* slot = sweep_slots(tb);
    const int nt = 3 * P.sweep_leaves;
    for (int i = tid; i < nt; i += 256) lds_scene[i] = P.tris[3 * slot[i / 3] + i % 3];
    __syncthreads();
    P.tris = lds_scene;
    P.hit_tris = P.tris;   // hits are leaf indices
  } else if (LDS) {
    extern __shared__ float4 lds_scene[];
    const int nn = 2 * P.n_nodes, nt = 3 * P.n_tris;
    for (int i = tid; i < nn; i += 256) lds_scene[i] = P.nodes[i];
    for (int i = tid; i < nt; i += 256) lds_scene[nn + i] = P.tris[i];
    __syncthreads();
    P.nodes = lds_scene;
    P.tris = lds_scene + nn;
    P.hit_tris = P.tris;
  }
  {
    const v3 cpos = mk(P.cam_pos[0], P.cam_pos[1], P.cam_pos[2]);
    const v3 cdir = mk(P.cam_dir[0], P.cam_dir[1], P.cam_dir[2]);
    const float aspect = (float)W / (float)H;
    const v3 right = mk(P.cam_right[0], P.cam_right[1], P.cam_right[2]);
    const v3 up = mk(P.cam_upv[0], P.cam_upv[1], P.cam_upv[2]);
    const float tanFov = P.tan_fov;
    for (uint32_t base = 0; base < P.n_batches; base += (uint32_t)spl) {
     const uint32_t s = base + (uint32_t)j;
     float4 col4 = make_float4(0.0f, 0.0f, 0.0f, 1.0f);
     if (active && live && s < P.n_batches) {
      // render_kernel's sample, op for op: the seed's batch carries the seed base, the fold's does not
      const uint32_t batch = (P.first_batch + P.seed_base) + s;
      const uint32_t seed = (batch * (uint32_t)H + (uint32_t)py) * (uint32_t)W + (uint32_t)px;
      uint32_t rng = seed;
      const float u1a = fmax_(1e-38f, rng_next(&rng));
      const float u2a = rng_next(&rng);
      const float u1j = fmax_(1e-38f, rng_next(&rng));
      const float u2j = rng_next(&rng);
      if (tight || u1a < P.cull_u0 || u1j < P.cull_u0) {
      float r = sqrt_(-2.0f * log_(u1a));
      float th = (2.0f * 0x1.921fb6p+1f) * u2a;
      float sn, cs;
      sincos_(th, &sn, &cs);
      const float ax = (r * cs) * 0.02f;
      const float ay = (r * sn) * 0.02f;
      const v3 origin = add(add(cpos, muls(right, ax)), muls(up, ay));
      r = sqrt_(-2.0f * log_(u1j));
      th = (2.0f * 0x1.921fb6p+1f) * u2j;
      sincos_(th, &sn, &cs);
      const float jx = r * cs, jy = r * sn;
      const float ndcX = ndcX0 + (jx * 0.5f) / (float)W;
      const float ndcY = ndcY0 + (jy * 0.5f) / (float)H;
      const v3 bdir = normalize(sub(add(cdir, muls(neg(right), (ndcX * tanFov) * aspect)), muls(up, ndcY * tanFov)));
      const v3 focal = add(cpos, muls(bdir, 3.0f));
      const v3 dir = normalize(sub(focal, origin));
      v3 col;
      if (LDS)
        col = path_trace<false, !LDS, false, SWEEP>(P, origin, dir, seed, c, cand);
      else
        col = path_trace_fused<false, EXIT>(P, origin, dir, seed, cand, c);
      col4 = make_float4(col.x, col.y, col.z, 1.0f);
      }
     }
     if (spl == 1) {   // uniform: each lane folds its own sample, no hand-off
      if (active && live) {
        const uint32_t batch = P.first_batch + base;   // wave-uniform
        acc[0] = fold_one(acc[0], col4.x, batch);
        acc[1] = fold_one(acc[1], col4.y, batch);
        acc[2] = fold_one(acc[2], col4.z, batch);
        acc[3] = fold_one(acc[3], col4.w, batch);
        const float L = ptdn::lum(col4.x, col4.y, col4.z);
        mom1 = fold_one(mom1, L, batch);
        mom2 = fold_one(mom2, L * L, batch);
      }
      continue;
     }
     // hand the chunk's colours to the folding lanes of the same pixel
     colw[lane] = col4.x;
     colw[64 + lane] = col4.y;
     colw[128 + lane] = col4.z;
     colw[192 + lane] = col4.w;
     colw[256 + lane] = ptdn::lum(col4.x, col4.y, col4.z);
     __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
     __builtin_amdgcn_wave_barrier();
     __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
     if (active && live) {
      const uint32_t m = min((uint32_t)spl, P.n_batches - base);
      const int first_lane = lane - j;
      for (uint32_t t = 0; t < m; ++t) {
        const uint32_t batch = P.first_batch + base + t;
        const float* cc = colw + first_lane + (int)t;
#pragma unroll
        for (int ch = 0; ch < 4; ++ch)
          if (ch % spl == j) acc[ch] = fold_one(acc[ch], cc[ch * 64], batch);
        if (j == 0) {
          const float L = cc[256];
          mom1 = fold_one(mom1, L, batch);
          mom2 = fold_one(mom2, L * L, batch);
        }
      }
     }
     __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
     __builtin_amdgcn_wave_barrier();
     __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
  }
  if (active) store_lane(P.accum + pix, acc, spl, j);
  if (active && live && j == 0) P.moments[pix] = make_float2(mom1, mom2);
}
