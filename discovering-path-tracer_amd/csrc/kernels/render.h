// kernels/render.h — render_kernel (the path-recursive kernel) with its fold,
// emit, culled-item fill and gathered-frame unpack helpers, and the
// PT_WG_TRACE probe's buffer.
// A fragment: csrc/pt_device.hip includes it after kernels/shading.h, inside
// namespace ptd's anonymous namespace.

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// CNT kernels: add the wave's traced-work counters to P.stats[4..8]
// (closest walks, shadow walks, nodes visited, triangle tests, primaries).
__device__ __forceinline__ void flush_traced(const RenderParams& P, const Ctr& c, int lane) {
  const unsigned long long v0 = wave_sum(c.rays), v1 = wave_sum(c.srays), v2 = wave_sum(c.nodes),
                           v3_ = wave_sum(c.leaves), v4 = wave_sum(c.prim);
  if (lane == 0) {
    atomicAdd(&P.stats[4], v0);
    atomicAdd(&P.stats[5], v1);
    atomicAdd(&P.stats[6], v2);
    atomicAdd(&P.stats[7], v3_);
    atomicAdd(&P.stats[8], v4);
  }
}

// Running mean of n_batches constant colours (0,0,0,1) over this lane's
// channels (c = j mod spl), op for op the fold below.  Closed form where it is
// exact: (acc*b + 0)/(b+1) stays +0 once acc is +-0, and a batch-0 fold of
// any finite acc gives acc*0 + 0 = +0; (acc*b + 1)/(b+1) likewise stays 1.
__device__ __forceinline__ void fold_constant(const RenderParams& P, float* acc, int spl, int j) {
  if (P.n_batches == 0) return;
#pragma unroll
  for (int ch = 0; ch < 4; ++ch) {
    if (ch % spl != j) continue;
    const float k = ch < 3 ? 0.0f : 1.0f;
    if (acc[ch] == k || (P.first_batch == 0 && __builtin_isfinite(acc[ch]))) {
      acc[ch] = k;
    } else {
      for (uint32_t t = 0; t < P.n_batches; ++t) {
        const uint32_t batch = P.first_batch + t;
        acc[ch] = (acc[ch] * (float)batch + k) / (float)(batch + 1u);
      }
    }
  }
}

// This lane's channels (c = j mod spl) of the pixel's running mean.
__device__ __forceinline__ void store_lane(float4* px, const float* acc, int spl, int j) {
  float* a = (float*)px;
#pragma unroll
  for (int ch = 0; ch < 4; ++ch)
    if (ch % spl == j) a[ch] = acc[ch];
}

// The pixel's result: into the accumulation buffer, or (pt_render_packed)
// into this workgroup's slot of the packed live-item layout, where pixels
// outside the image are zeros (acc of an inactive lane is never loaded).
__device__ __forceinline__ void emit_lane(const RenderParams& P, bool active, size_t pix, int q, const float* acc,
                                          int spl, int j) {
  if (P.pack_out)
    store_lane(P.pack_out + (size_t)blockIdx.x * (size_t)(256 / spl) + (size_t)q, acc, spl, j);
  else if (active)
    store_lane(P.accum + pix, acc, spl, j);
}

// Whether a point lies in one region of the footprint table (pt_cull.h): a rectangle cut by half-planes.
__device__ __forceinline__ bool region_holds(const float* __restrict__ f, float x, float y) {
  bool in = x >= f[0] && x <= f[1] && y >= f[2] && y <= f[3];
#pragma unroll
  for (int k = 0; k < kFootprintPlanes; ++k) in = in && f[4 + 3 * k] * x + f[5 + 3 * k] * y <= f[6 + 3 * k];
  return in;
}

// What a pixel's samples with both radius draws at least P.cull_u0 are: kSkipNever, they are traced like
// any other (the pixel can reach something, or there are no tight rectangles); kSkipBlack, (0,0,0): the
// pixel lies outside every tight rectangle, or with footprints (PT_OPT_CULL_FOOTPRINT, P.n_foot > 0: a
// table in device memory walked with a run-time loop) outside every footprint; l >= 0, the intensity of
// light l: the pixel lies in that light's sure region and in no footprint but the light's own.  Without
// footprints the rectangles are tested with static indices: P stays in SGPRs/kernarg.
constexpr int kSkipNever = -2, kSkipBlack = -1;
__device__ __forceinline__ int pixel_skip(const RenderParams& P, float ndcX0, float ndcY0) {
  if (P.n_cull_tight < 0) return kSkipNever;
  if (P.n_foot > 0) {   // uniform
    int inside = 0, last = 0;
    for (int r = 0; r < P.n_foot; ++r) {   // at most kMaxCullRects (the host's table holds as many)
      const bool in = region_holds(P.foot + kFootprintFloats * r, ndcX0, ndcY0);
      inside += in ? 1 : 0;
      last = in ? r : last;
    }
    if (inside == 0) return kSkipBlack;
    // object r > 0 is light r - 1; its sure region follows the kMaxCullRects footprints
    if (inside == 1 && last >= 1 && last <= P.n_sure &&
        region_holds(P.foot + kFootprintFloats * (kMaxCullRects + last - 1), ndcX0, ndcY0))
      return last - 1;
    return kSkipNever;
  }
  bool tight = false;
#pragma unroll
  for (int r = 0; r < kMaxCullRects; ++r)
    tight = tight || (r < P.n_cull_tight && ndcX0 >= P.cull_tight[r][0] && ndcX0 <= P.cull_tight[r][1] &&
                      ndcY0 >= P.cull_tight[r][2] && ndcY0 <= P.cull_tight[r][3]);
  return tight ? kSkipNever : kSkipBlack;
}
// ... for the kernels that know only the black skip: a pixel of a sure region counts as tight and is traced.
__device__ __forceinline__ bool pixel_tight(const RenderParams& P, float ndcX0, float ndcY0) {
  return pixel_skip(P, ndcX0, ndcY0) != kSkipBlack;
}
// The light of a pixel that pixel_skip found sure: such a pixel lies in no other light's footprint, hence in
// no other light's sure region.  From operands the compiler cannot match with the prologue's: it would
// otherwise keep the index in a VGPR across the sample loop.
__device__ __forceinline__ int skip_again(const RenderParams& P, float ndcX0, float ndcY0) {
  asm volatile("" : "+v"(ndcX0), "+v"(ndcY0));
  int l = 0;
  for (int k = 1; k < P.n_sure; ++k)
    l = region_holds(P.foot + kFootprintFloats * (kMaxCullRects + k), ndcX0, ndcY0) ? k : l;
  return l;
}
// The colour of a skipped sample.
__device__ __forceinline__ float4 skip_colour(const RenderParams& P, int skip) {
  if (skip < 0) return make_float4(0.0f, 0.0f, 0.0f, 1.0f);
  const LightDev* L = P.lights + skip;
  return make_float4(L->inten[0], L->inten[1], L->inten[2], 1.0f);
}

// Items (tile parts) whose every pixel is culled, listed by the host with
// their first pixel: each thread folds the constant colour (0,0,0,1) into one
// pixel's running mean, closed form where exact (fold_constant) — kPixPerFill
// pixels per thread.  Runs as the trailing workgroups of the render launch,
// so it overlaps the render tail instead of costing a launch of its own.
// An item is 256 / spl pixels (a power of two), so a pixel's item and place
// in it are a shift and a mask: the per-pixel tile arithmetic (a 64-bit
// division, the partition's and the rotated tile order's) cost more than the
// fill itself -- box 1080p8, 70 % of the pixels culled: see DESIGN A.4.
#ifndef PT_PIX_PER_FILL
#define PT_PIX_PER_FILL 8
#endif
constexpr int kPixPerFill = PT_PIX_PER_FILL;
__device__ __forceinline__ int item_shift(int spl) { return 8 - __builtin_ctz((unsigned)spl); }   // log2(256 / spl)
__device__ __forceinline__ void fill_culled(const RenderParams& P, const int2* __restrict__ org, int n, int block) {
  const int lg = item_shift(P.spl);
  const long long total = (long long)n << lg;
  for (int k = 0; k < kPixPerFill; ++k) {
    const long long g = ((long long)block * kPixPerFill + k) * 256 + threadIdx.x;
    if (g >= total) return;
    const int2 o = org[g >> lg];
    const int q = (int)g & ((1 << lg) - 1);
    const int px = o.x + (q & 15);
    const int py = o.y + (q >> 4);
    if (px >= P.width || py >= P.height) continue;
    float4* dst = P.accum + (size_t)py * (size_t)P.width + (size_t)px;
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (!(P.fresh && P.first_batch == 0)) {
      const float4 a = *dst;
      acc[0] = a.x; acc[1] = a.y; acc[2] = a.z; acc[3] = a.w;
    }
    fold_constant(P, acc, 1, 0);
    *dst = make_float4(acc[0], acc[1], acc[2], acc[3]);
  }
}

// Pixel q of part `part` of tile `tile` (the render kernel's mapping).
__device__ __forceinline__ bool tile_pixel(const RenderParams& P, int tile, int part, int q, size_t* pix) {
  const int spl = P.spl;
  int bx, by;
  tile_block(tile, P.blocks_x, &bx, &by);
  const int px = bx * 16 + q % 16;
  const int py = by * 16 + part * (16 / spl) + q / 16;
  *pix = (size_t)py * (size_t)P.width + (size_t)px;
  return px < P.width && py < P.height;
}

// One pixel-slot g of the gathered-frame assembly (items_unpack_kernel, and
// the trailing workgroups of a pt_render_packed launch): a live item's pixel
// from its rank's slot, a culled item's pixel as (0,0,0,1).  Table entries
// are {rank, x0, y0, slot}: the item's first pixel comes from the host, so
// a pixel costs a shift and a mask (fill_culled).
__device__ __forceinline__ void unpack_pixel(const RenderParams& P, float4* __restrict__ frame,
                                             const float4* __restrict__ src, size_t slot_f4,
                                             const int* __restrict__ table, long long g) {
  const int lg = item_shift(P.spl);
  const int4 e = ((const int4*)table)[g >> lg];
  const int q = (int)g & ((1 << lg) - 1);
  const int px = e.y + (q & 15), py = e.z + (q >> 4);
  if (px >= P.width || py >= P.height) return;
  frame[(size_t)py * (size_t)P.width + (size_t)px] =
      e.w >= 0 ? src[(size_t)e.x * slot_f4 + ((size_t)e.w << lg) + q] : make_float4(0.0f, 0.0f, 0.0f, 1.0f);
}

__device__ __forceinline__ void unpack_block(const RenderParams& P, int block) {
  const long long total = (long long)P.n_unpack * (256 / P.spl);
  for (int k = 0; k < kPixPerFill; ++k) {
    const long long g = ((long long)block * kPixPerFill + k) * 256 + threadIdx.x;
    if (g >= total) return;
    unpack_pixel(P, P.unpack_frame, P.unpack_src, (size_t)P.unpack_slot_f4, P.unpack_table, g);
  }
}

// One step of the running mean (:467-469); its two exact shortcuts are explained above.
__device__ __forceinline__ float fold_one(float a, float c, uint32_t batch) {
  const float fb = (float)batch, fb1 = (float)(batch + 1u);
  if (a == 1.0f && c == 1.0f && batch < (1u << 24)) return 1.0f;
  const float x = a * fb + c;
  if (((batch + 1u) & batch) == 0u && batch + 1u != 0u) return x * (1.0f / fb1);
  return x / fb1;
}

#ifdef PT_WG_TRACE   // probe builds only (tools/r06_wg_trace.py): per live workgroup {t0, t1, hw_id << 32 | xcc | spl << 8, x0 << 32 | y0}
constexpr int kWgTraceCap = 1 << 16;
__device__ unsigned long long g_wg_trace[kWgTraceCap][4];
#endif

// LDS=true stages the whole scene (threaded nodes + triangle records) in LDS
// once per workgroup; chosen by the host for scenes of at most a few tens of
// KB (box.obj is 1.3 KB), where every lane re-reads the same few nodes.
// SWEEP (LDS, no counters): a tiny scene's walks are the box sweep over
// P.sweep; only the triangle records are staged, by leaf.  SWEEP 2: the table
// has hull faces (P.sweep_hull) and the walk reuses the root's slab products
// for them; a table without any runs SWEEP 1, the walk that keeps nothing
// from the root's test.  SWEEP 3: the cube table (P.sweep_cube: every box but
// the root is a hull face), walked straight-line from P.root_lo / root_hi and
// P.cube_under / cube_all with no read through P.sweep (PT_OPT_SWEEP_CUBE).
// MOMENTS (PT_OPT_MOMENTS; never with STATS or CNT): the lane that folds a
// pixel's red also folds the sample luminances L and L * L into P.moments, in
// batch order with the colour's own step (fold_one).
// EXIT (device-memory scenes, never with STATS): path_trace_fused's instantiation
// with the exit skip; the LDS-staged kernels branch on P.exit_skip instead.
template <bool STATS, bool LDS, bool CNT = false, int SWEEP = 0, bool MOMENTS = false, bool EXIT = false>
#ifndef PT_RENDER_MIN_BLOCKS
#define PT_RENDER_MIN_BLOCKS 5
#endif
// the parked walks (sweep, and LDS without stats) run 6 blocks per CU (kPark above)
__global__ __launch_bounds__(256, SWEEP || (LDS && !STATS) ? 6 : PT_RENDER_MIN_BLOCKS) void render_kernel(RenderParams P) {
  const int tid = (int)threadIdx.x;
  // Work mapping.  A 16x16 pixel tile (the partition unit) is split into
  // SPL workgroups; lane l of wave w handles pixel q = w*(64/SPL) + l/SPL of
  // its workgroup and sample slot j = l % SPL, so the SPL lanes of a pixel
  // trace that pixel's samples side by side: coherent rays, and SPL times
  // finer work granularity than one pixel per thread, which is what keeps a
  // tile-split frame fast on 8 GPUs (pixels on geometry cost ~10x the others).
  // A persistent variant pulling wave-sized items from per-XCD queues was
  // measured slower at every SPL, on 1 GPU and on a 1/8 tile share.
  if ((P.items || P.pack_out) && (int)blockIdx.x >= P.n_items) {   // trailing workgroups (uniform)
    if (P.pack_out)
      unpack_block(P, (int)blockIdx.x - P.n_items);   // assemble the previous gathered frame
    else
      fill_culled(P, P.culled_org, P.n_culled_items, (int)blockIdx.x - P.n_items);
    return;
  }
  // item = (owned tile, part); with culling the host launches only items that
  // can hold a live pixel, listed in P.items.  With mixed lanes (P.mix) each
  // live item carries its own lane count: whole tiles at one lane per pixel
  // first (the cheapest per sample), parts at P.spl lanes after them (short
  // workgroups that fill the launch's drain).  Uniform per workgroup.
  // cost feedback (PT_OPT_MIXED_LANES' measured schedule): each wave adds
  // its duration on the GPU wall clock to the counter of the 16x4 part of
  // the frame its pixels lie in
  const unsigned long long cost_t0 = P.cost_out ? wall_clock64() : 0ull;
  int gx0, gy0;
  bool tile_ok = true;
  int spl = P.spl;
  if (P.items_org) {
    const int2 o = P.items_org[blockIdx.x];
    gx0 = o.x & ((1 << kMixShift) - 1);
    gy0 = o.y;
    if (P.mix) spl = 1 << (o.x >> kMixShift);
  } else {
    const int item = (int)blockIdx.x;
    const int tile = rank_tile(P, item / spl);
    int bx, by;
    tile_block(tile, P.blocks_x, &bx, &by);
    gx0 = bx * 16;
    gy0 = by * 16 + (item % spl) * (16 / spl);
    tile_ok = tile < P.blocks_total;
  }
#ifdef PT_WG_TRACE
  const unsigned long long wg_t0 = wall_clock64();
#endif
  const int wave = tid >> 6, lane = tid & 63;
  // per wave: the leaf-candidate queue, then a [slot][lane] area that holds
  // the path state parked during walks (kPark floats) and, between samples,
  // the colour hand-off (4 floats) -- never both at once
  static_assert(!SWEEP || (LDS && !STATS && !CNT), "the sweep walk is the plain LDS kernel's");
  constexpr int kQueue = SWEEP ? 0 : kCand;   // the sweep walk queues nothing
  static_assert(!MOMENTS || (!STATS && !CNT), "moments: the plain kernels only");
  constexpr int kHand = MOMENTS ? 5 : 4;              // floats handed off per sample: the colour, then L
  static_assert(kPark >= kHand, "the hand-off shares the parked state's area");
  __shared__ int cand_buf[4][kQueue + kPark][64];
  int* cand = &cand_buf[wave][0][lane];
  float* colw = (float*)&cand_buf[wave][kQueue][0];   // colour hand-off, [channel][lane]
  const int q = wave * (64 / spl) + lane / spl;       // pixel within the workgroup
  const int j = lane % spl;                           // sample slot
  const int px = gx0 + q % 16;
  const int py = gy0 + q / 16;
  const bool active = tile_ok && px < P.width && py < P.height;   // :425-428
  Ctr c = {0u, 0u, 0u, 0u, 0u};
  const int W = P.width, H = P.height;
  // Per-pixel constants of main() (:430-432, :446-447, :457), hoisted out of
  // the sample loop — same values every sample.
  const float ndcX0 = (2.0f * (float)px / (float)W) - 1.0f;
  const float ndcY0 = (2.0f * (float)py / (float)H) - 1.0f;
  // Primary-ray culling (pt_primary_cull_rects): outside every rectangle no
  // primary ray of this pixel can reach the root box or a light, so each
  // sample is (0,0,0) — the value the trace below would produce.  A workgroup
  // with no live pixel skips the scene staging and the sample loop.
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
  // The tight rectangles (pt_cull.h, PT_OPT_CULL_TIGHT): the same theorem per
  // sample, for radii of at most kCullTightR.  A live pixel outside all of
  // them traces a sample only if one of the sample's two radius draws is below
  // P.cull_u0 (its radius may then exceed the bound); every other sample of it
  // is (0,0,0), the value the trace would produce.  Stats mode never skips.
  // With footprints a pixel of a light's sure region skips them with the light's intensity (pixel_skip).
  // Two lane masks are kept across the sample loop, not the light's index: a third live VGPR costs this
  // kernel two more spilled ones, so a sure pixel's skipped sample finds its light again (skip_again).
  const int skip0 = STATS ? kSkipNever : pixel_skip(P, ndcX0, ndcY0);
  const bool tight = skip0 == kSkipNever;
  const bool sure = skip0 >= 0;
  const size_t pix = (size_t)py * (size_t)W + (size_t)px;
  uint32_t nsamp = 0;
  if (active && (uint32_t)j < P.n_batches)
    nsamp = (P.n_batches - (uint32_t)j + (uint32_t)spl - 1) / (uint32_t)spl;
  // Running mean (:467-469): lane j of a pixel folds channels c = j (mod spl)
  // of that pixel, sample by sample in batch order.
  float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  // fresh: a launch that starts at batch 0 begins a new accumulation from a
  // cleared (+0) image — what pt_clear_accum would have stored — without
  // reading it (PT_OPT_FRESH_BATCH0).
  if (active && !(P.fresh && P.first_batch == 0)) {
    const float* a = (const float*)&P.accum[pix];
#pragma unroll
    for (int ch = 0; ch < 4; ++ch)
      if (ch % spl == j) acc[ch] = a[ch];
  }
  // A culled pixel's colours are all (0,0,0,1): its lanes fold them without
  // the colour hand-off (fold_constant), the live pixels' lanes below.
  if (!live && active) fold_constant(P, acc, spl, j);
  // the pixel's moments, on its first lane: a launch from batch 0 starts from +0 (m * 0 + L = L)
  float mom1 = 0.0f, mom2 = 0.0f;
  if constexpr (MOMENTS) {
    if (active && live && j == 0 && P.first_batch != 0) {
      const float2 m = P.moments[pix];
      mom1 = m.x;
      mom2 = m.y;
    }
  }
  if (!wg_live) {   // uniform per workgroup; stats mode never culls
    emit_lane(P, active, pix, q, acc, spl, j);
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
    P.hit_tris = P.tris;   // no wide walk here: hits are slots
  }
  {
    const v3 cpos = mk(P.cam_pos[0], P.cam_pos[1], P.cam_pos[2]);
    const v3 cdir = mk(P.cam_dir[0], P.cam_dir[1], P.cam_dir[2]);
    const float aspect = (float)W / (float)H;
    // Camera frame (:430-432): computed once on the host with the same ops.
    const v3 right = mk(P.cam_right[0], P.cam_right[1], P.cam_right[2]);
    const v3 up = mk(P.cam_upv[0], P.cam_upv[1], P.cam_upv[2]);
    const float tanFov = P.tan_fov;
    for (uint32_t base = 0; base < P.n_batches; base += (uint32_t)spl) {
     const uint32_t s = base + (uint32_t)j;
     float4 col4 = make_float4(0.0f, 0.0f, 0.0f, 1.0f);
     if (active && live && s < P.n_batches) {
      const uint32_t batch = (P.first_batch + P.seed_base) + s;   // the seed's batch (PT_OPT_SEED_BASE); the fold's is below
      const uint32_t seed = (batch * (uint32_t)H + (uint32_t)py) * (uint32_t)W + (uint32_t)px;
      uint32_t rng = seed;
      // randomGaussian x2 (:218-226, :445, :451): the four draws first, in
      // the shader's order; a wave none of whose lanes needs its path (no
      // lane in a tight rectangle, every radius draw at least P.cull_u0)
      // goes straight to the fold with (0,0,0,1)
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
      const v3 origin = add(add(cpos, muls(right, ax)), muls(up, ay));   // :448
      r = sqrt_(-2.0f * log_(u1j));
      th = (2.0f * 0x1.921fb6p+1f) * u2j;
      sincos_(th, &sn, &cs);
      const float jx = r * cs, jy = r * sn;
      const float ndcX = ndcX0 + (jx * 0.5f) / (float)W;                 // :453-454
      const float ndcY = ndcY0 + (jy * 0.5f) / (float)H;
      const v3 bdir = normalize(sub(add(cdir, muls(neg(right), (ndcX * tanFov) * aspect)), muls(up, ndcY * tanFov)));
      const v3 focal = add(cpos, muls(bdir, 3.0f));                       // :459
      const v3 dir = normalize(sub(focal, origin));                       // :460
      // PF (prefetch node k+1) for the stats walk from device memory; on an
      // LDS-staged scene it measured slower at every tile share (1080p box:
      // +7 % on a whole frame, +12 % on a 1/8 share: registers)
      // Scenes walked from device memory pair each shadow ray with the next
      // closest-hit ray (path_trace_fused: two node round trips in flight,
      // sphere 20K tris -9 %); on an LDS-staged scene the round trip is short
      // and the pair's registers cost more than it hides (box +11 %).
      v3 col;
      if (CNT) c.prim++;
      if (STATS || LDS)
        col = path_trace<STATS, !LDS, CNT, SWEEP>(P, origin, dir, seed, c, cand);
      else
        col = path_trace_fused<CNT, EXIT>(P, origin, dir, seed, cand, c);
      col4 = make_float4(col.x, col.y, col.z, 1.0f);                      // vec4(color, 1.0)
      } else if (sure) {
        col4 = skip_colour(P, skip_again(P, ndcX0, ndcY0));
      }
     }
     if (spl == 1) {   // uniform: each lane folds its own sample, no hand-off (:467-469)
      if (active && live) {
        const uint32_t batch = P.first_batch + base;   // wave-uniform
        acc[0] = fold_one(acc[0], col4.x, batch);
        acc[1] = fold_one(acc[1], col4.y, batch);
        acc[2] = fold_one(acc[2], col4.z, batch);
        acc[3] = fold_one(acc[3], col4.w, batch);
        if constexpr (MOMENTS) {
          const float L = ptdn::lum(col4.x, col4.y, col4.z);
          mom1 = fold_one(mom1, L, batch);
          mom2 = fold_one(mom2, L * L, batch);
        }
      }
      continue;
     }
     // hand the chunk's colours to the folding lanes of the same pixel
     colw[lane] = col4.x;
     colw[64 + lane] = col4.y;
     colw[128 + lane] = col4.z;
     colw[192 + lane] = col4.w;
     if constexpr (MOMENTS) colw[256 + lane] = ptdn::lum(col4.x, col4.y, col4.z);
     __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
     __builtin_amdgcn_wave_barrier();
     __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
     if (active && live) {
      const uint32_t m = min((uint32_t)spl, P.n_batches - base);
      const int first_lane = lane - j;
      for (uint32_t t = 0; t < m; ++t) {
        const uint32_t batch = P.first_batch + base + t;                    // :468
        const float* cc = colw + first_lane + (int)t;
#pragma unroll
        for (int ch = 0; ch < 4; ++ch)
          if (ch % spl == j) acc[ch] = fold_one(acc[ch], cc[ch * 64], batch);
        if constexpr (MOMENTS) {
          if (j == 0) {
            const float L = cc[256];
            mom1 = fold_one(mom1, L, batch);
            mom2 = fold_one(mom2, L * L, batch);
          }
        }
      }
     }
     __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
     __builtin_amdgcn_wave_barrier();
     __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
  }
  emit_lane(P, active, pix, q, acc, spl, j);
  if constexpr (MOMENTS) {
    if (active && live && j == 0) P.moments[pix] = make_float2(mom1, mom2);
  }
  if (!STATS && P.cost_out && lane == 0) {
    // the wave's pixels lie in one 16x4 part: its first pixel row / 4
    const int part_row = (gy0 + wave * (64 / spl) / 16) >> 2;
    const unsigned long long dt = wall_clock64() - cost_t0;
    atomicAdd(&P.cost_out[part_row * P.blocks_x + (gx0 >> 4)], (unsigned)(dt < 0xffffffull ? dt : 0xffffffull));
  }
#ifdef PT_WG_TRACE
  if (!STATS && !CNT) {
    __syncthreads();
    if (tid == 0 && blockIdx.x < (unsigned)kWgTraceCap) {
      const unsigned hw = __builtin_amdgcn_s_getreg((31 << 11) | 4);    // HW_ID: wave, SIMD, CU, SE
      const unsigned xcc = __builtin_amdgcn_s_getreg((31 << 11) | 20);  // XCC_ID
      g_wg_trace[blockIdx.x][0] = wg_t0;
      g_wg_trace[blockIdx.x][1] = wall_clock64();
      g_wg_trace[blockIdx.x][2] = (unsigned long long)hw << 32 | (unsigned long long)((xcc & 0xff) | (spl << 8));
      g_wg_trace[blockIdx.x][3] = (unsigned long long)(unsigned)gx0 << 32 | (unsigned)gy0;
    }
  }
#endif
  if (STATS) {
    const unsigned long long rays = wave_sum(c.rays), nodes = wave_sum(c.nodes), leaves = wave_sum(c.leaves);
    const unsigned long long smp = wave_sum((unsigned long long)nsamp);
    if (lane == 0) {
      atomicAdd(&P.stats[0], rays);
      atomicAdd(&P.stats[1], nodes);
      atomicAdd(&P.stats[2], leaves);
      atomicAdd(&P.stats[3], smp);
    }
  }
  if (CNT) flush_traced(P, c, lane);
}
