// kernels/radiance.h — radiance queries (pt_trace_radiance): pathTrace along the
// caller's own rays from the caller's seeds, and the camera's own rays as
// queries (pt_camera_rays).
// A fragment: csrc/pt_device.hip includes it last (the kernels before it keep
// their places in the code object), inside namespace ptd's anonymous namespace.
//
// A query is a pt_ray read as {o.xyz, d.x} {d.yz, -, seed}; its answer one
// float4, the running mean (:467-469) of S samples from {+0, +0, +0, +0}.
// Path l of a chunk that starts at query q0 is sample s = l % S of query
// q0 + l / S, traced from the seed seed_q + s * stride (uint32 wrap-around); a
// chunk holds whole queries and fewer than 2^31 paths, so l is an int.  Each
// path's colour goes to colors[l], library-owned; radiance_fold_kernel then
// folds every query's S colours in order.  Two kernels make the colours:
// radiance_kernel for the scenes plan_launch renders path-recursively, and
// wf_gen_rays_kernel in front of the wavefront pipeline's own rounds for the
// others.  Nothing here counts anything, culls anything or knows a camera.
//
// All are templates (the single-valued ones over ONE = 1): a template is
// emitted where it is first named, the tables at the end of pt_device.hip, so
// every earlier kernel keeps its place (kernels/wf_adaptive.h).

struct RadianceQuery {
  v3 o, d;
  uint32_t seed;
};
// Two 16-byte loads a lane; a wave reads 64 consecutive paths' queries.
__device__ __forceinline__ RadianceQuery radiance_load(const float4* __restrict__ rays, size_t q) {
  const float4 r0 = rays[2 * q], r1 = rays[2 * q + 1];
  RadianceQuery r;
  r.o = mk(r0.x, r0.y, r0.z);
  r.d = mk(r0.w, r1.x, r1.y);
  r.seed = __float_as_uint(r1.w);
  return r;
}

// The path-recursive kernel, one path per lane: render_kernel's scene staging, walks, candidate and park
// columns (what path_trace and path_trace_fused expect) around the caller's ray in place of a pixel's; a
// sibling of render_kernel as render_adaptive_kernel is (kernels/adaptive.h), with its launch bounds.
// m: paths of the chunk; S: samples a query; q0: the chunk's first query.
template <bool LDS, int SWEEP, bool EXIT>
__global__ __launch_bounds__(256, SWEEP || LDS ? 6 : PT_RENDER_MIN_BLOCKS) void radiance_kernel(
    RenderParams P, const float4* __restrict__ rays, float4* __restrict__ colors, long long q0, int m, uint32_t S,
    uint32_t stride) {
  static_assert(!SWEEP || LDS, "the sweep walk is the LDS kernel's");
  static_assert(!EXIT || !LDS, "the LDS-staged kernels branch on P.exit_skip");
  const int tid = (int)threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  constexpr int kQueue = SWEEP ? 0 : kCand;   // the sweep walk queues nothing
  __shared__ int cand_buf[4][kQueue + kPark][64];
  int* cand = &cand_buf[wave][0][lane];
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
  const long long l = (long long)blockIdx.x * 256 + tid;
  if (l >= m) return;   // after the only barrier
  const uint32_t ql = (uint32_t)l / S;
  const uint32_t s = (uint32_t)l - ql * S;
  const RadianceQuery r = radiance_load(rays, (size_t)(q0 + ql));
  const uint32_t seed = r.seed + s * stride;
  Ctr c = {0u, 0u, 0u, 0u, 0u};
  v3 col;
  if (LDS)
    col = path_trace<false, !LDS, false, SWEEP>(P, r.o, r.d, seed, c, cand);
  else
    col = path_trace_fused<false, EXIT>(P, r.o, r.d, seed, cand, c);
  colors[l] = make_float4(col.x, col.y, col.z, 1.0f);
}

// The wavefront pipeline's generation for a chunk of queries: wf_gen_kernel's body with PH_BEGIN's camera
// ray (kernels/wf_state.h path_step) replaced by the caller's ray and seed -- S.rng = seed, thr = 1, rad = 0,
// depth = 0, the same `need` rule (max_depth > 0, or some light's plane is hit), trav_start, PH_PRIMARY --
// and no culling.  The trace, wide, tail and shading kernels then run as they are: they see a path through
// its list slot, and no path of theirs is ever in PH_BEGIN.  A primary ray the wide walk does not take
// (wide_ray_ok) comes back from wf_trace_wide_kernel as kNeedExactClosest and the shading round walks it
// exactly before path_step sees it, as it does a bounce ray; the tail kernel does the same in its own lane.
template <int ONE>
__global__ __launch_bounds__(256, 4) void wf_gen_rays_kernel(RenderParams P, WfBuffers B,
                                                             const float4* __restrict__ rays, long long q0, int m,
                                                             uint32_t S, uint32_t stride) {
  const long long l = (long long)blockIdx.x * 256 + threadIdx.x;
  bool need = false;
  Trav T;
  PathSt S0;
  if (l < m) {
    const uint32_t ql = (uint32_t)l / S;
    const uint32_t s = (uint32_t)l - ql * S;
    const RadianceQuery r = radiance_load(rays, (size_t)(q0 + ql));
    S0.s = s;
    S0.rng = r.seed + s * stride;   // :307
    S0.thr = mk(1.0f, 1.0f, 1.0f);
    S0.rad = mk(0.0f, 0.0f, 0.0f);
    S0.depth = 0;
    S0.li = S0.k = 0;
    S0.travel = 0.0f;
    S0.hp = S0.hn = S0.acc3 = S0.pend = S0.sss_thr = S0.so = S0.sd = S0.cp = S0.sn = mk(0.0f, 0.0f, 0.0f);
    need = P.max_depth > 0;
    for (int i = 0; i < P.n_lights && !need; ++i) {
      float tl;
      need = intersect_area_light(r.o, r.d, load_light(P, i), &tl);
    }
    if (need) {
      trav_start(T, r.o, r.d, false, 0.0f);
      S0.phase = PH_PRIMARY;
    } else {
      B.colors[l] = make_float4(0.0f, 0.0f, 0.0f, 1.0f);   // no light in view and max_depth 0: radiance 0
    }
  }
  // list slots: one atomic per workgroup (wf_gen_kernel)
  __shared__ int wave_n[4], wave_base[4];
  const unsigned long long mk_ = __ballot(need);
  const int w = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
  if (lane == 0) wave_n[w] = (int)__popcll(mk_);
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
  const int slot = wave_base[w] +
                   (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mk_ >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mk_, 0u));
  if (need) {
    wf_push(B, 0, slot, (int)l, T, fuse_bits(P, S0, T), S0.rng);
    wf_store_state(B, 0, slot, S0);
  }
}

// The running mean (:467-469) of each query's S colours in order, from {+0, +0, +0, +0}; always applied, so
// S = 1 is (0 * 0 + c) / 1 and a -0 radiance comes out +0.  One lane per query; nq queries from q0.
template <int ONE>
__global__ __launch_bounds__(256) void radiance_fold_kernel(const float4* __restrict__ colors, float4* __restrict__ out,
                                                           long long q0, int nq, uint32_t S) {
  const int i = (int)(blockIdx.x * 256 + threadIdx.x);
  if (i >= nq) return;
  const float4* col = colors + (size_t)i * S;
  float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  for (uint32_t s = 0; s < S; ++s) {
    const float4 c = col[s];
    const float fb = (float)s, fb1 = (float)(s + 1u);
    acc[0] = (acc[0] * fb + c.x) / fb1;
    acc[1] = (acc[1] * fb + c.y) / fb1;
    acc[2] = (acc[2] * fb + c.z) / fb1;
    acc[3] = (acc[3] * fb + 1.0f) / fb1;
  }
  out[q0 + i] = make_float4(acc[0], acc[1], acc[2], acc[3]);
}

// main()'s own ray of pixel pixels[i] (null: pixel i) and sample batch `batch`, as a query: camera_ray
// (pt_camera_ray.h) of P's camera and size, limit 1e30f, reserved the sample's seed.  One lane per entry.
template <int ONE>
__global__ __launch_bounds__(256) void camera_rays_kernel(RenderParams P, uint32_t batch,
                                                         const int* __restrict__ pixels, long long n,
                                                         float4* __restrict__ rays) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const long long pix = pixels ? (long long)pixels[i] : i;
  const int px = (int)(pix % P.width), py = (int)(pix / P.width);
  v3 cpos, cdir, right, up;
  load_camera(P, &cpos, &cdir, &right, &up);
  const CamFrame F = cam_frame(cpos, cdir, right, up, P.tan_fov, P.width, P.height, px, py);
  const uint32_t seed = camera_seed(batch, P.width, P.height, px, py);
  v3 o, d;
  camera_ray(F, seed, &o, &d);
  rays[2 * i] = make_float4(o.x, o.y, o.z, d.x);
  rays[2 * i + 1] = make_float4(d.y, d.z, 1e30f, __uint_as_float(seed));
}
