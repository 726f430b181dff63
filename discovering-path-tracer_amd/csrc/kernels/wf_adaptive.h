// kernels/wf_adaptive.h — wf_gen_adaptive_kernel and wf_fold_adaptive_kernel: an
// adaptive round (pt_adaptive_begin / pt_adaptive_advance with
// PT_OPT_ADAPTIVE_WF) on the wavefront pipeline.  They are wf_gen_kernel and
// wf_fold_kernel<true> with the pixel of a path taken from the round's live
// list instead of wf_pixel's item arithmetic; the trace, tail and shading
// kernels between them see paths only through list slots and counters and run
// as they are.
// A fragment: csrc/pt_device.hip includes it after kernels/wf_shade.h, inside
// namespace ptd's anonymous namespace.
//
// Siblings, not further instantiations, for render_adaptive_kernel's reason
// (kernels/adaptive.h): a template argument would have put the list and its
// length into RenderParams and a test of them on every workgroup's way, in
// kernels whose code is to stay as it is (profiles/adaptive_wf/resource_usage.md).
//
// Numbering (pt_device.h wf_adaptive_path): in a chunk of nb batches, path
// g = (e * 256 + q) * nb + s is sample s of pixel q of live entry e.  256 * nb
// is a multiple of 256, so a generation workgroup lies inside one entry and a
// fold workgroup is one entry: the list load and the test against *n_live are
// workgroup-uniform (scalar), and a workgroup past the live length leaves as a
// whole, before any barrier.  Every live entry of one round carries the same
// {first_batch, n_batches} (pt_device.h launch_wavefront_adaptive), which the
// host has put into P; the entry supplies the tile's origin only.
//
// Both are templates over an argument that has one value, LIST = 1 ("the pixel
// comes from a live list"): a template is emitted where it is first named, the
// table at the end of pt_device.hip, so the two lie behind every earlier kernel
// of the code object and those keep their places; a plain kernel would be
// emitted here, in the middle, and move all that follow.

// Ray generation + shading up to the primary trace of the live tiles' paths:
// wf_gen_kernel<false>'s body, op for op, behind the list's pixel.
template <int LIST>
__global__ __launch_bounds__(256, 4) void wf_gen_adaptive_kernel(RenderParams P, WfBuffers B,
                                                                 const int4* __restrict__ list,
                                                                 const int* __restrict__ n_live) {
  const WfAdaptivePath a = wf_adaptive_path((uint32_t)blockIdx.x, (uint32_t)threadIdx.x, P.n_batches);
  if ((int)a.entry >= *n_live) return;   // uniform per workgroup
  const int4 en = list[a.entry];
  const long long g = a.g;
  bool need = false;
  Trav T;
  PathSt S;
  CamFrame F;
  F.px = en.x + a.q % 16;
  F.py = en.y + a.q / 16;
  if (F.px < P.width && F.py < P.height) {
    F.W = P.width;
    F.H = P.height;
    load_camera(P, &F.cpos, &F.cdir, &F.right, &F.up);
    F.ndcX0 = (2.0f * (float)F.px / (float)F.W) - 1.0f;
    F.ndcY0 = (2.0f * (float)F.py / (float)F.H) - 1.0f;
    F.aspect = (float)F.W / (float)F.H;
    F.tanFov = P.tan_fov;
    v3 col = mk(0.0f, 0.0f, 0.0f);
    S.s = a.s;
    // the per-sample skip (PT_OPT_CULL_TIGHT), as wf_gen_kernel
    bool reach = pixel_live(P, F.ndcX0, F.ndcY0);
    if (reach && !pixel_tight(P, F.ndcX0, F.ndcY0)) {
      const uint32_t batch = (P.first_batch + P.seed_base) + S.s;   // the seed's batch (PT_OPT_SEED_BASE)
      uint32_t rng = (batch * (uint32_t)F.H + (uint32_t)F.py) * (uint32_t)F.W + (uint32_t)F.px;
      const float u1a = fmax_(1e-38f, rng_next(&rng));
      rng_next(&rng);
      const float u1j = fmax_(1e-38f, rng_next(&rng));
      reach = u1a < P.cull_u0 || u1j < P.cull_u0;
    }
    if (reach) {
      S.phase = PH_BEGIN;
      Ctr c = {0u, 0u, 0u, 0u, 0u};
      need = path_step<false>(P, F, S, T, c, &col);
    }
    if (!need) B.colors[g] = make_float4(col.x, col.y, col.z, 1.0f);
  }
  // list slots: one atomic per workgroup (wf_gen_kernel)
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
}

// Running mean (:467-469) of each live pixel's samples and of its luminance
// moments, in batch order: wf_fold_kernel<true>'s body behind the list's pixel,
// one workgroup per entry.  A culled pixel's colours are (0,0,0,1): its moments
// fold L = +0 into +0, the bits the path-recursive round leaves there.
template <int LIST>
__global__ __launch_bounds__(256) void wf_fold_adaptive_kernel(RenderParams P, WfBuffers B,
                                                               const int4* __restrict__ list,
                                                               const int* __restrict__ n_live) {
  const int entry = (int)blockIdx.x;
  if (entry >= *n_live) return;   // uniform per workgroup
  const int4 en = list[entry];
  const int q = (int)threadIdx.x;
  const int px = en.x + q % 16, py = en.y + q / 16;
  if (px >= P.width || py >= P.height) return;
  float4* dst = P.accum + (size_t)py * (size_t)P.width + (size_t)px;
  float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (!(P.fresh && P.first_batch == 0)) {
    const float4 a = *dst;
    acc[0] = a.x; acc[1] = a.y; acc[2] = a.z; acc[3] = a.w;
  }
  float mom1 = 0.0f, mom2 = 0.0f;
  float2* mdst = P.moments + (size_t)py * (size_t)P.width + (size_t)px;
  if (P.first_batch != 0) {
    const float2 m = *mdst;
    mom1 = m.x;
    mom2 = m.y;
  }
  const float4* col = B.colors + wf_adaptive_index(entry, q, 0u, P.n_batches);
  for (uint32_t s = 0; s < P.n_batches; ++s) {
    const float4 c = col[s];
    const uint32_t batch = P.first_batch + s;
    const float fb = (float)batch, fb1 = (float)(batch + 1u);
    acc[0] = (acc[0] * fb + c.x) / fb1;
    acc[1] = (acc[1] * fb + c.y) / fb1;
    acc[2] = (acc[2] * fb + c.z) / fb1;
    acc[3] = (acc[3] * fb + 1.0f) / fb1;
    const float L = ptdn::lum(c.x, c.y, c.z);
    mom1 = (mom1 * fb + L) / fb1;
    mom2 = (mom2 * fb + L * L) / fb1;
  }
  *mdst = make_float2(mom1, mom2);
  *dst = make_float4(acc[0], acc[1], acc[2], acc[3]);
}
