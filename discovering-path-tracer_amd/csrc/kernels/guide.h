// kernels/guide.h — guide_kernel, the first-hit guide image.
// A fragment: csrc/pt_device.hip includes it last, inside namespace ptd's
// anonymous namespace.

// First-hit guide image (pt_render_guide): one traceRay (:159-204) of each
// pixel's centre ray (pt_denoise.h guide_dir), stored as {n.xyz, t}, a miss as
// HitInfo's initial {0, 0, 0, 1e30}.  Every pixel of the frame, whatever the
// partition.  A workgroup takes 16x16 tiles in row-major order, a wave an 8x8
// quadrant.  MODE 0: the threaded exact walk from device memory; 1: the same
// with the scene staged in LDS; 2: the culled wide walk, one ray per lane
// (leaves queued and flushed per lane; a ray wide_ray_ok refuses -- a zero
// direction component -- takes the exact walk).  The wide walk's grid is
// bounded by the lanes that own a stack overflow area, so its workgroups
// stride over the tiles.  The answer is the reference's bit for bit on every
// path (wide_walk.h), so the three modes agree.
template <int MODE, bool QN>
__global__ __launch_bounds__(256) void guide_kernel(RenderParams P, float4* __restrict__ guide, int n_tiles) {
  const int tid = (int)threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  __shared__ int cq[4][kWideQ > kCand ? kWideQ : kCand][64];
  int* cand = &cq[wave][0][lane];
  __shared__ int2 stk[MODE == 2 ? 4 : 1][MODE == 2 ? kWideLds : 1][64];
  int2* lds = &stk[MODE == 2 ? wave : 0][0][lane];
  if (MODE == 1) {
    extern __shared__ float4 lds_scene[];
    const int nn = 2 * P.n_nodes, nt = 3 * P.n_tris;
    for (int i = tid; i < nn; i += 256) lds_scene[i] = P.nodes[i];
    for (int i = tid; i < nt; i += 256) lds_scene[nn + i] = P.tris[i];
    __syncthreads();
    P.nodes = lds_scene;
    P.tris = lds_scene + nn;
  }
  const long long os = (long long)gridDim.x * 256;
  int2* ovf = MODE == 2 ? P.wide_ovf + ((long long)blockIdx.x * 256 + tid) : nullptr;
  v3 cpos, cdir, right, up;
  load_camera(P, &cpos, &cdir, &right, &up);
  Ctr c = {0u, 0u, 0u, 0u, 0u};
  for (int tile = (int)blockIdx.x; tile < n_tiles; tile += (int)gridDim.x) {
    const int px = (tile % P.blocks_x) * 16 + (wave & 1) * 8 + (lane & 7);
    const int py = (tile / P.blocks_x) * 16 + (wave >> 1) * 8 + (lane >> 3);
    if (px >= P.width || py >= P.height) continue;
    const v3 d = ptdn::guide_dir(cdir, right, up, P.tan_fov, P.width, P.height, px, py);
    float t = 1e30f;
    const float4* rec = nullptr;   // the hit triangle's record
    bool exact = MODE != 2;
    if (MODE == 2) {
      WideRay R;
      wide_start(R, cpos, d, false, 0.0f);
      exact = !wide_ray_ok(R.o, R.d, R.inv);
      while (!exact) {
        const bool fin = wide_step<false, true, QN>(R, P.wide, P.wide_tris, lds, 64, ovf, os, P.wide_stack, &exact,
                                                    &c.nodes, &c.leaves, cand, P.wide_leafbox);
        if (exact) break;   // the builder's stack bound rules this out; stay exact anyway
        if (fin || R.nc > kWideQ - 4) wide_flush<false, QN>(R, P.wide_tris, cand, &c.leaves, P.wide_leafbox);
        if (fin) break;
      }
      if (!exact) {
        t = R.lim;
        if (R.best >= 0) rec = P.wide_tris + 3 * (size_t)R.best;
      }
    }
    if (exact) {
      const Hit h = MODE == 1 ? trace_closest<false, false, false>(P, cpos, d, c, cand)
                              : trace_closest<false, false, true>(P, cpos, d, c, cand);
      t = h.t;
      rec = h.tri >= 0 ? P.tris + 3 * (size_t)h.tri : nullptr;
    }
    float4 g = make_float4(0.0f, 0.0f, 0.0f, 1e30f);
    if (rec) {
      const float4 C = rec[2];   // {e2.z, n.xyz}
      g = make_float4(C.y, C.z, C.w, t);
    }
    guide[(size_t)py * (size_t)P.width + (size_t)px] = g;
  }
}
