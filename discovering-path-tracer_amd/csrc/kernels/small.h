// kernels/small.h — the small kernels: triangle and light setup, the rank
// gather, clear, tile and item pack / unpack, and the math self-tests.
// A fragment: csrc/pt_device.hip includes it after kernels/render.h (whose
// tile_pixel and unpack_pixel it uses), inside namespace ptd's anonymous
// namespace.

__global__ __launch_bounds__(256) void setup_tris_kernel(const float* __restrict__ V, const uint32_t* __restrict__ I,
                                                         int n_tris, float4* __restrict__ out) {
  const int t = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (t >= n_tris) return;
  const uint32_t i0 = I[3 * t + 0] * 3u, i1 = I[3 * t + 1] * 3u, i2 = I[3 * t + 2] * 3u;
  const v3 v0 = mk(V[i0], V[i0 + 1], V[i0 + 2]);
  const v3 v1 = mk(V[i1], V[i1 + 1], V[i1 + 2]);
  const v3 v2 = mk(V[i2], V[i2 + 1], V[i2 + 2]);
  const v3 e1 = sub(v1, v0), e2 = sub(v2, v0);
  const v3 n = normalize(cross(e1, e2));
  out[3 * t + 0] = make_float4(v0.x, v0.y, v0.z, e1.x);
  out[3 * t + 1] = make_float4(e1.y, e1.z, e2.x, e2.y);
  out[3 * t + 2] = make_float4(e2.z, n.x, n.y, n.z);
}

// Per-light constants of sampleAreaLight / intersectAreaLight (:261-264,
// :284-287, :295-296), computed with the shader's ops.
// Triangle records in leaf-rank order for the wide walk.
__global__ __launch_bounds__(256) void gather_tris_kernel(const float4* __restrict__ tris,
                                                          const int* __restrict__ tri_of, int n,
                                                          float4* __restrict__ dst) {
  const int i = (int)(blockIdx.x * 256 + threadIdx.x);
  if (i >= 3 * n) return;
  const int r = i / 3, k = i - 3 * r;
  dst[i] = tris[3 * (size_t)tri_of[r] + k];
}

__global__ __launch_bounds__(64) void setup_lights_kernel(const LightRec* __restrict__ in, int n,
                                                          LightDev* __restrict__ out) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n) return;
  const LightRec L = in[i];
  const v3 nr = mk(L.normal[0], L.normal[1], L.normal[2]);
  const v3 nn = normalize(nr);
  const v3 basis = fabs_(nn.y) < 0.999f ? mk(0.0f, 1.0f, 0.0f) : mk(1.0f, 0.0f, 0.0f);
  const v3 right = normalize(cross(nn, basis));
  const v3 up = cross(right, nn);
  LightDev d;
  for (int c = 0; c < 3; ++c) {
    d.pos[c] = L.position[c];
    d.nraw[c] = L.normal[c];
    d.inten[c] = L.intensity[c];
  }
  d.right[0] = right.x; d.right[1] = right.y; d.right[2] = right.z;
  d.up[0] = up.x; d.up[1] = up.y; d.up[2] = up.z;
  d.size[0] = L.size[0];
  d.size[1] = L.size[1];
  d.half[0] = L.size[0] * 0.5f;
  d.half[1] = L.size[1] * 0.5f;
  d.finite = (__builtin_isfinite(d.inten[0]) && __builtin_isfinite(d.inten[1]) && __builtin_isfinite(d.inten[2]))
                 ? 1.0f : 0.0f;
  out[i] = d;
}

__global__ __launch_bounds__(256) void clear_kernel(float4* accum, int W, int H, int m, int cnt,
                                                    const int* __restrict__ pos) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)W * (size_t)H) return;
  const int x = (int)(i % (size_t)W), y = (int)(i / (size_t)W);
  const int blocks_x = (W + 15) / 16;
  const int b = block_tile(x / 16, y / 16, blocks_x);
  bool own = false;
  for (int i = 0; i < cnt; ++i) own = own || pos[i] == b % m;
  const float z = own ? 0.0f : -0.0f;
  accum[i] = make_float4(z, z, z, z);
}

// Owned 16x16 tiles <-> a dense buffer (tile o = the rank's o-th tile, part_tile,
// 256 float4 row-major inside the tile, zeros outside the image): what a rank
// ships to the root so the frame can be assembled by a gather.
template <bool PACK>
__global__ __launch_bounds__(256) void tiles_kernel(float4* frame, float4* packed, int W, int H, int blocks_x,
                                                    int m, int cnt, const int* __restrict__ pos) {
  const int o = (int)blockIdx.x;
  const int b = (o / cnt) * m + pos[o % cnt];
  const int t = (int)threadIdx.x;
  int bx, by;
  tile_block(b, blocks_x, &bx, &by);
  const int x = bx * 16 + (t & 15), y = by * 16 + (t >> 4);
  const bool in = x < W && y < H;
  const size_t pi = (size_t)y * (size_t)W + (size_t)x;
  const size_t ti = (size_t)o * 256 + (size_t)t;
  if (PACK)
    packed[ti] = in ? frame[pi] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  else if (in)
    frame[pi] = packed[ti];
}

__global__ __launch_bounds__(256) void items_pack_kernel(RenderParams P, const float4* __restrict__ frame,
                                                         float4* __restrict__ packed, const int* __restrict__ items,
                                                         int n) {
  const int per = 256 / P.spl;
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  if (g >= (long long)n * per) return;
  size_t pix;
  const int item = items[g / per];
  const bool in = tile_pixel(P, rank_tile(P, item / P.spl), item % P.spl, (int)(g % per), &pix);
  packed[g] = in ? frame[pix] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

__global__ __launch_bounds__(256) void items_unpack_kernel(RenderParams P, float4* __restrict__ frame,
                                                           const float4* __restrict__ src, size_t slot_f4,
                                                           const int* __restrict__ table, int n) {
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  if (g >= (long long)n * (256 / P.spl)) return;
  unpack_pixel(P, frame, src, slot_f4, table, g);
}

__global__ __launch_bounds__(256) void math_kernel(int fn, const float* __restrict__ x, float* __restrict__ y,
                                                   size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float v = x[i];
  float r;
  switch (fn) {
    case 0: r = log_(v); break;
    case 1: r = exp_(v); break;
    case 2: r = sin_(v); break;
    case 3: r = cos_(v); break;
    case 4: r = tan_(v); break;
    case 5: r = acos_(v); break;
    case 6: r = sqrt_(v); break;
    case 7: { uint32_t s = __float_as_uint(v); r = rng_next(&s); break; }
    case 8: r = rcp_(v); break;
    default: r = v; break;
  }
  y[i] = r;
}

// Exhaustive equivalence of the device's fast-quotient math with the IEEE
// definitions (pt_math.h): every one of the 2^32 input bit patterns.
// fn 0 rcp_ vs 1/x, 1 log_, 2 exp_, 3 acos_ (each vs its FAST=false
// form).  NaN results compare equal when both are NaN.
// The wave-uniform fast forms are checked on their pieces, since consecutive
// inputs share a wave and the guarded function would answer the 63 inputs next
// to a range boundary from the IEEE side: fn 4 sqrt_in_range(x) implies
// sqrt_fast_(x) is __builtin_sqrtf(x), 5 rcp_in_range(x) implies rcp_fast_(x)
// is 1/x, 7 div1p5_in_range(x) implies div1p5_fast_(x) is x / 1.5f (an input
// out of range counts as equal).  fn 6: sincos_ against sin_ and cos_, both
// results.
__global__ __launch_bounds__(256) void exhaustive_kernel(int fn, unsigned long long* bad, uint32_t* first_bad) {
  unsigned long long nbad = 0;
  uint32_t first = 0xffffffffu;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (1ull << 32); i += stride) {
    const float x = __uint_as_float((uint32_t)i);
    float a, b, a2 = 0.0f, b2 = 0.0f;
    switch (fn) {
      case 0: a = rcp_(x); b = 1.0f / x; break;
      case 1: a = log_(x); b = log_impl<false>(x); break;
      case 2: a = exp_(x); b = exp_impl<false>(x); break;
      case 4: b = __builtin_sqrtf(x); a = sqrt_in_range(x) ? sqrt_fast_(x) : b; break;
      case 5: b = 1.0f / x; a = rcp_in_range(x) ? rcp_fast_(x) : b; break;
      case 6: sincos_(x, &a, &a2); b = sin_(x); b2 = cos_(x); break;
      case 7: b = x / 1.5f; a = div1p5_in_range(x) ? div1p5_fast_(x) : b; break;
      default: a = acos_(x); b = acos_impl<false>(x); break;
    }
    const bool same = (__float_as_uint(a) == __float_as_uint(b) || (a != a && b != b)) &&
                      (__float_as_uint(a2) == __float_as_uint(b2) || (a2 != a2 && b2 != b2));
    if (!same) {
      ++nbad;
      first = min(first, (uint32_t)i);
    }
  }
  if (nbad) {
    atomicAdd(bad, nbad);
    atomicMin(first_bad, first);
  }
}
