// pt_isect.h — the reference's two intersection tests, shared by the device
// kernels (kernels/*.h, pt_device.hip) and host-side checks of the culled wide walk
// (wide_walk.h, tests/wide_check.cpp).  Same float ops, same order as the
// shader; compiled with -ffp-contract=off like everything in pt_math.h.
#pragma once
#include "pt_math.h"

namespace ptd {
using namespace ptm;

// intersectAABB (raytrace_comp.comp:102-112) with invDir hoisted (same value
// every node).
PT_FN bool slab(v3 o, v3 inv, float4 a, float4 b) {
  const float t0x = (a.x - o.x) * inv.x, t0y = (a.y - o.y) * inv.y, t0z = (a.z - o.z) * inv.z;
  const float t1x = (b.x - o.x) * inv.x, t1y = (b.y - o.y) * inv.y, t1z = (b.z - o.z) * inv.z;
  const float tmin = fmax_(fmax_(fmin_(t0x, t1x), fmin_(t0y, t1y)), fmin_(t0z, t1z));
  const float tmax = fmin_(fmin_(fmax_(t0x, t1x), fmax_(t0y, t1y)), fmax_(t0z, t1z));
  return tmin <= tmax && tmax >= 0.0f;
}

// intersectTriangle (:114-157), edges precomputed; UV tail is dead code.
// Record {v0.xyz, e1.x} {e1.yz, e2.xy} {e2.z, n.xyz} (pt_device.h tris).
PT_FN bool tri_test(v3 o, v3 d, float4 A, float4 B, float4 C, float* tout) {
  const float EPS = 0.000001f;
  const v3 v0 = mk(A.x, A.y, A.z);
  const v3 e1 = mk(A.w, B.x, B.y);
  const v3 e2 = mk(B.z, B.w, C.x);
  const v3 p = cross(d, e2);
  const float det = dot(e1, p);
  if (fabs_(det) < EPS) return false;
  const float inv = rcp_(det);
  const v3 s = sub(o, v0);
  const float u = inv * dot(s, p);
  if (u < 0.0f || u > 1.0f) return false;
  const v3 q = cross(s, e1);
  const float v = inv * dot(d, q);
  if (v < 0.0f || u + v > 1.0f) return false;
  const float t = inv * dot(e2, q);
  if (t <= EPS) return false;
  *tout = t;
  return true;
}

// intersectTriangle's barycentrics (:137, :143) of a record tri_test accepted:
// u = inv * dot(s, p), v = inv * dot(d, q), the values its range tests read.
// For the one winning record of a ray query (pt_trace_rays); tri_test itself
// keeps its instruction stream.
PT_FN void tri_uv(v3 o, v3 d, float4 A, float4 B, float4 C, float* uout, float* vout) {
  const v3 v0 = mk(A.x, A.y, A.z);
  const v3 e1 = mk(A.w, B.x, B.y);
  const v3 e2 = mk(B.z, B.w, C.x);
  const v3 p = cross(d, e2);
  const float inv = rcp_(dot(e1, p));
  const v3 s = sub(o, v0);
  *uout = inv * dot(s, p);
  *vout = inv * dot(d, cross(s, e1));
}

// sampleHemisphere (:229-243) from its two draws, r1 first.
__host__ __device__ static __forceinline__ v3 hemisphere_dir(v3 n, float r1, float r2) {
  const float th = acos_(sqrt_(1.0f - r1));
  const float ph = (2.0f * 0x1.921fb6p+1f) * r2;
  float st, ct, sp, cp;
  sincos_(th, &st, &ct);
  sincos_(ph, &sp, &cp);
  const v3 l = mk(st * cp, st * sp, ct);
  const v3 upv = fabs_(n.z) < 0.999f ? mk(0.0f, 0.0f, 1.0f) : mk(1.0f, 0.0f, 0.0f);
  const v3 t = normalize(cross(upv, n));
  const v3 b = cross(n, t);
  return add(add(muls(t, l.x), muls(b, l.y)), muls(n, l.z));
}

// The exit skip (PT_OPT_EXIT_SKIP): whether the bounce ray from
// ro = hp + hn * OFFSET provably misses the root box [lo, hi] whatever its
// hemisphere direction, given r1, the draw sample_hemisphere makes first.
// True only when, for one axis a: hn's other two components are +-0 bitwise
// and 0.999 <= |hn.a| <= 2; ro lies more than 1e-30 beyond the root's face on
// the side hn.a points to; and r1 < 1 (the cosine sincos_ returns for
// acos_(sqrt_(1 - r1)) is positive on [0, 1) and negative at 1.0f).  Then the
// direction's a component is hn.a * ct exactly, both root slab products on a
// are negative and slab() is false.  tests/exit_skip_check.cpp checks it.
PT_FN bool exit_axis(float n, float o, float lo, float hi) {
  const float an = fabs_(n);
  const float d = n > 0.0f ? o - hi : lo - o;
  return an >= 0.999f && an <= 2.0f && d > 1e-30f;
}
PT_FN bool exit_skip(v3 hn, v3 ro, float r1, v3 lo, v3 hi) {
  const bool zx = (f2u(hn.x) << 1) == 0u, zy = (f2u(hn.y) << 1) == 0u, zz = (f2u(hn.z) << 1) == 0u;
  bool out = false;
  if (zy && zz) out = exit_axis(hn.x, ro.x, lo.x, hi.x);
  else if (zx && zz) out = exit_axis(hn.y, ro.y, lo.y, hi.y);
  else if (zx && zy) out = exit_axis(hn.z, ro.z, lo.z, hi.z);
  return out && r1 < 1.0f;
}
// Condition 1 alone: a normal for which exit_skip can ever hold (the host's
// per-scene flag).
PT_FN bool exit_normal(v3 hn) {
  const bool zx = (f2u(hn.x) << 1) == 0u, zy = (f2u(hn.y) << 1) == 0u, zz = (f2u(hn.z) << 1) == 0u;
  const float an = fabs_(zy && zz ? hn.x : zx && zz ? hn.y : hn.z);
  return ((zy && zz) || (zx && zz) || (zx && zy)) && an >= 0.999f && an <= 2.0f;
}

}  // namespace ptd
