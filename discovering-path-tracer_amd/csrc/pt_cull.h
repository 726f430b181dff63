// pt_cull.h — the radius bounds of primary-ray culling, shared by the host
// derivation (pt_cull.cpp cull_rects), the render kernel's per-sample test
// (kernels/render.h) and tests/cull_radius_check.cpp.
#pragma once
#include "pt_math.h"

struct pt_area_light;   // include/pathtracer.h

namespace ptd {

// Every Box-Muller radius sqrt(-2 log u1) with u1 >= 1e-38
// (raytrace_comp.comp:220) is below this: sqrt(-2 ln 1e-38) = 13.2286.
constexpr double kGaussR = 13.25;

// The tight bound (PT_OPT_CULL_TIGHT): a second set of rectangles is derived
// with it, and a sample of a pixel outside them is traced only if one of its
// two radii can exceed it.  A radius above 4.25 is drawn with probability
// e^-9.03 = 1.2e-4.  (The two macros are for A/B builds of other bounds; they
// go together: tests/cull_radius_check.cpp R prints the u0 of a bound R.)
#ifndef PT_CULL_TIGHT_R
#define PT_CULL_TIGHT_R 4.25
#define PT_CULL_TIGHT_U0 0x1.f5b12ep-14f
#endif
constexpr double kCullTightR = PT_CULL_TIGHT_R;

// randomGaussian's radius (:218-226) for the draw u, the kernel's own ops.
PT_FN float cull_radius(float u) { return ptm::sqrt_(-2.0f * ptm::log_(ptm::fmax_(1e-38f, u))); }

// The least float u0 such that cull_radius(u) <= kCullTightR for every float
// u in [u0, 1]: all 1.1e8 of them evaluated, none assumed monotone, by
// tests/cull_radius_check.cpp (bits 0x38fad897: radius 4.25 exactly; the float
// below it gives 4.25000048).  A draw u1 >= kCullTightU0 has its radius within
// the tight bound.
constexpr float kCullTightU0 = PT_CULL_TIGHT_U0;

// The cull rectangles of a frame (pt_cull.cpp, host only): {x0, x1, y0, y1} in
// NDC for the root box lo..hi, then for each light.  Returns the rectangle
// count (>= 0) or -1 when no guarantee is derived.  Rg: the bound on the
// Box-Muller radii the rectangles hold for.
__attribute__((visibility("hidden"))) int cull_rects(const float cam[16], int W, int H, const float* lo,
                                                     const float* hi, const pt_area_light* lights, int n_lights,
                                                     float* rects, int max_rects, double Rg = kGaussR);

// A footprint (PT_OPT_CULL_FOOTPRINT): a convex region of pixel origins in
// NDC, {x0, x1, y0, y1} cut by kFootprintPlanes half-planes {a, b, c}, a pixel
// being inside when a * x + b * y <= c for each (an unused one is {0, 0, 1}).
// One per object, in the order of cull_rects and with its guarantee -- outside
// every footprint no primary ray with radii of at most Rg reaches the root box
// or a light -- but the hull of the corners' own boxes, each dilated by its
// own depth against the focal depths of the rays that can reach the object,
// instead of one rectangle dilated by the worst pair.  Each footprint lies in
// the object's rectangle for the same Rg.  Returns the count or -1.
constexpr int kMaxCullObjects = 8;   // the root box and 7 lights (pt_device.h kMaxCullRects)
constexpr int kFootprintPlanes = 4;
constexpr int kFootprintFloats = 4 + 3 * kFootprintPlanes;
__attribute__((visibility("hidden"))) int cull_footprints(const float cam[16], int W, int H, const float* lo,
                                                          const float* hi, const pt_area_light* lights, int n_lights,
                                                          float* foot, int max_foot, double Rg);

// The sure regions (PT_OPT_CULL_FOOTPRINT), one per light in a footprint's
// layout (an empty one where none is derived: a non-finite intensity, a size
// that is not positive, a light seen within 3 degrees of edge-on, a corner
// behind the camera): every
// primary ray with radii of at most Rg from a pixel inside passes
// intersectAreaLight's float tests for that light.  Where the pixel also lies
// outside the footprint at Rg of the root box and of every other light, the
// pre-pass hits exactly this light, the closest walk finds nothing, and the
// sample is (intensity, 1).  Returns the count of non-empty regions or -1.
__attribute__((visibility("hidden"))) int cull_sure(const float cam[16], int W, int H, const float* lo, const float* hi,
                                                    const pt_area_light* lights, int n_lights, float* sure,
                                                    int max_sure, double Rg);

}  // namespace ptd
