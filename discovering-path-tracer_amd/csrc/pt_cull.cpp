// pt_cull.cpp — primary-ray bundle culling: the NDC rectangles
// outside which every primary ray misses the scene and every light
// (ptd::cull_rects, pt_cull.h), and their entry points in the C ABI.
//
// Camera model of raytrace_comp.comp:430-460 in the orthonormal camera frame
// (right, up, ez = dir/|dir|) centred on the camera position, with the
// kernel's right = normalize(cross(dir, -up0)), up = normalize(cross(right, dir)):
//   origin O = (ox, oy, 0),     |ox|, |oy| <= 0.02 * Rg        (aperture, :445-448)
//   bdir ∝ (a, b, 1),  a = -ndcX*T*A/L, b = -ndcY*T/L          (:456-457)
//   ndcX = ndcX0 + jx*0.5/W,    |jx| <= Rg                     (:451-454)
//   F = 3*bdir,  dir ∝ F - O                                   (:459-460)
// where Rg bounds every Box-Muller radius sqrt(-2 log u1) with u1 >= 1e-38
// (:220): sqrt(-2 ln 1e-38) = 13.2286.  The ray reaches depth Z at slope
//   X/Z = a + ox (1/Z - 1/Fz),  Fz = 3/sqrt(1+a^2+b^2),
// so a point of depth Z > 0 with slope s is reachable from a pixel only if
// |s - a| <= 0.02 Rg max|1/Z - 1/Fz| for some a of the pixel's jittered range.
// Every object (root box corners, light rectangle corners — convex sets whose
// slope hull is the hull of the corners' slopes) therefore maps to an NDC
// rectangle of pixel origins that can reach it; outside all rectangles every
// primary ray misses the root box (so traceRay returns no hit) and every light
// (the pre-pass hits nothing), and the sample is exactly (0,0,0).  All maths
// in double with margins far above the kernel's float rounding.
// The derivation holds for any bound Rg on the two radii of a sample: with
// ptd::kGaussR it covers every sample; with ptd::kCullTightR it covers the
// samples whose two draws u1 are at least ptd::kCullTightU0 (pt_cull.h), which
// the kernel checks per sample before it skips one (PT_OPT_CULL_TIGHT).
// The footprints (ptd::cull_footprints, PT_OPT_CULL_FOOTPRINT) are the same
// theorem with each corner dilated by its own depth against the focal depths
// of the rays that can reach the object, and the hull of the corners' boxes in
// place of their bounding rectangle (object_footprint; proof in DESIGN.md §4).
// The sure regions (ptd::cull_sure) are the converse for a light: pixel origins
// from which every such ray hits it (light_sure).
#include <math.h>

#include "pt_context.h"
#include "pt_cull.h"

namespace {

struct D3 { double x, y, z; };
D3 d3(const float* f) { return {f[0], f[1], f[2]}; }
D3 dsub(D3 a, D3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
D3 dadd(D3 a, D3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
D3 dmul(D3 a, double s) { return {a.x * s, a.y * s, a.z * s}; }
double ddot(D3 a, D3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
D3 dcross(D3 a, D3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
double dlen(D3 a) { return sqrt(ddot(a, a)); }

// The camera frame and the bounds every derivation shares, for the radius bound Rg.
struct CullFrame {
  D3 cpos, right, up, ez;
  double L, T, A, jx, jy, fz_min, fz_max, rho;
};

bool cull_frame(const float cam[16], int W, int H, double Rg, CullFrame* f) {
  if (W <= 0 || H <= 0 || !(Rg >= 0.0 && Rg <= ptd::kGaussR)) return false;
  const D3 cdir = d3(cam + 4), cup = d3(cam + 8);
  f->cpos = d3(cam);
  const double fov = cam[12];
  const double L = dlen(cdir);
  if (!(L > 1e-6 && L < 1e6) || !(fov > 0.01 && fov < 170.0)) return false;
  const D3 rx = dcross(cdir, dmul(cup, -1.0));
  const double rl = dlen(rx);
  if (!(rl > 1e-6 * L * dlen(cup))) return false;
  f->right = dmul(rx, 1.0 / rl);
  const D3 ux = dcross(f->right, cdir);
  f->up = dmul(ux, 1.0 / dlen(ux));
  f->ez = dmul(cdir, 1.0 / L);
  const double T = tan(fov * 0.5 * M_PI / 180.0), A = (double)W / (double)H;
  const double jx = Rg * 0.5 / W, jy = Rg * 0.5 / H;                        // jitter in NDC
  const double amax = (1.0 + jx) * T * A / L, bmax = (1.0 + jy) * T / L;
  f->L = L; f->T = T; f->A = A; f->jx = jx; f->jy = jy;
  f->fz_min = 3.0 / sqrt(1.0 + amax * amax + bmax * bmax);
  f->fz_max = 3.0;
  f->rho = 0.02 * Rg * 1.001;
  return true;
}

// The corners of the root box, dilated for the slab test's float rounding.
void root_points(const float* lo, const float* hi, D3 pts[8]) {
  double m = 0.0;
  for (int k = 0; k < 3; ++k) m = fmax(m, fmax(fabs((double)lo[k]), fabs((double)hi[k])));
  m = 1e-4 * m + 1e-6;
  for (int i = 0; i < 8; ++i)
    pts[i] = {(i & 1 ? hi[0] + m : lo[0] - m), (i & 2 ? hi[1] + m : lo[1] - m), (i & 4 ? hi[2] + m : lo[2] - m)};
}

// The corners of a light rectangle: pos ± right*half0 ± up*half1 with the
// frame of setup_lights_kernel (:261-264), halves dilated, as a thin slab.
bool light_points(const pt_area_light& li, D3 pts[8]) {
  const D3 nr = d3(li.normal);
  const double nl = dlen(nr);
  if (!(nl > 0.0)) return false;
  const D3 nn = dmul(nr, 1.0 / nl);
  // the kernel picks the basis from its float normalize; near the switch
  // point either basis may be taken, and the rectangle's orientation is
  // then unknown — use its circumscribed square (both orientations inside)
  const D3 basis = fabs(nn.y) < 0.999 ? D3{0, 1, 0} : D3{1, 0, 0};
  const D3 lr = dmul(dcross(nn, basis), 1.0 / dlen(dcross(nn, basis)));
  const D3 lu = dcross(lr, nn);
  double h0 = fabs((double)li.size[0]) * 0.5, h1 = fabs((double)li.size[1]) * 0.5;
  const D3 pos = d3(li.position);
  const double pm = fmax(fmax(fabs(pos.x), fabs(pos.y)), fabs(pos.z));
  if (fabs(fabs(nn.y) - 0.999) < 1e-4) h0 = h1 = fmax(h0, h1) * 1.41422;
  h0 = h0 * 1.0001 + 1e-4 * pm + 1e-6;
  h1 = h1 * 1.0001 + 1e-4 * pm + 1e-6;
  if (!(h0 < 1e30 && h1 < 1e30)) return false;
  for (int i = 0; i < 4; ++i) {
    const D3 c = dadd(dadd(pos, dmul(lr, i & 1 ? h0 : -h0)), dmul(lu, i & 2 ? h1 : -h1));
    // a thin slab around the plane covers the float plane-intersection error
    const double th = 1e-4 * (pm + h0 + h1) + 1e-6;
    pts[2 * i] = dadd(c, dmul(nn, th));
    pts[2 * i + 1] = dadd(c, dmul(nn, -th));
  }
  return true;
}

// An object's corners in the camera frame: slopes, inverse depths and their
// ranges.  False: a corner at or behind the camera plane (or NaN).
struct Projected {
  double sx[8], sy[8], z[8];
  double sx0, sx1, sy0, sy1, z0, z1;
};
bool project(const CullFrame& f, const D3* pts, int np, Projected* o) {
  o->sx0 = o->sy0 = o->z0 = INFINITY;
  o->sx1 = o->sy1 = o->z1 = -INFINITY;
  for (int i = 0; i < np; ++i) {
    const D3 r = dsub(pts[i], f.cpos);
    const double X = ddot(r, f.right), Y = ddot(r, f.up), Z = ddot(r, f.ez);
    if (!(Z > 1e-4 * (1.0 + dlen(r)))) return false;   // at or behind the camera plane (or NaN)
    o->sx[i] = X / Z; o->sy[i] = Y / Z; o->z[i] = Z;
    o->sx0 = fmin(o->sx0, X / Z); o->sx1 = fmax(o->sx1, X / Z);
    o->sy0 = fmin(o->sy0, Y / Z); o->sy1 = fmax(o->sy1, Y / Z);
    o->z0 = fmin(o->z0, Z); o->z1 = fmax(o->z1, Z);
  }
  return true;
}

// The rectangle of pixel origins that can reach the object (before the jitter
// and the margins), its slope dilation and the margins.
struct RectD {
  double x0, x1, y0, y1, del, mx, my;
};
RectD object_rect(const CullFrame& f, const Projected& p, int W, int H) {
  const double dd = fmax(fmax(fabs(1.0 / p.z0 - 1.0 / f.fz_min), fabs(1.0 / p.z0 - 1.0 / f.fz_max)),
                         fmax(fabs(1.0 / p.z1 - 1.0 / f.fz_min), fabs(1.0 / p.z1 - 1.0 / f.fz_max)));
  RectD r;
  r.del = f.rho * dd;
  // slope -> NDC (the maps are decreasing), then the jitter and a margin of
  // ~1 pixel plus 1e-4 relative for the kernel's float evaluation
  r.x0 = -(p.sx1 + r.del) * f.L / (f.T * f.A); r.x1 = -(p.sx0 - r.del) * f.L / (f.T * f.A);
  r.y0 = -(p.sy1 + r.del) * f.L / f.T; r.y1 = -(p.sy0 - r.del) * f.L / f.T;
  r.mx = 2.0 / W + 1e-4 * (1.0 + fabs(r.x0) + fabs(r.x1));
  r.my = 2.0 / H + 1e-4 * (1.0 + fabs(r.y0) + fabs(r.y1));
  return r;
}

bool rect_floats(const CullFrame& f, RectD r, float* o) {
  r.x0 -= f.jx + r.mx; r.x1 += f.jx + r.mx; r.y0 -= f.jy + r.my; r.y1 += f.jy + r.my;
  if (!(r.x0 == r.x0 && r.x1 == r.x1 && r.y0 == r.y0 && r.y1 == r.y1)) return false;
  o[0] = nextafterf((float)r.x0, -INFINITY); o[1] = nextafterf((float)r.x1, INFINITY);
  o[2] = nextafterf((float)r.y0, -INFINITY); o[3] = nextafterf((float)r.y1, INFINITY);
  return true;
}

// The footprint of one object (pt_cull.h): the convex hull of its corners'
// pixel-origin boxes.  A point of the object is a convex combination of the
// corners in (slope, 1/Z) -- (X, Y, Z) -> (X/Z, Y/Z, 1/Z) is projective, so it
// keeps segments -- and |1/Z - 1/Fz| is convex in 1/Z, so the box of pixel
// slopes that reach the point (half width rho |1/Z - 1/Fz|) lies in the same
// combination of the corners' boxes, each with its own depth.  Fz ranges over
// the pixel slopes that can reach the object at all: the object's slope
// range widened by the rectangle derivation's dilation `del`.
bool object_footprint(const CullFrame& f, const Projected& p, int np, int W, int H, float* o) {
  const RectD r = object_rect(f, p, W, H);
  float pub[4];
  if (!rect_floats(f, r, pub)) return false;
  auto sq_range = [](double lo, double hi, double* mn, double* mx) {
    *mn = lo <= 0.0 && hi >= 0.0 ? 0.0 : fmin(lo * lo, hi * hi);
    *mx = fmax(lo * lo, hi * hi);
  };
  double a0, a1, b0, b1;
  sq_range(p.sx0 - r.del, p.sx1 + r.del, &a0, &a1);
  sq_range(p.sy0 - r.del, p.sy1 + r.del, &b0, &b1);
  const double fz_lo = fmax(f.fz_min, 3.0 / sqrt(1.0 + a1 + b1)), fz_hi = fmin(f.fz_max, 3.0 / sqrt(1.0 + a0 + b0));
  if (!(fz_lo <= fz_hi)) return false;
  double px[32], py[32];
  const double kx = f.L / (f.T * f.A), ky = f.L / f.T;
  for (int i = 0; i < np; ++i) {
    const double w = 1.0 / p.z[i];
    const double d = f.rho * fmax(fabs(w - 1.0 / fz_lo), fabs(w - 1.0 / fz_hi));
    const double cx = -p.sx[i] * kx, cy = -p.sy[i] * ky;
    const double ex = d * kx + f.jx + r.mx, ey = d * ky + f.jy + r.my;
    for (int k = 0; k < 4; ++k) {
      px[4 * i + k] = cx + (k & 1 ? ex : -ex);
      py[4 * i + k] = cy + (k & 2 ? ey : -ey);
      if (!(fabs(px[4 * i + k]) < 1e30 && fabs(py[4 * i + k]) < 1e30)) return false;
    }
  }
  const int n = 4 * np;
  // the bounding rectangle, never outside the rectangle derivation's
  double x0 = INFINITY, x1 = -INFINITY, y0 = INFINITY, y1 = -INFINITY;
  for (int i = 0; i < n; ++i) {
    x0 = fmin(x0, px[i]); x1 = fmax(x1, px[i]);
    y0 = fmin(y0, py[i]); y1 = fmax(y1, py[i]);
  }
  o[0] = fmaxf(pub[0], nextafterf((float)x0, -INFINITY)); o[1] = fminf(pub[1], nextafterf((float)x1, INFINITY));
  o[2] = fmaxf(pub[2], nextafterf((float)y0, -INFINITY)); o[3] = fminf(pub[3], nextafterf((float)y1, INFINITY));
  for (int k = 0; k < ptd::kFootprintPlanes; ++k) { o[4 + 3 * k] = 0.0f; o[5 + 3 * k] = 0.0f; o[6 + 3 * k] = 1.0f; }
  // convex hull, counter-clockwise (monotone chain)
  int idx[32];
  for (int i = 0; i < n; ++i) idx[i] = i;
  for (int i = 1; i < n; ++i)
    for (int j = i; j > 0 && (px[idx[j]] < px[idx[j - 1]] || (px[idx[j]] == px[idx[j - 1]] && py[idx[j]] < py[idx[j - 1]])); --j) {
      const int t = idx[j]; idx[j] = idx[j - 1]; idx[j - 1] = t;
    }
  auto turn = [&](int a, int b, int c) { return (px[b] - px[a]) * (py[c] - py[a]) - (py[b] - py[a]) * (px[c] - px[a]); };
  int hull[66], m = 0;
  for (int i = 0; i < n; ++i) {
    while (m >= 2 && turn(hull[m - 2], hull[m - 1], idx[i]) <= 0.0) --m;
    hull[m++] = idx[i];
  }
  for (int i = n - 2, t = m + 1; i >= 0; --i) {
    while (m >= t && turn(hull[m - 2], hull[m - 1], idx[i]) <= 0.0) --m;
    hull[m++] = idx[i];
  }
  --m;   // the first point again
  if (m < 3) return true;   // no area: the rectangle alone
  // the longest edges that are not the rectangle's own, as a x + b y <= c with
  // the interior on the left of each edge; c padded for the float coefficients
  // and the kernel's float evaluation at |x|, |y| <= 1
  double len[ptd::kFootprintPlanes] = {};
  for (int e = 0; e < m; ++e) {
    const int u = hull[e], v = hull[(e + 1) % m];
    const double dx = px[v] - px[u], dy = py[v] - py[u];
    const double l = sqrt(dx * dx + dy * dy);
    if (!(l > 0.0) || fabs(dx) <= 1e-9 * l || fabs(dy) <= 1e-9 * l) continue;
    const double a = dy / l, b = -dx / l, c = a * px[u] + b * py[u];
    const float af = (float)a, bf = (float)b;
    const float cf = nextafterf((float)(c + 4e-6 + 2e-6 * fabs(c)), INFINITY);
    if (!(af == af && bf == bf && cf == cf)) continue;
    int k = 0;   // replace the shortest kept edge
    for (int t = 1; t < ptd::kFootprintPlanes; ++t)
      if (len[t] < len[k]) k = t;
    if (l <= len[k]) continue;
    len[k] = l;
    o[4 + 3 * k] = af; o[5 + 3 * k] = bf; o[6 + 3 * k] = cf;
  }
  return true;
}

// A sure region's empty form: no pixel is inside.
void sure_none(float* o) {
  o[0] = 1.0f; o[1] = -1.0f; o[2] = 1.0f; o[3] = -1.0f;
  for (int k = 0; k < ptd::kFootprintPlanes; ++k) { o[4 + 3 * k] = 0.0f; o[5 + 3 * k] = 0.0f; o[6 + 3 * k] = -1.0f; }
}

// The sure region of one light (pt_cull.h): the slope quadrilateral of its
// rectangle, shrunk, eroded by the box a boundary point's slope can lie from
// the pixel's.  Scale the aperture offset from 0 to its value: the hit point
// on the light's plane moves continuously and starts at the pixel's own slope,
// inside the rectangle.  Were it to reach the rectangle's boundary, its depth
// would lie in the corners' range, so its slope would lie within
// rho max |1/Z_i - 1/Fz| of the pixel's -- but the pixel is farther than that
// from the quadrilateral's boundary.  It cannot run off to infinity (the
// plane seen edge-on) or to t = 0 without crossing the boundary first.  So the
// exact hit lies in the shrunk rectangle, in front of the origin; the shrink
// and the bound on |n . dir| below cover the kernel's float evaluation.
void light_sure(const CullFrame& f, const pt_area_light& li, int W, int H, double Rg, float* o) {
  sure_none(o);
  for (int k = 0; k < 3; ++k)
    if (!isfinite(li.intensity[k])) return;
  const D3 nr = d3(li.normal);
  const double nl = dlen(nr);
  if (!(nl >= 0.02 && nl < 1e6)) return;
  const D3 nn = dmul(nr, 1.0 / nl);
  if (fabs(fabs(nn.y) - 0.999) < 1e-4) return;   // the kernel's basis is not known here
  const D3 basis = fabs(nn.y) < 0.999 ? D3{0, 1, 0} : D3{1, 0, 0};
  const D3 lr = dmul(dcross(nn, basis), 1.0 / dlen(dcross(nn, basis)));
  const D3 lu = dcross(lr, nn);
  // the kernel's halves are signed, size * 0.5f (setup_lights_kernel), and fabs(u) <= half never holds for a
  // negative one: such a light cannot be hit at all.  (light_points may take fabs: it bounds from outside.)
  if (!(li.size[0] > 0.0f && li.size[1] > 0.0f)) return;
  const double h0 = (double)li.size[0] * 0.5, h1 = (double)li.size[1] * 0.5;
  const D3 pos = d3(li.position);
  const double pm = fmax(fmax(fabs(pos.x), fabs(pos.y)), fabs(pos.z));
  const double far = dlen(dsub(pos, f.cpos)) + h0 + h1;   // no point of the rectangle is farther from the camera
  if (!(far < 1e6)) return;
  // |n . dir| of a ray that hits inside: (distance of its origin from the plane) / (length to the hit)
  const double off = 0.02 * Rg * 1.001 * M_SQRT2;
  const double cosmin = (fabs(ddot(nn, dsub(pos, f.cpos))) - off) / (far + off);
  if (!(cosmin >= 0.05)) return;   // fabs(denom) >= 0.0001f holds with |n| >= 0.02; t's relative float error is below 2e-5
  const double shrink = 1e-4 * (pm + h0 + h1 + far) + 1e-6;
  const double g0 = h0 * 0.9999 - shrink, g1 = h1 * 0.9999 - shrink;
  if (!(g0 > 0.0 && g1 > 0.0)) return;
  D3 pts[4];
  const int order[4] = {0, 1, 3, 2};   // around the rectangle
  for (int i = 0; i < 4; ++i) {
    const int k = order[i];
    pts[i] = dadd(dadd(pos, dmul(lr, k & 1 ? g0 : -g0)), dmul(lu, k & 2 ? g1 : -g1));
  }
  Projected p;
  if (!project(f, pts, 4, &p)) return;
  // Fz over the pixel slopes of the region, which lie in the quadrilateral
  auto sq_range = [](double lo, double hi, double* mn, double* mx) {
    *mn = lo <= 0.0 && hi >= 0.0 ? 0.0 : fmin(lo * lo, hi * hi);
    *mx = fmax(lo * lo, hi * hi);
  };
  double a0, a1, b0, b1;
  sq_range(p.sx0, p.sx1, &a0, &a1);
  sq_range(p.sy0, p.sy1, &b0, &b1);
  const double fz_lo = fmax(f.fz_min, 3.0 / sqrt(1.0 + a1 + b1)), fz_hi = fmin(f.fz_max, 3.0 / sqrt(1.0 + a0 + b0));
  if (!(fz_lo <= fz_hi)) return;
  double e = 0.0;
  for (int i = 0; i < 4; ++i) {
    const double w = 1.0 / p.z[i];
    e = fmax(e, f.rho * fmax(fabs(w - 1.0 / fz_lo), fabs(w - 1.0 / fz_hi)));
  }
  const double kx = f.L / (f.T * f.A), ky = f.L / f.T;
  double qx[4], qy[4], x0 = INFINITY, x1 = -INFINITY, y0 = INFINITY, y1 = -INFINITY;
  for (int i = 0; i < 4; ++i) {
    qx[i] = -p.sx[i] * kx; qy[i] = -p.sy[i] * ky;
    x0 = fmin(x0, qx[i]); x1 = fmax(x1, qx[i]); y0 = fmin(y0, qy[i]); y1 = fmax(y1, qy[i]);
  }
  const double ex = e * kx + f.jx + 2.0 / W + 1e-4 * (1.0 + fabs(x0) + fabs(x1));
  const double ey = e * ky + f.jy + 2.0 / H + 1e-4 * (1.0 + fabs(y0) + fabs(y1));
  if (!(ex < 1e30 && ey < 1e30 && fabs(x0) < 1e30 && fabs(x1) < 1e30 && fabs(y0) < 1e30 && fabs(y1) < 1e30)) return;
  // a convex quadrilateral, made counter-clockwise
  double turn[4], area = 0.0;
  for (int i = 0; i < 4; ++i) {
    const int j = (i + 1) % 4, k = (i + 2) % 4;
    turn[i] = (qx[j] - qx[i]) * (qy[k] - qy[j]) - (qy[j] - qy[i]) * (qx[k] - qx[j]);
    area += qx[i] * qy[j] - qx[j] * qy[i];
  }
  const double sg = area > 0.0 ? 1.0 : -1.0;
  for (int i = 0; i < 4; ++i)
    if (!(sg * turn[i] > 0.0)) return;
  float out[ptd::kFootprintFloats];
  out[0] = nextafterf((float)(x0 + ex), INFINITY); out[1] = nextafterf((float)(x1 - ex), -INFINITY);
  out[2] = nextafterf((float)(y0 + ey), INFINITY); out[3] = nextafterf((float)(y1 - ey), -INFINITY);
  for (int i = 0; i < 4; ++i) {
    const int j = (i + 1) % 4;
    const double dx = sg * (qx[j] - qx[i]), dy = sg * (qy[j] - qy[i]);
    const double l = sqrt(dx * dx + dy * dy);
    if (!(l > 0.0)) return;
    const double a = dy / l, b = -dx / l, c = a * qx[i] + b * qy[i];   // inside: a x + b y <= c
    const float af = (float)a, bf = (float)b;
    const float cf = nextafterf((float)(c - (fabs(a) * ex + fabs(b) * ey) - (4e-6 + 2e-6 * fabs(c))), -INFINITY);
    if (!(af == af && bf == bf && cf == cf)) return;
    out[4 + 3 * i] = af; out[5 + 3 * i] = bf; out[6 + 3 * i] = cf;
  }
  for (int k = 0; k < ptd::kFootprintFloats; ++k) o[k] = out[k];
}

}  // namespace

int ptd::cull_sure(const float cam[16], int W, int H, const float* lo, const float* hi, const pt_area_light* lights,
                   int n_lights, float* sure, int max_sure, double Rg) {
  CullFrame f;
  if (n_lights < 0 || n_lights > max_sure || !cull_frame(cam, W, H, Rg, &f)) return -1;
  int n = 0;
  for (int l = 0; l < n_lights; ++l) {
    light_sure(f, lights[l], W, H, Rg, sure + kFootprintFloats * l);
    const float* r = sure + kFootprintFloats * l;
    n += r[0] <= r[1] && r[2] <= r[3] ? 1 : 0;
  }
  return n;
}

int ptd::cull_rects(const float cam[16], int W, int H, const float* lo, const float* hi, const pt_area_light* lights,
                    int n_lights, float* rects, int max_rects, double Rg) {
  CullFrame f;
  if (n_lights < 0 || n_lights + 1 > max_rects || !cull_frame(cam, W, H, Rg, &f)) return -1;
  int n = 0;
  D3 pts[8];
  Projected p;
  root_points(lo, hi, pts);
  if (!project(f, pts, 8, &p) || !rect_floats(f, object_rect(f, p, W, H), rects + 4 * n++)) return -1;
  for (int l = 0; l < n_lights; ++l)
    if (!light_points(lights[l], pts) || !project(f, pts, 8, &p) ||
        !rect_floats(f, object_rect(f, p, W, H), rects + 4 * n++))
      return -1;
  return n;
}

int ptd::cull_footprints(const float cam[16], int W, int H, const float* lo, const float* hi,
                         const pt_area_light* lights, int n_lights, float* foot, int max_foot, double Rg) {
  CullFrame f;
  if (n_lights < 0 || n_lights + 1 > max_foot || !cull_frame(cam, W, H, Rg, &f)) return -1;
  int n = 0;
  D3 pts[8];
  Projected p;
  root_points(lo, hi, pts);
  if (!project(f, pts, 8, &p) || !object_footprint(f, p, 8, W, H, foot + kFootprintFloats * n++)) return -1;
  for (int l = 0; l < n_lights; ++l)
    if (!light_points(lights[l], pts) || !project(f, pts, 8, &p) ||
        !object_footprint(f, p, 8, W, H, foot + kFootprintFloats * n++))
      return -1;
  return n;
}

extern "C" {

int pt_primary_cull_rects(const float cam[16], int w, int h, const float root_min[3], const float root_max[3],
                          const pt_area_light* lights, int n_lights, float* rects, int max_rects, int* n_rects) {
  return pt_primary_cull_rects_r(cam, w, h, root_min, root_max, lights, n_lights, ptd::kGaussR, rects, max_rects, n_rects,
                                 nullptr);
}

int pt_primary_cull_rects_r(const float cam[16], int w, int h, const float root_min[3], const float root_max[3],
                            const pt_area_light* lights, int n_lights, double radius_bound, float* rects,
                            int max_rects, int* n_rects, float* u0) {
  if (!cam || !root_min || !root_max || !rects || !n_rects || (n_lights > 0 && !lights))
    return fail(PT_ERR_INVALID, "null argument");
  if (max_rects < 1) return fail(PT_ERR_INVALID, "max_rects must be >= 1");
  const double R = radius_bound < 0.0 ? ptd::kCullTightR : radius_bound;
  if (!(R <= ptd::kGaussR)) return fail(PT_ERR_INVALID, "radius bound above 13.25");
  *n_rects = ptd::cull_rects(cam, w, h, root_min, root_max, lights, n_lights, rects, max_rects, R);
  if (u0) *u0 = ptd::kCullTightU0;
  return PT_OK;
}

int pt_primary_cull_footprints(const float cam[16], int w, int h, const float root_min[3], const float root_max[3],
                               const pt_area_light* lights, int n_lights, double radius_bound, float* footprints,
                               int max_footprints, int* n_footprints) {
  if (!cam || !root_min || !root_max || !footprints || !n_footprints || (n_lights > 0 && !lights))
    return fail(PT_ERR_INVALID, "null argument");
  if (max_footprints < 1) return fail(PT_ERR_INVALID, "max_footprints must be >= 1");
  const double R = radius_bound < 0.0 ? ptd::kCullTightR : radius_bound;
  if (!(R <= ptd::kGaussR)) return fail(PT_ERR_INVALID, "radius bound above 13.25");
  *n_footprints = ptd::cull_footprints(cam, w, h, root_min, root_max, lights, n_lights, footprints, max_footprints, R);
  return PT_OK;
}

int pt_primary_cull_sure(const float cam[16], int w, int h, const float root_min[3], const float root_max[3],
                         const pt_area_light* lights, int n_lights, double radius_bound, float* regions,
                         int max_regions, int* n_sure) {
  if (!cam || !root_min || !root_max || !regions || !n_sure || (n_lights > 0 && !lights))
    return fail(PT_ERR_INVALID, "null argument");
  const double R = radius_bound < 0.0 ? ptd::kCullTightR : radius_bound;
  if (!(R <= ptd::kGaussR)) return fail(PT_ERR_INVALID, "radius bound above 13.25");
  // no footprints, no sure regions: a region holds only outside the other objects' footprints
  float foot[ptd::kMaxCullObjects * ptd::kFootprintFloats];
  *n_sure = -1;
  if (n_lights <= max_regions &&
      ptd::cull_footprints(cam, w, h, root_min, root_max, lights, n_lights, foot, ptd::kMaxCullObjects, R) >= 0)
    *n_sure = ptd::cull_sure(cam, w, h, root_min, root_max, lights, n_lights, regions, max_regions, R);
  return PT_OK;
}

}  // extern "C"
