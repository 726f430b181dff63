// pt_radiance_host.cpp — pathTrace on the host (pt_radiance_host.h): the
// operations of kernels/shading.h path_trace in the shader's order, with
// pt_math.h's IEEE forms and pt_rays_host.cpp's depth-first walk.
#include "pt_radiance_host.h"

#include <string.h>

#include <algorithm>
#include <thread>
#include <vector>

#include "pt_camera_ray.h"
#include "pt_denoise.h"
#include "pt_isect.h"
#include "pt_rays_host.h"

namespace ptr {
using namespace ptd;

namespace {

// A light with its sampling frame, as setup_lights_kernel computes it (:261-264, :284-287, :295-296).
struct Light {
  v3 pos, nraw, inten, right, up;
  float size[2], half[2];
};

Light make_light(const float* L) {   // position, normal, intensity, size: 4 floats each
  Light d;
  d.pos = mk(L[0], L[1], L[2]);
  d.nraw = mk(L[4], L[5], L[6]);
  d.inten = mk(L[8], L[9], L[10]);
  const v3 nn = normalize(d.nraw);
  const v3 basis = fabs_(nn.y) < 0.999f ? mk(0.0f, 1.0f, 0.0f) : mk(1.0f, 0.0f, 0.0f);
  d.right = normalize(cross(nn, basis));
  d.up = cross(d.right, nn);
  d.size[0] = L[12];
  d.size[1] = L[13];
  d.half[0] = L[12] * 0.5f;
  d.half[1] = L[13] * 0.5f;
  return d;
}

// sampleAreaLight (:255-268)
v3 sample_area_light(const Light& L, uint32_t* rng) {
  const float u = rng_next(rng) * 2.0f - 1.0f;
  const float v = rng_next(rng) * 2.0f - 1.0f;
  return add(add(L.pos, muls(muls(muls(L.right, u), L.size[0]), 0.5f)), muls(muls(muls(L.up, v), L.size[1]), 0.5f));
}

// intersectAreaLight (:271-298)
bool intersect_area_light(v3 o, v3 d, const Light& L, float* t) {
  const float denom = dot(L.nraw, d);
  if (fabs_(denom) < 0.0001f) return false;
  const float tt = dot(L.nraw, sub(L.pos, o)) / denom;
  *t = tt;
  if (tt <= 0.0f) return false;
  const v3 hp = add(o, muls(d, tt));
  const v3 th = sub(hp, L.pos);
  const float u = dot(th, L.right);
  const float v = dot(th, L.up);
  return fabs_(u) <= L.half[0] && fabs_(v) <= L.half[1];
}

// One light's sample seen from p with the normal n (:350-357, :386-392): kernels/shading.h sample_light.
struct LightSample {
  v3 dir;
  float diff, dist;
};
LightSample sample_light(const Light& L, v3 p, v3 n, uint32_t* rng) {
  const v3 lp = sample_area_light(L, rng);
  LightSample s;
  const v3 d = sub(lp, p);
  const float len = sqrt_(dot(d, d));
  s.dir = muls(d, rcp_(len));
  s.diff = fmax_(dot(n, s.dir), 0.0f);
  s.dist = len;
  return s;
}

// sampleSphere (:246-253)
v3 sample_sphere(uint32_t* rng) {
  const float z = 2.0f * rng_next(rng) - 1.0f;
  const float th = (2.0f * 0x1.921fb6p+1f) * rng_next(rng);
  const float r = sqrt_(1.0f - z * z);
  float sn, cs;
  sincos_(th, &sn, &cs);
  return mk(r * cs, r * sn, z);
}

struct Tracer {
  const Scene& scene;
  const std::vector<Light>& lights;
  int max_depth, sss_bounces;
  std::vector<int32_t> stack;

  struct Hit {
    float t;
    int32_t tri;
  };
  Hit closest(v3 o, v3 d) {
    Hit h;
    (void)walk(scene, o, d, nullptr, stack, &h.t, &h.tri);
    return h;
  }
  bool shadowed(v3 o, v3 d, float limit) {
    float t;
    int32_t tri;
    return walk(scene, o, d, &limit, stack, &t, &tri);
  }
  v3 normal(int32_t tri) const {
    const float4 C = scene.tris[3 * (size_t)tri + 2];
    return mk(C.y, C.z, C.w);
  }

  // pathTrace (:300-418).  Every shadow ray is walked and every draw made where the shader makes it; the
  // kernels' shortcuts (a shadow ray whose term is +-0, the last bounce's unused direction, the exit skip)
  // leave the same bits.
  v3 path_trace(v3 ro, v3 rd, uint32_t seed) {
    const float OFFSET = 0.001f;
    v3 thr = mk(1.0f, 1.0f, 1.0f);
    v3 rad = mk(0.0f, 0.0f, 0.0f);
    uint32_t rng = seed;   // :307 re-seed
    Hit h0 = {1e30f, -1};
    bool have_h0 = false;
    for (const Light& L : lights) {   // :311-328
      float tl;
      if (intersect_area_light(ro, rd, L, &tl)) {
        if (!have_h0) {
          h0 = closest(ro, rd);
          have_h0 = true;
        }
        if (h0.tri < 0 || h0.t > tl) return L.inten;
      }
    }
    const v3 albedo = mk(0.8f, 0.8f, 0.8f);
    const v3 sss_albedo = mk(1.0f, 0.2f, 0.1f);
    const float sss_radius = 1.0f;
    for (int depth = 0; depth < max_depth; ++depth) {   // :331
      Hit h;
      if (depth == 0 && have_h0)
        h = h0;
      else
        h = closest(ro, rd);
      if (h.tri < 0) {
        rad = add(rad, mul(thr, mk(0.0f, 0.0f, 0.0f)));   // background (:336)
        break;
      }
      const v3 hp = add(ro, muls(rd, h.t));   // :188
      const v3 hn = normal(h.tri);            // :189
      v3 direct = mk(0.0f, 0.0f, 0.0f);
      for (const Light& L : lights) {   // :345-366
        const LightSample s = sample_light(L, hp, hn, &rng);
        if (!shadowed(add(hp, muls(hn, OFFSET)), s.dir, s.dist - OFFSET))
          direct = add(direct, mul(albedo, muls(muls(L.inten, s.diff), rcp_(fmax_(s.dist * s.dist, 0.01f)))));
      }
      rad = add(rad, mul(thr, direct));

      v3 sss_thr = mk(1.0f, 1.0f, 1.0f);   // :371-408
      v3 so = sub(hp, muls(hn, OFFSET));
      v3 sd = sample_sphere(&rng);
      for (int k = 0; k < sss_bounces; ++k) {
        const Hit sh = closest(so, sd);
        if (sh.tri < 0) break;
        const float travel = sh.t;
        const v3 cp = add(so, muls(sd, travel));
        const v3 sn = normal(sh.tri);
        v3 sl = mk(0.0f, 0.0f, 0.0f);
        for (const Light& L : lights) {
          const LightSample s = sample_light(L, cp, sn, &rng);
          if (!shadowed(add(cp, muls(sn, OFFSET)), s.dir, s.dist - OFFSET))
            sl = add(sl, muls(mul(muls(sss_albedo, s.diff), L.inten), rcp_(fmax_(s.dist * s.dist, 0.01f))));
        }
        rad = add(rad, muls(mul(mul(thr, sss_thr), sl), 1.0f + sss_radius * 0.5f));
        sss_thr = mul(sss_thr, muls(sss_albedo, exp_(-travel / (sss_radius * 1.5f))));
        so = sub(cp, muls(sn, OFFSET));
        sd = sample_sphere(&rng);
      }

      ro = add(hp, muls(hn, OFFSET));   // :411-414
      const float r1 = rng_next(&rng);
      const float r2 = rng_next(&rng);
      const v3 bd = hemisphere_dir(hn, r1, r2);
      thr = mul(thr, muls(albedo, dot(hn, bd)));
      rd = bd;
    }
    return rad;
  }
};

void run(const Scene& scene, const std::vector<Light>& lights, int max_depth, int sss_bounces, uint32_t n_samples,
         uint32_t seed_stride, const float* rays, size_t i0, size_t i1, float* out) {
  Tracer tr{scene, lights, max_depth, sss_bounces, {}};
  tr.stack.reserve(64);
  for (size_t i = i0; i < i1; ++i) {
    const float* r = rays + 8 * i;
    const v3 o = mk(r[0], r[1], r[2]), d = mk(r[3], r[4], r[5]);
    uint32_t seed0;
    memcpy(&seed0, &r[7], 4);
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (uint32_t s = 0; s < n_samples; ++s) {   // the running mean (:467-469)
      const v3 c = tr.path_trace(o, d, seed0 + s * seed_stride);
      const float fb = (float)s, fb1 = (float)(s + 1u);
      acc[0] = (acc[0] * fb + c.x) / fb1;
      acc[1] = (acc[1] * fb + c.y) / fb1;
      acc[2] = (acc[2] * fb + c.z) / fb1;
      acc[3] = (acc[3] * fb + 1.0f) / fb1;
    }
    memcpy(out + 4 * i, acc, sizeof acc);
  }
}

}  // namespace

std::string trace_radiance_host(const float* V, size_t nvf, const uint32_t* I, size_t ni, const float* nodes, size_t nn,
                                bool int_bits, const float* lights, size_t n_lights, int max_depth, int sss_bounces,
                                uint32_t n_samples, uint32_t seed_stride, const float* rays, size_t n, float* out,
                                int threads) {
  Scene s;
  const std::string bad = make_scene(V, nvf, I, ni, nodes, nn, int_bits, &s);
  if (!bad.empty()) return bad;
  std::vector<Light> ls;
  for (size_t i = 0; i < n_lights; ++i) ls.push_back(make_light(lights + 16 * i));
  size_t nth = threads > 0 ? (size_t)threads : std::max(1u, std::thread::hardware_concurrency());
  nth = std::min<size_t>(std::min<size_t>(nth, 256), std::max<size_t>(1, n / 8));
  if (nth <= 1) {
    run(s, ls, max_depth, sss_bounces, n_samples, seed_stride, rays, 0, n, out);
    return "";
  }
  std::vector<std::thread> pool;
  const size_t per = (n + nth - 1) / nth;
  for (size_t k = 0; k < nth; ++k) {
    const size_t i0 = std::min(n, k * per), i1 = std::min(n, i0 + per);
    if (i0 < i1)
      pool.emplace_back([&s, &ls, max_depth, sss_bounces, n_samples, seed_stride, rays, i0, i1, out] {
        run(s, ls, max_depth, sss_bounces, n_samples, seed_stride, rays, i0, i1, out);
      });
  }
  for (auto& th : pool) th.join();
  return "";
}

void camera_rays_host(const float cam[16], int W, int H, uint32_t batch, const int32_t* pixels, size_t n, float* rays) {
  const ptdn::CamBasis b = ptdn::cam_basis(cam);
  for (size_t i = 0; i < n; ++i) {
    const long long pix = pixels ? (long long)pixels[i] : (long long)i;
    const int px = (int)(pix % W), py = (int)(pix / W);
    const CamFrame F = cam_frame(b.pos, b.dir, b.right, b.up, b.tan_fov, W, H, px, py);
    const uint32_t seed = camera_seed(batch, W, H, px, py);
    v3 o, d;
    camera_ray(F, seed, &o, &d);
    float r[8] = {o.x, o.y, o.z, d.x, d.y, d.z, 1e30f, 0.0f};
    memcpy(&r[7], &seed, 4);
    memcpy(rays + 8 * i, r, sizeof r);
  }
}

}  // namespace ptr
