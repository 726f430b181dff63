// Test infrastructure: a stand-alone host program around the footprint
// derivation (csrc/pt_cull.cpp, PT_OPT_CULL_FOOTPRINT), for sanitizer runs on
// the CPU.  It compiles pt_cull.cpp beside itself and links nothing else of
// the library, so
//
//   hipcc -O1 -g -std=c++17 -D__HIP_PLATFORM_AMD__ -ffp-contract=off -fno-fast-math \
//         -fsanitize=address,undefined -fno-sanitize-recover=all -I discovering-path-tracer_amd/csrc \
//         tests/cull_footprint_check.cpp discovering-path-tracer_amd/csrc/pt_cull.cpp -o cull_footprint_check
//
// instruments every line under test; tests/test_cull_footprint.py builds and
// runs exactly that.  Output arrays are exactly as large as the call says, so
// a write past them is an error the sanitizer reports.  Cases: the cameras of
// the tests at radius bounds 0, 4.25 and 13.25, and degenerate inputs -- a
// zero-size light, NaN and infinity in the camera and in a light, a light
// behind the camera, a root box touching the camera plane, a camera inside the
// box, 7 lights (8 objects: the most) and 8 lights (no guarantee).  Every
// derived footprint is finite and lies in the rectangle of the same object and
// bound; every sure region is finite and lies in its light's footprint.  Exit status 0 and one "ok" line, or 1 and what failed.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../include/pathtracer.h"

int pt_fail_internal(int code, const std::string&) { return code; }

namespace {

int fails = 0, checks = 0;
void expect(bool ok, const char* what, int k = -1) {
  ++checks;
  if (!ok) {
    fprintf(stderr, "FAILED: %s (%d)\n", what, k);
    ++fails;
  }
}

struct Cam { float v[16]; };
Cam camera(float px, float py, float pz, float dx, float dy, float dz, float fov) {
  Cam c{};
  c.v[0] = px; c.v[1] = py; c.v[2] = pz;
  c.v[4] = dx; c.v[5] = dy; c.v[6] = dz;
  c.v[9] = 1.0f;
  c.v[12] = fov;
  return c;
}

pt_area_light light(float x, float y, float z, float nx, float ny, float nz, float s0, float s1) {
  pt_area_light l{};
  l.position[0] = x; l.position[1] = y; l.position[2] = z;
  l.normal[0] = nx; l.normal[1] = ny; l.normal[2] = nz;
  l.intensity[0] = l.intensity[1] = l.intensity[2] = 10.0f;
  l.size[0] = s0; l.size[1] = s1;
  return l;
}

// One derivation at one bound: the footprints against the rectangles.  Returns the count.
int derive(const Cam& cam, int W, int H, const float* lo, const float* hi, const std::vector<pt_area_light>& L,
           double R, int max_n, int tag) {
  std::vector<float> rects((size_t)max_n * 4), foot((size_t)max_n * 16);   // exactly sized
  int nr = 0, nf = 0;
  const pt_area_light* lp = L.empty() ? nullptr : L.data();
  expect(pt_primary_cull_rects_r(cam.v, W, H, lo, hi, lp, (int)L.size(), R, rects.data(), max_n, &nr, nullptr) == PT_OK,
         "rectangles: call", tag);
  expect(pt_primary_cull_footprints(cam.v, W, H, lo, hi, lp, (int)L.size(), R, foot.data(), max_n, &nf) == PT_OK,
         "footprints: call", tag);
  expect(nf == -1 || nf == nr, "footprints: one per rectangle, or none", tag);
  {
    std::vector<float> sure(L.empty() ? 1 : L.size() * 16);   // exactly sized
    int ns = 0;
    expect(pt_primary_cull_sure(cam.v, W, H, lo, hi, lp, (int)L.size(), R, sure.data(), (int)(sure.size() / 16), &ns) == PT_OK,
           "sure regions: call", tag);
    expect((nf < 0) == (ns < 0) || max_n <= (int)L.size(), "sure regions: with the footprints or not at all", tag);
    expect(ns <= (int)L.size(), "sure regions: at most one per light", tag);
    for (int l = 0; ns >= 0 && l < (int)L.size(); ++l) {
      const float* s = &sure[(size_t)l * 16];
      for (int k = 0; k < 16; ++k) expect(isfinite(s[k]), "sure region: finite", tag);
      if (nf > l + 1 && s[0] <= s[1] && s[2] <= s[3]) {
        const float* f = &foot[(size_t)(l + 1) * 16];
        expect(s[0] >= f[0] && s[1] <= f[1] && s[2] >= f[2] && s[3] <= f[3], "sure region inside its light's footprint", tag);
      }
    }
  }
  expect(nr >= 0 || nf == -1, "no rectangles, no footprints", tag);
  for (int r = 0; r < nf; ++r) {
    const float* f = &foot[(size_t)r * 16];
    const float* q = &rects[(size_t)r * 4];
    for (int k = 0; k < 16; ++k) expect(isfinite(f[k]), "finite", tag);
    expect(f[0] >= q[0] && f[1] <= q[1] && f[2] >= q[2] && f[3] <= q[3], "inside its rectangle", tag);
    expect(f[0] <= f[1] && f[2] <= f[3], "not empty", tag);
    for (int k = 0; k < 4; ++k) {
      const float a = f[4 + 3 * k], b = f[5 + 3 * k], c = f[6 + 3 * k];
      const bool unused = a == 0.0f && b == 0.0f && c == 1.0f;
      expect(unused || fabs(sqrt((double)a * a + (double)b * b) - 1.0) < 1e-5, "half-plane: unit normal or unused", tag);
      // the rectangle's centre lies in the hull of the corners' boxes
      expect(a * (0.5f * (f[0] + f[1])) + b * (0.5f * (f[2] + f[3])) <= c, "half-plane keeps the centre", tag);
    }
  }
  return nf;
}

}  // namespace

int main() {
  const float lo[3] = {-1, -1, -1}, hi[3] = {1, 1, 1};
  const std::vector<pt_area_light> ref = {light(0, 2, 0, 0, -1, 0, 2.5f, 2.5f)};
  const std::vector<pt_area_light> two = {ref[0], light(1.5f, 0.5f, 2.0f, 0, -1, 0, 0.5f, 1.0f)};
  const Cam def = camera(0, 0, 5, 0, 0, -1, 60);
  const Cam orbit = camera(3, 2, 4, -0.557086f, -0.371391f, -0.742781f, 60);
  const Cam far_wide = camera(0, 0.5f, 12, 0, -0.041631f, -0.999133f, 100);
  const double bounds[3] = {0.0, 4.25, 13.25};
  int tag = 0;
  for (double R : bounds) {
    expect(derive(def, 96, 54, lo, hi, ref, R, 8, tag++) == 2, "default camera: two footprints");
    expect(derive(def, 1920, 1080, lo, hi, ref, R, 2, tag++) == 2, "benchmark frame, room for exactly two");
    expect(derive(orbit, 80, 60, lo, hi, ref, R, 8, tag++) == 2, "orbit camera");
    expect(derive(far_wide, 64, 64, lo, hi, two, R, 8, tag++) == 3, "two lights");
    expect(derive(def, 17, 13, lo, hi, {}, R, 1, tag++) == 1, "no light, room for one");
  }
  // degenerate inputs
  tag = 100;
  expect(derive(def, 96, 54, lo, hi, {light(0, 2, 0, 0, -1, 0, 0, 0)}, 4.25, 8, tag++) == 2, "zero-size light");
  {   // a light no ray ever hits (the kernel's half is the signed size * 0.5f): footprints, but no sure region
    const std::vector<pt_area_light> pos = {light(0, 2, 0, 0, -1, 0, 2.5f, 2.5f)};
    const std::vector<std::vector<pt_area_light>> negs = {{light(0, 2, 0, 0, -1, 0, -2.5f, 2.5f)},
                                                          {light(0, 2, 0, 0, -1, 0, 2.5f, -2.5f)},
                                                          {light(0, 2, 0, 0, -1, 0, -2.5f, -2.5f)},
                                                          {light(0, 2, 0, 0, -1, 0, 0.0f, 2.5f)},
                                                          {light(0, 2, 0, 0, -1, 0, NAN, 2.5f)}};
    float reg[16];
    int ns = -2;
    expect(pt_primary_cull_sure(def.v, 320, 180, lo, hi, pos.data(), 1, 4.25, reg, 1, &ns) == PT_OK && ns == 1,
           "positive sizes: a sure region");
    for (const auto& L : negs) {
      ns = -2;
      const int rc = pt_primary_cull_sure(def.v, 320, 180, lo, hi, L.data(), 1, 4.25, reg, 1, &ns);
      expect(rc == PT_OK && ns <= 0 && (ns < 0 || reg[0] > reg[1]), "a size that is not positive: no sure region", tag++);
    }
  }
  expect(derive(def, 96, 54, lo, hi, {light(0, 2, 0, 0, 0, 0, 1, 1)}, 4.25, 8, tag++) == -1, "light without a normal");
  expect(derive(def, 96, 54, lo, hi, {light(0, 2, 0, 0, -1, 0, INFINITY, 1)}, 4.25, 8, tag++) == -1, "infinite light");
  expect(derive(def, 96, 54, lo, hi, {light(NAN, 2, 0, 0, -1, 0, 1, 1)}, 4.25, 8, tag++) == -1, "NaN light");
  expect(derive(def, 96, 54, lo, hi, {light(0, 2, 9, 0, -1, 0, 1, 1)}, 4.25, 8, tag++) == -1, "light behind the camera");
  for (int k = 0; k < 16; ++k) {
    Cam c = def;
    c.v[k] = NAN;
    const int n = derive(c, 96, 54, lo, hi, ref, 4.25, 8, tag++);
    expect(n == -1 || !(k < 3 || (k >= 4 && k < 7) || (k >= 8 && k < 11) || k == 12), "NaN in the camera: no guarantee", k);
    c.v[k] = INFINITY;
    derive(c, 96, 54, lo, hi, ref, 4.25, 8, tag++);
  }
  expect(derive(camera(0, 0, 1.0001f, 0, 0, -1, 60), 96, 54, lo, hi, ref, 4.25, 8, tag++) == -1, "box touching the camera plane");
  expect(derive(camera(0, 0, 1.01f, 0, 0, -1, 60), 96, 54, lo, hi, ref, 4.25, 8, tag++) >= -1, "box just in front of the camera");
  expect(derive(camera(0, 0, 0.5f, 0, 0, -1, 60), 96, 54, lo, hi, ref, 4.25, 8, tag++) == -1, "camera inside the box");
  expect(derive(camera(0, 0, 5, 0, 0, 0, 60), 96, 54, lo, hi, ref, 4.25, 8, tag++) == -1, "camera without a direction");
  expect(derive(def, 0, 54, lo, hi, ref, 4.25, 8, tag++) == -1, "empty frame");
  {
    const float nlo[3] = {NAN, -1, -1};
    expect(derive(def, 96, 54, nlo, hi, ref, 4.25, 8, tag++) == -1, "NaN root box");
    const float big[3] = {3e38f, 3e38f, 3e38f}, nbig[3] = {-3e38f, -3e38f, -3e38f};
    expect(derive(def, 96, 54, nbig, big, ref, 4.25, 8, tag++) == -1, "huge root box");
  }
  std::vector<pt_area_light> ring;
  for (int k = 0; k < 8; ++k)
    ring.push_back(light(1.5f * cosf(k * 0.785f), 2, 1.5f * sinf(k * 0.785f), 0, -1, 0, 0.6f, 0.6f));
  expect(derive(def, 96, 54, lo, hi, ring, 4.25, 8, tag++) == -1, "8 lights: no guarantee");
  ring.pop_back();
  expect(derive(def, 96, 54, lo, hi, ring, 4.25, 8, tag++) == 8, "7 lights: 8 footprints");
  // refused arguments
  {
    float out[16];
    int n = 0;
    expect(pt_primary_cull_footprints(def.v, 96, 54, lo, hi, nullptr, 0, 13.5, out, 1, &n) == PT_ERR_INVALID, "bound above 13.25");
    expect(pt_primary_cull_footprints(def.v, 96, 54, lo, hi, nullptr, 0, NAN, out, 1, &n) == PT_ERR_INVALID, "NaN bound");
    expect(pt_primary_cull_footprints(def.v, 96, 54, lo, hi, nullptr, 1, 4.25, out, 1, &n) == PT_ERR_INVALID, "lights missing");
    expect(pt_primary_cull_footprints(def.v, 96, 54, lo, hi, nullptr, 0, 4.25, out, 0, &n) == PT_ERR_INVALID, "no room");
    expect(pt_primary_cull_footprints(nullptr, 96, 54, lo, hi, nullptr, 0, 4.25, out, 1, &n) == PT_ERR_INVALID, "null camera");
  }
  if (fails) {
    fprintf(stderr, "%d of %d checks failed\n", fails, checks);
    return 1;
  }
  printf("ok: %d checks\n", checks);
  return 0;
}
