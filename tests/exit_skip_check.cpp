// exit_skip_check.cpp -- the exit skip's predicate (csrc/pt_isect.h exit_skip,
// DESIGN.md section 4) on the CPU, with the headers the kernels compile.  A
// stand-alone program (tests/test_exit_skip.py builds and runs it; it is also
// the program for host sanitizer runs):
//   (a) the cosine sincos_ returns for acos_(sqrt_(1 - r1)) over every float
//       r1 in [0, 1): none may be <= 0; and its value at r1 == 1.0f;
//   (b) generated hits on the faces of root boxes for which the predicate
//       holds: slab() on the root box with the full hemisphere direction
//       (hemisphere_dir) from ro must be false for each;
//   (c) generated hits for which it must not hold, by kind, with how often it
//       was asked and how often it held (0).
// One line per part; exit status 1 when anything is wrong.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <thread>
#include <vector>

#include "pt_isect.h"

using namespace ptd;

namespace {

int n_threads() {
  const unsigned hw = std::thread::hardware_concurrency();
  return (int)std::min(16u, hw ? hw : 1u);
}

float cos_theta(float r1) {
  float st, ct;
  sincos_(acos_(sqrt_(1.0f - r1)), &st, &ct);
  return ct;
}

struct Lcg {
  uint64_t s;
  uint32_t next() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(s >> 32);
  }
  float unit() { return (float)(next() >> 8) * 0x1.0p-24f; }   // [0, 1)
  float in(float a, float b) { return a + (b - a) * unit(); }
};

float step_ulps(float x, int k) {   // x moved by k ulp (k in -3..3; x != 0 keeps its sign here)
  if (x == 0.0f) return (k < 0 ? -1.0f : 1.0f) * u2f((uint32_t)abs(k));   // +-k denormal steps off zero
  uint32_t u = f2u(x);
  u = (x > 0.0f) ? u + (uint32_t)k : u - (uint32_t)k;
  return u2f(u);
}

struct Box { v3 lo, hi; };
// box.obj's cube, the hull test's cuboid, flat_quad's root (lo.z == hi.z), floor_and_cloud's root
// (about), a root far from the origin
const Box kBoxes[] = {
    {{-1.0f, -1.0f, -1.0f}, {1.0f, 1.0f, 1.0f}},
    {{0.375f, -1.25f, 2.0f}, {1.125f, -0.75f, 3.5f}},
    {{-1.0f, -1.0f, 0.0f}, {1.0f, 1.0f, 0.0f}},
    {{-20.0f, -0.6f, -20.0f}, {20.0f, 0.5099f, 20.0f}},
    {{299.0f, 299.0f, 299.0f}, {301.0f, 301.0f, 301.0f}},
};
constexpr int kNBoxes = (int)(sizeof kBoxes / sizeof kBoxes[0]);

float comp(v3 v, int a) { return a == 0 ? v.x : a == 1 ? v.y : v.z; }
void set(v3* v, int a, float x) { (a == 0 ? v->x : a == 1 ? v->y : v->z) = x; }

// A hit on face (axis a, side s = +-1) of box B: the normal's magnitude mag on a with sign nsign, tangent
// components +-0, the hit's a coordinate k ulp off the plane, the others anywhere in the face (corners
// and edges at times).
void make_hit(Lcg& g, const Box& B, int a, int s, float mag, int nsign, int k, v3* hp, v3* hn) {
  for (int c = 0; c < 3; ++c) {
    const float lo = comp(B.lo, c), hi = comp(B.hi, c);
    const uint32_t pick = g.next() & 15u;
    set(hp, c, pick == 0 ? lo : pick == 1 ? hi : g.in(lo, hi));
    set(hn, c, (g.next() & 1u) ? 0.0f : -0.0f);
  }
  set(hp, a, step_ulps(s > 0 ? comp(B.hi, a) : comp(B.lo, a), k));
  set(hn, a, nsign > 0 ? mag : -mag);
}

float draw_r2(Lcg& g) {
  switch (g.next() & 15u) {
    case 0: return 0.0f;
    case 1: return 0.25f;
    case 2: return 0.5f;
    case 3: return 0.75f;
    case 4: return 1.0f;
    default: return g.unit();
  }
}
float draw_r1(Lcg& g, bool with_one) {
  switch (g.next() & 15u) {
    case 0: return 0.0f;
    case 1: return 0x1.fffffep-1f;   // the last float below 1
    case 2: return with_one ? 1.0f : 0.5f;
    case 3: return u2f(g.next() % 0x3f800000u);   // any float of [0, 1) by bits: tiny ones too
    default: return g.unit();
  }
}

// slab() on the root box for the bounce ray the kernels would trace
bool root_hit(const Box& B, v3 ro, v3 hn, float r1, float r2) {
  const v3 bd = hemisphere_dir(hn, r1, r2);
  const v3 inv = mk(rcp_(bd.x), rcp_(bd.y), rcp_(bd.z));
  return slab(ro, inv, make_float4(B.lo.x, B.lo.y, B.lo.z, 0.0f), make_float4(B.hi.x, B.hi.y, B.hi.z, 0.0f));
}

struct Tally {
  unsigned long long cases = 0, fired = 0, wrong = 0;
  unsigned long long asked[5] = {}, held[5] = {};   // (c): inward, tangent ulp, 0.998, r1 one, on plane
};

void run_cases(uint64_t seed, unsigned long long n, Tally* out) {
  Lcg g{seed};
  const float OFFSET = 0.001f;
  Tally t;
  for (unsigned long long i = 0; i < n; ++i) {
    const Box& B = kBoxes[g.next() % kNBoxes];
    const int a = (int)(g.next() % 3u), s = (g.next() & 1u) ? 1 : -1;
    const float mag = (g.next() & 1u) ? 1.0f : 0.9995f;
    const int k = (int)(g.next() % 7u) - 3;
    v3 hp, hn;
    const uint32_t kind = g.next() % 16u;
    if (kind >= 5) {
      // (b) an outward normal on its own face, r1 == 1.0f mixed in: wherever the predicate holds the
      // ray must miss the root
      make_hit(g, B, a, s, mag, s, k, &hp, &hn);
      const v3 ro = add(hp, muls(hn, OFFSET));
      const float r1 = draw_r1(g, true), r2 = draw_r2(g);
      t.cases++;
      if (exit_skip(hn, ro, r1, B.lo, B.hi)) {
        t.fired++;
        if (root_hit(B, ro, hn, r1, r2)) t.wrong++;
      }
      continue;
    }
    // (c) the predicate must be false
    bool held = false;
    if (kind == 0) {   // a root face whose normal points inward (a floor at the root's lo, normal up)
      if (comp(B.lo, a) == comp(B.hi, a)) continue;   // a flat root has no inside
      make_hit(g, B, a, s, mag, -s, k, &hp, &hn);
      held = exit_skip(hn, add(hp, muls(hn, OFFSET)), draw_r1(g, false), B.lo, B.hi);
    } else if (kind == 1) {   // a tangent component of one ulp
      make_hit(g, B, a, s, mag, s, k, &hp, &hn);
      set(&hn, (a + 1 + (int)(g.next() & 1u)) % 3, (g.next() & 1u) ? u2f(1u) : u2f(0x80000001u));
      held = exit_skip(hn, add(hp, muls(hn, OFFSET)), draw_r1(g, false), B.lo, B.hi);
    } else if (kind == 2) {   // |hn.a| below the bound
      make_hit(g, B, a, s, 0.998f, s, k, &hp, &hn);
      held = exit_skip(hn, add(hp, muls(hn, OFFSET)), draw_r1(g, false), B.lo, B.hi);
    } else if (kind == 3) {   // r1 == 1.0f: the cosine is negative
      make_hit(g, B, a, s, mag, s, k, &hp, &hn);
      held = exit_skip(hn, add(hp, muls(hn, OFFSET)), 1.0f, B.lo, B.hi);
    } else {   // ro.a exactly on the plane
      make_hit(g, B, a, s, mag, s, k, &hp, &hn);
      v3 ro = add(hp, muls(hn, OFFSET));
      set(&ro, a, s > 0 ? comp(B.hi, a) : comp(B.lo, a));
      held = exit_skip(hn, ro, draw_r1(g, false), B.lo, B.hi);
    }
    t.asked[kind]++;
    t.held[kind] += held ? 1 : 0;
  }
  *out = t;
}

}  // namespace

int main(int argc, char** argv) {
  const unsigned long long n_cases = argc > 1 ? strtoull(argv[1], nullptr, 10) : 20000000ull;
  const int nt = n_threads();
  int bad = 0;

  // (a)
  {
    const uint32_t end = 0x3f800000u;   // bits of 1.0f: every float of [0, 1) lies below
    std::vector<unsigned long long> nonpos((size_t)nt, 0);
    std::vector<float> least((size_t)nt, 2.0f);
    std::vector<std::thread> th;
    for (int i = 0; i < nt; ++i)
      th.emplace_back([&, i] {
        const uint32_t b0 = (uint32_t)((uint64_t)end * (uint64_t)i / (uint64_t)nt);
        const uint32_t b1 = (uint32_t)((uint64_t)end * (uint64_t)(i + 1) / (uint64_t)nt);
        unsigned long long np = 0;
        float mn = 2.0f;
        for (uint32_t b = b0; b < b1; ++b) {
          const float ct = cos_theta(u2f(b));
          np += !(ct > 0.0f);
          mn = ct < mn ? ct : mn;
        }
        nonpos[(size_t)i] = np;
        least[(size_t)i] = mn;
      });
    for (auto& t : th) t.join();
    unsigned long long np = 0;
    float mn = 2.0f;
    for (int i = 0; i < nt; ++i) {
      np += nonpos[(size_t)i];
      mn = std::min(mn, least[(size_t)i]);
    }
    const float at_one = cos_theta(1.0f);
    printf("ct_sweep inputs=%u nonpositive=%llu min_ct=%.9g ct_at_one=%.9g\n", end, np, (double)mn, (double)at_one);
    if (np != 0 || !(mn > 0.0f)) bad = 1;
  }

  // (b), (c)
  {
    std::vector<Tally> part((size_t)nt);
    std::vector<std::thread> th;
    for (int i = 0; i < nt; ++i)
      th.emplace_back(run_cases, 0x9e3779b97f4a7c15ull * (uint64_t)(i + 1), n_cases / (unsigned long long)nt + 1, &part[(size_t)i]);
    for (auto& t : th) t.join();
    Tally s;
    for (const Tally& p : part) {
      s.cases += p.cases;
      s.fired += p.fired;
      s.wrong += p.wrong;
      for (int k = 0; k < 5; ++k) {
        s.asked[k] += p.asked[k];
        s.held[k] += p.held[k];
      }
    }
    printf("fire cases=%llu fired=%llu wrong=%llu\n", s.cases, s.fired, s.wrong);
    printf("nofire inward=%llu/%llu tangent_ulp=%llu/%llu n0998=%llu/%llu r1_one=%llu/%llu on_plane=%llu/%llu\n",
           s.held[0], s.asked[0], s.held[1], s.asked[1], s.held[2], s.asked[2], s.held[3], s.asked[3], s.held[4],
           s.asked[4]);
    if (s.wrong != 0 || s.fired == 0) bad = 1;
    for (int k = 0; k < 5; ++k)
      if (s.held[k] != 0 || s.asked[k] == 0) bad = 1;
  }
  return bad;
}
