// Test infrastructure: the radius guarantee of the tight cull rectangles
// (csrc/pt_cull.h).  A stand-alone program: it evaluates cull_radius -- the
// kernel's own sqrt_(-2.0f * log_(fmax_(1e-38f, u))), pt_math.h's host
// functions -- for every float u in [kCullTightU0, 1], about 1.1e8 of them, on
// a few threads, and prints the largest radius found, the radius of the float
// just below kCullTightU0, and whether the constant holds:
//   every radius in the range is at most kCullTightR, and
//   the float below kCullTightU0 gives a radius above it (u0 is the least).
// With an argument R it searches instead: the least float u0 such that every
// float in [u0, 1] has its radius at most R (how the constant was found).
// Exit status 0 iff the constant holds (or the search ended).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <thread>
#include <vector>

#include "pt_cull.h"

namespace {

uint32_t bits_of(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
}
float float_of(uint32_t u) {
  float f;
  memcpy(&f, &u, 4);
  return f;
}

struct Part {
  float max_r = -1.0f;        // the largest radius of the part
  uint32_t max_at = 0;        // ... and a float that gives it
  uint32_t highest_bad = 0;   // the highest bit pattern whose radius is above the bound or NaN (0: none)
};

// Positive floats order as their bit patterns: [lo, hi] inclusive.
void scan(uint32_t lo, uint32_t hi, float bound, Part* out) {
  Part p;
  for (uint64_t b = lo; b <= hi; ++b) {
    const float r = ptd::cull_radius(float_of((uint32_t)b));
    if (!(r <= bound)) p.highest_bad = (uint32_t)b;
    if (r > p.max_r) {
      p.max_r = r;
      p.max_at = (uint32_t)b;
    }
  }
  *out = p;
}

Part scan_threads(uint32_t lo, uint32_t hi, float bound, int nthreads) {
  std::vector<Part> parts((size_t)nthreads);
  std::vector<std::thread> th;
  const uint64_t n = (uint64_t)hi - lo + 1, per = (n + nthreads - 1) / nthreads;
  for (int t = 0; t < nthreads; ++t) {
    const uint64_t a = lo + per * t, b = a + per - 1 < hi ? a + per - 1 : hi;
    if (a > hi) break;
    th.emplace_back(scan, (uint32_t)a, (uint32_t)b, bound, &parts[(size_t)t]);
  }
  for (auto& t : th) t.join();
  Part all;
  for (const Part& p : parts) {
    if (p.max_r > all.max_r) {
      all.max_r = p.max_r;
      all.max_at = p.max_at;
    }
    if (p.highest_bad > all.highest_bad) all.highest_bad = p.highest_bad;
  }
  return all;
}

}  // namespace

int main(int argc, char** argv) {
  const uint32_t one = bits_of(1.0f);
  const int nthreads = 8;
  if (argc > 1) {
    // search: scan [2^-24, 1] (radius 5.77 at its low end, above any bound of interest below that)
    const float bound = (float)atof(argv[1]);
    const uint32_t lo = bits_of(0x1p-24f);
    const Part p = scan_threads(lo, one, bound, nthreads);
    if (p.highest_bad == 0) {
      printf("no float in [2^-24, 1] has a radius above %.9g\n", (double)bound);
      return 1;
    }
    const uint32_t u0 = p.highest_bad + 1;
    printf("R=%.9g u0=%a bits=%#x radius(u0)=%.9g radius(below)=%.9g\n", (double)bound, (double)float_of(u0), u0,
           (double)ptd::cull_radius(float_of(u0)), (double)ptd::cull_radius(float_of(u0 - 1)));
    return 0;
  }
  const float bound = (float)ptd::kCullTightR;
  const uint32_t u0 = bits_of(ptd::kCullTightU0);
  if (!(ptd::kCullTightU0 > 0.0f && ptd::kCullTightU0 < 1.0f) || (double)bound != ptd::kCullTightR) {
    printf("bad constants\n");
    return 1;
  }
  const Part p = scan_threads(u0, one, bound, nthreads);
  const float below = ptd::cull_radius(float_of(u0 - 1));
  const bool holds = p.highest_bad == 0 && p.max_r <= bound, least = below > bound;
  printf("floats=%llu bound=%.9g u0=%a bits=%#x max_radius=%.9g at=%a above_bound=%d radius_below_u0=%.9g holds=%d "
         "least=%d\n",
         (unsigned long long)((uint64_t)one - u0 + 1), (double)bound, (double)ptd::kCullTightU0, u0, (double)p.max_r,
         (double)float_of(p.max_at), p.highest_bad != 0, (double)below, (int)holds, (int)least);
  return holds && least ? 0 : 1;
}
