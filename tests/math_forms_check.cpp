// Test infrastructure: the plain-C++ forms of csrc/pt_math.h that the device
// kernels rely on, checked on the host bit for bit.  A stand-alone program:
//   sincos_(x) against sin_(x) and cos_(x): every float in [0, 2*pi] (the
//     shader's domain), the specials, and a million random bit patterns
//     outside that range;
//   div1p5_fast_(x) against x / 1.5f for all 2^32 inputs: no input inside
//     div1p5_in_range may differ; the count of differing inputs in range or
//     not (-0, +inf and -inf: 3) and the finite one of the largest magnitude
//     (none: 0) are reported, which pins the range;
//   sqrt_in_range / rcp_in_range / div1p5_in_range at their boundary bit
//     patterns, printed as strings of 0 and 1 in the order listed below.
// One key=value line; exit status 0 iff nothing differs.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <thread>
#include <vector>

#include "pt_math.h"

namespace {

float float_of(uint32_t u) {
  float f;
  memcpy(&f, &u, 4);
  return f;
}
uint32_t bits_of(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
}
bool same(float a, float b) { return bits_of(a) == bits_of(b) || (a != a && b != b); }

struct Part {
  uint64_t n = 0, bad = 0;
  uint32_t first_bad = 0xffffffffu;
  uint64_t fails = 0;          // div: inputs at which the fast form differs, in range or not
  uint32_t max_fail_abs = 0;   // ... and the largest |x| bits among the finite ones
};

void note(Part* p, uint32_t b) {
  ++p->bad;
  if (b < p->first_bad) p->first_bad = b;
}

void sincos_one(uint32_t b, Part* p) {
  const float x = float_of(b);
  float s, c;
  ptm::sincos_(x, &s, &c);
  ++p->n;
  if (!same(s, ptm::sin_(x)) || !same(c, ptm::cos_(x))) note(p, b);
}

void sincos_scan(uint32_t lo, uint32_t hi, Part* out) {
  Part p;
  for (uint64_t b = lo; b <= hi; ++b) sincos_one((uint32_t)b, &p);
  *out = p;
}

void div_scan(uint32_t lo, uint32_t hi, Part* out) {
  Part p;
  for (uint64_t b = lo; b <= hi; ++b) {
    const float x = float_of((uint32_t)b);
    const bool eq = same(ptm::div1p5_fast_(x), x / 1.5f);
    ++p.n;
    if (!eq) {
      ++p.fails;
      if (ptm::div1p5_in_range(x)) note(&p, (uint32_t)b);
      const uint32_t ab = (uint32_t)b & 0x7fffffffu;
      if (ab < 0x7f800000u && ab > p.max_fail_abs) p.max_fail_abs = ab;
    }
  }
  *out = p;
}

Part threads(void (*scan)(uint32_t, uint32_t, Part*), uint32_t lo, uint32_t hi, int nthreads) {
  std::vector<Part> parts((size_t)nthreads);
  std::vector<std::thread> th;
  const uint64_t n = (uint64_t)hi - lo + 1, per = (n + nthreads - 1) / nthreads;
  for (int t = 0; t < nthreads; ++t) {
    const uint64_t a = lo + per * t, b = a + per - 1 < hi ? a + per - 1 : hi;
    if (a > hi) break;
    th.emplace_back(scan, (uint32_t)a, (uint32_t)b, &parts[(size_t)t]);
  }
  for (auto& t : th) t.join();
  Part all;
  for (const Part& p : parts) {
    all.n += p.n;
    all.bad += p.bad;
    all.fails += p.fails;
    if (p.first_bad < all.first_bad) all.first_bad = p.first_bad;
    if (p.max_fail_abs > all.max_fail_abs) all.max_fail_abs = p.max_fail_abs;
  }
  return all;
}

template <class F>
std::string flags(F in_range, const std::vector<uint32_t>& bits) {
  std::string s;
  for (uint32_t b : bits) s += in_range(float_of(b)) ? '1' : '0';
  return s;
}

}  // namespace

int main() {
  const int nthreads = 16;
  const uint32_t two_pi = bits_of(2.0f * 0x1.921fb6p+1f);   // the largest angle the shader forms: (2 * pi) * u, u <= 1

  Part sc = threads(sincos_scan, 0u, two_pi, nthreads);
  Part sp;
  const uint32_t specials[] = {0x80000000u, 0x00000001u, 0x80000001u, 0x007fffffu, 0x00800000u, 0x7f7fffffu, 0xff7fffffu,
                               0x7f800000u, 0xff800000u, 0x7fc00000u, 0xffc00000u, 0x7f800001u, two_pi + 1u,
                               bits_of(6400.0f), bits_of(-6400.0f), bits_of(1e9f), bits_of(-1.0f), bits_of(-6.2831855f)};
  for (uint32_t b : specials) sincos_one(b, &sp);
  Part rn;
  uint64_t lcg = 0x9e3779b97f4a7c15ull;
  while (rn.n < 1000000u) {
    lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
    const uint32_t b = (uint32_t)(lcg >> 32);
    if (b > two_pi) sincos_one(b, &rn);   // outside [0, 2*pi]: negatives, larger angles, inf, NaN
  }

  Part dv = threads(div_scan, 0u, 0xffffffffu, nthreads);

  // boundary bit patterns, in this order (tests/test_math_forms.py states what each must give)
  const std::vector<uint32_t> sq = {0x0f800000u, 0x0f7fffffu, 0x7f7fffffu, 0x7f800000u, 0x7fc00000u, 0x00000000u,
                                    0x80000000u, 0x8f800000u, 0xbf800000u, 0x00000001u, 0x3f800000u};
  const std::vector<uint32_t> rc = {0x00800000u, 0x007fffffu, 0x7e800000u, 0x7e800001u, 0x80800000u, 0x807fffffu,
                                    0xfe800000u, 0xfe800001u, 0x00000000u, 0x80000000u, 0x7f800000u, 0xff800000u,
                                    0x7fc00000u, 0x3f800000u};
  const uint32_t dlo = bits_of(ptm::kDiv1p5Lo);
  const std::vector<uint32_t> dq = {dlo, dlo - 1u, 0x7f7fffffu, 0x7f800000u, dlo | 0x80000000u, (dlo - 1u) | 0x80000000u,
                                    0xff7fffffu, 0xff800000u, 0x00000000u, 0x80000000u, 0x7fc00000u, 0x3f800000u};

  printf("sincos_n=%llu sincos_bad=%llu sincos_first=%#x special_n=%llu special_bad=%llu random_n=%llu random_bad=%llu "
         "div_n=%llu div_bad=%llu div_first=%#x div_fails=%llu div_max_fail_abs=%#x div_lo=%#x sqrt_bounds=%s rcp_bounds=%s div_bounds=%s\n",
         (unsigned long long)sc.n, (unsigned long long)sc.bad, sc.first_bad, (unsigned long long)sp.n,
         (unsigned long long)sp.bad, (unsigned long long)rn.n, (unsigned long long)rn.bad, (unsigned long long)dv.n,
         (unsigned long long)dv.bad, dv.first_bad, (unsigned long long)dv.fails, dv.max_fail_abs, dlo, flags(ptm::sqrt_in_range, sq).c_str(),
         flags(ptm::rcp_in_range, rc).c_str(), flags(ptm::div1p5_in_range, dq).c_str());
  return sc.bad || sp.bad || rn.bad || dv.bad ? 1 : 0;
}
