// display_check — the 8-bit sRGB encode of csrc/pt_display.h on the host:
// srgb8_code (the table of 255 thresholds, searched in eight steps) against
// srgb8_pow (the double-precision statement pt_write_image encodes with) for
// all 2^32 bit patterns, on up to 16 threads; only the ~1.07e9 patterns in
// (0, 1) reach pow.  Also: the thresholds are strictly increasing, each is the
// least float of its code, and both branches of srgb8_pow give the same code at
// the seam.  Prints key=value fields; the exit status is 0 when nothing differs.
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <atomic>
#include <thread>
#include <vector>

#include "pt_display.h"

int main() {
  using namespace ptdp;
  // the table itself
  int increasing = 1, least = 1;
  for (int k = 1; k < 256; ++k) {
    if (!(kSrgb8T[k] > kSrgb8T[k - 1])) increasing = 0;
    // T[k] has code >= k and the float below it a smaller one
    if (!(srgb8_pow(ptm::u2f(kSrgb8T[k])) >= k && srgb8_pow(ptm::u2f(kSrgb8T[k] - 1u)) < k)) least = 0;
  }
  const float seam = 0.0031308f;
  const int seam_lin = (int)(unsigned char)(12.92 * seam * 255.0 + 0.5);
  const int seam_pow = (int)(unsigned char)((1.055 * pow((double)seam, 1.0 / 2.4) - 0.055) * 255.0 + 0.5);

  const unsigned hw = std::thread::hardware_concurrency();
  const int nt = (int)std::min(16u, hw ? hw : 1u);
  std::atomic<unsigned long long> bad(0), checked(0);
  std::atomic<uint64_t> first(~0ull);
  // interleaved chunks of 2^20 patterns, so that every thread gets its share of (0, 1)
  const uint64_t kChunk = 1ull << 20, kChunks = (1ull << 32) / kChunk;
  std::vector<std::thread> pool;
  for (int t = 0; t < nt; ++t)
    pool.emplace_back([&, t] {
      unsigned long long b = 0, n = 0;
      uint64_t f = ~0ull;
      for (uint64_t c = (uint64_t)t; c < kChunks; c += (uint64_t)nt)
        for (uint64_t u = c * kChunk; u < (c + 1) * kChunk; ++u) {
          const float x = ptm::u2f((uint32_t)u);
          ++n;
          if (srgb8_code(x) != (uint32_t)srgb8_pow(x)) {
            ++b;
            f = std::min(f, u);
          }
        }
      bad += b;
      checked += n;
      uint64_t cur = first.load();
      while (f < cur && !first.compare_exchange_weak(cur, f)) {
      }
    });
  for (auto& th : pool) th.join();
  printf("threads=%d\n", nt);
  printf("encode_n=%llu\n", checked.load());
  printf("encode_bad=%llu\n", bad.load());
  printf("encode_first=%#010llx\n", (unsigned long long)(bad.load() ? first.load() : 0ull));
  printf("table_increasing=%d\n", increasing);
  printf("table_least=%d\n", least);
  printf("seam_codes=%d,%d\n", seam_lin, seam_pow);
  // the codes at the ends: every NaN, negative and zero 0, +inf 255
  printf("ends=%u,%u,%u,%u,%u\n", srgb8_code(ptm::u2f(0x7fc00000u)), srgb8_code(-1.0f), srgb8_code(-0.0f),
         srgb8_code(ptm::u2f(0x7f800000u)), srgb8_code(1.0f));
  const bool ok = bad.load() == 0 && checked.load() == (1ull << 32) && increasing && least && seam_lin == seam_pow;
  return ok ? 0 : 1;
}
