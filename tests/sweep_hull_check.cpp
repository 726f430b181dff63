// Test infrastructure: the hull faces of the sweep table (scene/small_sweep.h:
// flat boxes that are faces of the root box carry a code, and sweep_cands
// tests them with the root's slab products, csrc/sweep_walk.h sweep_slab_hull)
// beside the two-pass restatement sweep_leaves(sweep_mask(...)), which goes
// through slab for every box, ray by ray; the same table packed without codes
// beside both; each code beside its definition.  Built by
// tests/test_sweep_hull.py with hipcc (host code only); with -DSWEEP_HULL_MAIN
// it is a stand-alone program that checks two built-in scenes (for sanitizer
// runs).
//
// The scene building and the triangle records are tests/sweep_check.cpp's own,
// included as they stand.
#include "sweep_check.cpp"

namespace {

// The first flat axis of a record (lo == hi bitwise), or -1.
int flat_axis(const float* r) {
  for (int a = 0; a < 3; ++a)
    if (memcmp(r + a, r + 4 + a, 4) == 0) return a;
  return -1;
}

// A hull code by its definition: the box is flat on an axis, its flat
// coordinate is bitwise the root's lo (1) or hi (2) there, and its other four
// extents are bitwise the root's.
uint32_t code_by_definition(const float* r, const float* r0) {
  const int a = flat_axis(r);
  if (a < 0) return 0u;
  for (int c = 0; c < 3; ++c)
    if (c != a && (memcmp(r + c, r0 + c, 4) != 0 || memcmp(r + 4 + c, r0 + 4 + c, 4) != 0)) return 0u;
  if (memcmp(r + a, r0 + a, 4) == 0) return 1u;
  if (memcmp(r + a, r0 + 4 + a, 4) == 0) return 2u;
  return 0u;
}

uint32_t code_of(const float* table, int bx) {
  uint32_t c;
  memcpy(&c, table + 8 * (size_t)bx + 7, 4);
  return c;
}

// The two-pass mask without the early exit (a lane riding along).
uint32_t two_pass_riding(v3 o, v3 inv, const SweepTable& tb, bool root) {
  const SweepBoxP B = sweep_boxes(tb);
  uint64_t sb = root ? 1u : 0u;
  for (int b = 1; b < tb.n_boxes; ++b) sb |= sweep_slab(o, inv, B[b]) ? (uint64_t)1 << b : (uint64_t)0;
  return sweep_wide(tb.n_boxes) ? sweep_leaves<uint64_t>(sb, tb) : sweep_leaves<uint32_t>((uint32_t)sb, tb);
}

}  // namespace

extern "C" {

// rays as sweep_check's.  stats (12 words): rays whose [0] leaf mask, [1]
// `none` differ between sweep_cands on the coded table and
// sweep_leaves(sweep_mask); [2] the same for the table packed without codes
// and for sweep_cands<false>, the sweep that ignores codes, on both tables;
// [3] rays whose sweep_fold (either table) differs from the two passes without
// the early exit; [4] (ray, hull box) pairs whose sweep_slab_hull differs from
// slab of the record; [5] first bad ray or ~0; [6] boxes whose code differs
// from its definition, plus coded words in the table packed without codes;
// [7] (ray, hull box) pairs whose product on the flat axis is NaN; [8] rays
// passing the root, [9] failing it; [10] OR of all leaf masks; [11]
// candidates.  info: [0] boxes, [1] leaves, [2] flat boxes, [3] coded boxes
// (by the table), [4] SmallSweep::n_hull.  Returns 0, 2 (no table) or 1 (err).
int sweep_hull_check(const float* V, size_t nvf, const uint32_t* I, size_t nt, const float* N, size_t nn, int int_bits,
                     const float* rays, size_t n, uint64_t* st, int* info, char* err, size_t errlen) {
  Built b;
  const std::string why = build(V, I, nt, N, nn, int_bits, &b);
  if (!why.empty()) {
    snprintf(err, errlen, "%s", why.c_str());
    return 1;
  }
  if (!b.has_table) return 2;
  const pt::SmallSweep& s = b.sweep;
  const std::vector<float> plain_v = s.pack(false);
  float* plain = (float*)aligned_alloc(64, (plain_v.size() * sizeof(float) + 63) / 64 * 64);
  memcpy(plain, plain_v.data(), plain_v.size() * sizeof(float));
  const SweepTable tb = {(const float4*)b.table, s.n_boxes, s.n_leaves};
  const SweepTable tp = {(const float4*)plain, s.n_boxes, s.n_leaves};
  memset(st, 0, 12 * sizeof(uint64_t));
  st[5] = ~0ull;
  info[0] = s.n_boxes;
  info[1] = s.n_leaves;
  info[2] = info[3] = 0;
  info[4] = s.n_hull;
  for (int bx = 1; bx < s.n_boxes; ++bx) {
    const float* r = b.table + 8 * (size_t)bx;
    info[2] += flat_axis(r) >= 0;
    info[3] += code_of(b.table, bx) != 0u;
    st[6] += code_of(b.table, bx) != code_by_definition(r, b.table);
    st[6] += code_of(plain, bx) != 0u;
    // the two tables differ in the code words only
    st[6] += memcmp(r, plain + 8 * (size_t)bx, 28) != 0;
  }
  st[6] += memcmp(b.table, plain, 32) != 0;
  st[6] += memcmp(b.table + 8 * (size_t)s.n_boxes, plain + 8 * (size_t)s.n_boxes,
                  (plain_v.size() - 8 * (size_t)s.n_boxes) * sizeof(float)) != 0;
  for (size_t i = 0; i < n; ++i) {
    const float* r = rays + 8 * i;
    const v3 o = mk(r[0], r[1], r[2]), d = mk(r[3], r[4], r[5]);
    const v3 inv = mk(rcp_(d.x), rcp_(d.y), rcp_(d.z));
    bool none_old, none_new, none_plain;
    const uint32_t lm_old = sweep_wide(tb.n_boxes) ? sweep_leaves(sweep_mask<uint64_t>(o, inv, tb, &none_old), tb)
                                                   : sweep_leaves(sweep_mask<uint32_t>(o, inv, tb, &none_old), tb);
    const uint32_t lm = sweep_cands(o, inv, tb, &none_new);
    const uint32_t lm_plain = sweep_cands(o, inv, tp, &none_plain);
    // ... and the sweep that ignores codes (the kernel of a table without hull faces), on both tables
    bool none_a, none_b;
    const uint32_t lm_a = sweep_cands<false>(o, inv, tb, &none_a), lm_b = sweep_cands<false>(o, inv, tp, &none_b);
    const bool root = sweep_slab(o, inv, sweep_boxes(tb)[0]);
    const uint32_t ride = two_pass_riding(o, inv, tb, root);
    const bool bad_ride = sweep_fold(o, inv, tb, root) != ride || sweep_fold(o, inv, tp, root) != ride ||
                          (!root && (sweep_fold(o, inv, tb, false) != 0u || sweep_fold(o, inv, tp, false) != 0u));
    const SweepRootVals R = sweep_root_vals(o, inv, sweep_boxes(tb)[0]);
    uint64_t bad_hull = 0;
    for (int bx = 1; bx < tb.n_boxes; ++bx) {
      const uint32_t code = code_of(b.table, bx);
      if (code == 0u) continue;
      const SweepBox rb = sweep_boxes(tb)[bx];
      const int a = flat_axis(b.table + 8 * (size_t)bx);
      const bool h = a == 0 ? sweep_slab_hull<0>(R, code) : a == 1 ? sweep_slab_hull<1>(R, code) : sweep_slab_hull<2>(R, code);
      bad_hull += h != sweep_slab(o, inv, rb);
      const float ta = (rb[a] - (a == 0 ? o.x : a == 1 ? o.y : o.z)) * (a == 0 ? inv.x : a == 1 ? inv.y : inv.z);
      st[7] += ta != ta;
    }
    const bool bad_mask = lm != lm_old, bad_none = none_new != none_old;
    const bool bad_plain = lm_plain != lm_old || none_plain != none_old || lm_a != lm_old || none_a != none_old ||
                           lm_b != lm_old || none_b != none_old;
    st[0] += bad_mask;
    st[1] += bad_none;
    st[2] += bad_plain;
    st[3] += bad_ride;
    st[4] += bad_hull;
    if ((bad_mask || bad_none || bad_plain || bad_ride || bad_hull) && st[5] == ~0ull) st[5] = i;
    st[8] += root;
    st[9] += !root;
    st[10] |= lm;
    st[11] += (uint64_t)__builtin_popcount(lm);
  }
  free(plain);
  return 0;
}

}  // extern "C"

#ifdef SWEEP_HULL_MAIN
namespace {

// A cuboid [lo, hi] of 12 triangles under a hand-made tree: a chain of five
// nodes with the cuboid's box over six face nodes with flat boxes, each over
// its two triangles -- with `extra`, beside one tilted triangle under a root of
// their union (then no face box is a face of the root).
int run(const float* lo3, const float* hi3, bool extra, int want_hull) {
  std::vector<float> V;
  for (int i = 0; i < 8; ++i) {
    V.push_back(i & 1 ? hi3[0] : lo3[0]);
    V.push_back(i & 2 ? hi3[1] : lo3[1]);
    V.push_back(i & 4 ? hi3[2] : lo3[2]);
  }
  const float tilted[9] = {hi3[0] + 0.25f, lo3[1] + 0.25f, lo3[2] + 0.625f, hi3[0] + 0.75f, lo3[1] + 0.5f,
                           lo3[2] + 0.25f, hi3[0] + 0.375f, hi3[1] + 0.125f, lo3[2] + 0.75f};
  if (extra) V.insert(V.end(), tilted, tilted + 9);
  const int F[6][4] = {{0, 2, 6, 4}, {1, 5, 7, 3}, {0, 4, 5, 1}, {2, 3, 7, 6}, {0, 1, 3, 2}, {4, 6, 7, 5}};
  std::vector<uint32_t> I;
  for (auto& f : F) {
    const uint32_t t[6] = {(uint32_t)f[0], (uint32_t)f[1], (uint32_t)f[2], (uint32_t)f[0], (uint32_t)f[2], (uint32_t)f[3]};
    I.insert(I.end(), t, t + 6);
  }
  const uint32_t last[3] = {8, 9, 10};
  if (extra) I.insert(I.end(), last, last + 3);
  std::vector<float> N;
  auto node = [&](const float* lo, const float* hi, int l, int r) {
    const float rec[8] = {lo[0], lo[1], lo[2], (float)l, hi[0], hi[1], hi[2], (float)r};
    N.insert(N.end(), rec, rec + 8);
  };
  auto bounds = [&](const uint32_t* vi, int nv, float* lo, float* hi) {
    for (int c = 0; c < 3; ++c) {
      lo[c] = 1e30f;
      hi[c] = -1e30f;
    }
    for (int k = 0; k < nv; ++k)
      for (int c = 0; c < 3; ++c) {
        lo[c] = fmin_(lo[c], V[3 * vi[k] + c]);
        hi[c] = fmax_(hi[c], V[3 * vi[k] + c]);
      }
  };
  // with `extra`: node 0 the root (left: the chain at 1, right: the tilted
  // triangle's leaf, last); the chain, the faces, their leaves follow
  const int base = extra ? 1 : 0;
  if (extra) {
    float tlo[3], thi[3], rlo[3], rhi[3];
    bounds(last, 3, tlo, thi);
    for (int c = 0; c < 3; ++c) {
      rlo[c] = fmin_(lo3[c], tlo[c]);
      rhi[c] = fmax_(hi3[c], thi[c]);
    }
    node(rlo, rhi, 1, 24);
  }
  for (int i = 0; i < 5; ++i) node(lo3, hi3, base + (i < 4 ? 1 + i : 10), base + 5 + i);   // the chain
  for (int f = 0; f < 6; ++f) {                                                              // the faces
    float lo[3], hi[3];
    const uint32_t vi[4] = {(uint32_t)F[f][0], (uint32_t)F[f][1], (uint32_t)F[f][2], (uint32_t)F[f][3]};
    bounds(vi, 4, lo, hi);
    node(lo, hi, base + 11 + 2 * f, base + 12 + 2 * f);
  }
  for (int f = 0; f < 6; ++f)                                                                // their leaves
    for (int h = 0; h < 2; ++h) {
      float lo[3], hi[3];
      memcpy(lo, &N[8 * (size_t)(base + 5 + f)], 12);
      memcpy(hi, &N[8 * (size_t)(base + 5 + f) + 4], 12);
      node(lo, hi, -1, 2 * f + h);
    }
  if (extra) {
    float tlo[3], thi[3];
    bounds(last, 3, tlo, thi);
    node(tlo, thi, -1, 12);
  }
  uint32_t s = 2463534242u;
  auto rnd = [&]() { s = s * 1664525u + 1013904223u; return (float)(s >> 8) * (1.0f / 16777216.0f) * 2.0f - 1.0f; };
  std::vector<float> rays;
  const int n = 6000;
  const float mid[3] = {0.5f * (lo3[0] + hi3[0]), 0.5f * (lo3[1] + hi3[1]), 0.5f * (lo3[2] + hi3[2])};
  const float ext[3] = {hi3[0] - lo3[0], hi3[1] - lo3[1], hi3[2] - lo3[2]};
  for (int i = 0; i < n; ++i) {
    float r[8] = {mid[0] + rnd() * ext[0], mid[1] + rnd() * ext[1], mid[2] + rnd() * ext[2], rnd(), rnd(), rnd(),
                  (rnd() + 1.0f) * 2.0f, 0.0f};
    if (i % 4 == 1) r[3 + i % 3] = 0.0f;                                       // a zero direction component
    if (i % 4 == 2) r[i % 3] = (i & 8) ? hi3[i % 3] : lo3[i % 3];              // origin in a face plane
    if (i % 8 == 3) { r[i % 3] = (i & 16) ? hi3[i % 3] : lo3[i % 3]; r[3 + i % 3] = 0.0f; }  // ray lying in a face plane
    if (i % 8 == 4) for (int c = 0; c < 3; ++c) r[c] = mid[c] + 0.45f * (r[c] - mid[c]);   // origin inside
    rays.insert(rays.end(), r, r + 8);
  }
  uint64_t st[12];
  int info[5] = {0, 0, 0, 0, 0};
  char err[256] = "";
  const int rc = sweep_hull_check(V.data(), V.size(), I.data(), I.size() / 3, N.data(), N.size() / 8, 0, rays.data(),
                                  (size_t)n, st, info, err, sizeof err);
  if (rc != 0) {
    printf("rc=%d %s\n", rc, err);
    return 1;
  }
  printf("boxes=%d leaves=%d flat_boxes=%d hull_boxes=%d mask=%llu none=%llu plain=%llu riding=%llu hull=%llu codes=%llu "
         "hull_nan=%llu root_pass=%llu root_fail=%llu covered=%#llx candidates=%llu\n",
         info[0], info[1], info[2], info[3], (unsigned long long)st[0], (unsigned long long)st[1],
         (unsigned long long)st[2], (unsigned long long)st[3], (unsigned long long)st[4], (unsigned long long)st[6],
         (unsigned long long)st[7], (unsigned long long)st[8], (unsigned long long)st[9], (unsigned long long)st[10],
         (unsigned long long)st[11]);
  const bool ok = info[2] == 6 && info[3] == want_hull && info[4] == want_hull &&
                  st[0] + st[1] + st[2] + st[3] + st[4] + st[6] == 0 && st[10] == (1ull << info[1]) - 1 && st[8] > 0 &&
                  st[9] > 0 && (want_hull == 0 || st[7] > 0);
  return ok ? 0 : 1;
}

}  // namespace

// Stand-alone: a cuboid of three different extents off the origin, alone (its
// six faces are hull faces) and beside a tilted triangle (none is).  Exit
// status 0 iff nothing differs and every leaf was a candidate of some ray.
int main() {
  const float lo[3] = {0.375f, -1.25f, 2.0f}, hi[3] = {1.125f, -0.75f, 3.5f};
  const int a = run(lo, hi, false, 6);
  const int b = run(lo, hi, true, 0);
  return a | b;
}
#endif
