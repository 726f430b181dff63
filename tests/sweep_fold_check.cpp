// Test infrastructure: sweep_cands (csrc/sweep_walk.h, the one-pass sweep the
// LDS render kernel runs, compiled for the host) beside its two-pass
// restatement sweep_leaves(sweep_mask(...)) and beside the threaded walk, ray
// by ray, both from the same packed table; the flat boxes' slab test beside
// slab and the table's order beside the boxes.  Built by tests/test_sweep_fold.py
// with hipcc (host code only); with -DSWEEP_FOLD_MAIN it is a stand-alone
// program that checks a built-in scene (for sanitizer runs).
//
// The scene building, the threaded walk and the triangle records are
// tests/sweep_check.cpp's own, included as they stand.
#include "sweep_check.cpp"

namespace {

// The two-pass mask without the early exit: what a lane that fails the root
// computes on the device when another lane of its wave passes it.
uint32_t two_pass_riding(v3 o, v3 inv, const SweepTable& tb, bool root) {
  const SweepBoxP B = sweep_boxes(tb);
  uint64_t sb = root ? 1u : 0u;
  for (int b = 1; b < tb.n_boxes; ++b) sb |= sweep_slab(o, inv, B[b]) ? (uint64_t)1 << b : (uint64_t)0;
  return sweep_wide(tb.n_boxes) ? sweep_leaves<uint64_t>(sb, tb) : sweep_leaves<uint32_t>((uint32_t)sb, tb);
}

// under[] of the struct and of the packed records against the definition,
// taken from the packed need words: the boxes that differ.
uint64_t under_mismatches(const Built& b) {
  const pt::SmallSweep& s = b.sweep;
  const SweepTable tb = {(const float4*)b.table, s.n_boxes, s.n_leaves};
  const uint32_t* need = (const uint32_t*)(b.table + 8 * (size_t)s.n_boxes);
  const bool wide = sweep_wide(s.n_boxes);
  uint64_t bad = s.under.size() != (size_t)s.n_boxes;
  for (int bx = 0; bx < s.n_boxes && !bad; ++bx) {
    uint32_t want = 0u;
    for (int l = 0; l < s.n_leaves; ++l) {
      const uint64_t nd = wide ? need[2 * l] | (uint64_t)need[2 * l + 1] << 32 : need[l];
      if (nd != s.need[(size_t)l]) return ~0ull;   // pack() changed need[]
      want |= (nd >> bx & 1u) ? 1u << l : 0u;
    }
    uint32_t rec;
    memcpy(&rec, b.table + 8 * (size_t)bx + 3, 4);
    const SweepBox r = sweep_boxes(tb)[bx];
    bad += (s.under[(size_t)bx] != want) || rec != want || f2u(r[3]) != want;
  }
  return bad;
}

// The kind of box bx by the table's counts word: 0 root, 1 general, 2 + a flat in axis a.
int kind_of(const Built& b, int bx) {
  uint32_t cnt;
  memcpy(&cnt, b.table + 7, 4);
  if (bx == 0) return 0;
  int e = 1;
  for (int k = 1; k <= 4; ++k) {
    e += (int)(cnt >> (8 * (k - 1)) & 0xffu);
    if (bx < e) return k;
  }
  return -1;
}

// The table's order against the boxes themselves: the counts add up to
// n_boxes - 1, a box listed as flat in axis a has lo == hi bitwise there and
// on no earlier axis, a general box on none.  The boxes that break it.
uint64_t order_mismatches(const Built& b) {
  uint64_t bad = 0;
  for (int bx = 1; bx < b.sweep.n_boxes; ++bx) {
    const float* r = b.table + 8 * (size_t)bx;
    int first = -1;
    for (int a = 2; a >= 0; --a)
      if (memcmp(r + a, r + 4 + a, 4) == 0) first = a;
    bad += kind_of(b, bx) != (first < 0 ? 1 : 2 + first);
  }
  return bad + (kind_of(b, b.sweep.n_boxes) != -1);
}

void fold_rays(const Built& b, const float* rays, size_t n, uint64_t* st) {
  memset(st, 0, 16 * sizeof(uint64_t));
  st[5] = ~0ull;
  const SweepTable tb = {(const float4*)b.table, b.sweep.n_boxes, b.sweep.n_leaves};
  std::vector<int> want;
  for (size_t i = 0; i < n; ++i) {
    const float* r = rays + 8 * i;
    const v3 o = mk(r[0], r[1], r[2]), d = mk(r[3], r[4], r[5]);
    const float limit = r[6];
    const v3 inv = mk(rcp_(d.x), rcp_(d.y), rcp_(d.z));
    // the old two passes and the fold, as the device calls them
    bool none_old, none_new;
    const uint32_t lm_old = sweep_wide(tb.n_boxes) ? sweep_leaves(sweep_mask<uint64_t>(o, inv, tb, &none_old), tb)
                                                   : sweep_leaves(sweep_mask<uint32_t>(o, inv, tb, &none_old), tb);
    const uint32_t lm = sweep_cands(o, inv, tb, &none_new);
    // ... and past the root's test whatever its answer (a lane riding along)
    const bool root = sweep_slab(o, inv, sweep_boxes(tb)[0]);
    const bool bad_ride = sweep_fold(o, inv, tb, root) != two_pass_riding(o, inv, tb, root) ||
                          (!root && sweep_fold(o, inv, tb, false) != 0u);
    // the flat loops' test against slab, box by box; a NaN on the flat axis counted
    for (int bx = 1; bx < tb.n_boxes; ++bx) {
      const SweepBox rb = sweep_boxes(tb)[bx];
      const int kind = kind_of(b, bx);
      if (kind < 2) continue;
      const bool f = kind == 2 ? sweep_slab_flat<0>(o, inv, rb) : kind == 3 ? sweep_slab_flat<1>(o, inv, rb)
                                                                              : sweep_slab_flat<2>(o, inv, rb);
      st[13] += f != sweep_slab(o, inv, rb);
      const int a = kind - 2;
      const float ta = (rb[a] - (a == 0 ? o.x : a == 1 ? o.y : o.z)) * (a == 0 ? inv.x : a == 1 ? inv.y : inv.z);
      st[14] += ta != ta;
    }
    // the threaded walk's answers (sweep_check.cpp check())
    threaded_leaves(b, o, inv, &want);
    float best = 1e30f;
    int bt = -1;
    bool occ = false;
    for (int tri : want) {
      const float4* T = &b.tris[3 * (size_t)tri];
      float t;
      if (tri_test(o, d, T[0], T[1], T[2], &t)) {
        if (t < best) {
          best = t;
          bt = tri;
        }
        occ = occ || (t < 1e30f && !(t >= limit));
      }
    }
    float sbest = 1e30f;
    int sl = -1;
    sweep_closest(o, d, lm, b.leaf_tris.data(), &sbest, &sl);
    const int stri = sl < 0 ? -1 : b.sweep.slot[sl];
    const bool bad_mask = lm != lm_old, bad_none = none_new != none_old;
    const bool bad_hit = memcmp(&sbest, &best, 4) != 0 || stri != bt;
    const bool bad_occ = sweep_occluded(o, d, limit, lm, b.leaf_tris.data()) != occ;
    st[0] += bad_mask;
    st[1] += bad_none;
    st[2] += bad_ride;
    st[3] += bad_hit;
    st[4] += bad_occ;
    if ((bad_mask || bad_none || bad_ride || bad_hit || bad_occ) && st[5] == ~0ull) st[5] = i;
    st[6] |= lm;
    st[7] += !root;
    st[8] += root;
    st[9] += (uint64_t)__builtin_popcount(lm);
    st[10] += bt >= 0;
    st[11] += occ;
  }
  st[12] = under_mismatches(b);
  st[15] = order_mismatches(b);
}

}  // namespace

extern "C" {

// rays as sweep_check's.  stats (16 words): rays whose [0] leaf mask, [1]
// `none` differ between sweep_cands and sweep_leaves(sweep_mask); [2] rays
// whose sweep_fold differs from the two passes without the early exit, or is
// not 0 with the root failing; [3] closest-hit (t bits, triangle) and [4]
// shadow mismatches between the new mask and the threaded walk; [5] first bad
// ray or ~0; [6] OR of all leaf masks; [7] rays failing the root, [8] passing
// it; [9] candidates; [10] rays with a hit; [11] occluded rays; [12] boxes
// whose under word differs from its definition; [13] (ray, flat box) pairs
// whose sweep_slab_flat differs from slab; [14] such pairs whose t on the flat
// axis is NaN; [15] boxes out of the table's order (root, general, x-, y-,
// z-flat by the counts word).  info: [0] boxes, [1] leaves, [2] boxes listed
// as flat.  slots[32]: the triangle slot of each leaf in visit order.
// Returns 0, 2 (no table) or 1 (err).
int sweep_fold_check(const float* V, size_t nvf, const uint32_t* I, size_t nt, const float* N, size_t nn, int int_bits,
                     const float* rays, size_t n, uint64_t* stats, int* info, int* slots, char* err, size_t errlen) {
  Built b;
  const std::string why = build(V, I, nt, N, nn, int_bits, &b);
  if (!why.empty()) {
    snprintf(err, errlen, "%s", why.c_str());
    return 1;
  }
  if (!b.has_table) return 2;
  info[0] = b.sweep.n_boxes;
  info[1] = b.sweep.n_leaves;
  info[2] = 0;
  for (int bx = 1; bx < b.sweep.n_boxes; ++bx) info[2] += kind_of(b, bx) >= 2;
  for (int l = 0; l < b.sweep.n_leaves; ++l) slots[l] = b.sweep.slot[(size_t)l];
  fold_rays(b, rays, n, stats);
  return 0;
}

}  // extern "C"

#ifdef SWEEP_FOLD_MAIN
// Stand-alone: a unit cube of 12 triangles under a hand-made tree (a chain of
// five nodes with the cube's box over six face nodes with flat boxes, each
// over its two triangles) plus one tilted triangle beside it under a root of
// their union, so flat and general boxes share the table.  Rays from a fixed
// LCG including zero direction components and origins in face planes.  Exit
// status 0 iff nothing differs and every leaf was a candidate of some ray.
int main() {
  std::vector<float> V;
  for (int i = 0; i < 8; ++i) {
    V.push_back(i & 1 ? 0.5f : -0.5f);
    V.push_back(i & 2 ? 0.5f : -0.5f);
    V.push_back(i & 4 ? 0.5f : -0.5f);
  }
  const float tilted[9] = {0.75f, -0.25f, 0.125f, 1.25f, 0.0f, -0.25f, 0.875f, 0.375f, 0.25f};
  V.insert(V.end(), tilted, tilted + 9);
  const int F[6][4] = {{0, 2, 6, 4}, {1, 5, 7, 3}, {0, 4, 5, 1}, {2, 3, 7, 6}, {0, 1, 3, 2}, {4, 6, 7, 5}};
  std::vector<uint32_t> I;
  for (auto& f : F) {
    const uint32_t t[6] = {(uint32_t)f[0], (uint32_t)f[1], (uint32_t)f[2], (uint32_t)f[0], (uint32_t)f[2], (uint32_t)f[3]};
    I.insert(I.end(), t, t + 6);
  }
  const uint32_t last[3] = {8, 9, 10};
  I.insert(I.end(), last, last + 3);
  // 25 nodes: 0 the root (left: the cube's chain at 1, right: the tilted
  // triangle's leaf 24); 1-5 the chain; 6-11 the faces; 12-23 their leaves
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
  const float clo[3] = {-0.5f, -0.5f, -0.5f}, chi[3] = {0.5f, 0.5f, 0.5f};
  float tlo[3], thi[3], rlo[3], rhi[3];
  bounds(last, 3, tlo, thi);
  for (int c = 0; c < 3; ++c) {
    rlo[c] = fmin_(clo[c], tlo[c]);
    rhi[c] = fmax_(chi[c], thi[c]);
  }
  node(rlo, rhi, 1, 24);
  for (int i = 0; i < 5; ++i) node(clo, chi, i < 4 ? 2 + i : 11, 6 + i);   // nodes 1-5
  for (int f = 0; f < 6; ++f) {                                             // nodes 6-11
    float lo[3], hi[3];
    const uint32_t vi[4] = {(uint32_t)F[f][0], (uint32_t)F[f][1], (uint32_t)F[f][2], (uint32_t)F[f][3]};
    bounds(vi, 4, lo, hi);
    node(lo, hi, 12 + 2 * f, 13 + 2 * f);
  }
  for (int f = 0; f < 6; ++f)                                               // nodes 12-23
    for (int h = 0; h < 2; ++h) {
      float lo[3], hi[3];
      memcpy(lo, &N[8 * (6 + f)], 12);
      memcpy(hi, &N[8 * (6 + f) + 4], 12);
      node(lo, hi, -1, 2 * f + h);
    }
  node(tlo, thi, -1, 12);                                                   // node 24
  uint32_t s = 12345u;
  auto rnd = [&]() { s = s * 1664525u + 1013904223u; return (float)(s >> 8) * (1.0f / 16777216.0f) * 2.0f - 1.0f; };
  std::vector<float> rays;
  const int n = 4000;
  for (int i = 0; i < n; ++i) {
    float r[8] = {rnd() * 1.5f, rnd() * 1.5f, rnd() * 1.5f, rnd(), rnd(), rnd(), (rnd() + 1.0f) * 2.0f, 0.0f};
    if (i % 4 == 1) r[3 + i % 3] = 0.0f;                      // a zero direction component
    if (i % 4 == 2) r[i % 3] = (i & 8) ? 0.5f : -0.5f;        // origin in a face plane
    if (i % 8 == 3) { r[i % 3] = 0.5f; r[3 + i % 3] = 0.0f; }  // ray lying in a face plane
    if (i % 16 == 4) {                                         // aimed at the tilted triangle
      r[3] = 0.95f - r[0];
      r[4] = 0.05f - r[1];
      r[5] = 0.05f - r[2];
    }
    rays.insert(rays.end(), r, r + 8);
  }
  uint64_t st[16];
  char err[256] = "";
  int info[3] = {0, 0, 0}, slots[32];
  const int rc = sweep_fold_check(V.data(), V.size(), I.data(), 13, N.data(), 25, 0, rays.data(), (size_t)n, st, info,
                                  slots, err, sizeof err);
  if (rc != 0) {
    printf("rc=%d %s\n", rc, err);
    return 1;
  }
  printf("boxes=%d leaves=%d flat_boxes=%d mask=%llu none=%llu riding=%llu hit=%llu shadow=%llu under=%llu flat=%llu "
         "order=%llu flat_nan=%llu covered=%#llx root_fail=%llu root_pass=%llu candidates=%llu hits=%llu occluded=%llu\n",
         info[0], info[1], info[2], (unsigned long long)st[0], (unsigned long long)st[1], (unsigned long long)st[2],
         (unsigned long long)st[3], (unsigned long long)st[4], (unsigned long long)st[12], (unsigned long long)st[13],
         (unsigned long long)st[15], (unsigned long long)st[14], (unsigned long long)st[6],
         (unsigned long long)st[7], (unsigned long long)st[8], (unsigned long long)st[9], (unsigned long long)st[10],
         (unsigned long long)st[11]);
  const bool ok = info[1] == 13 && info[2] == 6 && st[0] + st[1] + st[2] + st[3] + st[4] + st[12] + st[13] + st[15] == 0 &&
                  st[6] == (1ull << 13) - 1 && st[7] > 0 && st[8] > 0 && st[10] > 0 && st[14] > 0;
  return ok ? 0 : 1;
}
#endif
