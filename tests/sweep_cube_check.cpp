// Test infrastructure: the cube table of the sweep walk (scene/small_sweep.h
// SmallSweep::cube: every box other than the root is a hull face of it) and
// its straight-line walk (csrc/sweep_walk.h sweep_cands_cube) beside
// sweep_cands<true>, the walk it replaces, and beside the two-pass restatement
// sweep_leaves(sweep_mask(...)), ray by ray, in leaf mask and in `none`; the
// predicate beside its definition; cube_under[] and cube_all beside under[].
// Built by tests/test_sweep_cube.py with hipcc (host code only); with
// -DSWEEP_CUBE_MAIN it is a stand-alone program that checks built-in scenes
// (for sanitizer runs).
//
// The scene building is tests/sweep_check.cpp's own, included as it stands.
#include "sweep_check.cpp"

namespace {

int first_flat_axis(const float* r) {
  for (int a = 0; a < 3; ++a)
    if (memcmp(r + a, r + 4 + a, 4) == 0) return a;
  return -1;
}

uint32_t word(const float* p) {
  uint32_t w;
  memcpy(&w, p, 4);
  return w;
}

// The predicate by its definition, from the packed table: no general box,
// every flat box has a hull code, at most one box per (axis, code).  Fills
// face[2 * axis + code - 1] with the box index (or -1).
bool cube_by_definition(const float* table, int n_boxes, int face[6]) {
  for (int f = 0; f < 6; ++f) face[f] = -1;
  bool cube = (word(table + 7) & 0xffu) == 0u;   // the root record's count of general boxes
  for (int b = 1; b < n_boxes; ++b) {
    const float* r = table + 8 * (size_t)b;
    const int a = first_flat_axis(r);
    const uint32_t code = word(r + 7);
    if (a < 0 || (code != 1u && code != 2u)) {
      cube = false;
      continue;
    }
    // a code by its definition: the flat coordinate is the root's lo (1) or hi (2), the other extents the root's
    bool is_face = memcmp(r + a, table + (code == 1u ? 0 : 4) + a, 4) == 0;
    for (int c = 0; c < 3; ++c)
      if (c != a) is_face = is_face && memcmp(r + c, table + c, 4) == 0 && memcmp(r + 4 + c, table + 4 + c, 4) == 0;
    if (!is_face || face[2 * a + (int)code - 1] >= 0) cube = false;
    face[2 * a + (int)code - 1] = b;
  }
  return cube;
}

}  // namespace

extern "C" {

// rays as sweep_check's.  stats (12 words): rays whose [0] leaf mask, [1]
// `none` differ between sweep_cands_cube and sweep_cands<true>; [2] rays whose
// mask or `none` differ from sweep_leaves(sweep_mask); [3] first bad ray or
// ~0; [4] 1 when SmallSweep::cube differs from the definition; [5] words of
// cube_under[] / cube_all that differ from under[] (all must be 0 without a
// cube table); [6] rays passing the root, [7] failing it; [8] OR of all leaf
// masks; [9] candidates; [10] rays with a NaN among the root's six products;
// [11] rays walked by sweep_cands_cube.  info: [0] boxes, [1] leaves, [2]
// SmallSweep::n_hull, [3] SmallSweep::cube, [4] faces present.  Returns 0, 2
// (no table) or 1 (err).
int sweep_cube_check(const float* V, size_t nvf, const uint32_t* I, size_t nt, const float* N, size_t nn, int int_bits,
                     const float* rays, size_t n, uint64_t* st, int* info, char* err, size_t errlen) {
  Built b;
  const std::string why = build(V, I, nt, N, nn, int_bits, &b);
  if (!why.empty()) {
    snprintf(err, errlen, "%s", why.c_str());
    return 1;
  }
  if (!b.has_table) return 2;
  const pt::SmallSweep& s = b.sweep;
  const SweepTable tb = {(const float4*)b.table, s.n_boxes, s.n_leaves};
  memset(st, 0, 12 * sizeof(uint64_t));
  st[3] = ~0ull;
  int face[6];
  const bool want_cube = cube_by_definition(b.table, s.n_boxes, face);
  st[4] = want_cube != s.cube;
  info[0] = s.n_boxes;
  info[1] = s.n_leaves;
  info[2] = s.n_hull;
  info[3] = s.cube;
  info[4] = 0;
  for (int f = 0; f < 6; ++f) {
    info[4] += want_cube && face[f] >= 0;
    const uint32_t want = want_cube && face[f] >= 0 ? s.under[(size_t)face[f]] : 0u;
    st[5] += s.cube_under[f] != want;
    // ... and under[] is what the table's records hold
    if (want_cube && face[f] >= 0) st[5] += word(b.table + 8 * (size_t)face[f] + 3) != want;
  }
  st[5] += s.cube_all != (want_cube ? s.under[0] : 0u);
  if (want_cube) st[5] += word(b.table + 3) != s.cube_all;
  if (!s.cube || !want_cube) return 0;
  // the root box as the upload takes it: box 0 of the table, bitwise
  const float lo[3] = {b.table[0], b.table[1], b.table[2]}, hi[3] = {b.table[4], b.table[5], b.table[6]};
  for (size_t i = 0; i < n; ++i) {
    const float* r = rays + 8 * i;
    const v3 o = mk(r[0], r[1], r[2]), d = mk(r[3], r[4], r[5]);
    const v3 inv = mk(rcp_(d.x), rcp_(d.y), rcp_(d.z));
    bool none_two, none_hull, none_cube;
    const uint32_t lm_two = sweep_leaves(sweep_mask<uint32_t>(o, inv, tb, &none_two), tb);   // a cube table has 7 boxes at most
    const uint32_t lm_hull = sweep_cands<true>(o, inv, tb, &none_hull);
    const uint32_t lm_cube = sweep_cands_cube(o, inv, lo, hi, s.cube_under, s.cube_all, &none_cube);
    const bool bad_mask = lm_cube != lm_hull, bad_none = none_cube != none_hull;
    const bool bad_two = lm_cube != lm_two || none_cube != none_two;
    st[0] += bad_mask;
    st[1] += bad_none;
    st[2] += bad_two;
    if ((bad_mask || bad_none || bad_two) && st[3] == ~0ull) st[3] = i;
    const SweepRootVals R = sweep_root_vals(o, inv, sweep_boxes(tb)[0]);
    const bool root = sweep_root_pass(R);
    st[6] += root;
    st[7] += !root;
    st[8] |= lm_cube;
    st[9] += (uint64_t)__builtin_popcount(lm_cube);
    st[10] += R.t0x != R.t0x || R.t0y != R.t0y || R.t0z != R.t0z || R.t1x != R.t1x || R.t1y != R.t1y || R.t1z != R.t1z;
    st[11] += 1;
  }
  return 0;
}

}  // extern "C"

#ifdef SWEEP_CUBE_MAIN
namespace {

// A cuboid [lo, hi] under a hand-made tree: a chain of nodes with the cuboid's
// box over one node per face of `faces` (bit f: face f of x lo, x hi, y lo,
// y hi, z lo, z hi), each flat and over its two triangles -- with `extra`,
// beside one triangle inside the cuboid under a root of the same box (a general
// box: no cube table).
int run(const float* lo3, const float* hi3, unsigned faces, bool extra, bool want_cube) {
  std::vector<float> V;
  for (int i = 0; i < 8; ++i) {
    V.push_back(i & 1 ? hi3[0] : lo3[0]);
    V.push_back(i & 2 ? hi3[1] : lo3[1]);
    V.push_back(i & 4 ? hi3[2] : lo3[2]);
  }
  const float mid[3] = {0.5f * (lo3[0] + hi3[0]), 0.5f * (lo3[1] + hi3[1]), 0.5f * (lo3[2] + hi3[2])};
  const float ext[3] = {hi3[0] - lo3[0], hi3[1] - lo3[1], hi3[2] - lo3[2]};
  const float inner[9] = {mid[0] - 0.25f * ext[0], mid[1] - 0.125f * ext[1], mid[2] + 0.125f * ext[2],
                          mid[0] + 0.25f * ext[0], mid[1] - 0.25f * ext[1],  mid[2] - 0.125f * ext[2],
                          mid[0],                  mid[1] + 0.25f * ext[1],  mid[2] + 0.25f * ext[2]};
  if (extra) V.insert(V.end(), inner, inner + 9);
  const int Q[6][4] = {{0, 2, 6, 4}, {1, 5, 7, 3}, {0, 4, 5, 1}, {2, 3, 7, 6}, {0, 1, 3, 2}, {4, 6, 7, 5}};
  std::vector<int> F;
  for (int f = 0; f < 6; ++f)
    if (faces >> f & 1u) F.push_back(f);
  const int nf = (int)F.size();
  std::vector<uint32_t> I;
  for (int f : F) {
    const uint32_t t[6] = {(uint32_t)Q[f][0], (uint32_t)Q[f][1], (uint32_t)Q[f][2],
                           (uint32_t)Q[f][0], (uint32_t)Q[f][2], (uint32_t)Q[f][3]};
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
  // with `extra`: node 0 the root (left: the chain at 1, right: the inner
  // triangle's leaf, last); then nf - 1 chain nodes, nf face nodes, 2 nf leaves
  const int base = extra ? 1 : 0;
  const int chain = nf - 1, face0 = base + chain, leaf0 = face0 + nf;
  if (extra) node(lo3, hi3, 1, leaf0 + 2 * nf);
  for (int i = 0; i < chain; ++i) node(lo3, hi3, i < chain - 1 ? base + i + 1 : face0 + nf - 1, face0 + i);
  for (int k = 0; k < nf; ++k) {
    float lo[3], hi[3];
    const uint32_t vi[4] = {(uint32_t)Q[F[k]][0], (uint32_t)Q[F[k]][1], (uint32_t)Q[F[k]][2], (uint32_t)Q[F[k]][3]};
    bounds(vi, 4, lo, hi);
    node(lo, hi, leaf0 + 2 * k, leaf0 + 2 * k + 1);
  }
  for (int k = 0; k < nf; ++k)
    for (int h = 0; h < 2; ++h) {
      float lo[3], hi[3];
      memcpy(lo, &N[8 * (size_t)(face0 + k)], 12);
      memcpy(hi, &N[8 * (size_t)(face0 + k) + 4], 12);
      node(lo, hi, -1, 2 * k + h);
    }
  if (extra) {
    float tlo[3], thi[3];
    bounds(last, 3, tlo, thi);
    node(tlo, thi, -1, 2 * nf);
  }
  uint32_t s = 2463534242u;
  auto rnd = [&]() { s = s * 1664525u + 1013904223u; return (float)(s >> 8) * (1.0f / 16777216.0f) * 2.0f - 1.0f; };
  std::vector<float> rays;
  const int n = 20000;
  for (int i = 0; i < n; ++i) {
    float r[8] = {mid[0] + rnd() * ext[0], mid[1] + rnd() * ext[1], mid[2] + rnd() * ext[2], rnd(), rnd(), rnd(),
                  (rnd() + 1.0f) * 2.0f, 0.0f};
    const int a = i % 3;
    if (i % 8 == 1) r[3 + a] = 0.0f;                                            // a zero direction component
    if (i % 8 == 2) r[a] = (i & 8) ? hi3[a] : lo3[a];                           // origin in a face plane
    if (i % 8 == 3) { r[a] = (i & 16) ? hi3[a] : lo3[a]; r[3 + a] = (i & 32) ? -0.0f : 0.0f; }   // lying in it
    if (i % 8 == 4) for (int c = 0; c < 3; ++c) r[c] = mid[c] + 0.45f * (r[c] - mid[c]);         // origin inside
    if (i % 8 == 5) { r[a] = (i & 16) ? hi3[a] : lo3[a]; r[3 + a] = (i & 32) ? -1e-41f : 1e-41f; }   // subnormal
    if (i % 8 == 6) { r[3 + (a + 1) % 3] = 0.0f; r[3 + (a + 2) % 3] = -0.0f; }  // axis-parallel
    rays.insert(rays.end(), r, r + 8);
  }
  uint64_t st[12];
  int info[5] = {0, 0, 0, 0, 0};
  char err[256] = "";
  const int rc = sweep_cube_check(V.data(), V.size(), I.data(), I.size() / 3, N.data(), N.size() / 8, 0, rays.data(),
                                  (size_t)n, st, info, err, sizeof err);
  if (rc != 0) {
    printf("rc=%d %s\n", rc, err);
    return 1;
  }
  printf("boxes=%d leaves=%d hull_boxes=%d cube=%d faces=%d mask=%llu none=%llu two_pass=%llu predicate=%llu under=%llu "
         "root_pass=%llu root_fail=%llu covered=%#llx candidates=%llu nan=%llu walked=%llu\n",
         info[0], info[1], info[2], info[3], info[4], (unsigned long long)st[0], (unsigned long long)st[1],
         (unsigned long long)st[2], (unsigned long long)st[4], (unsigned long long)st[5], (unsigned long long)st[6],
         (unsigned long long)st[7], (unsigned long long)st[8], (unsigned long long)st[9], (unsigned long long)st[10],
         (unsigned long long)st[11]);
  bool ok = st[0] + st[1] + st[2] + st[4] + st[5] == 0 && (info[3] != 0) == want_cube;
  if (want_cube)
    ok = ok && info[4] == nf && st[11] == (uint64_t)n && st[8] == (1ull << info[1]) - 1 && st[6] > 0 && st[7] > 0 &&
         st[10] > 0;
  else
    ok = ok && st[11] == 0;
  return ok ? 0 : 1;
}

}  // namespace

// Stand-alone: a cuboid of three different extents off the origin (a cube
// table of six faces), the same without its y hi face (five), and the whole
// one beside a triangle inside it (a general box: no cube table).  Exit status
// 0 iff nothing differs and every leaf was a candidate of some ray.
int main() {
  const float lo[3] = {0.375f, -1.25f, 2.0f}, hi[3] = {1.125f, -0.75f, 3.5f};
  const int a = run(lo, hi, 0x3fu, false, true);
  const int b = run(lo, hi, 0x3fu & ~8u, false, true);
  const int c = run(lo, hi, 0x3fu, true, false);
  return a | b | c;
}
#endif
