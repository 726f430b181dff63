// Test infrastructure: the sweep walk of tiny scenes (csrc/sweep_walk.h, the
// code the LDS render kernel runs, compiled for the host) beside the threaded
// walk it replaces, ray by ray.  Built by tests/test_sweep.py with hipcc (host
// code only); with -DSWEEP_CHECK_MAIN it is a stand-alone program that checks
// a built-in scene (for sanitizer runs).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "scene/small_sweep.h"
#include "scene/threaded_bvh.h"
#include "sweep_walk.h"

using namespace ptd;

namespace {

struct Built {
  std::vector<float> collapsed;   // threaded, implied internal nodes dropped: 8 floats per kept node
  size_t n_kept = 0;
  pt::SmallSweep sweep;
  bool has_table = false;
  std::vector<float4> tris;       // by slot: {v0, e1.x} {e1.yz, e2.xy} {e2.z, n}
  std::vector<float4> leaf_tris;  // by leaf of the table
  float* table = nullptr;         // pack(), 64-B aligned like a device allocation
  ~Built() { free(table); }
};

std::string build(const float* V, const uint32_t* I, size_t nt, const float* N, size_t nn, int int_bits, Built* b) {
  std::vector<float> threaded;
  const std::string why = pt::thread_bvh(N, nn, int_bits != 0, nt, &threaded);
  if (!why.empty()) return why;
  pt::collapse_implied(threaded, &b->collapsed);
  b->n_kept = b->collapsed.size() / 8;
  b->tris.resize(3 * nt);
  for (size_t t = 0; t < nt; ++t) {   // setup_tris_kernel's records
    v3 p[3];
    for (int c = 0; c < 3; ++c) {
      const uint32_t vi = I[3 * t + c];
      p[c] = mk(V[3 * vi], V[3 * vi + 1], V[3 * vi + 2]);
    }
    const v3 e1 = sub(p[1], p[0]), e2 = sub(p[2], p[0]);
    const v3 n = normalize(cross(e1, e2));
    b->tris[3 * t] = make_float4(p[0].x, p[0].y, p[0].z, e1.x);
    b->tris[3 * t + 1] = make_float4(e1.y, e1.z, e2.x, e2.y);
    b->tris[3 * t + 2] = make_float4(e2.z, n.x, n.y, n.z);
  }
  b->has_table = pt::build_small_sweep(b->collapsed.data(), b->n_kept, &b->sweep);
  if (b->has_table) {
    const std::vector<float> t = b->sweep.pack();
    b->table = (float*)aligned_alloc(64, (t.size() * sizeof(float) + 63) / 64 * 64);
    memcpy(b->table, t.data(), t.size() * sizeof(float));
    for (int l = 0; l < b->sweep.n_leaves; ++l)
      for (int c = 0; c < 3; ++c) b->leaf_tris.push_back(b->tris[3 * (size_t)b->sweep.slot[l] + c]);
  }
  return "";
}

// The threaded walk of csrc/kernels/walks.h (trace_closest / occluded) for one ray:
// the slots of the leaves whose triangles it tests, in visit order.
void threaded_leaves(const Built& b, v3 o, v3 inv, std::vector<int>* leaves) {
  const float4* nodes = (const float4*)b.collapsed.data();
  leaves->clear();
  size_t k = 0;
  while (k < b.n_kept) {
    const float4 a = nodes[2 * k], c = nodes[2 * k + 1];
    const int raw = (int)f2u(a.w), tri = (int)f2u(c.w);
    const bool h = slab(o, inv, a, c) || raw < 0;
    if (h && tri >= 0) leaves->push_back(tri);
    k = (h && tri < 0) ? k + 1 : (size_t)(raw & 0x7fffffff);
  }
}

int check(const Built& b, const float* rays, size_t n, uint64_t* st) {
  memset(st, 0, 8 * sizeof(uint64_t));
  st[3] = ~0ull;
  const SweepTable tb = {(const float4*)b.table, b.sweep.n_boxes, b.sweep.n_leaves};
  std::vector<int> want;
  for (size_t i = 0; i < n; ++i) {
    const float* r = rays + 8 * i;
    const v3 o = mk(r[0], r[1], r[2]), d = mk(r[3], r[4], r[5]);
    const float limit = r[6];
    const v3 inv = mk(rcp_(d.x), rcp_(d.y), rcp_(d.z));
    threaded_leaves(b, o, inv, &want);
    // threaded answers: the candidates in order with the strict '<'; any accepted below the limit
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
    // the sweep
    bool none;
    const uint32_t lm = sweep_wide(tb.n_boxes) ? sweep_leaves(sweep_mask<uint64_t>(o, inv, tb, &none), tb)
                                               : sweep_leaves(sweep_mask<uint32_t>(o, inv, tb, &none), tb);
    bool bad_seq = (size_t)__builtin_popcount(lm) != want.size();
    uint32_t m = lm;
    for (size_t j = 0; !bad_seq && j < want.size(); ++j, m &= m - 1u)
      bad_seq = b.sweep.slot[__builtin_ctz(m)] != want[j];
    float sbest = 1e30f;
    int sl = -1;
    sweep_closest(o, d, lm, b.leaf_tris.data(), &sbest, &sl);
    const int stri = sl < 0 ? -1 : b.sweep.slot[sl];
    const bool bad_hit = memcmp(&sbest, &best, 4) != 0 || stri != bt;
    const bool bad_occ = sweep_occluded(o, d, limit, lm, b.leaf_tris.data()) != occ;
    st[0] += bad_seq;
    st[1] += bad_hit;
    st[2] += bad_occ;
    if ((bad_seq || bad_hit || bad_occ) && st[3] == ~0ull) st[3] = i;
    st[4] += want.size();
    st[5] += bt >= 0;
    st[6] += occ;
  }
  return 0;
}

}  // namespace

extern "C" {

// info[0] distinct boxes, info[1] leaves, info[2] leaves whose need lacks bit
// 0, info[3] kept nodes.  Returns 0, 2 when the scene gets no table, or 1 (err).
int sweep_info(const float* V, size_t nvf, const uint32_t* I, size_t nt, const float* N, size_t nn, int int_bits,
               int* info, char* err, size_t errlen) {
  Built b;
  const std::string why = build(V, I, nt, N, nn, int_bits, &b);
  if (!why.empty()) {
    snprintf(err, errlen, "%s", why.c_str());
    return 1;
  }
  info[0] = b.sweep.n_boxes;
  info[1] = b.sweep.n_leaves;
  info[2] = 0;
  for (uint64_t nd : b.sweep.need) info[2] += (nd & 1u) ? 0 : 1;
  info[3] = (int)b.n_kept;
  return b.has_table ? 0 : 2;
}

// rays: n x 8 floats {o.xyz, d.xyz, shadow limit, 0}; every ray is checked as
// a closest-hit walk and as a shadow query.  stats: [0] rays whose candidate
// leaf sequence differs, [1] closest-hit (t bits, triangle) mismatches, [2]
// shadow mismatches, [3] first bad ray or ~0, [4] candidates, [5] rays with a
// hit, [6] occluded rays.  Returns 0, 2 (no table) or 1 (err).
int sweep_check(const float* V, size_t nvf, const uint32_t* I, size_t nt, const float* N, size_t nn, int int_bits,
                const float* rays, size_t n, uint64_t* stats, char* err, size_t errlen) {
  Built b;
  const std::string why = build(V, I, nt, N, nn, int_bits, &b);
  if (!why.empty()) {
    snprintf(err, errlen, "%s", why.c_str());
    return 1;
  }
  if (!b.has_table) return 2;
  return check(b, rays, n, stats);
}

}  // extern "C"

#ifdef SWEEP_CHECK_MAIN
// Stand-alone: a unit cube of 12 triangles under a hand-made tree (root, six
// face nodes with flat boxes, the faces' two triangles sharing the face box),
// rays from a fixed LCG including axis-parallel directions and origins on
// face planes.  Exit status 0 iff nothing differs.
int main() {
  std::vector<float> V;
  for (int i = 0; i < 8; ++i) {
    V.push_back(i & 1 ? 0.5f : -0.5f);
    V.push_back(i & 2 ? 0.5f : -0.5f);
    V.push_back(i & 4 ? 0.5f : -0.5f);
  }
  const int F[6][4] = {{0, 2, 6, 4}, {1, 5, 7, 3}, {0, 4, 5, 1}, {2, 3, 7, 6}, {0, 1, 3, 2}, {4, 6, 7, 5}};
  std::vector<uint32_t> I;
  for (auto& f : F) {
    const uint32_t t[6] = {(uint32_t)f[0], (uint32_t)f[1], (uint32_t)f[2], (uint32_t)f[0], (uint32_t)f[2], (uint32_t)f[3]};
    I.insert(I.end(), t, t + 6);
  }
  // 23 nodes: a left-leaning chain of 5 internal nodes over 6 face nodes, each over 2 leaves
  std::vector<float> N;
  auto node = [&](const float* lo, const float* hi, int l, int r) {
    const float rec[8] = {lo[0], lo[1], lo[2], (float)l, hi[0], hi[1], hi[2], (float)r};
    N.insert(N.end(), rec, rec + 8);
  };
  const float clo[3] = {-0.5f, -0.5f, -0.5f}, chi[3] = {0.5f, 0.5f, 0.5f};
  // nodes 0-4: chain (node i: left = i + 1 or face 10, right = face 5 + i)
  for (int i = 0; i < 5; ++i) node(clo, chi, i < 4 ? i + 1 : 10, 5 + i);
  for (int f = 0; f < 6; ++f) {   // nodes 5-10: faces over leaves 11 + 2f, 12 + 2f
    float lo[3] = {1e30f, 1e30f, 1e30f}, hi[3] = {-1e30f, -1e30f, -1e30f};
    for (int k = 0; k < 4; ++k)
      for (int c = 0; c < 3; ++c) {
        lo[c] = fmin_(lo[c], V[3 * F[f][k] + c]);
        hi[c] = fmax_(hi[c], V[3 * F[f][k] + c]);
      }
    node(lo, hi, 11 + 2 * f, 12 + 2 * f);
  }
  for (int f = 0; f < 6; ++f)
    for (int h = 0; h < 2; ++h) {
      float lo[3], hi[3];
      memcpy(lo, &N[8 * (5 + f)], 12);
      memcpy(hi, &N[8 * (5 + f) + 4], 12);
      node(lo, hi, -1, 2 * f + h);
    }
  uint32_t s = 12345u;
  auto rnd = [&]() { s = s * 1664525u + 1013904223u; return (float)(s >> 8) * (1.0f / 16777216.0f) * 2.0f - 1.0f; };
  std::vector<float> rays;
  for (int i = 0; i < 4000; ++i) {
    float r[8] = {rnd() * 1.5f, rnd() * 1.5f, rnd() * 1.5f, rnd(), rnd(), rnd(), (rnd() + 1.0f) * 2.0f, 0.0f};
    if (i % 4 == 1) r[3 + i % 3] = 0.0f;                      // a zero direction component
    if (i % 4 == 2) r[i % 3] = (i & 8) ? 0.5f : -0.5f;        // origin in a face plane
    if (i % 8 == 3) { r[i % 3] = 0.5f; r[3 + i % 3] = 0.0f; }  // ray lying in a face plane
    rays.insert(rays.end(), r, r + 8);
  }
  uint64_t st[8];
  char err[256] = "";
  int info[4];
  const int ri = sweep_info(V.data(), V.size(), I.data(), 12, N.data(), 23, 0, info, err, sizeof err);
  const int rc = sweep_check(V.data(), V.size(), I.data(), 12, N.data(), 23, 0, rays.data(), 4000, st, err, sizeof err);
  printf("info rc=%d boxes=%d leaves=%d need_without_root=%d kept=%d\n", ri, info[0], info[1], info[2], info[3]);
  printf("check rc=%d seq=%llu hit=%llu shadow=%llu candidates=%llu hits=%llu occluded=%llu %s\n", rc,
         (unsigned long long)st[0], (unsigned long long)st[1], (unsigned long long)st[2], (unsigned long long)st[4],
         (unsigned long long)st[5], (unsigned long long)st[6], err);
  return (ri == 0 && rc == 0 && info[2] == 0 && st[0] + st[1] + st[2] == 0 && st[5] > 0) ? 0 : 1;
}
#endif
