// sweep_walk.h — the exact walk of a tiny scene as a wave-uniform box sweep
// (scene/small_sweep.h builds the table; the LDS render kernel, through kernels/walks.h, and
// tests/sweep_check.cpp, tests/sweep_fold_check.cpp run these functions).
//
// Why it returns the threaded walk's hits bit for bit:
//   * slab(o, inv, lo, hi) is a pure function of the ray and the 24 bytes of
//     a box, and takes no tmax: nothing is culled by distance.  So the threaded
//     walk tests the triangle of a leaf exactly when the leaf's box and every
//     ancestor's box pass the slab test (an implied node passes with its
//     parent, whose box it has bitwise), in kept-node index order.
//   * The table holds each distinct box once.  need[l] is the OR of the box
//     bits of leaf l and all its ancestors: leaf l is a candidate iff every
//     box of need[l] passes.  Which leaves a box guards is a property of the
//     box, the same for every ray, so each box's record carries
//     under[b] = { l : need[l] has bit b } in its fourth word, and the sweep
//     (sweep_cands) ORs the under masks of the boxes that fail: the
//     candidates are the leaves no failing box guards.  One pass, one 32-bit
//     leaf mask per lane whatever the number of boxes (up to 64).
//   * A box with lo == hi bitwise on an axis (every axis-aligned face: six of
//     the box's seven) has t0 == t1 there, so slab's fmin_(t, t) and
//     fmax_(t, t) are t itself.  The table lists the root, the general boxes,
//     then the x-, y- and z-flat ones, and the sweep runs one loop per group;
//     the flat loops (sweep_slab_flat) skip one subtract, multiply, min and
//     max per box and answer as slab does, NaNs included.
//   * A flat box that is a face of the root box -- its flat coordinate bitwise
//     the root's lo or hi on that axis, its other four extents bitwise the
//     root's: the cube's six -- is a hull face, marked by a code (1 lo, 2 hi)
//     in its record's last word.  Each of the products (plane - o) * inv that
//     sweep_slab_flat would form from its record has, operand for operand,
//     the bits of one of the six the root's test formed, so it is that
//     product bit for bit.  sweep_cands<true> keeps the root's six products
//     and a hull face (sweep_slab_hull) takes the one of its code on the flat
//     axis and the root's pairs on the other two, through the same fmin_ /
//     fmax_ calls in the same order with the same operand order: same
//     operands, same operations, same bits, NaNs included.  The branch on the
//     code is scalar.  A table without hull faces is walked by
//     sweep_cands<false>, which keeps nothing from the root's test.
//   * A table all of whose boxes but the root are hull faces (the cube table:
//     the box, a cuboid, a cuboid without some face) needs no record at all:
//     sweep_cands_cube takes the root box and the faces' under words from its
//     caller and tests the six faces straight-line, their axis and code fixed
//     at compile time -- the booleans sweep_cands<true> forms, ORed in another
//     order.
//   * sweep_mask / sweep_leaves state the same predicate from need[] in two
//     passes (box bits, then (sb & need[l]) == need[l] per leaf).  The device
//     does not call them: they are the restatement the tests hold sweep_cands
//     to, ray by ray.
//   * Candidates are popped from the leaf mask lowest bit first -- the visit
//     order -- with the same tri_test and the same strict '<'.
// The sweep loop is wave-uniform: on the device the boxes arrive through the
// constant address space into scalar registers, with no LDS read and no
// per-lane address.
#pragma once
#include "pt_isect.h"

namespace ptd {
using namespace ptm;

// The device table of pt::SmallSweep::pack(): n_boxes records of 8 floats
// {lo.xyz, under, hi.xyz, 0} (under: the bit pattern of the box's leaf mask;
// slab never reads that word) in the order root, general, x-flat, y-flat,
// z-flat, the root's last word holding the four counts after it (general |
// x << 8 | y << 16 | z << 24), then need[] (one word per leaf, two -- low,
// high -- with more than 32 boxes) padded to a multiple of 4 words, then
// slot[n_leaves].  32-B aligned.
struct SweepTable {
  const float4* boxes;
  int n_boxes, n_leaves;
};

// Whole records through the constant address space: a wave-uniform index
// makes each a scalar load of 8 (4) dwords.
typedef float SweepBox __attribute__((ext_vector_type(8)));
typedef uint32_t SweepNeed4 __attribute__((ext_vector_type(4)));
#if defined(__HIP_DEVICE_COMPILE__)
typedef const __attribute__((address_space(4))) SweepBox* SweepBoxP;
typedef const __attribute__((address_space(4))) SweepNeed4* SweepNeedP;
#else
typedef const SweepBox* SweepBoxP;
typedef const SweepNeed4* SweepNeedP;
#endif
PT_FN bool sweep_wide(int n_boxes) { return n_boxes > 32; }
PT_FN int sweep_need_words(int n_boxes, int n_leaves) { return ((sweep_wide(n_boxes) ? 2 : 1) * n_leaves + 3) & ~3; }
PT_FN SweepBoxP sweep_boxes(const SweepTable& t) { return (SweepBoxP)t.boxes; }
PT_FN SweepNeedP sweep_need(const SweepTable& t) { return (SweepNeedP)(t.boxes + 2 * t.n_boxes); }
PT_FN const int* sweep_slots(const SweepTable& t) {
  return (const int*)(t.boxes + 2 * t.n_boxes) + sweep_need_words(t.n_boxes, t.n_leaves);
}
PT_FN bool sweep_slab(v3 o, v3 inv, SweepBox r) {
  return slab(o, inv, make_float4(r[0], r[1], r[2], r[3]), make_float4(r[4], r[5], r[6], r[7]));
}

// Boxes per trip of the sweep loop (their scalar loads are issued together).
#ifndef PT_SWEEP_UNROLL
#define PT_SWEEP_UNROLL 4
#endif

// Bit b set iff distinct box b passes the slab test.  Box 0 is the root's and
// every need mask holds bit 0: when no ray at hand passes it (no lane of the
// wave on the device) the other boxes are not tested and *none is set: the
// walk has no candidate.  M: uint32_t, or uint64_t for a table of more than
// 32 boxes.
template <class M>
PT_FN M sweep_mask(v3 o, v3 inv, const SweepTable& t, bool* none) {
  const SweepBoxP B = sweep_boxes(t);
  const bool root = sweep_slab(o, inv, B[0]);
#if defined(__HIP_DEVICE_COMPILE__)
  *none = __builtin_amdgcn_ballot_w64(root) == 0;
#else
  *none = !root;
#endif
  if (*none) return 0;
  M sb = root ? 1 : 0;
  const int nb = t.n_boxes;
#pragma clang loop vectorize(disable) unroll_count(PT_SWEEP_UNROLL)
  for (int b = 1; b < nb; ++b) sb |= sweep_slab(o, inv, B[b]) ? (M)1 << b : (M)0;
  return sb;
}

// Bit l set iff leaf l (in visit order) is a candidate of the ray: sb holds
// every box bit of need[l].  Four words of need[] per trip; the padding
// words' bits are masked off.
template <class M>
PT_FN uint32_t sweep_leaves(M sb, const SweepTable& t) {
  const SweepNeedP need = sweep_need(t);
  const int nl = t.n_leaves;
  uint32_t lm = 0u;
  if constexpr (sizeof(M) == 4) {
    const uint32_t s = (uint32_t)sb;
#pragma clang loop vectorize(disable)
    for (int l = 0; l < nl; l += 4) {
      const SweepNeed4 nd = need[l >> 2];
      uint32_t m = 0u;
      m |= (s & nd[0]) == nd[0] ? 1u : 0u;
      m |= (s & nd[1]) == nd[1] ? 2u : 0u;
      m |= (s & nd[2]) == nd[2] ? 4u : 0u;
      m |= (s & nd[3]) == nd[3] ? 8u : 0u;
      lm |= m << l;
    }
  } else {
    const uint64_t s = (uint64_t)sb;
#pragma clang loop vectorize(disable)
    for (int l = 0; l < nl; l += 2) {
      const SweepNeed4 nd = need[l >> 1];
      const uint64_t n0 = nd[0] | (uint64_t)nd[1] << 32, n1 = nd[2] | (uint64_t)nd[3] << 32;
      uint32_t m = 0u;
      m |= (s & n0) == n0 ? 1u : 0u;
      m |= (s & n1) == n1 ? 2u : 0u;
      lm |= m << l;
    }
  }
  return nl >= 32 ? lm : lm & ((1u << nl) - 1u);
}

// Flat boxes per trip of their loops (the box has two per axis; at four its
// pairs ran through the one-box remainder and measured slower, profiles/fold).
#ifndef PT_SWEEP_FLAT_UNROLL
#define PT_SWEEP_FLAT_UNROLL 2
#endif
// slab() for a box with lo == hi bitwise on AXIS: there t0 == t1, so
// fmin_(t, t) and fmax_(t, t) are t itself (a NaN stays a NaN and the outer
// min/max drop it as before).  Same operations in the same order otherwise.
template <int AXIS>
PT_FN bool sweep_slab_flat(v3 o, v3 inv, SweepBox r) {
  const float t0x = (r[0] - o.x) * inv.x, t0y = (r[1] - o.y) * inv.y, t0z = (r[2] - o.z) * inv.z;
  const float t1x = AXIS == 0 ? t0x : (r[4] - o.x) * inv.x;
  const float t1y = AXIS == 1 ? t0y : (r[5] - o.y) * inv.y;
  const float t1z = AXIS == 2 ? t0z : (r[6] - o.z) * inv.z;
  const float nx = AXIS == 0 ? t0x : fmin_(t0x, t1x), fx = AXIS == 0 ? t0x : fmax_(t0x, t1x);
  const float ny = AXIS == 1 ? t0y : fmin_(t0y, t1y), fy = AXIS == 1 ? t0y : fmax_(t0y, t1y);
  const float nz = AXIS == 2 ? t0z : fmin_(t0z, t1z), fz = AXIS == 2 ? t0z : fmax_(t0z, t1z);
  const float tmin = fmax_(fmax_(nx, ny), nz);
  const float tmax = fmin_(fmin_(fx, fy), fz);
  return tmin <= tmax && tmax >= 0.0f;
}
// The root's slab values: the six products (plane - o) * inv of its record,
// the operands of slab's per-axis min and max.  A hull face (below) reads them
// instead of computing its own.
struct SweepRootVals {
  float t0x, t0y, t0z, t1x, t1y, t1z;
};
PT_FN SweepRootVals sweep_root_vals(v3 o, v3 inv, SweepBox r) {
  SweepRootVals R;
  R.t0x = (r[0] - o.x) * inv.x, R.t0y = (r[1] - o.y) * inv.y, R.t0z = (r[2] - o.z) * inv.z;
  R.t1x = (r[4] - o.x) * inv.x, R.t1y = (r[5] - o.y) * inv.y, R.t1z = (r[6] - o.z) * inv.z;
  return R;
}
// slab() of the root's record from its products: slab's own tail.
PT_FN bool sweep_root_pass(const SweepRootVals& R) {
  const float tmin = fmax_(fmax_(fmin_(R.t0x, R.t1x), fmin_(R.t0y, R.t1y)), fmin_(R.t0z, R.t1z));
  const float tmax = fmin_(fmin_(fmax_(R.t0x, R.t1x), fmax_(R.t0y, R.t1y)), fmax_(R.t0z, R.t1z));
  return tmin <= tmax && tmax >= 0.0f;
}
// On the device the six products stay in registers from the root's test to
// the flat loops, but not the six min/max formed from them: the kernel has no
// registers to spare (80, 6 waves), and forming the four a face needs again
// costs less than spilling them.  An empty asm the compiler cannot see through
// keeps it from reusing the root test's.  The values are untouched.
#if defined(__HIP_DEVICE_COMPILE__)
#define PT_SWEEP_OPAQUE(x) __asm__ volatile("" : "+v"(x))
#else
#define PT_SWEEP_OPAQUE(x) ((void)0)
#endif
PT_FN void sweep_root_detach(SweepRootVals* R) {
  PT_SWEEP_OPAQUE(R->t0x); PT_SWEEP_OPAQUE(R->t0y); PT_SWEEP_OPAQUE(R->t0z);
  PT_SWEEP_OPAQUE(R->t1x); PT_SWEEP_OPAQUE(R->t1y); PT_SWEEP_OPAQUE(R->t1z);
}
// A hull face: a box flat on AXIS whose flat coordinate is bitwise the root's
// lo (code 1) or hi (code 2) there and whose extents on the other two axes are
// bitwise the root's (scene/small_sweep.h marks them in the record's last
// word).  Every product sweep_slab_flat<AXIS> would form from its record has
// the operands of one of the root's, so it is that product bit for bit.  The
// rest is sweep_slab_flat's: same calls, same order, same operand order.
template <int AXIS>
PT_FN bool sweep_slab_hull(const SweepRootVals& R, uint32_t code) {
  const float t0x = AXIS == 0 && code != 1u ? R.t1x : R.t0x, t1x = R.t1x;
  const float t0y = AXIS == 1 && code != 1u ? R.t1y : R.t0y, t1y = R.t1y;
  const float t0z = AXIS == 2 && code != 1u ? R.t1z : R.t0z, t1z = R.t1z;
  const float nx = AXIS == 0 ? t0x : fmin_(t0x, t1x), fx = AXIS == 0 ? t0x : fmax_(t0x, t1x);
  const float ny = AXIS == 1 ? t0y : fmin_(t0y, t1y), fy = AXIS == 1 ? t0y : fmax_(t0y, t1y);
  const float nz = AXIS == 2 ? t0z : fmin_(t0z, t1z), fz = AXIS == 2 ? t0z : fmax_(t0z, t1z);
  const float tmin = fmax_(fmax_(nx, ny), nz);
  const float tmax = fmin_(fmin_(fx, fy), fz);
  return tmin <= tmax && tmax >= 0.0f;
}
// One flat box of the sweep: the record's last word is 0 (sweep_slab_flat) or
// a hull code.  The word is the same for every lane: a scalar branch.
template <int AXIS>
PT_FN bool sweep_flat_pass(v3 o, v3 inv, const SweepRootVals& R, SweepBox r) {
  const uint32_t code = f2u(r[7]);
  if (code != 0u) return sweep_slab_hull<AXIS>(R, code);
  return sweep_slab_flat<AXIS>(o, inv, r);
}
// Bit l set iff leaf l (in visit order) is a candidate of the ray: no box that
// fails the slab test has l in its under mask (the record's fourth word).
// Box 0 is the root's and guards every leaf: when no ray at hand passes it (no
// lane of the wave on the device) the other boxes are not tested and *none is
// set: the walk has no candidate.  Equal to sweep_leaves(sweep_mask(...)) and
// its *none for every ray, NaNs of 0 * inf included: both go through slab's
// operations.
//
// sweep_fold_vals is the sweep past the root's test: R the root's values for
// this ray (HULL: the hull faces read them), `root` its answer, false in a
// lane that rides along because another lane of its wave passed.
template <bool HULL>
PT_FN uint32_t sweep_fold_vals(v3 o, v3 inv, const SweepTable& t, const SweepRootVals& R, bool root) {
  const SweepBoxP B = sweep_boxes(t);
  const SweepBox r0 = B[0];
  const uint32_t all = f2u(r0[3]);
  uint32_t fail = root ? 0u : all;
  // the table's order: root, general boxes, x-flat, y-flat, z-flat; their counts in the root record's last word
  const uint32_t cnt = f2u(r0[7]);
  int b = 1, e = 1 + (int)(cnt & 0xffu);
#pragma clang loop vectorize(disable) unroll_count(PT_SWEEP_UNROLL)
  for (; b < e; ++b) {
    const SweepBox r = B[b];
    fail |= sweep_slab(o, inv, r) ? 0u : f2u(r[3]);
  }
  e += (int)(cnt >> 8 & 0xffu);
#pragma clang loop vectorize(disable) unroll_count(PT_SWEEP_FLAT_UNROLL)
  for (; b < e; ++b) {
    const SweepBox r = B[b];
    fail |= (HULL ? sweep_flat_pass<0>(o, inv, R, r) : sweep_slab_flat<0>(o, inv, r)) ? 0u : f2u(r[3]);
  }
  e += (int)(cnt >> 16 & 0xffu);
#pragma clang loop vectorize(disable) unroll_count(PT_SWEEP_FLAT_UNROLL)
  for (; b < e; ++b) {
    const SweepBox r = B[b];
    fail |= (HULL ? sweep_flat_pass<1>(o, inv, R, r) : sweep_slab_flat<1>(o, inv, r)) ? 0u : f2u(r[3]);
  }
  e += (int)(cnt >> 24 & 0xffu);
#pragma clang loop vectorize(disable) unroll_count(PT_SWEEP_FLAT_UNROLL)
  for (; b < e; ++b) {
    const SweepBox r = B[b];
    fail |= (HULL ? sweep_flat_pass<2>(o, inv, R, r) : sweep_slab_flat<2>(o, inv, r)) ? 0u : f2u(r[3]);
  }
  return all & ~fail;
}
PT_FN uint32_t sweep_fold(v3 o, v3 inv, const SweepTable& t, bool root) {
  return sweep_fold_vals<true>(o, inv, t, sweep_root_vals(o, inv, sweep_boxes(t)[0]), root);
}
// HULL false: the sweep for a table known to hold no hull code (or whose codes
// are to be ignored): every flat box through sweep_slab_flat, nothing kept
// from the root's test.  The same answer for any table.
template <bool HULL = true>
PT_FN uint32_t sweep_cands(v3 o, v3 inv, const SweepTable& t, bool* none) {
  SweepRootVals R = {};
  bool root;
  if constexpr (HULL) {
    R = sweep_root_vals(o, inv, sweep_boxes(t)[0]);
    root = sweep_root_pass(R);
  } else {
    root = sweep_slab(o, inv, sweep_boxes(t)[0]);
  }
#if defined(__HIP_DEVICE_COMPILE__)
  *none = __builtin_amdgcn_ballot_w64(root) == 0;
#else
  *none = !root;
#endif
  if (*none) return 0u;
  if constexpr (HULL) sweep_root_detach(&R);
  return sweep_fold_vals<HULL>(o, inv, t, R, root);
}

// The sweep of a cube table (scene/small_sweep.h SmallSweep::cube): every box
// other than the root [lo, hi] is a hull face of it, at most one per (axis,
// code).  A hull face's test reads nothing but the root's six products and its
// code (sweep_slab_hull), and the answer ORs the under words of the failing
// boxes, which does not depend on their order or on where their words come
// from.  So the walk needs no record: the six faces in the fixed order x lo,
// x hi, y lo, y hi, z lo, z hi with their axis and code known at compile time,
// under[f] the face's under word or 0 where the table has no such face (its
// boolean then ORs nothing), `all` the root's.  The same booleans from the same
// operands as sweep_cands<true>: the same leaf mask and *none bit for bit, NaNs
// of 0 * inf included.  No loop, no branch on the table, no load but the
// caller's lo, hi, under and all; the products are not detached from the root's
// test (sweep_root_detach): the compiler may keep the per-axis min/max.
PT_FN uint32_t sweep_cands_cube(v3 o, v3 inv, const float* lo, const float* hi, const uint32_t* under, uint32_t all,
                                bool* none) {
  const SweepBox r0 = {lo[0], lo[1], lo[2], 0.0f, hi[0], hi[1], hi[2], 0.0f};
  const SweepRootVals R = sweep_root_vals(o, inv, r0);
  const bool root = sweep_root_pass(R);
#if defined(__HIP_DEVICE_COMPILE__)
  *none = __builtin_amdgcn_ballot_w64(root) == 0;
#else
  *none = !root;
#endif
  if (*none) return 0u;
  uint32_t fail = root ? 0u : all;
  fail |= sweep_slab_hull<0>(R, 1u) ? 0u : under[0];
  fail |= sweep_slab_hull<0>(R, 2u) ? 0u : under[1];
  fail |= sweep_slab_hull<1>(R, 1u) ? 0u : under[2];
  fail |= sweep_slab_hull<1>(R, 2u) ? 0u : under[3];
  fail |= sweep_slab_hull<2>(R, 1u) ? 0u : under[4];
  fail |= sweep_slab_hull<2>(R, 2u) ? 0u : under[5];
  return all & ~fail;
}

// Closest hit over the leaf mask: leaves in visit order, triangle records by
// leaf (tris[3 * l ..]); *bt is the leaf index of the hit.
PT_FN void sweep_closest(v3 o, v3 d, uint32_t lm, const float4* tris, float* best, int* bt) {
  while (lm) {
    const int l = __builtin_ctz(lm);
    lm &= lm - 1u;
    const float4* T = tris + 3 * l;
    float t;
    if (tri_test(o, d, T[0], T[1], T[2], &t) && t < *best) {
      *best = t;
      *bt = l;
    }
  }
}

// Shadow query over the leaf mask: true iff some candidate the reference
// would accept (t < 1e30) has !(t >= limit).  "Any" does not depend on order.
PT_FN bool sweep_occluded(v3 o, v3 d, float limit, uint32_t lm, const float4* tris) {
  while (lm) {
    const int l = __builtin_ctz(lm);
    lm &= lm - 1u;
    const float4* T = tris + 3 * l;
    float t;
    if (tri_test(o, d, T[0], T[1], T[2], &t) && t < 1e30f && !(t >= limit)) return true;
  }
  return false;
}

}  // namespace ptd
