// The sweep table the LDS render kernel walks instead of the threaded node
// array of a tiny scene (scene/threaded_bvh.h builds that array;
// csrc/sweep_walk.h explains why the sweep returns the threaded walk's hits).
// Host only: no HIP, usable from tests.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

namespace pt {

// Largest table the sweep walk takes: one bit per leaf in a 32-bit mask
// (the walk's own, and each box's under word) and one per distinct box in a
// 64-bit need word (sweep_walk.h).  A tree of 32 leaves has 63 nodes, so the
// leaves bound both.
constexpr int kSweepMaxBoxes = 64;
constexpr int kSweepMaxLeaves = 32;

struct SmallSweep {
  // 8 floats per distinct box: {lo.xyz, under's bits} {hi.xyz, 0}.  Box 0 is the root's; then the general
  // boxes, then those flat (lo == hi bitwise) in x, in y, in z, each by its first flat axis.  The root's
  // last word holds the bits of: general | x-flat << 8 | y-flat << 16 | z-flat << 24 (counts, the root apart).
  // A flat box's last word holds the bits of its hull code: 1 (2) when its flat coordinate is bitwise the
  // root's lo (hi) on that axis and its other four extents are bitwise the root's (a face of the root box: its
  // slab values are the root's own, sweep_walk.h sweep_slab_hull), else 0
  std::vector<float> boxes;
  std::vector<uint64_t> need;    // per leaf in kept-node (visit) order: the box bits of the leaf and its ancestors
  std::vector<uint32_t> under;   // per box: the leaves whose need holds its bit (box 0: every leaf)
  std::vector<int32_t> slot;     // per leaf: its triangle slot
  int n_boxes = 0, n_leaves = 0;
  int n_hull = 0;                // boxes with a hull code
  // The cube table: no general box, every flat box has a hull code, at most one box per (axis, code) -- every box
  // other than the root is a face of it (the box, a cuboid, a cuboid without some face).  sweep_walk.h
  // sweep_cands_cube then needs no record: cube_under[] are the faces' under words in the fixed order x lo, x hi,
  // y lo, y hi, z lo, z hi (0: no such face), cube_all the root's
  bool cube = false;
  uint32_t cube_under[6] = {0, 0, 0, 0, 0, 0};
  uint32_t cube_all = 0;
  // The device table (sweep_walk.h SweepTable): boxes, need[] (32-bit words
  // for up to 32 boxes, else 64-bit) padded to whole float4s, slot[].
  // hull_codes false: the same table with every hull code 0.
  std::vector<float> pack(bool hull_codes = true) const;
};

// Builds the table from a collapsed threaded array (n_kept nodes, no padding
// node).  false (and an empty table) when the scene has more than max_boxes
// distinct boxes or max_leaves leaves.  hull_codes false leaves every flat
// box's code 0 (the walk then tests each with its own slab products).
bool build_small_sweep(const float* collapsed, size_t n_kept, SmallSweep* out, int max_boxes = kSweepMaxBoxes,
                       int max_leaves = kSweepMaxLeaves, bool hull_codes = true);

}  // namespace pt
