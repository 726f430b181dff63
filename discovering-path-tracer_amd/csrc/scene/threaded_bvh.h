// The threaded node arrays of the exact walk (pt_device.h), built from the
// reference's node array once per scene upload.  Host only: no HIP, usable
// from tests.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

namespace pt {

// Threads the reference node array (n nodes, 8 floats each: {min.xyz, left}
// {max.xyz, right}, links float- or int-encoded): renumbers nodes in the order
// the reference's DFS visits them (right child first) and records, for each,
// the node visited after its subtree.  out: 8 floats per node, {min.xyz, skip}
// {max.xyz, tri} with skip and tri as int bits (bit 31 of skip: bounds bitwise
// the parent's).  Returns "" or why the array is not a tree of valid nodes.
std::string thread_bvh(const float* nodes, size_t n, bool int_bits, size_t n_tris, std::vector<float>* out);

// Drops internal nodes flagged as implied-hit from a threaded array: such a
// node does nothing but continue at k+1, so every link into it can point at
// the next kept node instead.  The kept nodes' visit sequence (and every slab
// and triangle test) is unchanged; only the pass-through visits disappear.
void collapse_implied(const std::vector<float>& full, std::vector<float>* out);

}  // namespace pt
