// cells_dev.h — a node of an encoded blob's first-layer tree, on the device: what cells.hip (a cell's path) and bundles.hip (a bundle's
// shared witness) share, so that the two openers cannot drift apart.
//
// The encoded blob keeps its tree leaves-first without the leaf hashes; a tree built at or above its skip threshold also lacks the two
// levels above the leaves.  A node of a level that is not stored is re-hashed from the evaluation: at most four leaves and three nodes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tree_dev.h"

namespace frieda {
namespace k {
namespace cellsdev {

__device__ __forceinline__ void leaf_at(const uint32_t* __restrict__ v, size_t cs, size_t j, uint32_t (&l)[4]) {
    l[0] = v[j], l[1] = v[cs + j], l[2] = v[2 * cs + j], l[3] = v[3 * cs + j];
}

// node `node` of level n - up (up = 0: a leaf hash, 1: the parent of two leaves, 2: of four) from the evaluation v[4][2^n]
__device__ __forceinline__ void node_from_eval(const uint32_t* __restrict__ v, uint32_t n, uint32_t up, size_t node, uint32_t (&h)[8]) {
    const size_t cs = (size_t)1 << n;
    uint32_t l[4], r[4];
    if (up == 0) {
        leaf_at(v, cs, node, l);
        treedev::leaf_hash<B2_LAT>(l[0], l[1], l[2], l[3], h);
        return;
    }
    if (up == 1) {
        leaf_at(v, cs, 2 * node, l);
        leaf_at(v, cs, 2 * node + 1, r);
        treedev::pair_node<B2_LAT>(l, r, h);
        return;
    }
    uint32_t hb[8], m[16];
    leaf_at(v, cs, 4 * node, l);
    leaf_at(v, cs, 4 * node + 1, r);
    treedev::pair_node<B2_LAT>(l, r, hb);
#pragma unroll
    for (int w = 0; w < 8; w++) m[w] = hb[w];
    leaf_at(v, cs, 4 * node + 2, l);
    leaf_at(v, cs, 4 * node + 3, r);
    treedev::pair_node<B2_LAT>(l, r, hb);
#pragma unroll
    for (int w = 0; w < 8; w++) m[8 + w] = hb[w];
    b2_merkle_block<B2_LAT>(m, h);
}

// Is level `level` of the tree of 2^n leaves in the encoded blob?
// Deliberately conservative: decommit.hip's rule, by the threshold alone.  A route that wrote levels n - 1, n - 2 although n >= skip_log
// (the fused small-domain launch never skips them) is re-hashed all the same — the words are equal, and no route is ever read where
// it did not write.
__device__ __forceinline__ bool stored(uint32_t n, uint32_t skip_log, uint32_t level) { return level < n && !(n >= skip_log && level + 2 >= n); }

// the 32 bytes of node `node` of level `level` (n - 2 <= level where the level is not stored) -> o[0], o[1]
__device__ __forceinline__ void open_node(const uint32_t* __restrict__ eval, const uint8_t* __restrict__ tree, uint32_t n, uint32_t skip_log, uint32_t level,
                                          size_t node, uint4* o) {
    if (stored(n, skip_log, level)) {
        const uint4* p = reinterpret_cast<const uint4*>(tree + treedev::layer_off(n, level) + 32 * node);
        const uint4 x = p[0], y = p[1];
        o[0] = x, o[1] = y;
    } else {
        uint32_t h[8];
        node_from_eval(eval, n, n - level, node, h);
        o[0] = make_uint4(h[0], h[1], h[2], h[3]);
        o[1] = make_uint4(h[4], h[5], h[6], h[7]);
    }
}

}  // namespace cellsdev
}  // namespace k
}  // namespace frieda
