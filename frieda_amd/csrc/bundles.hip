// bundles.hip — cell bundles (gfx950): k cells of one blob under ONE shared Merkle witness instead of k separate paths.
//
// The witness of a bundle is stwo's hash witness (core/vcs/prover.rs MerkleProver::decommit / verifier.rs MerkleVerifier::verify) for
// the first-layer tree cut at level d = n - log_cell, with the bundle's strictly ascending cell indices as positions: the tables
// E_1, E_2, ..., E_d of queries_dev.h, E_s read at tree level d - s + 1, bottom-up and ascending within a level.  Its length depends
// on the indices alone, so the host computes every count and offset (bundles_host.h) and the kernels never size anything.
//
//   bundle_open_witness   one wave per (bundle, level s): the lanes run the emit rule over the bundle's indices 64 at a time; entry r of
//                         E_s (ballot + popcount rank) is written at level_base[b][s - 1] + r.  The node is read from the encoded tree
//                         where its level is stored and re-hashed from the evaluation where it is not: cells_dev.h, the code
//                         cells_open_paths runs.  (The values of the cells go through cells_open_values over the concatenated indices.)
//   bundle_walk<LEAF>     one wave per bundle, after cells_roots left every cell's subtree root (LEAF, log_cell 0: the lanes hash their
//                         leaves themselves).  The (position, hash) list sits in LDS, 36 bytes per cell, and is merged upward in chunks of
//                         64 and compacted in place level by level; a child that is not in the list comes from the witness at the prefix
//                         count of the missing children: walk_dev.h, the Merkle walk of verify_many_kernel.  The host has checked that
//                         the bundle's witness holds exactly the hashes its indices ask for, so the walk never reads past it; the wave
//                         ends with one status word.  Compressions are the plain form: one wave per bundle is latency-bound.
#include <hip/hip_runtime.h>

#include "cells_dev.h"
#include "kernels.h"
#include "queries_dev.h"
#include "tree_dev.h"
#include "walk_dev.h"

namespace frieda {
namespace k {

namespace {

constexpr int BO_THREADS = 256;  // four (bundle, level) waves per workgroup

__global__ __launch_bounds__(BO_THREADS) void bundle_open_witness_kernel(BundleOpenArgs a) {
    const uint32_t lane = threadIdx.x & 63;
    const unsigned long long lt_mask = (1ull << lane) - 1;
    const uint32_t depth = a.n - a.log_cell;
    const size_t wave = (size_t)blockIdx.x * (BO_THREADS / 64) + (threadIdx.x >> 6);
    if (wave >= (size_t)a.n_bundles * depth) return;  // (the whole wave leaves)
    const uint32_t b = (uint32_t)(wave / depth), s = (uint32_t)(wave - (size_t)b * depth) + 1;
    const BundleRow row = a.rows[b];
    const uint32_t* p = a.idx + row.first_cell;
    const uint32_t c = row.n_cells, level = depth - s + 1;
    uint4* out = a.out_witness + 2 * a.level_base[wave];
    uint32_t run = 0;
    for (uint32_t i0 = 0; i0 < c; i0 += 64) {
        uint32_t child = 0;
        const bool e = qdev::emit_of(p, c, i0 + lane, s, child);
        const unsigned long long m = __ballot(e);
        if (e) cellsdev::open_node(a.eval, a.tree, a.n, a.skip_log, level, child, out + 2 * (size_t)(run + (uint32_t)__popcll(m & lt_mask)));
        run += (uint32_t)__popcll(m);
    }
}

// LEAF (log_cell 0): lane i hashes the one leaf of cell i; else it takes the subtree root and the canonical flag cells_roots left
template <bool LEAF>
__global__ __launch_bounds__(64) void bundle_walk_kernel(BundleWalkArgs a) {
    extern __shared__ uint32_t lds[];
    const uint32_t lane = threadIdx.x, b = blockIdx.x;
    const BundleRow row = a.rows[b];
    const uint32_t c0 = row.n_cells;
    uint32_t* s_hp = lds;                 // node positions, ascending
    uint32_t* s_h = lds + a.max_cells;    // node hashes, 8 words each
    const uint32_t nh = (b + 1 < a.n_bundles ? a.rows[b + 1].first_hash : a.n_hashes) - row.first_hash;
    const uint32_t* hw = a.witness + 8 * (size_t)row.first_hash;
    bool bad = false;
    for (uint32_t i = lane; i < c0; i += 64) {
        const size_t cell = (size_t)row.first_cell + i;
        uint32_t h[8];
        if constexpr (LEAF) {
            const uint4 v = reinterpret_cast<const uint4*>(a.values)[cell];
            bad = bad || (v.x >= P31) | (v.y >= P31) | (v.z >= P31) | (v.w >= P31);
            treedev::leaf_hash<B2_LAT>(v.x, v.y, v.z, v.w, h);
        } else {
#pragma unroll
            for (int w = 0; w < 8; w++) h[w] = a.roots[(size_t)w * a.n_cells + cell];
            bad = bad || a.bad[cell] != 0;
        }
#pragma unroll
        for (int w = 0; w < 8; w++) s_h[8 * i + w] = h[w];
        s_hp[i] = a.idx[cell];
    }
    __syncthreads();
    uint32_t cn = c0, hbase = 0;
    for (uint32_t lv = a.n - a.log_cell; lv > 0; lv--) cn = walkdev::walk_level(s_hp, s_h, cn, lane, hw, nh, hbase, bad);
    // (the host checked the count: hbase == nh and cn == 1 restate it; a witness that ran short set `bad`)
    uint32_t diff = 0;  // (every lane compares the whole root: constant indices into the kernel arguments)
#pragma unroll
    for (int w = 0; w < 8; w++) diff |= s_h[w] ^ a.commitment[w];
    const bool reject = __any(bad) || diff != 0 || hbase != nh || cn != 1;
    if (lane == 0) a.status[b] = reject ? 0u : 1u;
}

}  // namespace

void bundle_open_witness(const Launch& L, const BundleOpenArgs& a) {
    const size_t waves = (size_t)a.n_bundles * (a.n - a.log_cell);
    if (!waves) return;
    // (no kernel-timer scope: every name the timer knows is tied to a row of tests/workspace_rows.py; the bundle launches have their
    // poisoned-workspace and caller's-stream runs in tests/test_gpu_bundles.py, and their times in profiles/r15_cell_bundles.txt)
    constexpr size_t per = BO_THREADS / 64;
    bundle_open_witness_kernel<<<(unsigned)((waves + per - 1) / per), BO_THREADS, 0, L.stream>>>(a);
}

size_t bundle_walk_lds_bytes(uint32_t max_cells) { return sizeof(uint32_t) * 9 * (size_t)max_cells; }

void bundle_walk(const Launch& L, const BundleWalkArgs& a) {
    if (!a.n_bundles) return;
    const size_t lds = bundle_walk_lds_bytes(a.max_cells);
    if (a.log_cell == 0)
        bundle_walk_kernel<true><<<a.n_bundles, 64, lds, L.stream>>>(a);
    else
        bundle_walk_kernel<false><<<a.n_bundles, 64, lds, L.stream>>>(a);
}

}  // namespace k
}  // namespace frieda
