// stripe_bundles.hip — stripe bundles (gfx950): k stripes of a block of n_blobs blobs (a stripe is cell j of every blob) under ONE shared
// Merkle witness per blob instead of k separate paths per blob.
//
// Every blob of a stripe bundle has the same indices, so what depends on the indices alone — the witness length W, the per-level
// offsets, the malformed rule, the whole merge structure — is computed once per bundle (bundles_host.h), not once per (bundle, blob).
// Blob j's piece of a bundle's witness is byte for byte the witness bundles.hip opens for that blob on the same indices: the pieces
// of a bundle lie back to back, W hashes each.  The n_blobs walks of a bundle are independent waves.
//
//   stripe_bundle_open_witness   one wave per (bundle, blob, level s): the lanes run the emit rule over the bundle's indices 64 at a time;
//                                entry r of E_s (ballot + popcount rank) is written at level_base[b][s - 1] + j * W + r.  eval, tree and
//                                skip_log come from blob j's row of the table the block opener uploads; the node is read or re-hashed by
//                                cells_dev.h.  (The values go through cells_open_blobs_values over (stripe, blob) pairs.)
//   stripe_bundle_walk<LEAF>     one wave per (bundle, blob), after cells_roots ran unchanged over all cells of the pass: stripe i of the
//                                bundle, blob j is pass cell (first_stripe + i) * n_blobs + j (LEAF, log_cell 0: the lane hashes its leaf
//                                itself).  Positions come from the shared index list; the list is merged upward by walk_dev.h as in
//                                bundle_walk; the root is compared with commitments[j] in device memory.  One status word per
//                                (bundle, blob).  Compressions are the plain form.
#include <hip/hip_runtime.h>

#include "cells_dev.h"
#include "kernels.h"
#include "queries_dev.h"
#include "tree_dev.h"
#include "walk_dev.h"

namespace frieda {
namespace k {

namespace {

constexpr int SO_THREADS = 256;  // four (bundle, blob, level) waves per workgroup

// the hashes of one blob's piece of bundle b: to the next row's first hash, or to the end of the per-blob count
__device__ __forceinline__ uint32_t piece_hashes(const BundleRow* rows, uint32_t b, uint32_t n_bundles, uint32_t n_hashes) {
    return (b + 1 < n_bundles ? rows[b + 1].first_hash : n_hashes) - rows[b].first_hash;
}

__global__ __launch_bounds__(SO_THREADS) void stripe_bundle_open_witness_kernel(StripeBundleOpenArgs a) {
    const uint32_t lane = threadIdx.x & 63;
    const unsigned long long lt_mask = (1ull << lane) - 1;
    const uint32_t depth = a.n - a.log_cell;
    // (the wave's number within the workgroup is the same in all its lanes: said so, the rows below come by scalar loads and the
    // stored-or-re-hashed choice is one branch for the wave)
    const size_t wave = (size_t)blockIdx.x * (SO_THREADS / 64) + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (wave >= (size_t)a.n_bundles * a.n_blobs * depth) return;  // (the whole wave leaves)
    const size_t pair = wave / depth;                              // (bundle, blob)
    const uint32_t s = (uint32_t)(wave - pair * depth) + 1;
    const uint32_t b = (uint32_t)(pair / a.n_blobs), j = (uint32_t)(pair - (size_t)b * a.n_blobs);
    const BundleRow row = a.rows[b];
    const CellsBlobRow blob = a.table[j];
    const uint32_t* p = a.idx + row.first_cell;
    const uint32_t c = row.n_cells, level = depth - s + 1;
    const size_t base = (size_t)a.level_base[(size_t)b * depth + (s - 1)] + (size_t)j * piece_hashes(a.rows, b, a.n_bundles, a.n_hashes);
    uint4* out = a.out_witness + 2 * base;
    uint32_t run = 0;
    for (uint32_t i0 = 0; i0 < c; i0 += 64) {
        uint32_t child = 0;
        const bool e = qdev::emit_of(p, c, i0 + lane, s, child);
        const unsigned long long m = __ballot(e);
        if (e) cellsdev::open_node(blob.eval, blob.tree, a.n, blob.skip_log, level, child, out + 2 * (size_t)(run + (uint32_t)__popcll(m & lt_mask)));
        run += (uint32_t)__popcll(m);
    }
}

// LEAF (log_cell 0): lane i hashes blob j's leaf of stripe i; else it takes the subtree root and the canonical flag cells_roots left
template <bool LEAF>
__global__ __launch_bounds__(64) void stripe_bundle_walk_kernel(StripeBundleWalkArgs a) {
    extern __shared__ uint32_t lds[];
    const uint32_t lane = threadIdx.x;
    const uint32_t b = blockIdx.x / a.n_blobs, j = blockIdx.x - b * a.n_blobs;
    const BundleRow row = a.rows[b];
    const uint32_t c0 = row.n_cells;
    uint32_t* s_hp = lds;               // node positions, ascending
    uint32_t* s_h = lds + a.max_cells;  // node hashes, 8 words each
    const uint32_t nh = piece_hashes(a.rows, b, a.n_bundles, a.n_hashes);
    const uint32_t* hw = a.witness + 8 * ((size_t)a.n_blobs * row.first_hash + (size_t)j * nh);
    bool bad = false;
    for (uint32_t i = lane; i < c0; i += 64) {
        const size_t cell = ((size_t)row.first_cell + i) * a.n_blobs + j;
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
        s_hp[i] = a.idx[row.first_cell + i];
    }
    __syncthreads();
    uint32_t cn = c0, hbase = 0;
    for (uint32_t lv = a.n - a.log_cell; lv > 0; lv--) cn = walkdev::walk_level(s_hp, s_h, cn, lane, hw, nh, hbase, bad);
    // (the host checked the count: hbase == nh and cn == 1 restate it; a witness that ran short set `bad`)
    const uint32_t* want = a.commitments + 8 * (size_t)j;
    uint32_t diff = 0;  // (every lane compares the whole root: the address is the same in all of them)
#pragma unroll
    for (int w = 0; w < 8; w++) diff |= s_h[w] ^ want[w];
    const bool reject = __any(bad) || diff != 0 || hbase != nh || cn != 1;
    if (lane == 0) a.status[blockIdx.x] = reject ? 0u : 1u;
}

}  // namespace

void stripe_bundle_open_witness(const Launch& L, const StripeBundleOpenArgs& a) {
    const size_t waves = (size_t)a.n_bundles * a.n_blobs * (a.n - a.log_cell);
    if (!waves) return;
    // (no kernel-timer scope, as in bundles.hip: every name the timer knows is tied to a row of tests/workspace_rows.py; the
    // poisoned-workspace and caller's-stream runs are in tests/test_gpu_stripe_bundles.py, the times in profiles/r16_stripe_bundles.txt)
    constexpr size_t per = SO_THREADS / 64;
    stripe_bundle_open_witness_kernel<<<(unsigned)((waves + per - 1) / per), SO_THREADS, 0, L.stream>>>(a);
}

void stripe_bundle_walk(const Launch& L, const StripeBundleWalkArgs& a) {
    if (!a.n_bundles || !a.n_blobs) return;
    const size_t lds = bundle_walk_lds_bytes(a.max_cells);
    const unsigned grid = a.n_bundles * a.n_blobs;  // (the caller keeps the product of a pass below 2^31)
    if (a.log_cell == 0)
        stripe_bundle_walk_kernel<true><<<grid, 64, lds, L.stream>>>(a);
    else
        stripe_bundle_walk_kernel<false><<<grid, 64, lds, L.stream>>>(a);
}

}  // namespace k
}  // namespace frieda
