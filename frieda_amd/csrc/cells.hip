// cells.hip — authenticated cells of an encoded blob: open (provider), verify and compact (sampling client).
//
// A cell is an aligned run of 2^c entries of the bit-reversed codeword, the same run of each of the 4 columns; its subtree root is node
// `cell` of level n - c of the first-layer tree, and its path the n - c siblings from there to the root.  Hashing is the prover's
// (blake2s.h / tree_dev.h): a leaf is the four column words of one position, a node its two children.
//
//   cells_open      per requested cell the four runs of 2^c words (16-byte copies from c = 2 on) and the siblings of its path, read from
//                   the encoded blob's tree where the level is stored and re-hashed from the evaluation where it is not (the leaf hashes
//                   never are; a tree built at or above its skip threshold also lacks the two levels above them): at most four leaves
//                   and three nodes, and only for c <= 2 (cells_dev.h: bundles.hip opens its shared witnesses by the same code).
//   cells_verify    two launches.  Roots: a lane per leaf pair (pair_node: two leaves and their parent), then an LDS reduction to the
//                   cell's subtree root; a workgroup covers 256 pairs, i.e. 2^(9 - c) cells (c = 10: one cell, two pairs per lane).  The
//                   canonical-word check runs there.  Walk: a lane per cell, n - c dependent compressions up the path, then the compare
//                   with the commitment.  The staged path image is level-major ([level][cell] hashes), so neighbouring lanes read
//                   neighbouring hashes; the roots pass between the launches word-planar for the same reason.  c = 0 has no first
//                   launch: the walk's lane hashes its one leaf itself.  (One fused launch would leave the walk with 2^(9 - c) busy lanes
//                   of 256 per workgroup; the compressions are the plain form — neither launch fills the chip at a client's cell counts.)
//   cells_gather    the accepted cells of a pass -> the pool the reconstruction reads (verify.hip's pairs_gather_kernel for cells).
//   *_blobs         the same kernels instantiated for cells of MANY blobs of one shape: open takes eval / tree / skip_log from the cell's row
//                   of a per-blob table, the walk its commitment from a table in device memory; cells_roots knows neither.
//   cells_stripe_*  a stripe = cell j of every blob of a block.  accept: a wave per stripe ANDs its cells' status words; gather: the fully
//                   accepted stripes -> the pool, which is the point reconstruction's layout at 4 * n_blobs columns.
#include <type_traits>

#include "cells_dev.h"
#include "kernels.h"
#include "tree_dev.h"

namespace frieda {
namespace k {

namespace {

constexpr int CL_THREADS = 256;

// The blob cell `cell` is opened from: the one of the call, or row bidx[cell] of the call's table (cell i is cell idx[i] of blob bidx[i]).
// The single-blob form reads the kernel arguments and nothing else.
struct BlobSource {
    const uint32_t* __restrict__ eval;
    const uint8_t* __restrict__ tree;
    uint32_t skip_log;
};
__device__ __forceinline__ BlobSource blob_of(const CellsOpenArgs& a, size_t) { return {a.eval, a.tree, a.skip_log}; }
__device__ __forceinline__ BlobSource blob_of(const CellsOpenBlobsArgs& a, size_t cell) {
    const CellsBlobRow& row = a.table[a.bidx[cell]];
    return {row.eval, row.tree, row.skip_log};
}

// out_values[cell][col][2^c]: VEC = 4 copies 16 bytes per thread (c >= 2: every run starts on a 16-byte boundary), VEC = 1 one word
template <int VEC, class Args>
__global__ __launch_bounds__(CL_THREADS) void cells_open_values_kernel(Args a) {
    const size_t e = (size_t)blockIdx.x * CL_THREADS + threadIdx.x;  // unit of VEC words of the output
    const uint32_t c = a.log_cell, lu = c - (VEC == 4 ? 2 : 0);      // log2 of the units of one run
    if (e >= ((size_t)a.n_cells * 4) << lu) return;
    const size_t run = e >> lu, cell = run >> 2;
    const uint32_t col = (uint32_t)(run & 3), u = (uint32_t)(e & (((size_t)1 << lu) - 1));
    const uint32_t* __restrict__ eval = blob_of(a, cell).eval;
    const size_t src = ((size_t)col << a.n) + ((size_t)a.idx[cell] << c) + (size_t)u * VEC;
    if constexpr (VEC == 4)
        reinterpret_cast<uint4*>(a.out_values)[e] = *reinterpret_cast<const uint4*>(eval + src);
    else
        a.out_values[e] = eval[src];
}

// out_paths[cell][s]: the sibling of the node above the cell at level n - c - s; the "stored" rule is evaluated for the cell's blob
template <class Args>
__global__ __launch_bounds__(CL_THREADS) void cells_open_paths_kernel(Args a) {
    const size_t e = (size_t)blockIdx.x * CL_THREADS + threadIdx.x;
    const uint32_t depth = a.n - a.log_cell;
    if (e >= (size_t)a.n_cells * depth) return;
    const size_t cell = e / depth;
    const uint32_t s = (uint32_t)(e - cell * depth), level = depth - s;
    const size_t node = (size_t)(a.idx[cell] >> s) ^ 1;
    const BlobSource b = blob_of(a, cell);
    uint4* o = a.out_paths + 2 * e;
    // stored levels are read, the others re-hashed from the evaluation (cells_dev.h: the rule bundles.hip opens by too)
    cellsdev::open_node(b.eval, b.tree, a.n, b.skip_log, level, node, o);
}

constexpr uint32_t CV_MAX_T = 512;  // pair nodes of a workgroup: 256, or the 512 of one cell of 2^10 entries

// subtree roots of the cells of 2^c >= 2 entries: roots[w][cell] (word-planar), bad[cell] != 0 iff a word is not a canonical M31
__global__ __launch_bounds__(CL_THREADS) void cells_roots_kernel(CellsVerifyArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t s_h[8 * (CV_MAX_T + 4)];
    __shared__ uint32_t s_bad[CL_THREADS];
    const uint32_t t = threadIdx.x, c = a.log_cell;
    const uint32_t lp = c - 1;                                  // log2 of the leaf pairs of a cell
    const uint32_t T = lp > 8 ? (1u << lp) : (uint32_t)CL_THREADS;  // pair nodes of this workgroup
    const uint32_t cpw = T >> lp, stride = T + 4;               // cells per workgroup
    const size_t cell0 = (size_t)blockIdx.x * cpw;
    s_bad[t] = 0;
    __syncthreads();
    for (uint32_t j = t; j < T; j += CL_THREADS) {
        const uint32_t lc = j >> lp, p = j & ((1u << lp) - 1);
        const size_t cell = cell0 + lc;
        if (cell < a.n_cells) {
            const uint32_t* v = a.values + ((cell * 4) << c) + 2 * p;
            uint32_t l[4], r[4];
            uint32_t bad = 0;
#pragma unroll
            for (int col = 0; col < 4; col++) {
                const uint2 x = *reinterpret_cast<const uint2*>(v + ((size_t)col << c));
                l[col] = x.x, r[col] = x.y;
                bad |= (x.x >= P31) | (x.y >= P31);
            }
            if (bad) atomicOr(&s_bad[lc], 1u);
            uint32_t h[8];
            treedev::pair_node<B2_LAT>(l, r, h);
            treedev::lds_put(s_h, stride, j, h);
        }
    }
    __syncthreads();
    // cells are aligned runs of 2^lp nodes: halving the whole array keeps them apart (the nodes of cells beyond n_cells are not
    // initialised and not used)
    for (uint32_t m = T >> 1; m >= cpw; m >>= 1) {
        uint32_t h[8];
        const bool live = t < m && cell0 + ((size_t)t * cpw) / m < a.n_cells;
        if (live) {
            uint32_t mm[16];
            treedev::lds_children(s_h, stride, t, mm);
            b2_merkle_block<B2_LAT>(mm, h);
        }
        __syncthreads();
        if (live) treedev::lds_put(s_h, stride, t, h);
        __syncthreads();
    }
    if (t < cpw && cell0 + t < a.n_cells) {
        const size_t cell = cell0 + t;
#pragma unroll
        for (int w = 0; w < 8; w++) a.roots[(size_t)w * a.n_cells + cell] = s_h[w * stride + t];
        a.bad[cell] = s_bad[t];
    }
}

// LEAF (c = 0): the lane hashes its cell's one leaf; else it takes the subtree root the first launch left.
// TABLE: lane `cell` compares with coms[bidx[cell]][8] in device memory; else with a.commitment, and bidx / coms are not read
template <bool LEAF, bool TABLE>
__global__ __launch_bounds__(CL_THREADS) void cells_walk_kernel(CellsVerifyArgs a, const uint32_t* __restrict__ bidx, const uint32_t* __restrict__ coms) {
    const size_t cell = (size_t)blockIdx.x * CL_THREADS + threadIdx.x;
    if (cell >= a.n_cells) return;
    uint32_t h[8], bad;
    if constexpr (LEAF) {
        const uint4 v = reinterpret_cast<const uint4*>(a.values)[cell];
        bad = (v.x >= P31) | (v.y >= P31) | (v.z >= P31) | (v.w >= P31);
        treedev::leaf_hash<B2_LAT>(v.x, v.y, v.z, v.w, h);
    } else {
#pragma unroll
        for (int w = 0; w < 8; w++) h[w] = a.roots[(size_t)w * a.n_cells + cell];
        bad = a.bad[cell];
    }
    const uint32_t idx = a.idx[cell], depth = a.n - a.log_cell;
#pragma unroll 1
    for (uint32_t s = 0; s < depth; s++) {
        const uint4* p = a.paths + 2 * ((size_t)s * a.n_cells + cell);
        const uint4 x = p[0], y = p[1];
        const uint32_t sib[8] = {x.x, x.y, x.z, x.w, y.x, y.y, y.z, y.w};
        const bool right = (idx >> s) & 1;  // this node is the right child
        uint32_t m[16];
#pragma unroll
        for (int w = 0; w < 8; w++) m[w] = right ? sib[w] : h[w], m[8 + w] = right ? h[w] : sib[w];
        b2_merkle_block<B2_LAT>(m, h);
    }
    uint32_t diff = bad;
    if constexpr (TABLE) {
        const uint4* want = reinterpret_cast<const uint4*>(coms + 8 * (size_t)bidx[cell]);
        const uint4 x = want[0], y = want[1];
        diff |= (h[0] ^ x.x) | (h[1] ^ x.y) | (h[2] ^ x.z) | (h[3] ^ x.w) | (h[4] ^ y.x) | (h[5] ^ y.y) | (h[6] ^ y.z) | (h[7] ^ y.w);
    } else {
#pragma unroll
        for (int w = 0; w < 8; w++) diff |= h[w] ^ a.commitment[w];
    }
    a.status[cell] = diff == 0 ? 1u : 0u;
}

// row r of the table: (slot of the pass, entry of the pool)
__global__ __launch_bounds__(CL_THREADS) void cells_gather_kernel(const uint32_t* __restrict__ tab, uint32_t n_rows, const uint32_t* __restrict__ values,
                                                                  const uint32_t* __restrict__ idx, uint32_t log_cell, uint32_t* __restrict__ pool_idx,
                                                                  uint32_t* __restrict__ pool_val) {
    const size_t e = (size_t)blockIdx.x * CL_THREADS + threadIdx.x;
    const uint32_t lw = log_cell + 2;  // log2 of the words of a cell
    if (e >= (size_t)n_rows << lw) return;
    const size_t row = e >> lw, w = e & (((size_t)1 << lw) - 1);
    const size_t src = tab[2 * row], dst = tab[2 * row + 1];
    pool_val[(dst << lw) + w] = values[(src << lw) + w];
    if (w == 0) pool_idx[dst] = idx[src];
}

// a wave per stripe: its lanes AND the status words of the stripe's n_blobs cells (any n_blobs: the lanes stride over them), one vote
__global__ __launch_bounds__(CL_THREADS) void cells_stripe_accept_kernel(const uint32_t* __restrict__ status, uint32_t n_stripes, uint32_t n_blobs,
                                                                         uint32_t* __restrict__ accept) {
    const uint32_t lane = threadIdx.x & 63;
    const size_t stripe = (size_t)blockIdx.x * (CL_THREADS / 64) + (threadIdx.x >> 6);
    if (stripe >= n_stripes) return;  // (the whole wave leaves)
    const uint32_t* st = status + stripe * n_blobs;
    bool ok = true;
    for (uint32_t b = lane; b < n_blobs; b += 64) ok = ok && st[b] == 1u;
    const bool all_ok = __all(ok);
    if (lane == 0) accept[stripe] = all_ok ? 1u : 0u;
}

// row r of the table: (stripe of the pass, entry of the pool); 16-byte copies (a cell is at least four words)
__global__ __launch_bounds__(CL_THREADS) void cells_stripe_gather_kernel(const uint32_t* __restrict__ tab, uint32_t n_rows, const uint32_t* __restrict__ values,
                                                                         const uint32_t* __restrict__ idx, uint32_t idx_stride, uint32_t n_blobs,
                                                                         uint32_t log_cell, uint32_t* __restrict__ pool_idx, uint32_t* __restrict__ pool_val) {
    const size_t e = (size_t)blockIdx.x * CL_THREADS + threadIdx.x;
    const size_t units = (size_t)n_blobs << log_cell;  // 16-byte units of a stripe
    if (e >= (size_t)n_rows * units) return;
    const size_t row = e / units, u = e - row * units;
    const size_t src = tab[2 * row], dst = tab[2 * row + 1];
    reinterpret_cast<uint4*>(pool_val)[dst * units + u] = reinterpret_cast<const uint4*>(values)[src * units + u];
    if (u == 0) pool_idx[dst] = idx[src * idx_stride];
}

unsigned blocks_for(size_t units) { return (unsigned)((units + CL_THREADS - 1) / CL_THREADS); }

template <class Args>
void open_values_launch(const Launch& L, const Args& a) {
    constexpr bool TABLE = std::is_same<Args, CellsOpenBlobsArgs>::value;
    if (!a.n_cells) return;
    Scope scope(L, TABLE ? "cells_open_blobs_values" : "cells_open_values", 32.0 * (double)(((size_t)a.n_cells) << a.log_cell));
    if (a.log_cell >= 2)
        cells_open_values_kernel<4><<<blocks_for(((size_t)a.n_cells * 4) << (a.log_cell - 2)), CL_THREADS, 0, L.stream>>>(a);
    else
        cells_open_values_kernel<1><<<blocks_for(((size_t)a.n_cells * 4) << a.log_cell), CL_THREADS, 0, L.stream>>>(a);
}

template <class Args>
void open_launch(const Launch& L, const Args& a) {
    constexpr bool TABLE = std::is_same<Args, CellsOpenBlobsArgs>::value;
    if (!a.n_cells) return;
    open_values_launch(L, a);
    if (a.n > a.log_cell) {
        Scope scope(L, TABLE ? "cells_open_blobs_paths" : "cells_open_paths", 64.0 * (double)a.n_cells * (a.n - a.log_cell));
        cells_open_paths_kernel<<<blocks_for((size_t)a.n_cells * (a.n - a.log_cell)), CL_THREADS, 0, L.stream>>>(a);
    }
}

void roots_launch(const Launch& L, const CellsVerifyArgs& a) {
    Scope scope(L, "cells_roots", 0.0);  // (knows neither index nor commitment)
    const uint32_t cpw = a.log_cell >= 10 ? 1u : 1u << (9 - a.log_cell);
    cells_roots_kernel<<<(a.n_cells + cpw - 1) / cpw, CL_THREADS, 0, L.stream>>>(a);
}

template <bool TABLE>
void verify_launch(const Launch& L, const CellsVerifyArgs& a, const uint32_t* d_bidx, const uint32_t* d_commitments) {
    if (!a.n_cells) return;
    if (a.log_cell == 0) {
        Scope scope(L, TABLE ? "cells_walk_blobs" : "cells_walk", 0.0);
        cells_walk_kernel<true, TABLE><<<blocks_for(a.n_cells), CL_THREADS, 0, L.stream>>>(a, d_bidx, d_commitments);
        return;
    }
    roots_launch(L, a);
    Scope scope(L, TABLE ? "cells_walk_blobs" : "cells_walk", 0.0);
    cells_walk_kernel<false, TABLE><<<blocks_for(a.n_cells), CL_THREADS, 0, L.stream>>>(a, d_bidx, d_commitments);
}

}  // namespace

void cells_open(const Launch& L, const CellsOpenArgs& a) { open_launch(L, a); }
void cells_open_values(const Launch& L, const CellsOpenArgs& a) { open_values_launch(L, a); }
void cells_open_blobs(const Launch& L, const CellsOpenBlobsArgs& a) { open_launch(L, a); }
void cells_open_blobs_values(const Launch& L, const CellsOpenBlobsArgs& a) { open_values_launch(L, a); }

void cells_verify(const Launch& L, const CellsVerifyArgs& a) { verify_launch<false>(L, a, nullptr, nullptr); }
void cells_roots(const Launch& L, const CellsVerifyArgs& a) {
    if (a.n_cells && a.log_cell) roots_launch(L, a);
}
void cells_verify_blobs(const Launch& L, const CellsVerifyArgs& a, const uint32_t* d_bidx, const uint32_t* d_commitments) {
    verify_launch<true>(L, a, d_bidx, d_commitments);
}

void cells_gather(const Launch& L, const uint32_t* d_tab, uint32_t n_rows, const uint32_t* d_values, const uint32_t* d_idx, uint32_t log_cell,
                  uint32_t* d_pool_idx, uint32_t* d_pool_val) {
    if (!n_rows) return;
    Scope scope(L, "cells_gather", 0.0);
    cells_gather_kernel<<<blocks_for((size_t)n_rows << (log_cell + 2)), CL_THREADS, 0, L.stream>>>(d_tab, n_rows, d_values, d_idx, log_cell, d_pool_idx,
                                                                                                  d_pool_val);
}

void cells_stripe_accept(const Launch& L, const uint32_t* d_status, uint32_t n_stripes, uint32_t n_blobs, uint32_t* d_accept) {
    if (!n_stripes) return;
    Scope scope(L, "cells_stripe_accept", 0.0);
    const uint32_t per = CL_THREADS / 64;
    cells_stripe_accept_kernel<<<(n_stripes + per - 1) / per, CL_THREADS, 0, L.stream>>>(d_status, n_stripes, n_blobs, d_accept);
}

void cells_stripe_gather(const Launch& L, const uint32_t* d_tab, uint32_t n_rows, const uint32_t* d_values, const uint32_t* d_idx, uint32_t idx_stride,
                         uint32_t n_blobs, uint32_t log_cell, uint32_t* d_pool_idx, uint32_t* d_pool_val) {
    if (!n_rows) return;
    Scope scope(L, "cells_stripe_gather", 0.0);
    cells_stripe_gather_kernel<<<blocks_for((size_t)n_rows * ((size_t)n_blobs << log_cell)), CL_THREADS, 0, L.stream>>>(d_tab, n_rows, d_values, d_idx, idx_stride,
                                                                                                                      n_blobs, log_cell, d_pool_idx, d_pool_val);
}

}  // namespace k
}  // namespace frieda
