// opening.hip — Level B openings on the device (gfx950): the batched Column::at (frieda_dev_gather*) and MerkleProver::decommit
// (stwo core/vcs/prover.rs) of a tree whose columns all sit on the leaf layer (frieda_merkle_decommit*), for arbitrary trees and
// arbitrary position lists.  decommit.hip does the same work inside a proof, for that proof's own trees and at most 1024 queries.
//
// Decommitment.  stwo's hash witness for the strictly ascending positions p is the E_s tables of queries_dev.h, E_1, E_2, ..., E_L, with
// E_s read at tree layer L - s + 1; every level needs only p, so all levels are computed independently:
//   small lists (n <= OPEN_SMALL_MAX): one workgroup, E tables in LDS, one launch;
//   otherwise: count (block of 1024 positions x level; ballot + popcount) -> one-workgroup exclusive scan in level-major order (stwo's
//   output order) -> emit (the same ballots, hashes gathered straight into the output; level 0 gathers the column values).
// Both routes write identical bytes.  Out-of-order, repeated or out-of-range positions (possible only through the device form: the
// host form refuses them before launching) set the count word to OPEN_BAD_COUNT and nothing else is written.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "queries_dev.h"

namespace frieda {
namespace k {

namespace {

constexpr int OP_THREADS = 256;
constexpr uint32_t OP_GRID_CAP = 8192;  // grid-stride beyond this many workgroups
constexpr uint32_t OPEN_BLOCK = 1024;   // positions per workgroup of the multi-block route (4 waves x 4 rounds of 64)
constexpr int SCAN_THREADS = 1024;
// LDS slots of the single-workgroup route: sum over s of min(n, 2^(L - s)) <= 19 * 512 + 511 for n <= 512, L <= 28
constexpr uint32_t OPEN_SMALL_E_CAP = 10240;
static_assert(OPEN_SMALL_MAX_LIMIT == 512, "OPEN_SMALL_E_CAP is sized for 512 positions");

uint32_t grid_for(size_t work) {
    const size_t g = (work + OP_THREADS - 1) / OP_THREADS;
    return (uint32_t)(g < OP_GRID_CAP ? (g ? g : 1) : OP_GRID_CAP);
}

// ---- gather ----
// SecureColumn rows: four loads, one 16-byte store per index
__global__ __launch_bounds__(OP_THREADS) void gather_rows4_kernel(const uint32_t* __restrict__ cols, size_t stride,
                                                                  const uint64_t* __restrict__ idx, size_t n, uint4* __restrict__ out) {
    for (size_t t = (size_t)blockIdx.x * OP_THREADS + threadIdx.x; t < n; t += (size_t)gridDim.x * OP_THREADS) {
        const uint64_t i = idx[t];
        uint4 v = make_uint4(OPEN_BAD_WORD, OPEN_BAD_WORD, OPEN_BAD_WORD, OPEN_BAD_WORD);
        if (i < stride) v = make_uint4(cols[i], cols[stride + i], cols[2 * stride + i], cols[3 * stride + i]);
        out[t] = v;
    }
}

// any ncols (and unaligned outputs): one thread per output word
__global__ __launch_bounds__(OP_THREADS) void gather_rows_kernel(const uint32_t* __restrict__ cols, size_t stride, uint32_t ncols,
                                                                 const uint64_t* __restrict__ idx, size_t n, uint32_t* __restrict__ out) {
    const size_t total = n * ncols;
    for (size_t t = (size_t)blockIdx.x * OP_THREADS + threadIdx.x; t < total; t += (size_t)gridDim.x * OP_THREADS) {
        const size_t r = t / ncols, c = t - r * ncols;
        const uint64_t i = idx[r];
        out[t] = i < stride ? cols[c * stride + i] : OPEN_BAD_WORD;
    }
}

// 32-byte hashes: one thread per 16-byte half
__global__ __launch_bounds__(OP_THREADS) void gather_hashes_kernel(const uint4* __restrict__ layer, size_t len,
                                                                   const uint64_t* __restrict__ idx, size_t n, uint4* __restrict__ out) {
    for (size_t t = (size_t)blockIdx.x * OP_THREADS + threadIdx.x; t < 2 * n; t += (size_t)gridDim.x * OP_THREADS) {
        const uint64_t i = idx[t >> 1];
        out[t] = i < len ? layer[2 * i + (t & 1)] : make_uint4(OPEN_BAD_WORD, OPEN_BAD_WORD, OPEN_BAD_WORD, OPEN_BAD_WORD);
    }
}

// ---- decommitment ----
__device__ __forceinline__ bool bad_at(const uint32_t* p, uint32_t i, uint32_t log_size) {
    return (p[i] >> log_size) != 0 || (i > 0 && p[i - 1] >= p[i]);
}

// the layer a level's hashes are read from, selected with constant indices (a run-time index into the kernel arguments would
// copy them to scratch)
__device__ __forceinline__ const uint4* layer_of(const OpenTree& tr, uint32_t layer_log) {
    const uint8_t* l = nullptr;
#pragma unroll
    for (uint32_t j = 0; j <= OPEN_MAX_LOG; j++)
        if (j == layer_log) l = tr.layers[j];
    return reinterpret_cast<const uint4*>(l);
}

// values[i][c] = column c at position i
__device__ __forceinline__ void gather_values(const DecommitOpen& a, const uint32_t* p, uint32_t i0, uint32_t i1, uint32_t t, uint32_t nt) {
    const uint32_t nc = a.ncols;
    for (size_t e = (size_t)i0 * nc + t; e < (size_t)i1 * nc; e += nt) {
        const size_t i = e / nc, c = e - i * nc;
        a.values[e] = a.cols[c * a.stride + p[i]];
    }
}

// single workgroup: n <= OPEN_SMALL_MAX_LIMIT positions, every level's E table in LDS
__global__ __launch_bounds__(OP_THREADS) void decommit_small_kernel(DecommitOpen a) {
    __shared__ uint32_t s_p[OPEN_SMALL_MAX_LIMIT];
    __shared__ uint32_t s_E[OPEN_SMALL_E_CAP];
    __shared__ uint32_t s_slot[OPEN_MAX_LOG + 2];  // slot of E_s in s_E
    __shared__ uint32_t s_cnt[OPEN_MAX_LOG + 2];   // |E_s|
    __shared__ uint32_t s_base[OPEN_MAX_LOG + 2];  // |E_1| + ... + |E_{s-1}|
    __shared__ const uint4* s_layer[OPEN_MAX_LOG + 1];
    const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const uint32_t n = a.n, L = a.log_size;
    bool bad = false;
    for (uint32_t i = t; i < n; i += OP_THREADS) {
        s_p[i] = a.pos[i];
        bad = bad || bad_at(a.pos, i, L);
    }
#pragma unroll
    for (uint32_t j = 0; j <= OPEN_MAX_LOG; j++)
        if (t == j) s_layer[j] = reinterpret_cast<const uint4*>(a.tree.layers[j]);
    if (t == 0) {
        uint32_t off = 0;
        for (uint32_t s = 1; s <= L; s++) {
            s_slot[s] = off;
            const uint32_t nodes = 1u << (L - s);  // |E_s| <= |U_s| <= min(n, nodes)
            off += n < nodes ? n : nodes;
        }
    }
    if (__syncthreads_or(bad)) {
        if (t == 0) *a.count = OPEN_BAD_COUNT;
        return;
    }
    for (uint32_t s = 1 + wave; s <= L; s += OP_THREADS / 64) {
        const uint32_t c = qdev::build_level(s_p, n, s, s_E + s_slot[s]);
        if (lane == 0) s_cnt[s] = c;
    }
    __syncthreads();
    if (t == 0) {
        uint32_t acc = 0;
        for (uint32_t s = 1; s <= L; s++) {
            s_base[s] = acc;
            acc += s_cnt[s];
        }
        s_base[L + 1] = acc;
        *a.count = acc;
    }
    __syncthreads();
    const uint32_t total = s_base[L + 1];
    if (a.ncols) gather_values(a, s_p, 0, n, t, OP_THREADS);
    for (uint32_t e = t; e < 2 * total; e += OP_THREADS) {
        const uint32_t o = e >> 1, half = e & 1;
        if (o >= a.max_hashes) break;
        uint32_t s = 1;
        while (s < L && s_base[s + 1] <= o) s++;
        const uint32_t child = s_E[s_slot[s] + (o - s_base[s])];
        a.hashes[e] = s_layer[L - s + 1][2 * (size_t)child + half];
    }
}

// multi-block route, step 1: |E_s| restricted to each block of OPEN_BLOCK positions -> counts[(s - 1) * nblk + blk]; the level-1
// workgroups also record whether their block is well formed (bad[blk])
__global__ __launch_bounds__(OP_THREADS) void decommit_count_kernel(DecommitOpen a, uint32_t* __restrict__ counts, uint32_t* __restrict__ bad) {
    __shared__ uint32_t s_w[OP_THREADS / 64];
    __shared__ uint32_t s_bad;
    const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const uint32_t blk = blockIdx.x, nblk = gridDim.x, s = blockIdx.y + 1;
    const uint32_t i0 = blk * OPEN_BLOCK + wave * (OPEN_BLOCK / 4);
    if (t == 0) s_bad = 0;
    __syncthreads();
    uint32_t c = 0;
    bool b = false;
#pragma unroll
    for (uint32_t r = 0; r < OPEN_BLOCK / 4 / 64; r++) {
        const uint32_t i = i0 + r * 64 + lane;
        uint32_t child;
        c += (uint32_t)__popcll(__ballot(qdev::emit_of(a.pos, a.n, i, s, child)));
        if (s == 1 && i < a.n) b = b || bad_at(a.pos, i, a.log_size);
    }
    if (lane == 0) s_w[wave] = c;
    if (b) s_bad = 1;
    __syncthreads();
    if (t == 0) {
        uint32_t sum = 0;
        for (int w = 0; w < OP_THREADS / 64; w++) sum += s_w[w];
        counts[(size_t)(s - 1) * nblk + blk] = sum;
        if (s == 1) bad[blk] = s_bad;
    }
}

// step 2: exclusive scan of counts[m] in place (one workgroup, tiles of 4096); the total, or OPEN_BAD_COUNT, to *count
__global__ __launch_bounds__(SCAN_THREADS) void decommit_scan_kernel(uint32_t* __restrict__ counts, uint32_t m, const uint32_t* __restrict__ bad,
                                                                     uint32_t nblk, uint32_t* __restrict__ count) {
    __shared__ uint32_t s_w[SCAN_THREADS / 64];
    __shared__ uint32_t s_tile;
    const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6;
    int b = 0;
    for (uint32_t i = t; i < nblk; i += SCAN_THREADS) b |= bad[i] ? 1 : 0;
    if (__syncthreads_or(b)) {
        if (t == 0) *count = OPEN_BAD_COUNT;
        return;
    }
    uint32_t carry = 0;
    for (uint32_t base = 0; base < m; base += 4 * SCAN_THREADS) {
        const uint32_t j = base + 4 * t;
        uint32_t v[4];
#pragma unroll
        for (int q = 0; q < 4; q++) v[q] = j + q < m ? counts[j + q] : 0u;
        const uint32_t sum = v[0] + v[1] + v[2] + v[3];
        uint32_t inc = sum;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t o = (uint32_t)__shfl_up((int)inc, off);
            if ((int)lane >= off) inc += o;
        }
        if (lane == 63) s_w[wave] = inc;
        __syncthreads();
        if (wave == 0) {
            const uint32_t w = lane < SCAN_THREADS / 64 ? s_w[lane] : 0u;
            uint32_t winc = w;
#pragma unroll
            for (int off = 1; off < SCAN_THREADS / 64; off <<= 1) {
                const uint32_t o = (uint32_t)__shfl_up((int)winc, off);
                if ((int)lane >= off) winc += o;
            }
            if (lane < SCAN_THREADS / 64) s_w[lane] = winc - w;
            if (lane == SCAN_THREADS / 64 - 1) s_tile = winc;
        }
        __syncthreads();
        uint32_t ex = carry + s_w[wave] + inc - sum;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            if (j + q < m) counts[j + q] = ex;
            ex += v[q];
        }
        carry += s_tile;
        __syncthreads();  // s_w / s_tile are rewritten by the next tile
    }
    if (t == 0) *count = carry;
}

// step 3: blockIdx.y = s >= 1: the hashes of E_s inside this block of positions, at offsets[(s - 1) * nblk + blk] + their rank;
// blockIdx.y = 0: the column values of the block's positions
__global__ __launch_bounds__(OP_THREADS) void decommit_emit_kernel(DecommitOpen a, const uint32_t* __restrict__ offsets) {
    __shared__ uint32_t s_w[OP_THREADS / 64];
    if (*a.count == OPEN_BAD_COUNT) return;
    const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const uint32_t blk = blockIdx.x, nblk = gridDim.x, s = blockIdx.y;
    const uint32_t n = a.n;
    if (s == 0) {
        if (a.ncols) {
            const uint32_t e = blk * OPEN_BLOCK + OPEN_BLOCK;
            gather_values(a, a.pos, blk * OPEN_BLOCK, e < n ? e : n, t, OP_THREADS);
        }
        return;
    }
    const unsigned long long lt_mask = (1ull << lane) - 1;
    const uint32_t i0 = blk * OPEN_BLOCK + wave * (OPEN_BLOCK / 4);
    unsigned long long m[OPEN_BLOCK / 4 / 64];
    uint32_t ch[OPEN_BLOCK / 4 / 64];
    uint32_t c = 0;
#pragma unroll
    for (uint32_t r = 0; r < OPEN_BLOCK / 4 / 64; r++) {
        ch[r] = 0;
        m[r] = __ballot(qdev::emit_of(a.pos, n, i0 + r * 64 + lane, s, ch[r]));
        c += (uint32_t)__popcll(m[r]);
    }
    if (lane == 0) s_w[wave] = c;
    __syncthreads();
    uint32_t o = offsets[(size_t)(s - 1) * nblk + blk];
    for (uint32_t w = 0; w < wave; w++) o += s_w[w];
    const uint4* layer = layer_of(a.tree, a.log_size - s + 1);
#pragma unroll
    for (uint32_t r = 0; r < OPEN_BLOCK / 4 / 64; r++) {
        if ((m[r] >> lane) & 1ull) {
            const size_t q = (size_t)o + (uint32_t)__popcll(m[r] & lt_mask);
            if (q < a.max_hashes) {
                const uint4 lo = layer[2 * (size_t)ch[r]], hi = layer[2 * (size_t)ch[r] + 1];
                a.hashes[2 * q] = lo;
                a.hashes[2 * q + 1] = hi;
            }
        }
        o += (uint32_t)__popcll(m[r]);
    }
}

}  // namespace

void gather_rows(const Launch& L, const uint32_t* d_cols, size_t stride, uint32_t ncols, const uint64_t* d_idx, size_t n, uint32_t* d_out) {
    if (n == 0 || ncols == 0) return;
    Scope scope(L, "gather_rows", 12.0 * n * ncols);
    if (ncols == 4 && (reinterpret_cast<uintptr_t>(d_out) & 15) == 0)
        gather_rows4_kernel<<<grid_for(n), OP_THREADS, 0, L.stream>>>(d_cols, stride, d_idx, n, reinterpret_cast<uint4*>(d_out));
    else
        gather_rows_kernel<<<grid_for(n * ncols), OP_THREADS, 0, L.stream>>>(d_cols, stride, ncols, d_idx, n, d_out);
}

void gather_hashes(const Launch& L, const uint8_t* d_layer, size_t layer_len, const uint64_t* d_idx, size_t n, uint8_t* d_out) {
    if (n == 0) return;
    Scope scope(L, "gather_hashes", 72.0 * n);
    gather_hashes_kernel<<<grid_for(2 * n), OP_THREADS, 0, L.stream>>>(reinterpret_cast<const uint4*>(d_layer), layer_len, d_idx, n,
                                                                        reinterpret_cast<uint4*>(d_out));
}

uint64_t decommit_hash_bound(uint64_t n_pos, uint32_t log_size) {
    uint64_t b = 0;
    for (uint32_t s = 1; s <= log_size; s++) {
        const uint64_t nodes = (uint64_t)1 << (log_size - s);
        b += n_pos < nodes ? n_pos : nodes;
    }
    return b;
}

bool decommit_small_route(uint32_t n_pos, uint32_t log_size, uint32_t small_max) { return log_size == 0 || n_pos <= small_max; }

size_t decommit_scratch_bytes(uint32_t n_pos, uint32_t log_size) {
    const size_t nblk = (n_pos + OPEN_BLOCK - 1) / OPEN_BLOCK;
    return sizeof(uint32_t) * nblk * (log_size + 1);
}

void merkle_decommit(const Launch& L, const DecommitOpen& a, uint32_t small_max, void* d_scratch) {
    if (decommit_small_route(a.n, a.log_size, small_max)) {
        Scope scope(L, "decommit_small", 0.0);
        decommit_small_kernel<<<1, OP_THREADS, 0, L.stream>>>(a);
        return;
    }
    const uint32_t nblk = (a.n + OPEN_BLOCK - 1) / OPEN_BLOCK;
    uint32_t* counts = static_cast<uint32_t*>(d_scratch);
    uint32_t* bad = counts + (size_t)nblk * a.log_size;
    {
        Scope scope(L, "decommit_count", 4.0 * a.n * a.log_size);
        decommit_count_kernel<<<dim3(nblk, a.log_size), OP_THREADS, 0, L.stream>>>(a, counts, bad);
    }
    {
        Scope scope(L, "decommit_scan", 8.0 * nblk * a.log_size);
        decommit_scan_kernel<<<1, SCAN_THREADS, 0, L.stream>>>(counts, nblk * a.log_size, bad, nblk, a.count);
    }
    {
        Scope scope(L, "decommit_emit", 0.0);
        decommit_emit_kernel<<<dim3(nblk, a.log_size + 1), OP_THREADS, 0, L.stream>>>(a, counts);
    }
}

}  // namespace k
}  // namespace frieda
