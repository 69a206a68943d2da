// aggregate.hip — the random linear combination of a block's codewords (gfx950; frieda_aggregate_encoded, block_host.cpp).
//
//   g(p) = sum over k < K of rho^k * f_k(p)      f_k(p): the four coordinate columns of handle k at position p, read as one QM31
//
// by Horner from k = K - 1 down to 0: acc = acc * rho + f_k.  rho is a kernel argument, so the 4 x 4 matrix of "multiply by rho"
// (field.h qm_matrix) sits in scalar registers; one step is 16 multiply-adds into four 64-bit sums (four 62-bit products and a 31-bit
// term fit 64 bits, as in qm_fold_pair) and four reductions, the accumulator canonical after every step.  A thread owns four
// consecutive positions: one 16-byte load per column and blob, one 16-byte store per column.  The K evaluation pointers come from a
// table in device memory (handles do not share a base); the index is wave-uniform, so the pointers are scalar loads.  The loads of four
// blobs are issued before their four steps, so that the chain waits for memory once per four blobs.
//
//   aggregate_kernel<V>        one thread per V positions (V = 4; V = 1 for domains of fewer than 4 points), the whole chain in one thread
//   aggregate_split_kernel     small domains under many blobs (64 blobs of 1 KiB: 512 threads of work and a 64-deep chain): the four waves
//                              of a workgroup share 64 position quads and take a quarter of the blob range each,
//                              S_w = sum over k in [w c, (w + 1) c) of rho^(k - w c) f_k; waves 1 .. 3 leave S_w in LDS and wave 0 adds
//                              rho^(w c) * S_w with the matrices of a host-made table.  Field arithmetic is exact and both routes store
//                              canonical words: the results are identical.
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace frieda {
namespace k {

namespace {

// a pointer read from the table is a generic pointer to the compiler: say that it is global memory, so that the loads are global loads
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(1))) uint32_t* GlobalWords;
typedef const __attribute__((address_space(1))) u32x4* GlobalQuads;

template <int V>
__device__ __forceinline__ void agg_load(const uint32_t* __restrict__ ev_, size_t N, size_t t, uint32_t (&f)[4][V]) {
    const GlobalWords ev = (GlobalWords)ev_;
    if constexpr (V == 4) {
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const u32x4 v = *(GlobalQuads)(ev + (size_t)c * N + 4 * t);
            f[c][0] = v.x, f[c][1] = v.y, f[c][2] = v.z, f[c][3] = v.w;
        }
    } else {
#pragma unroll
        for (int c = 0; c < 4; c++) f[c][0] = ev[(size_t)c * N + t];
    }
}

// acc = m * acc + f; every word canonical in, canonical out
template <int V>
__device__ __forceinline__ void agg_step(uint32_t (&acc)[4][V], const uint32_t (&f)[4][V], const QM31Mat& m) {
#pragma unroll
    for (int i = 0; i < V; i++) {
        uint32_t r[4];
#pragma unroll
        for (int row = 0; row < 4; row++) {
            uint64_t s = f[row][i];
#pragma unroll
            for (int j = 0; j < 4; j++) s += (uint64_t)m.m[row][j] * acc[j][i];
            r[row] = m31_reduce64(s);
        }
#pragma unroll
        for (int row = 0; row < 4; row++) acc[row][i] = r[row];
    }
}

// Horner over the blobs [k0, k1), k0 < k1
template <int V>
__device__ __forceinline__ void agg_range(const uint32_t* const* __restrict__ evals, uint32_t k0, uint32_t k1, size_t N, size_t t, const QM31Mat& m,
                                          uint32_t (&acc)[4][V]) {
    agg_load<V>(evals[k1 - 1], N, t, acc);
    uint32_t kk = k1 - 1;  // the blobs [k0, kk) remain
    while (kk - k0 >= 4) {
        uint32_t f[4][4][V];
#pragma unroll
        for (int u = 0; u < 4; u++) agg_load<V>(evals[kk - 1 - u], N, t, f[u]);
#pragma unroll
        for (int u = 0; u < 4; u++) agg_step<V>(acc, f[u], m);
        kk -= 4;
    }
    while (kk > k0) {
        uint32_t f[4][V];
        agg_load<V>(evals[kk - 1], N, t, f);
        agg_step<V>(acc, f, m);
        kk--;
    }
}

template <int V>
__device__ __forceinline__ void agg_store(uint32_t* __restrict__ out, size_t N, size_t t, const uint32_t (&acc)[4][V]) {
    if constexpr (V == 4) {
#pragma unroll
        for (int c = 0; c < 4; c++) *reinterpret_cast<uint4*>(out + (size_t)c * N + 4 * t) = make_uint4(acc[c][0], acc[c][1], acc[c][2], acc[c][3]);
    } else {
#pragma unroll
        for (int c = 0; c < 4; c++) out[(size_t)c * N + t] = acc[c][0];
    }
}

template <int V>
__global__ __launch_bounds__(256) void aggregate_kernel(AggregateArgs a) {
    const size_t N = (size_t)1 << a.log_n, t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= N / V) return;
    uint32_t acc[4][V];
    agg_range<V>(a.evals, 0, a.n_blobs, N, t, a.rho, acc);
    agg_store<V>(a.out, N, t, acc);
}

__global__ __launch_bounds__(256) void aggregate_split_kernel(AggregateArgs a) {
    __shared__ uint32_t part[AGG_SPLIT - 1][16][64];
    const size_t N = (size_t)1 << a.log_n, quads = N / 4;
    const uint32_t w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;  // (the wave's number, as a scalar)
    const size_t t = (size_t)blockIdx.x * 64 + lane;
    const bool live = t < quads;
    const uint32_t k0 = w * a.chunk, k1 = k0 + a.chunk < a.n_blobs ? k0 + a.chunk : a.n_blobs;  // (wave-uniform; empty when k0 >= n_blobs)
    uint32_t acc[4][4];
#pragma unroll
    for (int c = 0; c < 4; c++)
#pragma unroll
        for (int i = 0; i < 4; i++) acc[c][i] = 0;
    if (live && k0 < a.n_blobs) agg_range<4>(a.evals, k0, k1, N, t, a.rho, acc);
    if (w) {
#pragma unroll
        for (int c = 0; c < 4; c++)
#pragma unroll
            for (int i = 0; i < 4; i++) part[w - 1][4 * c + i][lane] = acc[c][i];
    }
    __syncthreads();
    if (w || !live) return;
#pragma unroll
    for (uint32_t x = 1; x < AGG_SPLIT; x++) {
        if (x * a.chunk >= a.n_blobs) break;  // (that wave's range was empty: its sum is zero)
        uint32_t s[4][4];
#pragma unroll
        for (int c = 0; c < 4; c++)
#pragma unroll
            for (int i = 0; i < 4; i++) s[c][i] = part[x - 1][4 * c + i][lane];
        // acc = rho^(x c) * S_x + acc: the step with the roles of addend and multiplicand exchanged
        agg_step<4>(s, acc, a.rho_pow[x - 1]);
#pragma unroll
        for (int c = 0; c < 4; c++)
#pragma unroll
            for (int i = 0; i < 4; i++) acc[c][i] = s[c][i];
    }
    agg_store<4>(a.out, N, t, acc);
}

}  // namespace

void aggregate(const Launch& L, const AggregateArgs& a, bool split) {
    const size_t N = (size_t)1 << a.log_n;
    // (no kernel-timer scope, as in bundles.hip: every name the timer knows is tied to a row of tests/workspace_rows.py; the kernels'
    // times come from a kernel trace, tools/block_proof_timing.py --aggregate-only)
    if (N < 4) {
        aggregate_kernel<1><<<1, 256, 0, L.stream>>>(a);
    } else if (split) {
        aggregate_split_kernel<<<(unsigned)((N / 4 + 63) / 64), 256, 0, L.stream>>>(a);
    } else {
        aggregate_kernel<4><<<(unsigned)((N / 4 + 255) / 256), 256, 0, L.stream>>>(a);
    }
}

}  // namespace k
}  // namespace frieda
