// encoded.hip — device code of the handles a rebuild returns (gfx950; frieda_rebuild_encoded_*, reconstruct.cpp).
//
//   blob_image_check   one pass over the 4 * 2^L coefficient words of every blob of the call (blockIdx.y = blob): a thread loads four
//                      words as one 16-byte load and compares each with the bound blob_image.h gives its index; a wave with a word
//                      out of bounds sets the blob's flag with ONE atomicOr (lane 0 after a ballot).  HBM-bound: 4 B read per word.
//   eval_to_slab       the point reconstruction re-encodes 4 * n_blobs columns at ONE stride; the handles of a block keep blob b's
//                      four columns back to back at b * bstride.  A 16-byte copy per thread (blockIdx.y = column, blockIdx.z = blob).
//
// Both are launched without a timer Scope.
#include <hip/hip_runtime.h>

#include "blob_image.h"
#include "kernels.h"

namespace frieda {
namespace k {

namespace {

__global__ __launch_bounds__(256) void blob_image_check_kernel(const uint4* __restrict__ coef, size_t n_quads, BlobImageRule rule,
                                                               uint32_t* __restrict__ flags) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    bool bad = false;
    if (t < n_quads) {
        const uint4 v = coef[(size_t)blockIdx.y * n_quads + t];
        const uint64_t k0 = 4 * (uint64_t)t;
        bad = v.x >= blob_image_limit(rule, k0) || v.y >= blob_image_limit(rule, k0 + 1) || v.z >= blob_image_limit(rule, k0 + 2) ||
              v.w >= blob_image_limit(rule, k0 + 3);
    }
    const unsigned long long m = __ballot(bad);
    if (m != 0 && (threadIdx.x & 63) == 0) atomicOr(&flags[blockIdx.y], 1u);
}

__global__ __launch_bounds__(256) void eval_to_slab_kernel(const uint4* __restrict__ ev, size_t ev_stride_quads, size_t col_quads,
                                                           uint8_t* __restrict__ slab, size_t bstride) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= col_quads) return;
    const uint32_t c = blockIdx.y, b = blockIdx.z;
    uint4* dst = reinterpret_cast<uint4*>(slab + (size_t)b * bstride) + (size_t)c * col_quads;
    dst[t] = ev[((size_t)4 * b + c) * ev_stride_quads + t];
}

}  // namespace

void blob_image_check(const Launch& L, const uint32_t* d_coef, size_t n_words, size_t len, uint32_t n_blobs, uint32_t* d_flags) {
    if (n_words == 0 || n_blobs == 0) return;
    const size_t quads = n_words / 4;
    const dim3 grid((unsigned)((quads + 255) / 256), n_blobs);
    blob_image_check_kernel<<<grid, 256, 0, L.stream>>>(reinterpret_cast<const uint4*>(d_coef), quads, blob_image_rule(len), d_flags);
}

void eval_to_slab(const Launch& L, const uint32_t* d_ev, size_t ev_stride, uint32_t n, uint32_t n_blobs, uint8_t* d_slab, size_t bstride) {
    if (n_blobs == 0) return;
    const size_t col_quads = ((size_t)1 << n) / 4;
    const dim3 grid((unsigned)((col_quads + 255) / 256), 4, n_blobs);
    eval_to_slab_kernel<<<grid, 256, 0, L.stream>>>(reinterpret_cast<const uint4*>(d_ev), ev_stride / 4, col_quads, d_slab, bstride);
}

}  // namespace k
}  // namespace frieda
