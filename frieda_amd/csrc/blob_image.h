// blob_image.h — the blob-image rule: which coefficient vectors are what unpack30 (codec.hip) makes of a blob of `len` bytes.
// unpack30 cuts the LSB-first bit stream into 30-bit felts, zero-extends the last one and pads with zeros, so word k of an image is
//   < 2^30                          for k <  F - 1,
//   < 2^(8 len - 30 (F - 1))        for k == F - 1      (the bits the blob still has for its last felt: 1 .. 30),
//   0                               for k >= F,          F = ceil(8 len / 30)   (len == 0: every word is 0).
// Exactly for such vectors unpack30(pack30(coef)[0 .. len)) == coef.  A rebuild that accepts the root of evaluate(coef) in place of
// commit(pack30(coef)) needs this check: a committer can publish the root of a polynomial that is no blob's image.
// HIP-free: the kernel (encoded.hip: blob_image_check) and the host restatement below share blob_image_limit.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define FRIEDA_IMAGE_HD __host__ __device__
#else
#define FRIEDA_IMAGE_HD
#endif

namespace frieda {

struct BlobImageRule {
    uint64_t n_felts;    // F
    uint32_t last_bits;  // bits of felt F - 1 (1 .. 30; 0 when F == 0)
};

FRIEDA_IMAGE_HD inline BlobImageRule blob_image_rule(uint64_t len) {
    BlobImageRule r;
    r.n_felts = (8 * len + 29) / 30;
    r.last_bits = r.n_felts ? (uint32_t)(8 * len - 30 * (r.n_felts - 1)) : 0;
    return r;
}

// the exclusive upper bound of word k (1: the word must be 0)
FRIEDA_IMAGE_HD inline uint32_t blob_image_limit(const BlobImageRule& r, uint64_t k) {
    if (k + 1 < r.n_felts) return 1u << 30;
    if (k + 1 == r.n_felts) return 1u << r.last_bits;
    return 1u;
}

// host restatement: true iff words[0 .. n_words) is the image of some blob of `len` bytes
inline bool blob_image_ok(const uint32_t* words, size_t n_words, uint64_t len) {
    const BlobImageRule r = blob_image_rule(len);
    for (size_t k = 0; k < n_words; k++)
        if (words[k] >= blob_image_limit(r, k)) return false;
    return true;
}

}  // namespace frieda
