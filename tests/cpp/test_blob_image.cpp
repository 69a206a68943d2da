// test_blob_image.cpp — the blob-image rule (frieda_amd/csrc/blob_image.h) on the host: a stand-alone program, built with
// -fsanitize=address,undefined by tests/test_encoded_host.py.
// For every blob length of the list: the unpack of random bytes passes the rule, pack(unpack(bytes)) == bytes, and every single
// mutation of one word into a forbidden region fails it (a word below the last felt raised to >= 2^30, the last felt given a bit the
// blob does not have, a padding word made non-zero).  unpack / pack below restate src/utils.rs:10-33 and its inverse independently of
// the rule: one felt is the 30 bits from bit 30 k of the LSB-first stream.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "blob_image.h"

using namespace frieda;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

static size_t padded_words(size_t len) {  // 4 columns of a power of two, at least 2 felts each (frieda_codec_shape)
    const size_t felts = (8 * len + 29) / 30;
    size_t k = 2;
    while (4 * k < felts) k *= 2;
    return 4 * k;
}

static std::vector<uint32_t> unpack(const std::vector<uint8_t>& bytes, size_t n_words) {
    std::vector<uint32_t> w(n_words, 0);
    for (size_t k = 0; k < n_words; k++) {
        uint32_t v = 0;
        for (int b = 0; b < 30; b++) {
            const size_t bit = 30 * k + b;
            if (bit / 8 < bytes.size() && ((bytes[bit / 8] >> (bit % 8)) & 1)) v |= 1u << b;
        }
        w[k] = v;
    }
    return w;
}

static std::vector<uint8_t> pack(const std::vector<uint32_t>& w, size_t len) {
    std::vector<uint8_t> out(len, 0);
    for (size_t bit = 0; bit < 8 * len; bit++) {
        const size_t k = bit / 30;
        if (k < w.size() && ((w[k] >> (bit % 30)) & 1)) out[bit / 8] |= (uint8_t)(1u << (bit % 8));
    }
    return out;
}

static int fails = 0;
#define EXPECT(cond, ...)              \
    do {                               \
        if (!(cond)) {                 \
            fails++;                   \
            printf("FAIL: " __VA_ARGS__); \
            printf("\n");              \
        }                              \
    } while (0)

static void check_len(size_t len) {
    const size_t n_words = padded_words(len);
    std::vector<uint8_t> bytes(len);
    for (auto& b : bytes) b = (uint8_t)rnd();
    if (len) bytes[len - 1] |= 0x80;  // (the blob's last bit set: the bound of the last felt is tight)
    const std::vector<uint32_t> w = unpack(bytes, n_words);
    EXPECT(blob_image_ok(w.data(), n_words, len), "len %zu: the unpack of a blob does not pass", len);
    EXPECT(pack(w, len) == bytes, "len %zu: pack(unpack(bytes)) != bytes", len);
    const size_t F = (8 * len + 29) / 30;
    const BlobImageRule r = blob_image_rule(len);
    EXPECT(r.n_felts == F, "len %zu: F", len);
    if (F) EXPECT(r.last_bits >= 1 && r.last_bits <= 30 && r.last_bits == 8 * len - 30 * (F - 1), "len %zu: last_bits %u", len, r.last_bits);
    auto mutant_fails = [&](size_t k, uint32_t v, const char* what) {
        std::vector<uint32_t> m = w;
        m[k] = v;
        EXPECT(!blob_image_ok(m.data(), n_words, len), "len %zu: word %zu = %u (%s) passes", len, k, v, what);
    };
    // words below the last felt: every value from 2^30 up is forbidden — both bits above the felt, alone and on top of the value
    for (size_t k = 0; k + 1 < F; k += (F > 64 ? F / 61 : 1)) {
        mutant_fails(k, w[k] | (1u << 30), "bit 30");
        mutant_fails(k, w[k] | (1u << 31), "bit 31");
        mutant_fails(k, 1u << 30, "2^30");
    }
    if (F >= 2) mutant_fails(F - 2, w[F - 2] | (1u << 30), "bit 30 of the felt before the last");
    // the last felt: every bit from last_bits up
    if (F)
        for (uint32_t b = r.last_bits; b < 32; b++) mutant_fails(F - 1, w[F - 1] | (1u << b), "a bit above the blob's last");
    // the padding: any non-zero word
    for (size_t k = F; k < n_words; k += (n_words - F > 64 ? (n_words - F) / 61 : 1)) {
        mutant_fails(k, 1, "padding = 1");
        mutant_fails(k, 1u << 29, "padding = 2^29");
        mutant_fails(k, 0xFFFFFFFFu, "padding = ~0");
    }
    if (F < n_words) mutant_fails(n_words - 1, 7, "the last word = 7");
    // the limits themselves: the largest allowed value of every region passes
    {
        std::vector<uint32_t> m = w;
        if (F >= 2) m[0] = (1u << 30) - 1;
        if (F) m[F - 1] = (uint32_t)((1ull << r.last_bits) - 1);
        EXPECT(blob_image_ok(m.data(), n_words, len), "len %zu: the largest allowed words do not pass", len);
    }
}

int main() {
    for (size_t len = 0; len <= 600; len++) check_len(len);
    for (size_t len : {1023u, 1024u, 1025u, 3839u, 3840u, 3841u, 65536u}) check_len(len);
    if (fails) {
        printf("FAILED %d\n", fails);
        return 1;
    }
    printf("OK\n");
    return 0;
}
