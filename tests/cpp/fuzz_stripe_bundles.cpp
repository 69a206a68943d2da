// fuzz_stripe_bundles.cpp — the host side of stripe bundles (bundles_host.h: the argument rule, the once-per-bundle malformed rule, the
// host verifier run per blob piece) under ASan + UBSan, fed with thousands of mutated images of one valid call over a block.
// Stand-alone host program with its own main: built and run by tests/test_stripe_bundles_sanitizers.py.
//
//   fuzz_stripe_bundles <image> <mutations>
// image (little-endian): u32 log_domain, log_cell, n_bundles, n_stripes, n_blobs; u64 n_hashes (per blob); u8 commitments[n_blobs][32];
// u32 bundle_first[n_bundles + 1]; u64 witness_first[n_bundles + 1]; u32 stripe_index[n_stripes];
// u32 values[n_stripes][n_blobs][4][2^log_cell]; u8 witness[n_blobs * n_hashes][32].
// Every array is copied into a heap block of exactly its size, so a read past any of them is an ASan report.  A mutant is one of: a
// flipped bit in the indices (touches the bundle's whole row), in the values or the witness (touches one (bundle, blob) byte), in a
// commitment (touches that blob's column); an entry of bundle_first or witness_first moved (kept monotone, as the entry points
// require); the witness cut or grown with witness_first following.  No mutant may be ACCEPTED in a byte it touches, and no untouched
// byte may lose its status.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "bundles_host.h"

using namespace frieda;

static uint64_t rng_state = 0x13198A2E03707344ull;
static uint64_t rnd() {
    rng_state ^= rng_state << 13, rng_state ^= rng_state >> 7, rng_state ^= rng_state << 17;
    return rng_state;
}

struct Image {
    uint32_t n, c, nb, k;
    std::vector<uint8_t> com;
    std::vector<uint32_t> first, idx, values;
    std::vector<uint64_t> wfirst;
    std::vector<uint8_t> witness;
};

// exact-size heap copies: the verifier sees no slack behind any array
template <class T>
static T* exact(const std::vector<T>& v) {
    T* p = static_cast<T*>(malloc(v.size() * sizeof(T) + (v.empty() ? 1 : 0)));
    if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T));
    return p;
}

static int run(const Image& im, std::vector<uint8_t>& status) {
    status.assign((size_t)im.nb * im.k, 0xEE);
    if (bundle_shape_error(im.n, im.c) || bundles_call_error(im.first.data(), im.wfirst.data(), im.nb)) return 1;
    // (the caller's arrays must hold what *_first says)
    if (im.first[im.nb] > im.idx.size() || im.wfirst[im.nb] * 32 * im.k > im.witness.size()) return 1;
    if ((((size_t)im.first[im.nb] * im.k * 4) << im.c) > im.values.size()) return 1;
    uint8_t* com = exact(im.com);
    uint32_t *first = exact(im.first), *idx = exact(im.idx), *values = exact(im.values);
    uint64_t* wfirst = exact(im.wfirst);
    uint8_t* witness = exact(im.witness);
    int rc = 0;
    if (stripe_bundles_args_error(com, im.k, 65536, im.n, im.c, idx, first, im.nb, values, witness, wfirst, status.data()))
        rc = 1;
    else
        verify_stripe_bundles_host(com, im.k, im.n, im.c, idx, first, im.nb, values, witness, wfirst, status.data());
    free(com), free(first), free(idx), free(values), free(wfirst), free(witness);
    return rc;
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    Image im;
    uint32_t hd[5];
    uint64_t nh;
    if (fread(hd, 4, 5, f) != 5 || fread(&nh, 8, 1, f) != 1) return 2;
    im.n = hd[0], im.c = hd[1], im.nb = hd[2], im.k = hd[4];
    if (im.k == 0 || im.k > 64 || im.nb == 0) return 2;
    im.com.resize(32 * (size_t)im.k), im.first.resize(im.nb + 1), im.wfirst.resize(im.nb + 1), im.idx.resize(hd[3]);
    im.values.resize(((size_t)hd[3] * im.k * 4) << im.c), im.witness.resize(32 * nh * im.k);
    if (fread(im.com.data(), 1, im.com.size(), f) != im.com.size() || fread(im.first.data(), 4, im.nb + 1, f) != im.nb + 1 ||
        fread(im.wfirst.data(), 8, im.nb + 1, f) != im.nb + 1 || fread(im.idx.data(), 4, im.idx.size(), f) != im.idx.size() ||
        fread(im.values.data(), 4, im.values.size(), f) != im.values.size() || fread(im.witness.data(), 1, im.witness.size(), f) != im.witness.size())
        return 2;
    fclose(f);
    const long mutations = atol(argv[2]);
    const size_t cells = (size_t)im.nb * im.k;
    std::vector<uint8_t> st, st0;
    if (run(im, st0) != 0) return 3;
    for (size_t e = 0; e < cells; e++)
        if (st0[e] != FRIEDA_BUNDLE_ACCEPTED) {
            printf("the unmutated call: bundle %zu blob %zu has status %u\n", e / im.k, e % im.k, st0[e]);
            return 3;
        }
    long accepted = 0, refused = 0, malformed = 0, rejected = 0;
    for (long m = 0; m < mutations; m++) {
        Image mu = im;
        std::vector<bool> touched(cells, false);
        auto row = [&](uint32_t b) {
            for (uint32_t j = 0; j < im.k; j++) touched[(size_t)b * im.k + j] = true;
        };
        auto bundle_of_stripe = [&](size_t t) {
            for (uint32_t b = 0; b < im.nb; b++)
                if (t >= im.first[b] && t < im.first[b + 1]) return b;
            return im.nb;
        };
        const unsigned kind = rnd() % 8;
        if (kind == 0 && !mu.idx.empty()) {  // the indices are shared: every blob of the bundle
            const size_t i = rnd() % mu.idx.size();
            mu.idx[i] ^= 1u << (rnd() % 32);
            row(bundle_of_stripe(i));
        } else if (kind == 1 && !mu.values.empty()) {
            const size_t i = rnd() % mu.values.size();
            mu.values[i] ^= 1u << (rnd() % 32);
            const size_t cell = i >> (2 + mu.c);  // stripe * n_blobs + blob
            touched[(size_t)bundle_of_stripe(cell / im.k) * im.k + cell % im.k] = true;
        } else if (kind == 2 && !mu.witness.empty()) {
            const size_t i = rnd() % mu.witness.size(), h = i / 32;
            mu.witness[i] ^= (uint8_t)(1u << (rnd() % 8));
            for (uint32_t b = 0; b < im.nb; b++) {
                const uint64_t w = im.wfirst[b + 1] - im.wfirst[b];
                if (h >= im.k * im.wfirst[b] && h < im.k * im.wfirst[b + 1]) touched[(size_t)b * im.k + (h - im.k * im.wfirst[b]) / w] = true;
            }
        } else if (kind == 3) {  // one blob's commitment: its column
            const size_t i = rnd() % mu.com.size();
            mu.com[i] ^= (uint8_t)(1u << (rnd() % 8));
            for (uint32_t b = 0; b < im.nb; b++) touched[(size_t)b * im.k + i / 32] = true;
        } else if (kind == 4 && im.nb >= 2) {  // an inner boundary of the stripes moved, kept monotone
            const uint32_t b = 1 + (uint32_t)(rnd() % (im.nb - 1));
            const uint32_t lo = mu.first[b - 1], hi = mu.first[b + 1];
            mu.first[b] = lo + (uint32_t)(rnd() % (hi - lo + 1));
            if (mu.first[b] != im.first[b]) row(b - 1), row(b);
        } else if (kind == 5 && im.nb >= 2) {  // an inner boundary of the witness moved, kept monotone
            const uint32_t b = 1 + (uint32_t)(rnd() % (im.nb - 1));
            const uint64_t lo = mu.wfirst[b - 1], hi = mu.wfirst[b + 1];
            mu.wfirst[b] = lo + rnd() % (hi - lo + 1);
            if (mu.wfirst[b] != im.wfirst[b]) row(b - 1), row(b);
        } else if (kind == 6 && !mu.witness.empty()) {  // the witness cut: the last bundle loses hashes per blob
            const uint64_t have = mu.wfirst[im.nb] - mu.wfirst[im.nb - 1];
            const uint64_t cut = 1 + rnd() % std::min<uint64_t>(4, have ? have : 1);
            if (have >= cut) {
                mu.wfirst[im.nb] -= cut;
                mu.witness.resize(32 * mu.wfirst[im.nb] * im.k);
                row(im.nb - 1);
            }
        } else if (kind == 7) {  // the witness grown: the last bundle gains hashes per blob
            const uint64_t add = 1 + rnd() % 4;
            mu.wfirst[im.nb] += add;
            mu.witness.resize(32 * mu.wfirst[im.nb] * im.k, (uint8_t)rnd());
            row(im.nb - 1);
        }
        if (run(mu, st) != 0) {
            refused++;
            continue;
        }
        for (size_t e = 0; e < cells; e++) {
            if (st[e] > FRIEDA_BUNDLE_MALFORMED) {
                printf("mutant %ld: bundle %zu blob %zu has no status\n", m, e / im.k, e % im.k);
                return 1;
            }
            if (!touched[e]) {
                if (st[e] != FRIEDA_BUNDLE_ACCEPTED) {
                    printf("mutant %ld (kind %u): untouched bundle %zu blob %zu lost its status (%u)\n", m, kind, e / im.k, e % im.k, st[e]);
                    return 1;
                }
                continue;
            }
            if (st[e] == FRIEDA_BUNDLE_ACCEPTED) {
                accepted++;
                printf("mutant %ld (kind %u): touched bundle %zu blob %zu ACCEPTED\n", m, kind, e / im.k, e % im.k);
            }
            malformed += st[e] == FRIEDA_BUNDLE_MALFORMED, rejected += st[e] == FRIEDA_BUNDLE_REJECTED;
        }
    }
    printf("mutants %ld refused %ld malformed %ld rejected %ld accepted_mutants %ld\n", mutations, refused, malformed, rejected, accepted);
    return accepted ? 1 : 0;
}
