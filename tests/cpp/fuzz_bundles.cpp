// fuzz_bundles.cpp — bundles_host.h (the malformed rule, the witness count, the host verifier of cell bundles) under ASan + UBSan, fed
// with thousands of mutated images of one valid call.  Stand-alone host program: built and run by tests/test_bundles_sanitizers.py.
//
//   fuzz_bundles <image> <mutations>
// image (little-endian): u32 log_domain, log_cell, n_bundles, n_cells; u64 n_hashes; u8 commitment[32]; u32 bundle_first[n_bundles + 1];
// u64 witness_first[n_bundles + 1]; u32 cell_index[n_cells]; u32 values[n_cells][4][2^log_cell]; u8 witness[n_hashes][32].
// Every array is copied into a heap block of exactly its size, so a read past any of them is an ASan report.  A mutant is one of: a
// flipped bit in the indices, the values, the witness or the commitment; an entry of bundle_first or witness_first moved (kept
// monotone, as the entry points require); the witness block cut or grown with witness_first following.  No mutant that differs from the
// original may be ACCEPTED in the bundle it touches.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "bundles_host.h"

using namespace frieda;

static uint64_t rng_state = 0x243F6A8885A308D3ull;
static uint64_t rnd() {
    rng_state ^= rng_state << 13, rng_state ^= rng_state >> 7, rng_state ^= rng_state << 17;
    return rng_state;
}

struct Image {
    uint32_t n, c, nb;
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
    status.assign(im.nb, 0xEE);
    if (bundle_shape_error(im.n, im.c) || bundles_call_error(im.first.data(), im.wfirst.data(), im.nb)) return 1;
    if (im.first[im.nb] > im.idx.size() || im.wfirst[im.nb] * 32 > im.witness.size()) return 1;  // (the caller's arrays must hold what *_first says)
    uint8_t* com = exact(im.com);
    uint32_t *first = exact(im.first), *idx = exact(im.idx), *values = exact(im.values);
    uint64_t* wfirst = exact(im.wfirst);
    uint8_t* witness = exact(im.witness);
    verify_cell_bundles_host(com, im.n, im.c, idx, first, im.nb, values, witness, wfirst, status.data());
    free(com), free(first), free(idx), free(values), free(wfirst), free(witness);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    Image im;
    uint32_t hd[4];
    uint64_t nh;
    if (fread(hd, 4, 4, f) != 4 || fread(&nh, 8, 1, f) != 1) return 2;
    im.n = hd[0], im.c = hd[1], im.nb = hd[2];
    im.com.resize(32), im.first.resize(im.nb + 1), im.wfirst.resize(im.nb + 1), im.idx.resize(hd[3]);
    im.values.resize(((size_t)hd[3] * 4) << im.c), im.witness.resize(32 * nh);
    if (fread(im.com.data(), 1, 32, f) != 32 || fread(im.first.data(), 4, im.nb + 1, f) != im.nb + 1 || fread(im.wfirst.data(), 8, im.nb + 1, f) != im.nb + 1 ||
        fread(im.idx.data(), 4, im.idx.size(), f) != im.idx.size() || fread(im.values.data(), 4, im.values.size(), f) != im.values.size() ||
        fread(im.witness.data(), 1, im.witness.size(), f) != im.witness.size())
        return 2;
    fclose(f);
    const long mutations = atol(argv[2]);
    std::vector<uint8_t> st, st0;
    if (run(im, st0) != 0) return 3;
    for (uint32_t b = 0; b < im.nb; b++)
        if (st0[b] != FRIEDA_BUNDLE_ACCEPTED) {
            printf("the unmutated call: bundle %u has status %u\n", b, st0[b]);
            return 3;
        }
    long accepted = 0, refused = 0, malformed = 0, rejected = 0;
    for (long m = 0; m < mutations; m++) {
        Image mu = im;
        std::vector<bool> touched(im.nb, false);
        auto bundle_of_cell = [&](size_t cell) {
            for (uint32_t b = 0; b < im.nb; b++)
                if (cell >= im.first[b] && cell < im.first[b + 1]) touched[b] = true;
        };
        auto bundle_of_hash = [&](size_t h) {
            for (uint32_t b = 0; b < im.nb; b++)
                if (h >= im.wfirst[b] && h < im.wfirst[b + 1]) touched[b] = true;
        };
        const unsigned kind = rnd() % 8;
        if (kind == 0 && !mu.idx.empty()) {
            const size_t i = rnd() % mu.idx.size();
            mu.idx[i] ^= 1u << (rnd() % 32);
            bundle_of_cell(i);
        } else if (kind == 1 && !mu.values.empty()) {
            const size_t i = rnd() % mu.values.size();
            mu.values[i] ^= 1u << (rnd() % 32);
            bundle_of_cell(i >> (2 + mu.c));
        } else if (kind == 2 && !mu.witness.empty()) {
            const size_t i = rnd() % mu.witness.size();
            mu.witness[i] ^= (uint8_t)(1u << (rnd() % 8));
            bundle_of_hash(i / 32);
        } else if (kind == 3) {
            mu.com[rnd() % 32] ^= (uint8_t)(1u << (rnd() % 8));
            touched.assign(im.nb, true);
        } else if (kind == 4 && im.nb >= 2) {  // an inner boundary of the cells moved, kept monotone
            const uint32_t b = 1 + (uint32_t)(rnd() % (im.nb - 1));
            const uint32_t lo = mu.first[b - 1], hi = mu.first[b + 1];
            mu.first[b] = lo + (uint32_t)(rnd() % (hi - lo + 1));
            if (mu.first[b] != im.first[b]) touched[b - 1] = touched[b] = true;
        } else if (kind == 5 && im.nb >= 2) {  // an inner boundary of the witness moved, kept monotone
            const uint32_t b = 1 + (uint32_t)(rnd() % (im.nb - 1));
            const uint64_t lo = mu.wfirst[b - 1], hi = mu.wfirst[b + 1];
            mu.wfirst[b] = lo + rnd() % (hi - lo + 1);
            if (mu.wfirst[b] != im.wfirst[b]) touched[b - 1] = touched[b] = true;
        } else if (kind == 6 && !mu.witness.empty()) {  // the witness cut: the last bundle loses hashes
            const uint64_t cut = 1 + rnd() % std::min<uint64_t>(4, mu.wfirst[im.nb] - mu.wfirst[im.nb - 1] ? mu.wfirst[im.nb] - mu.wfirst[im.nb - 1] : 1);
            if (mu.wfirst[im.nb] - mu.wfirst[im.nb - 1] >= cut) {
                mu.wfirst[im.nb] -= cut;
                mu.witness.resize(32 * mu.wfirst[im.nb]);
                touched[im.nb - 1] = true;
            }
        } else if (kind == 7) {  // the witness grown: the last bundle gains hashes
            const uint64_t add = 1 + rnd() % 4;
            mu.wfirst[im.nb] += add;
            mu.witness.resize(32 * mu.wfirst[im.nb], (uint8_t)rnd());
            touched[im.nb - 1] = true;
        }
        if (run(mu, st) != 0) {
            refused++;
            continue;
        }
        for (uint32_t b = 0; b < im.nb; b++) {
            if (st[b] > FRIEDA_BUNDLE_MALFORMED) {
                printf("mutant %ld: bundle %u has no status\n", m, b);
                return 1;
            }
            if (!touched[b]) {
                if (st[b] != FRIEDA_BUNDLE_ACCEPTED) {
                    printf("mutant %ld (kind %u): untouched bundle %u lost its status (%u)\n", m, kind, b, st[b]);
                    return 1;
                }
                continue;
            }
            if (st[b] == FRIEDA_BUNDLE_ACCEPTED) {
                accepted++;
                printf("mutant %ld (kind %u): touched bundle %u ACCEPTED\n", m, kind, b);
            }
            malformed += st[b] == FRIEDA_BUNDLE_MALFORMED, rejected += st[b] == FRIEDA_BUNDLE_REJECTED;
        }
    }
    printf("mutants %ld refused %ld malformed %ld rejected %ld accepted_mutants %ld\n", mutations, refused, malformed, rejected, accepted);
    return accepted ? 1 : 0;
}
