// test_encoded_slab.cpp — the owner of the allocation K encoded handles share (frieda_amd/csrc/encoded_slab.h) on the host: a
// stand-alone program, built with -fsanitize=address,undefined by tests/test_encoded_host.py (the two-thread case is checked by its
// counts, not by a race detector).
// The injected free counts its calls and checks its arguments; the "allocation" is a heap block, so that a free that runs early (a
// handle still alive reads its share afterwards), twice or never shows under AddressSanitizer as well as in the counts.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <atomic>
#include <thread>
#include <vector>

#include "encoded_slab.h"

using namespace frieda;

static std::atomic<int> frees{0};
static void* expect_base = nullptr;
static int expect_device = 0;
static int fails = 0;

static void counting_free(void* base, int device) {
    if (base != expect_base || device != expect_device) {
        printf("FAIL: free(%p, %d), expected (%p, %d)\n", base, device, expect_base, expect_device);
        fails++;
    }
    frees.fetch_add(1);
    free(base);
}

#define EXPECT(cond, ...)                 \
    do {                                  \
        if (!(cond)) {                    \
            fails++;                      \
            printf("FAIL: " __VA_ARGS__); \
            printf("\n");                 \
        }                                 \
    } while (0)

constexpr size_t SHARE = 64;

// K handles freed in `order`: the free runs exactly once, in the last drop; every handle still alive can read its share until then
static void run_order(const std::vector<uint32_t>& order, int device) {
    const uint32_t K = (uint32_t)order.size();
    uint8_t* base = static_cast<uint8_t*>(malloc(SHARE * K));
    for (size_t i = 0; i < SHARE * K; i++) base[i] = (uint8_t)(i / SHARE);
    expect_base = base;
    expect_device = device;
    frees = 0;
    EncodedSlab* s = slab_create(base, device, K, counting_free);
    std::vector<bool> alive(K, true);
    for (uint32_t step = 0; step < K; step++) {
        for (uint32_t h = 0; h < K; h++)
            if (alive[h]) EXPECT(base[SHARE * h] == (uint8_t)h && base[SHARE * h + SHARE - 1] == (uint8_t)h, "share %u unreadable before drop %u", h, step);
        const bool last = slab_drop(s);
        alive[order[step]] = false;
        EXPECT(last == (step + 1 == K), "K %u: drop %u returned %d", K, step, (int)last);
        EXPECT(frees.load() == (step + 1 == K ? 1 : 0), "K %u: %d frees after drop %u", K, frees.load(), step);
    }
    EXPECT(frees.load() == 1, "K %u: %d frees in all", K, frees.load());
}

int main() {
    // every order for K <= 4
    for (uint32_t K = 1; K <= 4; K++) {
        std::vector<uint32_t> order(K);
        for (uint32_t i = 0; i < K; i++) order[i] = i;
        do run_order(order, (int)K - 1);
        while (std::next_permutation(order.begin(), order.end()));
    }
    // a random order for K = 64
    {
        std::vector<uint32_t> order(64);
        for (uint32_t i = 0; i < 64; i++) order[i] = i;
        uint64_t x = 0x2545F4914F6CDD1Dull;
        for (uint32_t i = 63; i > 0; i--) {
            x ^= x << 13, x ^= x >> 7, x ^= x << 17;
            std::swap(order[i], order[x % (i + 1)]);
        }
        run_order(order, 5);
    }
    // two threads freeing disjoint halves, many rounds: one free per slab, after both halves
    for (int round = 0; round < 200; round++) {
        const uint32_t K = 64;
        uint8_t* base = static_cast<uint8_t*>(malloc(SHARE * K));
        for (size_t i = 0; i < SHARE * K; i++) base[i] = 1;
        expect_base = base;
        expect_device = 3;
        frees = 0;
        EncodedSlab* s = slab_create(base, 3, K, counting_free);
        std::atomic<int> lasts{0};
        std::atomic<uint32_t> sum{0};
        auto half = [&](uint32_t first) {
            for (uint32_t h = first; h < first + K / 2; h++) {
                sum.fetch_add(base[SHARE * h]);  // the handle's share, read before its own drop
                if (slab_drop(s)) lasts.fetch_add(1);
            }
        };
        std::thread a(half, 0u), b(half, K / 2);
        a.join();
        b.join();
        EXPECT(frees.load() == 1 && lasts.load() == 1 && sum.load() == K, "threads, round %d: %d frees, %d last drops, sum %u", round, frees.load(), lasts.load(), sum.load());
    }
    if (fails) {
        printf("FAILED %d\n", fails);
        return 1;
    }
    printf("OK\n");
    return 0;
}
