// verify_pass.h against its two rules written out here once more.
//   The cut: the passes of a call walked one by one against a plain restatement (bytes first, then — for a pass that may split — the
//   longest prefix whose scratch fits): a lone oversized proof, 1024 queries x 40 layers, mixed layer counts, a cap hit exactly, random lists.
//   The rule: for a proof of 4 layers (and one without inner layers) every combination of (first event of the chain wave, set of
//   failing walk layers) decoded from min-of-keys against the sequential verifier's order restated as a plain loop.
// Stand-alone (ASan + UBSan: tests/test_verify_split_host.py); prints OK.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "verify_pass.h"

using namespace frieda;

static long checks = 0;
#define EXPECT(cond)                                                 \
    do {                                                             \
        checks++;                                                    \
        if (!(cond)) {                                               \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                 \
        }                                                            \
    } while (0)

// ---------------------------------------------------------------- the cut
struct Expect {
    size_t end, words, scratch;
    uint32_t q_cap, max_layers;
    bool split;
};

static uint32_t pow2_at_least_64(uint32_t q) {
    uint32_t c = 64;
    while (c < q) c *= 2;
    return c;
}

// the rule in words: bytes first; then, where the pass may split, drop proofs from its end until proofs x layers x q_cap x 36 fits
static Expect restated(const std::vector<VerifyPassItem>& v, size_t first, size_t pass_bytes, size_t split_max, size_t cap) {
    size_t end = first, words = 0;
    while (end < v.size() && (end == first || 4 * (words + v[end].words) <= pass_bytes)) words += v[end++].words;
    auto shape = [&](size_t e, Expect& x) {
        x.end = e, x.words = 0, x.q_cap = 64, x.max_layers = 0;
        for (size_t i = first; i < e; i++) {
            x.words += v[i].words;
            x.q_cap = std::max(x.q_cap, pow2_at_least_64(v[i].n_queries));
            x.max_layers = std::max(x.max_layers, v[i].n_layers);
        }
        x.scratch = (e - first) * (size_t)x.max_layers * x.q_cap * 36;
    };
    Expect x;
    shape(end, x);
    x.split = split_max != 0 && end - first <= split_max;
    if (!x.split) {
        x.scratch = 0;
        return x;
    }
    while (x.end - first > 1 && x.scratch > cap) shape(x.end - 1, x);
    return x;
}

static size_t walk_call(const std::vector<VerifyPassItem>& v, size_t pass_bytes, size_t split_max, size_t cap) {
    size_t passes = 0;
    for (size_t first = 0; first < v.size(); passes++) {
        const VerifyPassCut c = verify_pass_cut([&](size_t i) { return v[i]; }, first, v.size(), pass_bytes, split_max, cap);
        const Expect x = restated(v, first, pass_bytes, split_max, cap);
        EXPECT(c.end == x.end && c.end > first && c.end <= v.size());
        EXPECT(c.words == x.words && c.q_cap == x.q_cap && c.max_layers == x.max_layers);
        EXPECT(c.split == x.split && c.scratch_bytes == x.scratch);
        if (c.split) {
            EXPECT(c.end - first <= split_max);
            EXPECT(c.scratch_bytes <= cap || c.end - first == 1);
            EXPECT(c.scratch_bytes == verify_split_scratch_bytes(c.end - first, c.max_layers, c.q_cap));
            // the longest such prefix: one proof more would pass the cap, the bytes or the list
            if (c.end < v.size() && 4 * (c.words + v[c.end].words) <= pass_bytes) {
                const uint32_t q = std::max(c.q_cap, pow2_at_least_64(v[c.end].n_queries)), ml = std::max(c.max_layers, v[c.end].n_layers);
                EXPECT((c.end - first + 1) * (size_t)ml * q * 36 > cap);
            }
        }
        first = c.end;
    }
    return passes;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
    rng_state ^= rng_state << 13, rng_state ^= rng_state >> 7, rng_state ^= rng_state << 17;
    return rng_state;
}

static void test_cut() {
    EXPECT(VERIFY_SPLIT_ENTRY_BYTES == 36 && VERIFY_PASS_BYTES == (size_t)32 << 20);
    const size_t CAP = VERIFY_SPLIT_SCRATCH_CAP, ALWAYS = (size_t)1 << 31;
    // a lone oversized proof: a pass of its own on either shape, whatever its scratch
    {
        std::vector<VerifyPassItem> v = {{100, 20, 8}, {(size_t)20 << 20, 1024, 40}, {100, 20, 8}};
        EXPECT(walk_call(v, 1 << 20, 0, CAP) == 3);
        EXPECT(walk_call(v, 1 << 20, ALWAYS, CAP) == 3);
        EXPECT(walk_call(v, 1 << 20, ALWAYS, 1) == 3);  // (a cap nothing fits: every proof alone)
        const VerifyPassCut c = verify_pass_cut([&](size_t i) { return v[i]; }, 1, 3, 1 << 20, ALWAYS, 1);
        EXPECT(c.end == 2 && c.split && c.scratch_bytes == (size_t)40 * 1024 * 36);
    }
    // 1024 queries x 40 layers: 1 474 560 bytes a proof, 182 of them under 256 MiB
    {
        std::vector<VerifyPassItem> v(1000, VerifyPassItem{5000, 1024, 40});
        const VerifyPassCut c = verify_pass_cut([&](size_t i) { return v[i]; }, 0, v.size(), VERIFY_PASS_BYTES, ALWAYS, CAP);
        EXPECT(c.split && c.end == CAP / ((size_t)40 * 1024 * 36) && c.end == 182 && c.q_cap == 1024 && c.max_layers == 40);
        EXPECT(walk_call(v, VERIFY_PASS_BYTES, ALWAYS, CAP) == (1000 + 181) / 182);
        EXPECT(walk_call(v, VERIFY_PASS_BYTES, 0, CAP) == 1);     // never split: the scratch does not cut
        EXPECT(walk_call(v, VERIFY_PASS_BYTES, 999, CAP) == 1);   // a pass of 1000 is beyond 999: one launch, uncut
        EXPECT(walk_call(v, VERIFY_PASS_BYTES, 1000, CAP) == 6);
    }
    // mixed layer counts and query counts: the pitch is the pass's largest of each, so one deep proof makes every slot deep
    {
        std::vector<VerifyPassItem> v;
        for (int i = 0; i < 300; i++) v.push_back({800, 20, 7});
        v.push_back({9000, 300, 15});
        for (int i = 0; i < 300; i++) v.push_back({800, 65, 3});
        walk_call(v, VERIFY_PASS_BYTES, ALWAYS, CAP);
        const size_t cap = 300 * (size_t)7 * 64 * 36;  // exactly the 300 shallow ones
        const VerifyPassCut c = verify_pass_cut([&](size_t i) { return v[i]; }, 0, v.size(), VERIFY_PASS_BYTES, ALWAYS, cap);
        EXPECT(c.end == 300 && c.scratch_bytes == cap && c.max_layers == 7 && c.q_cap == 64);  // a cap hit exactly is within the cap
        const VerifyPassCut d = verify_pass_cut([&](size_t i) { return v[i]; }, 0, v.size(), VERIFY_PASS_BYTES, ALWAYS, cap - 1);
        EXPECT(d.end == 299);
        const VerifyPassCut e = verify_pass_cut([&](size_t i) { return v[i]; }, 300, v.size(), VERIFY_PASS_BYTES, ALWAYS, cap);
        EXPECT(e.q_cap == 512 && e.max_layers == 15 && e.end - 300 == cap / ((size_t)15 * 512 * 36));
        for (size_t sm : {(size_t)1, (size_t)64, (size_t)300, (size_t)601}) walk_call(v, VERIFY_PASS_BYTES, sm, cap);
    }
    // the bytes cut hit exactly, and random lists under random budgets
    {
        std::vector<VerifyPassItem> v(10, VerifyPassItem{256, 20, 5});
        EXPECT(walk_call(v, 4 * 256 * 5, 0, CAP) == 2);
        EXPECT(walk_call(v, 4 * 256 * 5 - 1, 0, CAP) == 3);
        EXPECT(walk_call(v, 4 * 256 * 5, 5, CAP) == 2);
        EXPECT(walk_call(v, 4 * 256 * 5, 4, CAP) == 2);  // passes of 5 are beyond 4: one launch each
    }
    for (int round = 0; round < 400; round++) {
        std::vector<VerifyPassItem> v(1 + rnd() % 200);
        for (auto& it : v) it = VerifyPassItem{(size_t)(40 + rnd() % 20000), (uint32_t)(1 + rnd() % 1024), (uint32_t)(1 + rnd() % 40)};
        const size_t split_max[] = {0, 1, 16, 64, (size_t)1 << 31};
        walk_call(v, (size_t)1 << (10 + rnd() % 16), split_max[rnd() % 5], (size_t)1 << (12 + rnd() % 18));
    }
}

// ---------------------------------------------------------------- the rule
enum { REJECTED = 0, ACCEPTED = 1, INVARIANT = 2 };

// What the chain wave and the walk waves can see of a proof with nl inner layers.
struct Proof {
    uint32_t nl;
    bool pow_fails;
    int value_fail[5];  // per layer: -1 passes, else the status its value stage ends with (layer 0 may say INVARIANT)
    bool walk_fail[5];
    bool last_fails;
};

// verifier.cpp::verify as a plain loop: the first failing event decides
static uint32_t sequential(const Proof& p) {
    if (p.pow_fails) return REJECTED;
    for (uint32_t li = 0; li <= p.nl; li++) {
        if (p.value_fail[li] >= 0) return (uint32_t)p.value_fail[li];
        if (p.walk_fail[li]) return REJECTED;
        if (p.nl == 0) return INVARIANT;
    }
    return p.last_fails ? REJECTED : ACCEPTED;
}

// the two launches: the chain's first event as a key and the counts it leaves; every walk wave with a count lowers the key if it fails
static uint32_t split(const Proof& p) {
    uint32_t key = VERIFY_KEY_ACCEPTED, cnt[5] = {0, 0, 0, 0, 0};
    bool done = false;
    if (p.pow_fails) key = verify_key(verify_order_pow(), REJECTED), done = true;
    for (uint32_t li = 0; !done && li <= p.nl; li++) {
        if (p.value_fail[li] >= 0) {
            key = verify_key(verify_order_values(li), (uint32_t)p.value_fail[li]), done = true;
            break;
        }
        cnt[li] = 1;
        if (p.nl == 0) key = verify_key(verify_order_no_inner(), INVARIANT), done = true;
    }
    if (!done && p.last_fails) key = verify_key(verify_order_last(p.nl), REJECTED);
    for (uint32_t li = 0; li < 5; li++)  // (any order: a minimum)
        if (cnt[4 - li] && p.walk_fail[4 - li]) key = std::min(key, verify_key(verify_order_walk(4 - li), REJECTED));
    return verify_key_status(key, ACCEPTED);
}

static void test_rule() {
    // the orders interleave as written, and a key keeps its status
    EXPECT(verify_order_pow() < verify_order_values(0) && verify_order_values(0) < verify_order_walk(0));
    for (uint32_t li = 0; li < 40; li++) {
        EXPECT(verify_order_walk(li) < verify_order_values(li + 1) && verify_order_values(li + 1) < verify_order_walk(li + 1));
        EXPECT(verify_order_walk(li) < verify_order_last(li) && verify_order_last(li) == verify_order_values(li + 1));
        for (uint32_t st = 0; st < 3; st++) EXPECT(verify_key_status(verify_key(verify_order_walk(li), st), ACCEPTED) == st);
    }
    EXPECT(verify_order_walk(0) < verify_order_no_inner() && verify_order_no_inner() == verify_order_values(1));
    EXPECT(verify_key(verify_order_last(39), INVARIANT) < VERIFY_KEY_ACCEPTED && verify_key_status(VERIFY_KEY_ACCEPTED, ACCEPTED) == ACCEPTED);
    // the host's guard: what the two launches can leave for a proof of nl inner layers, and nothing else
    for (uint32_t nl : {0u, 3u, 39u}) {
        EXPECT(verify_key_valid(VERIFY_KEY_ACCEPTED, nl) && verify_key_valid(verify_key(verify_order_pow(), REJECTED), nl));
        EXPECT(verify_key_valid(verify_key(verify_order_values(0), INVARIANT), nl) && verify_key_valid(verify_key(verify_order_last(nl), REJECTED), nl));
        EXPECT(verify_key_valid(verify_key(verify_order_walk(nl), REJECTED), nl));
        EXPECT(!verify_key_valid(verify_key(verify_order_last(nl) + 1, REJECTED), nl) && !verify_key_valid(verify_key(verify_order_walk(0), ACCEPTED), nl));
        EXPECT(!verify_key_valid(verify_key(verify_order_walk(0), 3), nl) && !verify_key_valid(0xFFFFFFFEu, nl) && !verify_key_valid(0x7FFFFFFFu, nl));
    }
    // every (first chain event, set of failing walk layers) of a 4-layer proof (nl = 3) and of a proof without inner layers
    for (uint32_t nl : {3u, 0u}) {
        const uint32_t layers = nl + 1;
        // chain events: none, PoW, values of layer li (REJECTED; at layer 0 also INVARIANT), the last layer
        for (uint32_t ev = 0; ev < 3 + layers + 1; ev++) {
            for (uint32_t walks = 0; walks < (1u << layers); walks++) {
                Proof p{};
                p.nl = nl;
                for (uint32_t li = 0; li < 5; li++) p.value_fail[li] = -1, p.walk_fail[li] = li < layers && ((walks >> li) & 1u);
                if (ev == 1) p.pow_fails = true;
                if (ev == 2) p.last_fails = true;
                if (ev == 3) p.value_fail[0] = INVARIANT;
                if (ev >= 4) p.value_fail[ev - 4] = REJECTED;
                EXPECT(split(p) == sequential(p));
            }
        }
    }
    // the cases the order exists for
    {
        Proof p{};
        for (int li = 0; li < 5; li++) p.value_fail[li] = -1;
        p.nl = 0, p.walk_fail[0] = true;
        EXPECT(split(p) == REJECTED);  // no inner layers and a bad first-layer hash
        p.walk_fail[0] = false;
        EXPECT(split(p) == INVARIANT);
        p.nl = 3, p.value_fail[0] = INVARIANT, p.walk_fail[0] = true;
        EXPECT(split(p) == INVARIANT);  // too few evaluations, with a corrupted first-layer hash
        p.value_fail[0] = -1, p.walk_fail[0] = false, p.walk_fail[1] = true, p.value_fail[3] = REJECTED;
        EXPECT(split(p) == REJECTED);
        p.value_fail[3] = -1, p.walk_fail[1] = false, p.walk_fail[3] = true, p.last_fails = true;
        EXPECT(split(p) == REJECTED);
    }
}

int main() {
    test_cut();
    test_rule();
    printf("%ld checks\nOK\n", checks);
    return 0;
}
