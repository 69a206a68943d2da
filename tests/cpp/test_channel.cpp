// Host check of frieda_amd/csrc/channel.h: the streamed Channel::mix_felts against the buffer form it replaced (blake2s256 over the
// zero-padded buffer digest || words), Channel::draw_block against draw_random_words, and known answers for mix_u64 / draw_felt on a
// fixed digest (recorded from the buffer-form build, before mix_felts / draw_block existed).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "channel.h"

using namespace frieda;

static uint64_t sm_state = 7;
static uint32_t splitmix32() {
    uint64_t z = (sm_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (uint32_t)((z ^ (z >> 31)) >> 16);
}

static Channel fixed_channel() {
    Channel c;
    c.init();
    for (uint32_t i = 0; i < 8; i++) c.digest[i] = 0x9E3779B9u * (i + 1);
    c.n_challenges = 5;
    c.n_sent = 3;
    return c;
}

static bool same(const uint32_t* a, const uint32_t* b, int n) {
    for (int i = 0; i < n; i++)
        if (a[i] != b[i]) return false;
    return true;
}

int main() {
    long bad = 0;
    // mix_felts: 2 and 6 felts are messages of exactly 64 and 128 bytes (the block boundary), 2048 the longest last-layer polynomial
    const uint32_t sizes[] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 14, 15, 16, 17, 2048};
    for (uint32_t nf : sizes) {
        std::vector<uint32_t> words(4 * (size_t)nf);
        for (uint32_t& w : words) w = splitmix32();
        Channel ch = fixed_channel();
        std::vector<uint32_t> buf(8 + words.size());
        for (int i = 0; i < 8; i++) buf[i] = ch.digest[i];
        for (size_t i = 0; i < words.size(); i++) buf[8 + i] = words[i];
        const uint32_t len = (uint32_t)(4 * buf.size());
        buf.resize((buf.size() + 15) / 16 * 16, 0u);
        uint32_t want[8];
        b2s256_words(buf.data(), len, want);
        ch.mix_felts(words.data(), nf);
        if (!same(ch.digest, want, 8) || ch.n_challenges != 6 || ch.n_sent != 0) {
            printf("mix_felts differs at n_felts = %u\n", nf);
            bad++;
        }
    }
    // draw_block(k) is the draw of a channel whose n_sent is k, and leaves the channel alone
    const uint32_t counters[] = {0, 1, 2, 3, 7, 8, 127, 128, 0x80000000u, 0xFFFFFFFFu};
    for (uint32_t k : counters) {
        Channel a = fixed_channel(), b = fixed_channel();
        uint32_t ra[8], rb[8];
        a.draw_block(k, ra);
        b.n_sent = k;
        b.draw_random_words(rb);
        if (!same(ra, rb, 8) || a.n_sent != 3 || a.n_challenges != 5 || b.n_sent != k + 1 || !same(a.digest, b.digest, 8)) {
            printf("draw_block differs at counter %u\n", k);
            bad++;
        }
    }
    // known answers
    {
        const uint32_t want[8] = {0xB515B77Au, 0xB6BE5074u, 0xEA6D4FE1u, 0x779CC95Cu, 0x15802FD6u, 0x380D5183u, 0xC0427627u, 0xAC65F03Fu};
        Channel ch = fixed_channel();
        ch.mix_u64(0x0123456789ABCDEFull);
        if (!same(ch.digest, want, 8) || ch.n_challenges != 6 || ch.n_sent != 0) {
            printf("mix_u64 differs\n");
            bad++;
        }
    }
    {
        Channel ch = fixed_channel();
        const QM31 f = ch.draw_felt();
        if (!qm_eq(f, QM31{0x68281A0Eu, 0x18B8720Cu, 0x6BC282E2u, 0x08E69176u}) || ch.n_sent != 4) {
            printf("draw_felt differs\n");
            bad++;
        }
        // a lowered acceptance bound: the first draw is refused, the second taken
        Channel cr = fixed_channel();
        const QM31 g = cr.draw_felt(0xE0000000u);
        if (!qm_eq(g, QM31{0x3C79A7B2u, 0x21084429u, 0x6A8348D5u, 0x790CFCA1u}) || cr.n_sent != 5) {
            printf("draw_felt (retry) differs\n");
            bad++;
        }
    }
    printf("%s bad=%ld\n", bad ? "FAIL" : "OK", bad);
    return bad ? 1 : 0;
}
