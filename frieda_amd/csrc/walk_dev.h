// walk_dev.h — one level of a compacted Merkle walk by one wave: what verify.hip (the hash witness of a proof's layers) and
// bundles.hip (the shared witness of a cell bundle) share, so that the two verifiers read stwo's witness order the same way.
//
// The nodes of a level are an ascending list of positions with their hashes, both in LDS (hash i at h[8 i .. 8 i + 7]).  The parents are
// unique(positions >> 1); a child that is not in the list comes from the witness at the prefix count of the missing children (the E_s
// tables of queries_dev.h, read from the verifier's side).  The list is compacted in place: entry k of the next level is written after
// the entries >= k of this one were read (a wave executes its LDS accesses in program order), the neighbour below a 64-entry chunk is
// carried in a register.  Callers are 64-thread workgroups: every lane calls.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "blake2s.h"

namespace frieda {
namespace k {
namespace walkdev {

struct Group {
    bool first, miss, has_l, has_r;
    uint32_t x, k, w;
};

// One 64-entry chunk of a level: lane `lane` looks at entry i = i0 + lane of the ascending list p[0 .. c).  The first entry of every
// parent group (x >> 1) owns the group: k = its index in the next level, w = the index of its missing child among the missing children
// of the level (a group misses at most one).  `carry`: the entry below the chunk (valid for i0 > 0).
__device__ __forceinline__ Group group_of(const uint32_t* p, uint32_t c, uint32_t i0, uint32_t lane, uint32_t carry, uint32_t& kbase, uint32_t& wbase) {
    const unsigned long long lt_mask = (1ull << lane) - 1;
    const uint32_t i = i0 + lane;
    Group g;
    g.x = i < c ? p[i] : 0u;
    const uint32_t prev = lane == 0 ? carry : p[i < c ? i - 1 : 0];
    const uint32_t next = i + 1 < c ? p[i + 1] : 0xFFFFFFFFu;
    g.first = i < c && (i == 0 || (prev >> 1) != (g.x >> 1));
    g.has_l = !(g.x & 1u);
    g.has_r = (g.x & 1u) || next == g.x + 1;
    g.miss = g.first && !(g.has_l && g.has_r);
    const unsigned long long mf = __ballot(g.first), mm = __ballot(g.miss);
    g.k = kbase + (uint32_t)__popcll(mf & lt_mask);
    g.w = wbase + (uint32_t)__popcll(mm & lt_mask);
    kbase += (uint32_t)__popcll(mf);
    wbase += (uint32_t)__popcll(mm);
    return g;
}

// The walk step: the cn nodes (s_hp[i], s_h[8 i ..]) of a level -> their parents, in place.  hw: the witness, nh hashes of 8 words;
// hbase: the hashes the levels below consumed, advanced by this level's missing children.  A missing child beyond nh sets `bad` in
// its lane and hashes zeros instead (nothing is read past the witness).  Returns the number of parents.
__device__ __forceinline__ uint32_t walk_level(uint32_t* s_hp, uint32_t* s_h, uint32_t cn, uint32_t lane, const uint32_t* hw, uint32_t nh, uint32_t& hbase,
                                               bool& bad) {
    uint32_t kb = 0, cr = 0;
    for (uint32_t i0 = 0; i0 < cn; i0 += 64) {
        const Group g = group_of(s_hp, cn, i0, lane, cr, kb, hbase);
        const uint32_t i = i0 + lane;
        uint32_t mm[16];
        if (g.first) {
            const bool wok = !g.miss || g.w < nh;
            if (!wok) bad = true;  // WitnessTooShort
            const uint32_t* wsrc = hw + 8 * (size_t)(wok && g.miss ? g.w : 0);
            const uint32_t* own = s_h + 8 * i;
            const uint32_t* nxt = s_h + 8 * (g.has_l && g.has_r ? i + 1 : i);
#pragma unroll
            for (int w = 0; w < 8; w++) {
                const uint32_t wv = (g.miss && wok) ? wsrc[w] : 0u;
                mm[w] = g.has_l ? own[w] : wv;
                mm[8 + w] = (g.x & 1u) ? own[w] : (g.has_r ? nxt[w] : wv);
            }
        }
        cr = (uint32_t)__shfl((int)g.x, 63);
        __syncthreads();
        if (g.first) {
            uint32_t hp[8];
            b2_merkle_block<B2_LAT>(mm, hp);
#pragma unroll
            for (int w = 0; w < 8; w++) s_h[8 * g.k + w] = hp[w];
            s_hp[g.k] = g.x >> 1;
        }
        __syncthreads();
    }
    return kb;
}

}  // namespace walkdev
}  // namespace k
}  // namespace frieda
