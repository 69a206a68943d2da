// prove_jobs_plan.h — the arithmetic of a frieda_prove_jobs call (prover.cpp): the order its jobs run in, the table a pass uploads, and
// how a list is cut into passes.  No HIP, no context: everything here runs on the CPU against the rules written out again
// (tests/cpp/test_prove_jobs_plan.cpp).
//
// A job is (blob_index, seed).  The launches want the jobs of one blob side by side (the seed-looped first fold reads a blob's evaluation
// once per GROUP of jobs), so a call runs its jobs sorted by blob_index — a stable sort: the jobs of one blob keep the caller's order —
// and writes proof y of the sorted list back to the caller's slot order[y].
//   rows       the distinct blobs of a run of the sorted list, ascending; job_row[y]: the row of job y; row_first[r]: row r's first job
//   groups     every row's jobs cut into groups of at most g consecutive jobs, in job order: no group holds jobs of two rows, and only
//              a row's last group is short.  An entry is first job | count << 16 (a pass has at most 65535 jobs).  g = 0: no groups.
//              For the rectangle (S jobs on each of K blobs) entry r * ceil(S / g) + i starts at job r * S + i * g.
//   passes     jobs_per_pass is the largest p in [1, min(n_jobs, 65535)] whose workspace — ws(min(n_blobs, p), p), growing with p — is
//              within the limit, 1 when not even one job is; ceil(n_jobs / jobs_per_pass) passes over the sorted list, their sizes equal
//              to within one, the larger ones first.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace frieda {

constexpr uint32_t PROVE_JOBS_PASS_MAX = 65535;  // the jobs of one launch chain (blockIdx.y, and 16 bits of a group entry)

// order[y] = the caller's index of the y-th job of the list sorted by blob_index (stable); every blob_index[j] < n_blobs
inline void prove_jobs_sort(const uint32_t* blob_index, size_t n_jobs, uint32_t n_blobs, std::vector<uint32_t>& order) {
    std::vector<size_t> at((size_t)n_blobs + 1, 0);
    for (size_t j = 0; j < n_jobs; j++) at[blob_index[j] + 1]++;
    for (uint32_t b = 0; b < n_blobs; b++) at[b + 1] += at[b];
    order.resize(n_jobs);
    for (size_t j = 0; j < n_jobs; j++) order[at[blob_index[j]]++] = (uint32_t)j;
}

// slot_of[order[y]] = y
inline void prove_jobs_invert(const std::vector<uint32_t>& order, std::vector<uint32_t>& slot_of) {
    slot_of.resize(order.size());
    for (size_t y = 0; y < order.size(); y++) slot_of[order[y]] = (uint32_t)y;
}

struct ProveJobsRows {
    std::vector<uint32_t> blobs;      // row r is blob blobs[r]
    std::vector<uint32_t> job_row;    // n entries
    std::vector<uint32_t> row_first;  // rows + 1 entries: row r's jobs are [row_first[r], row_first[r + 1])
};

// the rows of n jobs whose blob numbers, sorted_blob[0 .. n), do not decrease
inline void prove_jobs_rows(const uint32_t* sorted_blob, uint32_t n, ProveJobsRows& out) {
    out.blobs.clear();
    out.row_first.clear();
    out.job_row.resize(n);
    for (uint32_t y = 0; y < n; y++) {
        if (y == 0 || sorted_blob[y] != sorted_blob[y - 1]) {
            out.blobs.push_back(sorted_blob[y]);
            out.row_first.push_back(y);
        }
        out.job_row[y] = (uint32_t)out.blobs.size() - 1;
    }
    out.row_first.push_back(n);
}

inline uint32_t prove_jobs_group_entry(uint32_t first, uint32_t count) { return first | count << 16; }
inline uint32_t prove_jobs_group_first(uint32_t entry) { return entry & 0xFFFFu; }
inline uint32_t prove_jobs_group_count(uint32_t entry) { return entry >> 16; }

// the groups of n <= 65535 jobs of rows row_first[0 .. rows]; g = 0: none
inline void prove_jobs_groups(const std::vector<uint32_t>& row_first, uint32_t g, std::vector<uint32_t>& groups) {
    groups.clear();
    if (g == 0) return;
    for (size_t r = 0; r + 1 < row_first.size(); r++)
        for (uint32_t y = row_first[r]; y < row_first[r + 1]; y += std::min(g, row_first[r + 1] - y))
            groups.push_back(prove_jobs_group_entry(y, std::min(g, row_first[r + 1] - y)));
}

// ws(n_blobs, n_jobs): the workspace bytes of one pass, growing with either count
template <class Ws>
inline uint32_t prove_jobs_per_pass(uint64_t n_jobs, uint32_t n_blobs, uint64_t limit, Ws ws) {
    uint32_t lo = 1, hi = (uint32_t)std::min<uint64_t>(n_jobs, PROVE_JOBS_PASS_MAX);  // the answer is in [lo, hi]; lo fits, or is 1
    auto fits = [&](uint32_t p) { return (uint64_t)ws(std::min(n_blobs, p), p) <= limit; };
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (fits(mid))
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

inline uint64_t prove_jobs_n_passes(uint64_t n_jobs, uint32_t per_pass) { return per_pass ? (n_jobs + per_pass - 1) / per_pass : 0; }

// the size of pass i of n_passes (equal to within one, the larger first)
inline uint32_t prove_jobs_pass_size(uint64_t n_jobs, uint64_t n_passes, uint64_t i) {
    return (uint32_t)(n_jobs / n_passes + (i < n_jobs % n_passes ? 1 : 0));
}

}  // namespace frieda
