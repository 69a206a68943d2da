// prove_jobs_plan.h against the rules of a frieda_prove_jobs call written out here once more: the stable sort by blob and the permutation
// back, the rows of the distinct blobs, the cut of every blob's run into groups of at most g jobs, the rectangle's table as
// frieda_prove_seeds_blobs always staged it, and the cut of a list into passes.  Stand-alone; prints OK.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <random>
#include <vector>

#include "prove_jobs_plan.h"

using namespace frieda;

static long checks = 0;
static const char* g_case = "";
static uint32_t g_group = 0;
#define EXPECT(cond)                                                                       \
    do {                                                                                   \
        checks++;                                                                          \
        if (!(cond)) {                                                                     \
            printf("FAILED %s:%d: %s (list: %s, group %u)\n", __FILE__, __LINE__, #cond, g_case, g_group); \
            exit(1);                                                                       \
        }                                                                                  \
    } while (0)

static const uint32_t GROUPS[] = {0, 1, 2, 4, 8, 65535};

struct Job {
    uint32_t blob;
    uint64_t seed;
};

static void check_list(const char* name, const std::vector<Job>& jobs, uint32_t n_blobs) {
    g_case = name;
    g_group = 0;
    const size_t n = jobs.size();
    std::vector<uint32_t> bidx(n);
    for (size_t j = 0; j < n; j++) bidx[j] = jobs[j].blob;
    std::vector<uint32_t> order, slot_of;
    prove_jobs_sort(bidx.data(), n, n_blobs, order);
    prove_jobs_invert(order, slot_of);
    // a permutation, sorted by blob, the caller's order kept inside a blob's run; the inverse inverts it
    EXPECT(order.size() == n && slot_of.size() == n);
    std::vector<char> seen(n, 0);
    for (size_t y = 0; y < n; y++) {
        EXPECT(order[y] < n && !seen[order[y]]);
        seen[order[y]] = 1;
        EXPECT(slot_of[order[y]] == y);
        if (y) {
            EXPECT(bidx[order[y - 1]] <= bidx[order[y]]);
            if (bidx[order[y - 1]] == bidx[order[y]]) EXPECT(order[y - 1] < order[y]);
        }
    }
    {  // the same order as the standard library's stable sort
        std::vector<uint32_t> want(n);
        for (size_t j = 0; j < n; j++) want[j] = (uint32_t)j;
        std::stable_sort(want.begin(), want.end(), [&](uint32_t a, uint32_t b) { return bidx[a] < bidx[b]; });
        EXPECT(want == order);
    }
    std::vector<uint32_t> sorted(n);
    for (size_t y = 0; y < n; y++) sorted[y] = bidx[order[y]];
    // rows: the distinct blobs, ascending; every job in its blob's row; a row's jobs one run
    ProveJobsRows rows;
    prove_jobs_rows(sorted.data(), (uint32_t)n, rows);
    std::vector<uint32_t> distinct(bidx);
    std::sort(distinct.begin(), distinct.end());
    distinct.erase(std::unique(distinct.begin(), distinct.end()), distinct.end());
    EXPECT(rows.blobs == distinct);
    EXPECT(rows.job_row.size() == n && rows.row_first.size() == distinct.size() + 1);
    EXPECT(rows.row_first.front() == 0 && rows.row_first.back() == n);
    for (size_t y = 0; y < n; y++) {
        const uint32_t r = rows.job_row[y];
        EXPECT(r < rows.blobs.size() && rows.blobs[r] == sorted[y]);
        EXPECT(rows.row_first[r] <= y && y < rows.row_first[r + 1]);
    }
    std::vector<uint32_t> jobs_of(n_blobs, 0);
    for (size_t j = 0; j < n; j++) jobs_of[bidx[j]]++;
    for (size_t r = 0; r < rows.blobs.size(); r++) EXPECT(rows.row_first[r + 1] - rows.row_first[r] == jobs_of[rows.blobs[r]]);
    for (uint32_t g : GROUPS) {
        g_group = g;
        std::vector<uint32_t> groups;
        prove_jobs_groups(rows.row_first, g, groups);
        if (g == 0) {
            EXPECT(groups.empty());
            continue;
        }
        EXPECT(groups.size() <= n);  // at most one entry per job: what the workspace plans
        // every job in exactly one group, the groups in job order; no group of two blobs or of more than g jobs; only a run's last is short
        size_t next = 0, expect_groups = 0;
        for (size_t r = 0; r < rows.blobs.size(); r++) expect_groups += (rows.row_first[r + 1] - rows.row_first[r] + (size_t)g - 1) / g;
        EXPECT(groups.size() == expect_groups);
        for (size_t i = 0; i < groups.size(); i++) {
            const uint32_t first = prove_jobs_group_first(groups[i]), count = prove_jobs_group_count(groups[i]);
            EXPECT(groups[i] == prove_jobs_group_entry(first, count));
            EXPECT(first == next && count >= 1 && count <= g && first + count <= n);
            const uint32_t r = rows.job_row[first];
            for (uint32_t y = first; y < first + count; y++) EXPECT(rows.job_row[y] == r);
            EXPECT((first - rows.row_first[r]) % g == 0);                       // a run's groups start g apart: contiguous, full ...
            if (count < g) EXPECT(first + count == rows.row_first[r + 1]);       // ... but the last
            next = first + count;
        }
        EXPECT(next == n);
    }
}

// the rectangle of frieda_prove_seeds_blobs: K blobs under S seeds, blob-major.  Its table was job_row[r * S + s] = r and, with
// gpb = ceil(S / g) groups per blob, group_first[r * gpb + i] = r * S + i * g, a group ending at min(first + g, (r + 1) * S)
static void check_rectangle(uint32_t K, uint32_t S) {
    g_case = "rectangle";
    std::vector<uint32_t> bidx((size_t)K * S);
    for (uint32_t y = 0; y < K * S; y++) bidx[y] = y / S;
    std::vector<uint32_t> order;
    prove_jobs_sort(bidx.data(), bidx.size(), K, order);
    for (uint32_t y = 0; y < K * S; y++) EXPECT(order[y] == y);  // sorted as it stands
    ProveJobsRows rows;
    prove_jobs_rows(bidx.data(), K * S, rows);
    EXPECT(rows.blobs.size() == K);
    for (uint32_t r = 0; r < K; r++)
        for (uint32_t s = 0; s < S; s++) EXPECT(rows.job_row[r * S + s] == r);
    for (uint32_t g : GROUPS) {
        g_group = g;
        std::vector<uint32_t> groups;
        prove_jobs_groups(rows.row_first, g, groups);
        const uint32_t gpb = g ? (S + g - 1) / g : 0;
        EXPECT(groups.size() == (size_t)K * gpb);
        for (uint32_t r = 0; r < K; r++)
            for (uint32_t i = 0; i < gpb; i++) {
                const uint32_t first = r * S + i * g, end = std::min<uint64_t>((uint64_t)first + g, (uint64_t)(r + 1) * S);
                EXPECT(prove_jobs_group_first(groups[r * gpb + i]) == first);
                EXPECT(prove_jobs_group_count(groups[r * gpb + i]) == end - first);
            }
    }
}

// the pass rule for a workspace of a + b * blobs + c * jobs bytes
static void check_passes(uint64_t n_jobs, uint32_t n_blobs, uint64_t a, uint64_t b, uint64_t c, uint64_t limit) {
    g_case = "passes";
    auto ws = [&](uint32_t kb, uint32_t p) { return a + b * kb + c * p; };
    const uint32_t per = prove_jobs_per_pass(n_jobs, n_blobs, limit, ws);
    const uint64_t cap = std::min<uint64_t>(n_jobs, 65535);
    EXPECT(per >= 1 && per <= cap);
    // the largest p within the limit, by walking down from the cap; 1 when none is
    uint64_t want = 1;
    for (uint64_t p = cap; p >= 1; p--)
        if (ws((uint32_t)std::min<uint64_t>(n_blobs, p), (uint32_t)p) <= limit) {
            want = p;
            break;
        }
    EXPECT(per == want);
    const uint64_t n_passes = prove_jobs_n_passes(n_jobs, per);
    EXPECT(n_passes == (n_jobs + per - 1) / per);
    uint64_t sum = 0;
    uint32_t lo = ~0u, hi = 0;
    for (uint64_t i = 0; i < n_passes; i++) {
        const uint32_t sz = prove_jobs_pass_size(n_jobs, n_passes, i);
        EXPECT(sz >= 1 && sz <= per && sz <= 65535);
        if (i) EXPECT(sz <= prove_jobs_pass_size(n_jobs, n_passes, i - 1));
        lo = std::min(lo, sz), hi = std::max(hi, sz);
        sum += sz;
    }
    EXPECT(sum == n_jobs && hi - lo <= 1);
}

int main() {
    std::mt19937_64 rng(0x6a6f6273);
    // the hand-made lists
    check_list("one job", {{0, 7}}, 1);
    check_list("one job of the last blob", {{4, 7}}, 5);
    {
        std::vector<Job> v;
        for (uint32_t j = 0; j < 37; j++) v.push_back({0, 100 + j});
        check_list("all jobs on one blob", v, 1);
        for (Job& x : v) x.blob = 2;
        check_list("all jobs on one blob of four", v, 4);
    }
    {
        std::vector<Job> v;
        for (uint32_t b = 0; b < 19; b++) v.push_back({18 - b, b});
        check_list("one job per blob, descending", v, 19);
    }
    check_list("a blob with no job", {{3, 1}, {0, 2}, {3, 3}, {0, 4}, {0, 5}}, 4);
    check_list("repeated pairs", {{1, 9}, {1, 9}, {0, 9}, {1, 9}, {0, 9}, {2, 1}}, 3);
    check_list("the queue of the GPU tests", {{2, 11}, {0, 13}, {2, ~0ull}, {1, 11}, {0, 11}, {2, 13}, {2, 0}, {0, 11}, {2, 11}}, 4);
    {
        std::vector<Job> v(65535);
        for (uint32_t j = 0; j < 65535; j++) v[j] = {(uint32_t)(rng() % 300), rng()};
        check_list("65535 jobs over 300 blobs", v, 300);
        for (uint32_t j = 0; j < 65535; j++) v[j].blob = 0;
        check_list("65535 jobs on one blob", v, 1);
        for (uint32_t j = 0; j < 65535; j++) v[j].blob = 65534 - j;
        check_list("65535 jobs, one per blob, descending", v, 65535);
    }
    // random lists: few blobs with long runs, many blobs with short ones
    for (int it = 0; it < 300; it++) {
        const uint32_t n_blobs = 1 + (uint32_t)(rng() % (it % 3 == 0 ? 3 : 40));
        const size_t n = 1 + (size_t)(rng() % 200);
        std::vector<Job> v(n);
        for (Job& x : v) x = {(uint32_t)(rng() % n_blobs), rng() % 4};
        check_list("random", v, n_blobs);
    }
    for (uint32_t K : {1u, 2u, 3u, 7u, 64u})
        for (uint32_t S : {1u, 2u, 3u, 4u, 5u, 8u, 9u, 17u, 64u, 1023u}) check_rectangle(K, S);
    check_rectangle(255, 257);  // 65535 jobs
    check_rectangle(1, 65535);
    check_rectangle(65535, 1);
    // passes
    for (uint64_t n_jobs : {1ull, 2ull, 9ull, 11ull, 100ull, 65535ull, 65536ull, 200000ull})
        for (uint32_t n_blobs : {1u, 4u, 1000u})
            for (uint64_t limit : {0ull, 999ull, 1000ull, 1099ull, 1100ull, 1101ull, 4000ull, 4399ull, 4400ull, 1000000ull, ~0ull >> 1})
                check_passes(n_jobs, n_blobs, 700, 100, 1000, limit);
    for (int it = 0; it < 2000; it++)
        check_passes(1 + rng() % 100000, 1 + (uint32_t)(rng() % 64), rng() % 5000, rng() % 300, 1 + rng() % 3000, rng() % 3000000);
    printf("%ld checks OK\n", checks);
    return 0;
}
