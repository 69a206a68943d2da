// cells_pass.h against the formulas of the cells verifier written out here once more: cells per pass, 256-byte rounding, the order of
// the staged image (indices | [blob numbers] | values | paths), what a pass asks of the pinned block and the arena, and whole calls
// walked pass by pass.  Stand-alone (UBSan: tests/test_host_sanitizers.py); prints OK.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>

#include "cells_pass.h"

using namespace frieda;

static long checks = 0;
#define EXPECT(cond)                                                         \
    do {                                                                     \
        checks++;                                                            \
        if (!(cond)) {                                                       \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);         \
            printf("  log_cell %u depth %u n_blobs %u stripes %d n_cells %zu budget %zu\n", g.log_cell, g.depth, g.n_blobs, (int)g.stripes, g_cells, g_budget); \
            exit(1);                                                         \
        }                                                                    \
    } while (0)

static CellsPassShape g;
static size_t g_cells, g_budget;

static size_t al(size_t b) { return (b + 255) / 256 * 256; }

// the two expressions the verifiers were written with
static size_t per_pass_one(size_t budget, size_t vb, size_t pb) { return std::max<size_t>(1, budget / (4 + vb + pb)); }
static size_t per_pass_blobs(size_t n_cells, size_t budget, size_t group, size_t vb, size_t pb) {
    return std::min<size_t>(n_cells, std::max<size_t>(1, budget / (group * (8 + vb + pb))) * group);
}

static void check_plan(size_t np) {
    const size_t vb = (size_t)16 << g.log_cell, pb = 32 * (size_t)g.depth;
    const CellsPassPlan p = cells_pass_plan(g, np);
    // the image, piece by piece
    size_t at = 0;
    EXPECT(p.i_idx == at);
    at += al(4 * np);
    if (g.n_blobs) {
        EXPECT(p.i_bidx == at);
        at += al(4 * np);
    }
    EXPECT(p.i_val == at);
    at += al(vb * np);
    EXPECT(p.i_path == at);
    at += al(pb * np);
    EXPECT(p.in_bytes == at);
    EXPECT(p.i_val % 256 == 0 && p.i_path % 256 == 0 && p.in_bytes % 256 == 0);
    if (g.depth == 0) EXPECT(p.in_bytes == p.i_path);  // no paths
    // results and table behind it in the pinned block
    const size_t ns = g.stripes ? np / g.n_blobs : 0, rows = g.n_blobs ? ns : np;
    EXPECT(p.n_stripes == ns && p.n_rows == rows);
    EXPECT(p.res_bytes == al(4 * np) + 4 * ns);
    EXPECT(p.p_res == p.in_bytes && p.p_tab == p.in_bytes + al(p.res_bytes));
    EXPECT(p.pinned == std::max(al(32 * (size_t)g.n_blobs), p.in_bytes + al(al(4 * np) + 4 * ns) + 8 * rows));
    // the arena: [commitments] | image | roots | bad | results | table, each from a 256-byte boundary
    at = 0;
    if (g.n_blobs) {
        EXPECT(p.a_com == 0);
        at = al(32 * (size_t)g.n_blobs);
    }
    EXPECT(p.a_in == at);
    at += al(p.in_bytes);
    EXPECT(p.a_roots == at);
    at += al(32 * np);
    EXPECT(p.a_bad == at);
    at += al(4 * np);
    EXPECT(p.a_res == at);
    at += al(p.res_bytes);
    EXPECT(p.a_tab == at);
    at += al(8 * rows);
    EXPECT(p.arena == at);
}

static size_t expected_per_pass(size_t n_cells, size_t budget) {
    const size_t vb = (size_t)16 << g.log_cell, pb = 32 * (size_t)g.depth;
    // (the one-commitment loop took min(per_pass, what is left): its first pass is min(per_pass, n_cells) cells)
    return g.n_blobs ? per_pass_blobs(n_cells, budget, g.stripes ? g.n_blobs : 1, vb, pb) : std::min(n_cells, per_pass_one(budget, vb, pb));
}

static void walk_call(size_t n_cells, size_t budget) {
    const size_t group = g.stripes ? g.n_blobs : 1;
    const size_t per = cells_per_pass(g, n_cells, budget);
    const CellsPassPlan first = cells_pass_plan(g, per);
    size_t covered = 0, passes = 0;
    for (size_t at = 0; at < n_cells; at += per) {
        const size_t np = std::min(per, n_cells - at);
        EXPECT(at == covered);            // the passes partition [0, n_cells)
        EXPECT(at % group == 0 && np % group == 0 && np >= group);  // no stripe straddles a pass
        const CellsPassPlan p = cells_pass_plan(g, np);
        EXPECT(p.arena <= first.arena && p.pinned <= first.pinned);  // every later pass fits the plan of the first
        EXPECT(p.a_com == first.a_com && p.a_in == first.a_in);      // (the commitments stay where the call put them)
        check_plan(np);
        covered += np;
        passes++;
    }
    EXPECT(covered == n_cells && passes == (n_cells + per - 1) / per);
}

int main() {
    const size_t cell_counts[] = {1, 63, 64, 65, 300};
    const uint32_t groups[] = {1, 3, 256};
    const size_t walked[] = {1, 4000, 40000, (size_t)32 << 20};
    EXPECT(CELLS_PASS_BYTES == (size_t)32 << 20);
    for (size_t b = 0; b < 2000; b++) EXPECT(cells_al(b) == al(b) && cells_al(b) % 256 == 0 && cells_al(b) >= b && cells_al(b) < b + 256);
    for (uint32_t log_cell = 0; log_cell <= 10; log_cell++)
        for (uint32_t depth = 0; depth <= 12; depth++)
            for (int form = 0; form < 3; form++)  // one commitment, many blobs, stripes
                for (uint32_t blobs : groups) {
                    if (form == 0 && blobs != 1) continue;
                    g = CellsPassShape{log_cell, depth, form == 0 ? 0u : blobs, form == 2};
                    const size_t group = form == 2 ? blobs : 1;
                    const size_t staged = (form == 0 ? 4 : 8) + ((size_t)16 << log_cell) + 32 * (size_t)depth;
                    EXPECT(g.value_bytes() == (size_t)16 << log_cell && g.path_bytes() == 32 * (size_t)depth && g.group() == group);
                    for (size_t count : cell_counts) {
                        const size_t n_cells = count * group;  // (a stripes call holds whole stripes)
                        g_cells = n_cells;
                        // budgets: one byte, the default, and exactly k cells (or stripes) and one byte less, for a few k
                        size_t budgets[2 + 2 * 4] = {1, CELLS_PASS_BYTES};
                        size_t nb = 2;
                        for (size_t k : {(size_t)1, (size_t)2, (size_t)5, (size_t)64}) budgets[nb++] = k * group * staged, budgets[nb++] = k * group * staged - 1;
                        for (size_t i = 0; i < nb; i++) {
                            const size_t budget = g_budget = budgets[i];
                            const size_t per = cells_per_pass(g, n_cells, budget);
                            EXPECT(per == expected_per_pass(n_cells, budget));
                            EXPECT(per >= group && per <= n_cells && per % group == 0);
                            if (budget == 1) EXPECT(per == group);  // one cell, or one whole stripe, is always admitted
                            if (i >= 2) {
                                const size_t k = (budget + 1) / (group * staged);  // exactly k, or one byte less: k - 1, but never none
                                const size_t want = (i % 2 == 0 ? k : std::max<size_t>(1, k - 1)) * group;
                                EXPECT(per == std::min(n_cells, want));
                            }
                            check_plan(per);
                        }
                        for (size_t budget : walked) {
                            g_budget = budget;
                            walk_call(n_cells, budget);
                        }
                    }
                }
    printf("OK %ld checks\n", checks);
    return 0;
}
