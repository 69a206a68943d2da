// cells_pass.h — the arithmetic of one pass of the cells verifier (cells_host.cpp: verify_cells_passes): how many cells a pass takes, where
// the pieces of its staged image lie, and what it asks of the pinned block and the arena.  No HIP, no context: the cuts run on the CPU
// against the formulas written out again (tests/cpp/test_cells_pass.cpp).
//
// A call has one of three forms:
//   one commitment (n_blobs 0)     the commitment rides in the kernel arguments: no blob numbers are staged, no table is uploaded;
//   many blobs (n_blobs >= 1)      cell i belongs to blob blob_index[i]: the blob numbers are staged beside the indices, the commitments sit
//                                  in front of the pass buffers;
//   stripes (n_blobs >= 1, pooled) the cells are [n_cells / n_blobs][n_blobs]: a stripe's cells never straddle two passes.
// Cells per pass, with vb = 16 << log_cell bytes of values and pb = 32 * depth bytes of path per cell and a budget of `pass_bytes`:
//   one commitment:  max(1, pass_bytes / (4 + vb + pb))
//   many blobs:      min(n_cells, max(1, pass_bytes / (group * (8 + vb + pb))) * group),   group = n_blobs for stripes, else 1
// (one cell, or one whole stripe, is always admitted; the first pass is the largest, so a call plans its arena once, from that.)
// Staged image (pinned block -> arena, one copy): indices | [blob numbers] | values, cell-major as given | paths, level-major; every piece
// from a 256-byte boundary.  Behind it in the pinned block: the result words as they come back (a status word per cell, 256-byte rounded,
// then an accept word per stripe), then the gather table the host builds from them (two words per row: a row per cell of a one-commitment
// pass, per stripe of a stripes pass).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

namespace frieda {

constexpr size_t CELLS_PASS_BYTES = (size_t)32 << 20;  // the default budget of a pass

struct CellsPassShape {
    uint32_t log_cell, depth;  // depth = log_domain - log_cell: the hashes of a path
    uint32_t n_blobs;          // 0: one commitment
    bool stripes;
    size_t value_bytes() const { return (size_t)16 << log_cell; }
    size_t path_bytes() const { return 32 * (size_t)depth; }
    size_t group() const { return stripes ? n_blobs : 1; }  // cells that stay in one pass
};

inline size_t cells_al(size_t b) { return (b + 255) & ~(size_t)255; }

inline size_t cells_per_pass(const CellsPassShape& s, size_t n_cells, size_t pass_bytes) {
    const size_t staged = (s.n_blobs ? 8 : 4) + s.value_bytes() + s.path_bytes();  // bytes a cell stages
    return std::min(n_cells, std::max<size_t>(1, pass_bytes / (s.group() * staged)) * s.group());
}

struct CellsPassPlan {
    size_t i_idx, i_bidx, i_val, i_path, in_bytes;               // the staged image (i_bidx: with blobs only)
    size_t n_stripes, n_rows;                                    // accept words; rows the gather table can take
    size_t res_bytes, p_res, p_tab, pinned;                      // pinned block: results at p_res, table at p_tab, `pinned` bytes in all
    size_t a_com, a_in, a_roots, a_bad, a_res, a_tab, arena;     // arena offsets, `arena` bytes in all
};

// the plan of a pass of np cells (a multiple of the group)
inline CellsPassPlan cells_pass_plan(const CellsPassShape& s, size_t np) {
    CellsPassPlan p;
    p.n_stripes = s.stripes ? np / s.n_blobs : 0;
    p.n_rows = s.n_blobs ? p.n_stripes : np;
    p.i_idx = 0, p.i_bidx = cells_al(4 * np);
    p.i_val = s.n_blobs ? p.i_bidx + cells_al(4 * np) : p.i_bidx;
    p.i_path = p.i_val + cells_al(s.value_bytes() * np), p.in_bytes = p.i_path + cells_al(s.path_bytes() * np);
    p.res_bytes = cells_al(4 * np) + 4 * p.n_stripes;
    p.p_res = p.in_bytes, p.p_tab = p.p_res + cells_al(p.res_bytes);
    p.pinned = std::max(cells_al(32 * (size_t)s.n_blobs), p.p_tab + 8 * p.n_rows);  // (the commitments go up through the block first)
    size_t off = 0;
    auto take = [&off](size_t bytes) {
        const size_t o = off;
        off = cells_al(off + bytes);
        return o;
    };
    p.a_com = take(32 * (size_t)s.n_blobs), p.a_in = take(p.in_bytes), p.a_roots = take(32 * np), p.a_bad = take(4 * np);
    p.a_res = take(p.res_bytes), p.a_tab = take(8 * p.n_rows);
    p.arena = off;
    return p;
}

}  // namespace frieda
