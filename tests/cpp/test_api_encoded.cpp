// test_api_encoded.cpp — the C++ wrappers of include/frieda.hpp for encoded handles of a block and from a rebuild
// (Context::encode_batch, Context::rebuild_encoded_*), called as a C++ integrator would: host code only, runs on the GPU box
// (tests/test_gpu_api_encoded.py).  Three 1 KiB blobs at blowup 2^4 (2^7 coefficients per column, a 2^11 codeword), cells of 8 entries.
#include <cstdio>
#include <cstring>
#include <vector>

#include "frieda.hpp"

using namespace frieda;

#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            return 1;                                                    \
        }                                                                \
    } while (0)

int main() {
    const uint32_t K = 3, B = 4, c = 3;
    const size_t len = 1024, stride = 1024 + 40;
    std::vector<uint8_t> flat(stride * K, 0xA5);
    std::vector<std::vector<uint8_t>> blobs(K, std::vector<uint8_t>(len));
    for (uint32_t b = 0; b < K; b++)
        for (size_t i = 0; i < len; i++) flat[b * stride + i] = blobs[b][i] = (uint8_t)(i * 31 + b * 7 + (i >> 5));
    Context ctx(0);

    // encode_batch: handle b is the lone handle of blob b
    std::vector<Encoded> encs = ctx.encode_batch(flat.data(), stride, len, K, B);
    CHECK(encs.size() == K);
    std::vector<Commitment> coms;
    for (uint32_t b = 0; b < K; b++) {
        Encoded lone = ctx.encode(blobs[b].data(), len, B);
        CHECK(encs[b].commitment() == lone.commitment() && encs[b].shape() == lone.shape() && encs[b].bytes() == lone.bytes());
        coms.push_back(lone.commitment());
    }
    const uint32_t L = encs[0].shape().first, n = encs[0].shape().second;
    CHECK(L == 7 && n == 11);
    const uint32_t need = (1u << (L - c)) + 1;
    std::vector<uint32_t> idx;
    for (uint32_t i = 0; i < need; i++) idx.push_back((i * 37 + 5) % (1u << (n - c)));  // 37 is odd: distinct

    // one blob from opened cells, with and without the bytes
    Context::OpenedCells oc = ctx.open_cells(encs[1], c, idx);
    std::vector<uint8_t> status;
    size_t used = 0;
    Context::RebuiltEncoded r = ctx.rebuild_encoded_from_opened_cells(coms[1], B, len, c, idx, oc.values, oc.paths, true, &status, &used);
    CHECK(r.bytes.size() == 1 && r.bytes[0] == blobs[1] && r.encs.size() == 1 && r.encs[0].commitment() == coms[1] && used == need);
    CHECK(status.size() == need);
    r = ctx.rebuild_encoded_from_opened_cells(coms[1], B, len, c, idx, oc.values, oc.paths, false);
    CHECK(r.bytes.empty() && r.encs.size() == 1 && r.encs[0].commitment() == coms[1]);
    // the rebuilt handle serves: the same cells again
    Context::OpenedCells again = ctx.open_cells(r.encs[0], c, idx);
    CHECK(again.values == oc.values && again.paths == oc.paths);
    // too few cells: an Error, statuses and count still reported
    {
        std::vector<uint32_t> fewer(idx.begin(), idx.end() - 1);
        std::vector<uint32_t> fv(oc.values.begin(), oc.values.end() - (4u << c));
        std::vector<uint8_t> fp(oc.paths.begin(), oc.paths.end() - 32 * (n - c));
        bool threw = false;
        try {
            ctx.rebuild_encoded_from_opened_cells(coms[1], B, len, c, fewer, fv, fp, true, &status, &used);
        } catch (const Error&) {
            threw = true;
        }
        CHECK(threw && used == need - 1 && status.size() == need - 1);
    }

    // one blob from cell bundles (the provider's half through the C ABI: two bundles)
    {
        std::vector<uint32_t> sorted(idx);
        std::sort(sorted.begin(), sorted.end());
        const std::vector<uint32_t> first = {0, need / 2, need};
        std::vector<uint64_t> wfirst(3, 0);
        CHECK(frieda_open_cell_bundles(ctx.handle(), encs[2].handle(), c, sorted.data(), first.data(), 2, nullptr, nullptr, 0, wfirst.data()) == FRIEDA_OK);
        std::vector<uint32_t> values((sorted.size() * 4) << c);
        std::vector<uint8_t> witness(32 * wfirst[2] + 32);
        CHECK(frieda_open_cell_bundles(ctx.handle(), encs[2].handle(), c, sorted.data(), first.data(), 2, values.data(), witness.data(), wfirst[2], wfirst.data()) ==
              FRIEDA_OK);
        witness.resize(32 * wfirst[2]);
        r = ctx.rebuild_encoded_from_cell_bundles(coms[2], B, len, c, sorted, first, values, witness, wfirst, true, &status, &used);
        CHECK(r.bytes.size() == 1 && r.bytes[0] == blobs[2] && r.encs[0].commitment() == coms[2] && used == need && status.size() == 2);
    }

    // the block from stripes and from stripe bundles
    std::vector<const Encoded*> ptrs;
    for (const Encoded& e : encs) ptrs.push_back(&e);
    {
        std::vector<uint32_t> bidx, cidx;
        for (uint32_t s = 0; s < need; s++)
            for (uint32_t b = 0; b < K; b++) bidx.push_back(b), cidx.push_back(idx[s]);
        Context::OpenedCells st = ctx.open_cells_blobs(ptrs, c, bidx, cidx);
        r = ctx.rebuild_encoded_blobs_from_opened_stripes(coms, B, len, c, idx, st.values, st.paths, true, &status, &used);
        CHECK(r.bytes == blobs && r.encs.size() == K && used == need && status.size() == (size_t)need * K);
        for (uint32_t b = 0; b < K; b++) CHECK(r.encs[b].commitment() == coms[b]);
        // the handles of the block are freed one by one: the middle one first, the others still serve
        r.encs[1] = Encoded();
        Context::OpenedCells o0 = ctx.open_cells(r.encs[0], c, idx), w0 = ctx.open_cells(encs[0], c, idx);
        CHECK(o0.values == w0.values && o0.paths == w0.paths);
    }
    {
        std::vector<uint32_t> sorted(idx);
        std::sort(sorted.begin(), sorted.end());
        const std::vector<uint32_t> first = {0, 3, need};
        Context::OpenedStripeBundles sb = ctx.open_stripe_bundles(ptrs, c, sorted, first);
        r = ctx.rebuild_encoded_blobs_from_stripe_bundles(coms, B, len, c, sorted, first, sb.values, sb.witness, sb.witness_first, false, &status, &used);
        CHECK(r.bytes.empty() && r.encs.size() == K && used == need && status.size() == 2 * K);
        for (uint32_t b = 0; b < K; b++) CHECK(r.encs[b].commitment() == coms[b]);
    }
    std::printf("ok\n");
    return 0;
}
