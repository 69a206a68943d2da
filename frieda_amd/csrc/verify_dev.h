// verify_dev.h — what the device verifiers of whole proofs share (verify.hip: one wave per proof; verify_split.hip: a wave per proof for
// the value chain and a wave per (proof, layer) for the Merkle walks): the domain points of a layer and the QM31 loads.
//
// The generator's doublings sit in constant memory, one table per translation unit that includes this header (the anonymous namespace):
// each unit uploads its own through upload_gen_pow2, once per device (verify_many.cpp: init_device_tables).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dev_transcript.h"
#include "kernels.h"

namespace frieda {
namespace k {

namespace {

__constant__ CPoint c_gen_pow2[31];  // 2^b * G of the circle group's generator (host: point_from_index)

inline hipError_t upload_gen_pow2(const CPoint (&gen_pow2)[31]) { return hipMemcpyToSymbol(HIP_SYMBOL(c_gen_pow2), gen_pow2, sizeof(gen_pow2)); }

__device__ __forceinline__ CPoint dev_point_from_index(uint32_t index) {
    CPoint res{1, 0};
    index &= 0x7fffffffu;
    for (uint32_t b = 0; index; b++, index >>= 1)
        if (index & 1u) res = cp_add(res, c_gen_pow2[b]);
    return res;
}

// point index of entry `i` of line_coset(n, n - li) (li = 0: Coset::half_odds(n - 1) itself)
__device__ __forceinline__ uint32_t coset_index(uint32_t n, uint32_t doublings, uint32_t i) {
    const unsigned long long init = (1ull << (30 - n)) << doublings, step = (1ull << (32 - n)) << doublings;
    return (uint32_t)((init + step * i) & 0x7fffffffull);
}

__device__ __forceinline__ QM31 load_qm(const uint32_t* p) { return QM31{p[0], p[1], p[2], p[3]}; }

constexpr uint32_t LAST_LOG_MAX = 11;  // log2 of DT_MAX_LAST_POLY
static_assert((1u << LAST_LOG_MAX) == DT_MAX_LAST_POLY, "the last-layer fold keeps one stack entry per bit of a coefficient index");

// LinePoly::eval_at_point of the last layer's np = 2^plog coefficients at the domain point with x-coordinate x.
// fold(coeffs, doublings) of LinePoly::eval_at_point, bottom up in one pass over the coefficients: bit b of a coefficient's
// index carries x doubled (plog - 1 - b) times; stk[b] holds the folded left half of an open 2^(b+1) block.  j is uniform
// over the wave, so the branches are scalar and the arrays stay in registers: np - 1 QM31 scalings per position.
__device__ __forceinline__ QM31 last_poly_eval_at(const uint32_t* last_poly, uint32_t np, uint32_t plog, uint32_t x) {
    uint32_t fb[LAST_LOG_MAX];
    {
        uint32_t xx = x;
#pragma unroll
        for (uint32_t b = 0; b < LAST_LOG_MAX; b++) fb[b] = 0;
#pragma unroll
        for (uint32_t d = 0; d < LAST_LOG_MAX; d++) {
#pragma unroll
            for (uint32_t b = 0; b < LAST_LOG_MAX; b++)
                if (b + d + 1 == plog) fb[b] = xx;
            xx = double_x(xx);
        }
    }
    QM31 stk[LAST_LOG_MAX], acc{0, 0, 0, 0};
#pragma unroll
    for (uint32_t b = 0; b < LAST_LOG_MAX; b++) stk[b] = QM31{0, 0, 0, 0};
    for (uint32_t j = 0; j < np; j++) {
        acc = load_qm(last_poly + 4 * (size_t)j);
        bool open = true;
#pragma unroll
        for (uint32_t b = 0; b < LAST_LOG_MAX; b++) {
            if (open) {
                if ((j >> b) & 1u) {
                    acc = qm_add(stk[b], qm_scale(acc, fb[b]));
                } else {
                    stk[b] = acc;
                    open = false;
                }
            }
        }
    }
    return acc;
}

}  // namespace

}  // namespace k
}  // namespace frieda
