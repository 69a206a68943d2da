"""Shared helpers of the block-proof tests: the block challenge from the oracle's channel, QM31 arithmetic on numpy uint64 columns with
the oracle's fo_qm31_mul as the only multiplication rule, and the aggregate of a block computed from the definition
(sum over k of rho^k * f_k, powers first — not the Horner form of the kernel)."""
import ctypes as C

import numpy as np

P = 2**31 - 1


def oracle_rho(oracle, commitments):
    """a default channel, mix_u64(K), mix_root of every commitment in order, one draw_felt"""
    L = oracle.lib()
    ch = oracle.Channel()
    L.fo_channel_init(C.byref(ch))
    L.fo_channel_mix_u64(C.byref(ch), len(commitments))
    for c in commitments:
        buf = (C.c_uint8 * 32)(*bytes(c))
        L.fo_channel_mix_root(C.byref(ch), buf)
    out = (C.c_uint32 * 4)()
    L.fo_channel_draw_felt(C.byref(ch), out)
    return tuple(int(x) for x in out)


def qm_mul(oracle, x, y):
    a = (C.c_uint32 * 4)(*[int(v) for v in x])
    b = (C.c_uint32 * 4)(*[int(v) for v in y])
    out = (C.c_uint32 * 4)()
    oracle.lib().fo_qm31_mul(a, b, out)
    return tuple(int(v) for v in out)


def qm_matrix(oracle, s):
    """multiplication by s as a 4 x 4 matrix over M31: column j is s times the j-th basis element"""
    m = np.zeros((4, 4), dtype=np.uint64)
    for j in range(4):
        e = [0, 0, 0, 0]
        e[j] = 1
        m[:, j] = qm_mul(oracle, s, e)
    return m


def qm_scale_columns(oracle, s, cols):
    """s * cols, cols uint [4, N] read as N QM31 values"""
    m = qm_matrix(oracle, s)
    cols = np.asarray(cols, dtype=np.uint64)
    out = np.zeros_like(cols)
    for r in range(4):
        for j in range(4):
            out[r] = (out[r] + (m[r, j] * cols[j]) % P) % P
    return out


def aggregate_reference(oracle, evals, rho):
    """sum over k of rho^k * evals[k]: uint32 [4, N]"""
    acc = np.zeros(np.asarray(evals[0]).shape, dtype=np.uint64)
    power = (1, 0, 0, 0)
    for ev in evals:
        acc = (acc + qm_scale_columns(oracle, power, ev)) % P
        power = qm_mul(oracle, power, rho)
    return acc.astype(np.uint32)


def combine_values(oracle, values, rho):
    """values uint32 [K, 4]: sum over k of rho^k * values[k] -> 4 words"""
    return tuple(int(v) for v in aggregate_reference(oracle, [np.asarray(v, dtype=np.uint64).reshape(4, 1) for v in values], rho)[:, 0])
