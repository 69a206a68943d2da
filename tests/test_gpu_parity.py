"""GPU: the HIP path, called through the C ABI, against the oracle on the same seeded inputs — bit-exact.

Level B (one backend operation at a time) first, then Level A (commit / generate_proof / verify), then the
size-independent properties at BASELINE.json's full sizes where the oracle would take minutes.
"""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import pattern_bytes, splitmix64_bytes
from util import DevBuf, blob_len_for, load_vectors, resolve_input

pytestmark = pytest.mark.gpu

P = 2**31 - 1


def _check(ctx, rc):
    from frieda_amd.api import _check as chk

    chk(rc, ctx._h)


def rand_m31(rng, shape):
    return rng.integers(0, P, shape, dtype=np.uint32)


# ------------------------------------------------------------------------------------------------
# Level B
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_bytes", [0, 1, 3, 4, 14, 15, 16, 29, 30, 31, 58, 60, 61, 119, 1000, 1024, 4097, 65536, 262146])
def test_unpack30(gpu_ctx, oracle, n_bytes):
    data = splitmix64_bytes(11, n_bytes)
    coef, L = oracle.polynomial_from_bytes(data)
    n_out = coef.size
    d_in = DevBuf.from_array(gpu_ctx, data if n_bytes else np.zeros(4, np.uint8))
    d_out = DevBuf(gpu_ctx, 4 * n_out)
    _check(gpu_ctx, gpu_ctx._L.frieda_unpack30(gpu_ctx._h, d_in.ptr, n_bytes, d_out.ptr, n_out))
    got = d_out.to_array(np.uint32, (n_out,))
    assert np.array_equal(got, coef.ravel())
    # shape helper agrees with the reference's f64 rule
    nf, npad, lg = C.c_size_t(), C.c_size_t(), C.c_uint32()
    gpu_ctx._L.frieda_codec_shape(n_bytes, C.byref(nf), C.byref(npad), C.byref(lg))
    assert (npad.value, lg.value) == (n_out, L)


def test_unpack30_unaligned_pointer(gpu_ctx, oracle):
    data = splitmix64_bytes(12, 1001)
    coef, _ = oracle.polynomial_from_bytes(data[1:])
    d_in = DevBuf.from_array(gpu_ctx, data)
    d_out = DevBuf(gpu_ctx, 4 * coef.size)
    _check(gpu_ctx, gpu_ctx._L.frieda_unpack30(gpu_ctx._h, C.c_void_p(d_in.ptr.value + 1), 1000, d_out.ptr, coef.size))
    assert np.array_equal(d_out.to_array(np.uint32, (coef.size,)), coef.ravel())


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 8, 11, 14, 17, 20, 22])
def test_twiddles(gpu_ctx, oracle, n):
    tw, itw = oracle.precompute_twiddles(n)
    p_tw, p_itw = C.c_void_p(), C.c_void_p()
    _check(gpu_ctx, gpu_ctx._L.frieda_precompute_twiddles(gpu_ctx._h, n, C.byref(p_tw), C.byref(p_itw)))
    got = np.zeros(tw.size, np.uint32)
    goti = np.zeros(tw.size, np.uint32)
    _check(gpu_ctx, gpu_ctx._L.frieda_dev_download(gpu_ctx._h, got.ctypes.data, p_tw, got.nbytes))
    _check(gpu_ctx, gpu_ctx._L.frieda_dev_download(gpu_ctx._h, goti.ctypes.data, p_itw, goti.nbytes))
    assert np.array_equal(got, tw)
    assert np.array_equal(goti, itw)


@pytest.mark.parametrize(
    "L,n", [(0, 1), (1, 1), (0, 2), (1, 2), (2, 2), (0, 4), (2, 6), (7, 11), (9, 13), (12, 16), (13, 17), (14, 15), (16, 20), (18, 18), (5, 5)]
)
def test_circle_evaluate(gpu_ctx, oracle, L, n):
    rng = np.random.default_rng(100 + n)
    ncols = 4 if n < 20 else 2
    coef = rand_m31(rng, (ncols, 1 << L))
    exp = oracle.circle_evaluate(coef, n)
    d_c = DevBuf.from_array(gpu_ctx, coef)
    d_o = DevBuf(gpu_ctx, 4 * ncols << n)
    _check(gpu_ctx, gpu_ctx._L.frieda_circle_evaluate(gpu_ctx._h, d_c.ptr, ncols, L, n, d_o.ptr))
    got = d_o.to_array(np.uint32, (ncols, 1 << n))
    assert np.array_equal(got, exp)


# 7/8/9 and 17/18: either side of the nine-levels-per-launch kernel's range; 21, 22: that kernel in node mode above a wide launch
@pytest.mark.parametrize("m", [0, 1, 2, 5, 7, 8, 9, 10, 11, 12, 16, 17, 18, 21, 22])
def test_merkle_commit_all_layers(gpu_ctx, oracle, m):
    rng = np.random.default_rng(200 + m)
    cols = rand_m31(rng, (4, 1 << m))
    layers = oracle.merkle_commit(cols)
    d_c = DevBuf.from_array(gpu_ctx, cols)
    total = 32 * ((2 << m) - 1)
    d_l = DevBuf(gpu_ctx, total)
    _check(gpu_ctx, gpu_ctx._L.frieda_merkle_commit(gpu_ctx._h, d_c.ptr, m, d_l.ptr))
    buf = d_l.to_array(np.uint8, (total,))
    for l in range(m + 1):
        off = gpu_ctx._L.frieda_merkle_layer_offset(m, l)
        assert off == oracle.lib().fo_merkle_layer_offset(m, l)
        assert np.array_equal(buf[off : off + (32 << l)].reshape(-1, 32), layers[l]), f"layer {l}"
    d_r = DevBuf(gpu_ctx, 32)
    _check(gpu_ctx, gpu_ctx._L.frieda_merkle_root(gpu_ctx._h, d_c.ptr, m, d_r.ptr))
    assert bytes(d_r.to_array(np.uint8, (32,))) == bytes(layers[0][0])


@pytest.mark.parametrize("ncols,with_prev", [(4, False), (0, True), (1, False), (3, True), (16, False), (17, True), (40, True)])
def test_merkle_commit_layer_general_shapes(gpu_ctx, oracle, ncols, with_prev):
    """MerkleOps::commit_on_layer for arbitrary column counts (the trait surface, not only frieda's two shapes)."""
    log_size = 7
    rng = np.random.default_rng(300 + ncols)
    cols = rand_m31(rng, (ncols, 1 << log_size)) if ncols else None
    prev = rng.integers(0, 256, (2 << log_size, 32), dtype=np.uint8) if with_prev else None
    exp = oracle.merkle_commit_layer(log_size, prev, cols)
    d_prev = DevBuf.from_array(gpu_ctx, prev) if with_prev else None
    d_cols = [DevBuf.from_array(gpu_ctx, cols[i]) for i in range(ncols)]
    ptrs = (C.c_void_p * max(ncols, 1))(*[b.ptr for b in d_cols])
    d_out = DevBuf(gpu_ctx, 32 << log_size)
    _check(gpu_ctx, gpu_ctx._L.frieda_merkle_commit_layer(gpu_ctx._h, log_size, d_prev.ptr if d_prev else None, ptrs, ncols, d_out.ptr))
    assert np.array_equal(d_out.to_array(np.uint8, (1 << log_size, 32)), exp)


@pytest.mark.parametrize("n", [1, 2, 3, 6, 12, 16, 20, 22])
def test_fold_circle_into_line(gpu_ctx, oracle, n):
    rng = np.random.default_rng(400 + n)
    src = rand_m31(rng, (4, 1 << n))
    alpha = rand_m31(rng, (4,))
    for dst0 in (np.zeros((4, 1 << (n - 1)), np.uint32), rand_m31(rng, (4, 1 << (n - 1)))):
        exp = oracle.fold_circle_into_line(src, alpha, dst0.copy())
        d_s, d_d = DevBuf.from_array(gpu_ctx, src), DevBuf.from_array(gpu_ctx, dst0)
        _check(gpu_ctx, gpu_ctx._L.frieda_fold_circle_into_line(gpu_ctx._h, d_d.ptr, d_s.ptr, n, alpha.ctypes.data))
        assert np.array_equal(d_d.to_array(np.uint32, (4, 1 << (n - 1))), exp)


@pytest.mark.parametrize("n,m", [(2, 1), (3, 2), (6, 5), (6, 1), (12, 11), (12, 7), (16, 15), (16, 9), (20, 19), (22, 21), (22, 13)])
def test_fold_line(gpu_ctx, oracle, n, m):
    rng = np.random.default_rng(500 + 31 * n + m)
    src = rand_m31(rng, (4, 1 << m))
    alpha = rand_m31(rng, (4,))
    exp = oracle.fold_line(src, n, alpha)
    d_s, d_d = DevBuf.from_array(gpu_ctx, src), DevBuf(gpu_ctx, 16 << (m - 1))
    _check(gpu_ctx, gpu_ctx._L.frieda_fold_line(gpu_ctx._h, d_s.ptr, m, n, alpha.ctypes.data, d_d.ptr))
    assert np.array_equal(d_d.to_array(np.uint32, (4, 1 << (m - 1))), exp)


@pytest.mark.parametrize("log_size", [0, 1, 2, 5, 11, 12, 13, 16, 20, 22])
@pytest.mark.parametrize("ncols", [1, 4])
def test_bit_reverse_column(gpu_ctx, oracle, log_size, ncols):
    """ColumnOps::bit_reverse_column for a BaseField column (ncols 1) and a SecureColumn (4 SoA coordinates), in place."""
    rng = np.random.default_rng(300 + log_size)
    cols = rand_m31(rng, (ncols, 1 << log_size))
    d = DevBuf.from_array(gpu_ctx, cols)
    _check(gpu_ctx, gpu_ctx._L.frieda_bit_reverse_column(gpu_ctx._h, d.ptr, 1 << log_size, ncols, log_size))
    got = d.to_array(np.uint32, (ncols, 1 << log_size))
    for c in range(ncols):
        assert np.array_equal(got[c], oracle.bit_reverse_column(cols[c]))
    # an involution: twice is the identity
    _check(gpu_ctx, gpu_ctx._L.frieda_bit_reverse_column(gpu_ctx._h, d.ptr, 1 << log_size, ncols, log_size))
    assert np.array_equal(d.to_array(np.uint32, (ncols, 1 << log_size)), cols)


def test_bit_reverse_column_strided_and_errors(gpu_ctx, oracle):
    rng = np.random.default_rng(7)
    buf = rand_m31(rng, (3, 5000))  # columns of 2^12 words inside rows of 5000
    d = DevBuf.from_array(gpu_ctx, buf)
    _check(gpu_ctx, gpu_ctx._L.frieda_bit_reverse_column(gpu_ctx._h, d.ptr, 5000, 3, 12))
    got = d.to_array(np.uint32, (3, 5000))
    for c in range(3):
        assert np.array_equal(got[c, :4096], oracle.bit_reverse_column(buf[c, :4096]))
        assert np.array_equal(got[c, 4096:], buf[c, 4096:])
    assert gpu_ctx._L.frieda_bit_reverse_column(gpu_ctx._h, d.ptr, 100, 3, 12) == 1  # stride smaller than the column
    assert gpu_ctx._L.frieda_bit_reverse_column(gpu_ctx._h, None, 100, 1, 3) == 1
    assert gpu_ctx._L.frieda_bit_reverse_column(gpu_ctx._h, d.ptr, 100, 1, 29) == 1


def test_blake2s_ceiling_is_plausible(gpu_ctx):
    """frieda_ctx_blake2s_ceiling: tens of G compressions per second on an MI355X; leaf-shaped messages are cheaper than node-shaped."""
    leaf, node = gpu_ctx.blake2s_ceiling()
    ex = gpu_ctx.blake2s_ceiling_ex()
    assert 1.2 < ex["node_clock_ghz"] < 3.0 and 1900 < ex["node_cycles_per_wave_compression"] < 6000 and ex["leaf_per_s"] > 1e10
    assert 1e10 < node < 1e11 and 1e10 < leaf < 1e11 and leaf > 0.98 * node


def test_blake2s_throughput_form_regression(gpu_ctx):
    """Guards the compression's instruction stream (VERDICT r05 task 1a): the throughput form — runs of one VALU rate class, the wave's
    priority switched at the run boundaries (blake2s.h, round 5), as one asm block per shape (blake2s_asm.h, round 6) — costs
    ~2260 (node) / ~2130 (leaf) SIMD cycles per wave-compression at 8 waves per SIMD (the pinned C++ form 2330 - 2390 / 2220 - 2260).
    The scheduler's own order of rounds 1 - 4 cost 3975 / 3810 and the idle-state form 3300 / 3150: both must fail here.  Cycles, not
    rates: the in-kernel clock moves with the box, the cycle count does not (best of three: a probe that shares the chip with another
    job's tail reads high)."""
    best = None
    for _ in range(3):
        ex = gpu_ctx.blake2s_ceiling_ex()
        cur = (ex["node_cycles_per_wave_compression"], ex["leaf_cycles_per_wave_compression"])
        best = cur if best is None else (min(best[0], cur[0]), min(best[1], cur[1]))
    assert best[0] <= 2600, f"node-shaped compression costs {best[0]:.0f} SIMD cycles per wave (guard 2600): the run / priority structure was lost"
    assert best[1] <= 2450, f"leaf-shaped compression costs {best[1]:.0f} SIMD cycles per wave (guard 2450): the run / priority structure was lost"


def test_dev_at(gpu_ctx):
    """Column::at on a BaseField column and on a SecureColumn."""
    rng = np.random.default_rng(8)
    cols = rand_m31(rng, (4, 1 << 10))
    d = DevBuf.from_array(gpu_ctx, cols)
    one = C.c_uint32()
    four = (C.c_uint32 * 4)()
    for idx in (0, 1, 511, 1023):
        _check(gpu_ctx, gpu_ctx._L.frieda_dev_at(gpu_ctx._h, d.ptr, idx, C.byref(one)))
        assert one.value == int(cols[0, idx])
        _check(gpu_ctx, gpu_ctx._L.frieda_dev_at(gpu_ctx._h, d.ptr, 3 * 1024 + idx, C.byref(one)))
        assert one.value == int(cols[3, idx])
        _check(gpu_ctx, gpu_ctx._L.frieda_dev_at_secure(gpu_ctx._h, d.ptr, 1024, idx, four))
        assert list(four) == [int(cols[c, idx]) for c in range(4)]
    assert gpu_ctx._L.frieda_dev_at_secure(gpu_ctx._h, d.ptr, 1024, 1024, four) == 1  # index beyond the column
    assert gpu_ctx._L.frieda_dev_at(gpu_ctx._h, None, 0, C.byref(one)) == 1


@pytest.mark.parametrize("pow_bits,seed", [(0, 1), (5, 2), (12, 3), (20, 4), (22, 5), (26, 11), (28, 11)])
def test_grind_returns_minimum_nonce(gpu_ctx, oracle, pow_bits, seed):
    """GrindOps::grind (src/proof.rs:58): the MINIMUM qualifying nonce, as the reference's sequential scan finds it.  The last two cases
    lie beyond 2^25 (nonces 49 847 113 and 59 792 498: 8 - 10 s of the oracle's scan each), i.e. tens of thousands of claimed windows."""
    ch = oracle.Channel()
    oracle.lib().fo_channel_init(C.byref(ch))
    oracle.lib().fo_channel_mix_u64(C.byref(ch), seed)
    exp = oracle.lib().fo_grind(C.byref(ch), pow_bits)
    got = C.c_uint64()
    _check(gpu_ctx, gpu_ctx._L.frieda_grind(gpu_ctx._h, bytes(ch.digest), pow_bits, C.byref(got)))
    assert got.value == exp


def test_config2_ntt_plus_fold_round(gpu_ctx, oracle):
    """BASELINE.json configs[1]: 2^20-element NTT + fold_circle_into_line + one fold_line, all three buffers bit-exact."""
    n, L = 20, 16
    data = splitmix64_bytes(1, blob_len_for(n))
    coef, lg = oracle.polynomial_from_bytes(data)
    assert lg == L
    alphas = (splitmix64_bytes(2, 32).view(np.uint32) % P).astype(np.uint32).reshape(2, 4)
    ev = oracle.circle_evaluate(coef, n)
    l1 = oracle.fold_circle_into_line(ev, alphas[0])
    l2 = oracle.fold_line(l1, n, alphas[1])
    d_c, d_e = DevBuf.from_array(gpu_ctx, coef), DevBuf(gpu_ctx, 16 << n)
    d_1, d_2 = DevBuf.from_array(gpu_ctx, np.zeros((4, 1 << (n - 1)), np.uint32)), DevBuf(gpu_ctx, 16 << (n - 2))
    L_ = gpu_ctx._L
    _check(gpu_ctx, L_.frieda_circle_evaluate(gpu_ctx._h, d_c.ptr, 4, L, n, d_e.ptr))
    _check(gpu_ctx, L_.frieda_fold_circle_into_line(gpu_ctx._h, d_1.ptr, d_e.ptr, n, alphas[0].ctypes.data))
    _check(gpu_ctx, L_.frieda_fold_line(gpu_ctx._h, d_1.ptr, n - 1, n, alphas[1].ctypes.data, d_2.ptr))
    assert np.array_equal(d_e.to_array(np.uint32, (4, 1 << n)), ev)
    assert np.array_equal(d_1.to_array(np.uint32, (4, 1 << (n - 1))), l1)
    assert np.array_equal(d_2.to_array(np.uint32, (4, 1 << (n - 2))), l2)


@pytest.mark.parametrize("L,n", [(16, 20), (12, 14), (12, 16), (13, 17), (17, 18), (18, 18), (17, 21), (11, 15), (5, 9), (1, 2), (0, 2)],
                         ids=lambda v: str(v))
@pytest.mark.parametrize("accumulate", [0, 1])
def test_circle_evaluate_fold2_matches_the_three_calls(gpu_ctx, oracle, L, n, accumulate):
    """frieda_circle_evaluate_fold2 (configs[1] in one pass: the folds ride in the transform's last pass when log_size >= 12; the three
    operations otherwise) against the oracle's evaluate / fold_circle_into_line / fold_line, every word of all three buffers; with
    `accumulate` line 1 starts from random contents (FriOps::fold_circle_into_line's dst * alpha^2 + fold)."""
    rng = np.random.default_rng(900 + 32 * L + n + accumulate)
    coef = rng.integers(0, P, (4, 1 << L), dtype=np.uint32)
    alphas = rng.integers(0, P, (2, 4), dtype=np.uint32)
    start = rng.integers(0, P, (4, 1 << (n - 1)), dtype=np.uint32)
    ev = oracle.circle_evaluate(coef, n)
    l1 = oracle.fold_circle_into_line(ev, alphas[0], dst=start.copy() if accumulate else None)
    l2 = oracle.fold_line(l1, n, alphas[1])
    d_c, d_e = DevBuf.from_array(gpu_ctx, coef), DevBuf(gpu_ctx, 16 << n)
    d_1, d_2 = DevBuf.from_array(gpu_ctx, start), DevBuf(gpu_ctx, max(16 << (n - 2), 16))
    _check(gpu_ctx, gpu_ctx._L.frieda_circle_evaluate_fold2(gpu_ctx._h, d_c.ptr, L, n, d_e.ptr, alphas[0].ctypes.data, accumulate, d_1.ptr,
                                                          alphas[1].ctypes.data, d_2.ptr))
    assert np.array_equal(d_e.to_array(np.uint32, (4, 1 << n)), ev)
    assert np.array_equal(d_1.to_array(np.uint32, (4, 1 << (n - 1))), l1)
    assert np.array_equal(d_2.to_array(np.uint32, (4, 1 << (n - 2))), l2)


def test_circle_evaluate_fold2_rejects_bad_arguments(gpu_ctx):
    import frieda_amd

    d = DevBuf(gpu_ctx, 1 << 12)
    good = np.array([1, 2, 3, 4], dtype=np.uint32)
    bad = np.array([1, 2, 3, P], dtype=np.uint32)  # not canonical
    L_ = gpu_ctx._L
    assert L_.frieda_circle_evaluate_fold2(gpu_ctx._h, d.ptr, 3, 1, d.ptr, good.ctypes.data, 0, d.ptr, good.ctypes.data, d.ptr) == frieda_amd._lib.ERR_ARG
    assert L_.frieda_circle_evaluate_fold2(gpu_ctx._h, d.ptr, 5, 4, d.ptr, good.ctypes.data, 0, d.ptr, good.ctypes.data, d.ptr) == frieda_amd._lib.ERR_ARG
    assert L_.frieda_circle_evaluate_fold2(gpu_ctx._h, d.ptr, 2, 4, d.ptr, bad.ctypes.data, 0, d.ptr, good.ctypes.data, d.ptr) == frieda_amd._lib.ERR_ARG
    assert L_.frieda_circle_evaluate_fold2(gpu_ctx._h, None, 2, 4, d.ptr, good.ctypes.data, 0, d.ptr, good.ctypes.data, d.ptr) == frieda_amd._lib.ERR_ARG
    # overlapping buffers (the one-pass form writes the lines while the evaluation is still being written): coefficients 4 x 2^2 words
    # at 0, evaluation 4 x 2^4 words at 64 B, line 1 at 320 B, line 2 at 448 B are disjoint; any shift into a neighbour is refused
    base = d.ptr.value
    ok = (base, base + 64, base + 320, base + 448)
    assert L_.frieda_circle_evaluate_fold2(gpu_ctx._h, ok[0], 2, 4, ok[1], good.ctypes.data, 0, ok[2], good.ctypes.data, ok[3]) == frieda_amd._lib.OK
    for bad_set in ((base, base + 48, base + 320, base + 448), (base, base + 64, base + 316, base + 448), (base, base + 64, base + 320, base + 444),
                    (base, base + 64, base + 320, base + 320)):
        assert L_.frieda_circle_evaluate_fold2(gpu_ctx._h, bad_set[0], 2, 4, bad_set[1], good.ctypes.data, 0, bad_set[2], good.ctypes.data,
                                               bad_set[3]) == frieda_amd._lib.ERR_ARG
    gpu_ctx.synchronize()


# ------------------------------------------------------------------------------------------------
# Level A
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vec", load_vectors()["commit"], ids=lambda v: v["input"][:24])
def test_commit_known_answers(gpu_ctx, blob, vec):
    """src/commit.rs:28-38 (golden root) and the secondary vectors, on the GPU."""
    data = resolve_input(vec["input"], blob)
    assert gpu_ctx.commit(data, vec["log_blowup_factor"]).hex() == vec["root"]


# 61440 bytes = 4 * 2^12 felts exactly: L = 12, the smallest polynomial whose last transform pass runs fused with leaf hashing (and
# the one shape where that pass reads the coefficients themselves, replicated, instead of a strided pass's output); 61441: L = 13
@pytest.mark.parametrize("n_bytes", [0, 1, 15, 16, 17, 58, 119, 120, 121, 300, 1023, 5000, 61440, 61441, 70001])
@pytest.mark.parametrize("B", [1, 2, 4])
def test_commit_matches_oracle_ragged(gpu_ctx, oracle, n_bytes, B):
    data = splitmix64_bytes(21 + B, n_bytes).tobytes()
    assert gpu_ctx.commit(data, B) == oracle.commit(data, B)


@pytest.mark.parametrize("n_bytes,B", [(61440, 1), (61440, 4), (61441, 2), (983040, 3)])
def test_fused_encode_tree_matches_oracle(gpu_ctx, oracle, n_bytes, B):
    """The last transform pass fused with leaf hashing (ntt_last_tree7) against the oracle: commit root, whole proof, and every
    stored tree level and the evaluation through the openings of 300 queries.  (The unfused build variants behind the getenv
    options are per context; tests/test_gpu_shapes.py::test_knob_variants_on_their_own_context runs them.)"""
    import frieda_amd

    data = splitmix64_bytes(77 + B, n_bytes).tobytes()
    assert gpu_ctx.commit(data, B) == oracle.commit(data, B)
    cfg = _cfg(frieda_amd, 6, B, 0, 300)
    root, proof = gpu_ctx.commit_and_generate_proof(data, 11, cfg)
    o_root, o_proof = oracle.commit_and_generate_proof(data, 11, oracle.make_config(6, B, 0, 300))
    assert root == o_root and proof.serialize() == o_proof.serialize()
    assert frieda_amd.verify(proof, 11)


def test_commit_without_twiddle_cache(gpu_ctx, oracle):
    data = pattern_bytes(4096).tobytes()
    gpu_ctx.set_twiddle_cache(False)
    try:
        assert gpu_ctx.commit(data, 4) == oracle.commit(data, 4)
        assert gpu_ctx.commit(data, 4) == oracle.commit(data, 4)
    finally:
        gpu_ctx.set_twiddle_cache(True)


def test_commit_device_resident(gpu_ctx, oracle):
    import torch

    data = splitmix64_bytes(5, blob_len_for(16))
    t = torch.from_numpy(data).cuda()
    root = torch.zeros(32, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    gpu_ctx.commit_device(t.data_ptr(), t.numel(), 4, root.data_ptr())
    gpu_ctx.synchronize()
    assert bytes(root.cpu().numpy()) == oracle.commit(data, 4)


def _cfg(frieda_amd, pow_bits, B, last, nq):
    return frieda_amd.PcsConfig(frieda_amd.FriConfig(B, last, nq), pow_bits)


PROVE_CASES = [
    ("pattern:1024", None, (20, 4, 0, 20)),
    ("pattern:1024", 1024, (20, 4, 0, 20)),
    ("pattern:4096", 4096, (20, 4, 1, 20)),
    ("pattern:65536", 65536, (20, 4, 0, 20)),
    ("ascii:This is the original data that needs to be made available.", None, (20, 4, 0, 20)),
    ("pattern:300", 9, (8, 2, 1, 12)),
    ("pattern:2000", 3, (6, 1, 2, 7)),
    ("pattern:700", None, (10, 3, 0, 33)),
    ("blob", None, (20, 4, 1, 20)),
    ("blob", 262146, (20, 4, 0, 20)),
    ("pattern:40000", 7, (10, 4, 8, 16)),  # last layer 2^12 points: beyond the device tail, host-channel policy
    ("pattern:9000", None, (9, 6, 3, 10)),
    ("pattern:120", 1, (4, 1, 0, 5)),  # tiny: L = 3, n = 4
    ("pattern:20", None, (4, 2, 0, 3)),  # L = 1, n = 3: no inner layer at all
    ("pattern:3000", 42, (24, 4, 0, 20)),  # 24-bit proof of work: the grind needs several scan chunks
    ("pattern:5000", 8, (10, 4, 1, 300)),  # many queries: dense decommitment with shared paths
    ("pattern:777", None, (6, 5, 2, 64)),
]


@pytest.mark.parametrize("host_channel", [False, True], ids=["devchannel", "hostchannel"])
@pytest.mark.parametrize("spec,seed,cfg", PROVE_CASES, ids=lambda v: str(v)[:28])
def test_prove_bit_exact_vs_oracle(gpu_ctx, oracle, blob, spec, seed, cfg, host_channel):
    """Whole proof (every root, alpha-dependent layer, nonce, witness, opening) byte-identical to the oracle's, with the
    transcript evaluated inside the device kernels and with the host-side channel policy."""
    import frieda_amd

    data = resolve_input(spec, blob)
    o_root, o_proof = oracle.commit_and_generate_proof(data, seed, oracle.make_config(*cfg))
    gpu_ctx.set_host_channel(host_channel)
    try:
        g_root, g_proof = gpu_ctx.commit_and_generate_proof(data, seed, _cfg(frieda_amd, *cfg))
    finally:
        gpu_ctx.set_host_channel(False)
    assert g_root == o_root
    assert g_proof.proof_of_work == o_proof.c.proof_of_work
    for li in range(g_proof.n_inner_layers + 1):
        ol = o_proof.c.first_layer if li == 0 else o_proof.c.inner_layers[li - 1]
        assert g_proof.layer(li)["commitment"] == bytes(ol.commitment), f"layer {li} root"
    assert g_proof.serialize() == o_proof.serialize()
    if g_proof.n_inner_layers > 0:
        assert frieda_amd.verify(g_proof, seed)
        assert oracle.verify(o_proof, seed)
    else:  # stwo's verifier asserts on proofs without inner layers (oracle and product both report the panic)
        with pytest.raises(frieda_amd.FriedaPanic):
            frieda_amd.verify(g_proof, seed)


@pytest.mark.parametrize("host_channel", [False, True], ids=["devchannel", "hostchannel"])
def test_draw_felt_retry_branch(gpu_ctx, oracle, host_channel):
    """Channel::draw_felt redraws when a word is >= 2P — once in ~3e8 draws.  With the acceptance bound lowered through the
    test hooks (same value on both sides) most draws are redrawn several times; the transcripts must still agree."""
    import frieda_amd

    data = pattern_bytes(6000).tobytes()
    cfg = (8, 4, 0, 16)
    bound = 0xE0000000  # each word passes with p = 7/8, all eight with p = 0.34
    oracle.lib().fo_test_set_draw_bound(bound)
    _check(gpu_ctx, gpu_ctx._L.frieda_ctx_test_set_draw_bound(gpu_ctx._h, bound))
    gpu_ctx.set_host_channel(host_channel)
    try:
        o_root, o_proof = oracle.commit_and_generate_proof(data, 3, oracle.make_config(*cfg))
        g_root, g_proof = gpu_ctx.commit_and_generate_proof(data, 3, _cfg(frieda_amd, *cfg))
    finally:
        oracle.lib().fo_test_set_draw_bound(0)
        gpu_ctx._L.frieda_ctx_test_set_draw_bound(gpu_ctx._h, 0)
        gpu_ctx.set_host_channel(False)
    assert g_proof.serialize() == o_proof.serialize()
    # and the branch really fired: the default-bound transcript differs
    d_root, d_proof = gpu_ctx.commit_and_generate_proof(data, 3, _cfg(frieda_amd, *cfg))
    assert d_root == g_root and d_proof.serialize() != g_proof.serialize()


@pytest.mark.parametrize("nq", [1, 2, 63, 128, 129, 1024])
def test_query_sort_and_compaction_seams(gpu_ctx, oracle, nq):
    """The seams of the sort / de-duplication the prover's openings and verify_many share (queries_dev.h): 1 and 2 queries (the
    smallest padded list), 63 (just under one wave), 128 (exactly two compaction chunks), 129 (a chunk plus one) and 1024 (the
    kernels' limit).  Two domains under blow-up 2^3, last-layer bound 1: 200 bytes -> 2^7 (at 1024 queries every position is drawn
    many times, at most 128 distinct) and 1500 bytes -> 2^10 (at 1024 queries ~650 distinct positions, several chunks, and the
    opening tables still fit the kernel).  Each proof byte for byte against the oracle's, then through verify_many and the host
    verifier, both accepting; at 1024 queries the openings must have come from the device kernel, not the host planner (whose
    fallback shows as a `gather` launch); at 129 also one batch of three blobs."""
    import frieda_amd

    cfg, ocfg = _cfg(frieda_amd, 4, 3, 1, nq), oracle.make_config(4, 3, 1, nq)
    datas = [splitmix64_bytes(600 + i, nbytes).tobytes() for i, nbytes in enumerate((200, 1500))]
    seeds = [17, 18]
    proofs = []
    for data, seed, log_domain in zip(datas, seeds, (7, 10)):
        o_root, o_proof = oracle.commit_and_generate_proof(data, seed, ocfg)
        gpu_ctx.set_kernel_timing(nq == 1024)
        try:
            g_root, g_proof = gpu_ctx.commit_and_generate_proof(data, seed, cfg)
            names = [k["name"] for k in gpu_ctx.kernel_timing_report()] if nq == 1024 else None
        finally:
            gpu_ctx.set_kernel_timing(False)
        assert g_proof.log_size_bound + 3 == log_domain
        assert g_root == o_root and g_proof.serialize() == o_proof.serialize()
        if names is not None:
            assert "decommit" in names and "gather" not in names, names
        assert frieda_amd.verify(g_proof, seed)
        proofs.append(g_proof)
    assert list(gpu_ctx.verify_many(proofs, seeds)) == [1, 1]  # VERIFY_ACCEPTED
    if nq == 129:
        blobs = [splitmix64_bytes(610 + i, 200).tobytes() for i in range(3)]
        got = gpu_ctx.commit_and_generate_proof_batch(blobs, [5, 6, 7], cfg)
        for i, (root, proof) in enumerate(got):
            o_root, o_proof = oracle.commit_and_generate_proof(blobs[i], 5 + i, ocfg)
            assert root == o_root and proof.serialize() == o_proof.serialize(), i
            assert frieda_amd.verify(proof, 5 + i)
        assert list(gpu_ctx.verify_many([p for _, p in got], [5, 6, 7])) == [1, 1, 1]


def test_reference_proof_tests_on_gpu(gpu_ctx, blob):
    """src/proof.rs:119-193 through the GPU prover and the C-ABI verifier."""
    import frieda_amd

    cfg = _cfg(frieda_amd, 20, 4, 1, 20)
    commitment, proof = gpu_ctx.commit_and_generate_proof(blob, None, cfg)
    assert proof.n_inner_layers != 0
    assert commitment == gpu_ctx.commit(blob, 4) and proof.commitment == commitment
    assert frieda_amd.verify(proof, None)
    p = proof.clone()
    p.proof_of_work += 1
    assert not frieda_amd.verify(p, None)
    p = proof.clone()
    e = p.evaluations
    e[0] = (e[0].astype(np.uint64) + 1) % P
    p.evaluations = e
    assert not frieda_amd.verify(p, None)
    p = proof.clone()
    p.evaluations = p.evaluations[::-1]
    assert not frieda_amd.verify(p, None)
    p = proof.clone()
    p.evaluations = p.evaluations[:-1]
    with pytest.raises(frieda_amd.FriedaPanic):
        frieda_amd.verify(p, None)
    p = proof.clone()
    e = p.evaluations
    e[[0, 1]] = e[[1, 0]]
    p.evaluations = e
    assert not frieda_amd.verify(p, None)
    p1 = gpu_ctx.generate_proof(blob, 1, cfg)
    p2 = gpu_ctx.generate_proof(blob, 2, cfg)
    assert p1.evaluations.tolist() != p2.evaluations.tolist()
    assert frieda_amd.verify(p1, 1) and frieda_amd.verify(p2, 2)
    assert not frieda_amd.verify(p1, 2) and not frieda_amd.verify(p2, 1)


@pytest.mark.parametrize("host_channel", [False, True], ids=["devchannel", "hostchannel"])
def test_device_transcript_reproduces_the_selfcheck_trace(gpu_ctx, blob, host_channel):
    """tests/golden/trace_selfcheck.json (SELF-GENERATED from the oracle by tools/dump_trace.py, not reference-held): the HIP
    path's transcript — roots, alphas, digest before the grind, nonce, query count, witness lengths, last-layer polynomial —
    value by value, under both transcript policies."""
    import json

    import frieda_amd
    from conftest import GOLDEN

    doc = json.load(open(os.path.join(GOLDEN, "trace_selfcheck.json")))
    gpu_ctx.set_host_channel(host_channel)
    try:
        for c in doc["cases"]:
            data = resolve_input(c["input"] if c["input"] == "blob" else c["input"], blob)
            k = c["config"]
            cfg = _cfg(frieda_amd, k["pow_bits"], k["log_blowup_factor"], k["log_last_layer_degree_bound"], k["n_queries"])
            root, proof = gpu_ctx.commit_and_generate_proof(data, c["seed"], cfg)
            tr = gpu_ctx.last_transcript()
            assert root.hex() == c["commitment"]
            n_layers = 1 + proof.n_inner_layers
            assert [proof.layer(i)["commitment"].hex() for i in range(n_layers)] == c["roots"]
            assert tr["alphas"] == c["alphas"]
            assert tr["digest_before_grind"].hex() == c["digest_before_grind"]
            assert proof.proof_of_work == c["nonce"]
            assert proof.evaluations.shape[0] == c["n_evaluations"] == len(c["queries"])
            assert [int(x) for x in proof.last_layer_poly.ravel()] == c["last_layer_poly"]
            got = [{"fri_witness": len(proof.layer(i)["fri_witness"]), "hash_witness": len(proof.layer(i)["hash_witness"]),
                    "column_witness": len(proof.layer(i)["column_witness"])} for i in range(n_layers)]
            assert got == c["witness_lengths"]
    finally:
        gpu_ctx.set_host_channel(False)


def test_pipelined_proofs_match_sequential(gpu_ctx, oracle):
    """Several proofs in flight on separate contexts (frieda_prove_begin / _finish) give byte-identical proofs."""
    import torch

    import frieda_amd

    cfg = _cfg(frieda_amd, 12, 4, 0, 20)
    blobs = [splitmix64_bytes(300 + i, blob_len_for(14 + (i % 3))) for i in range(7)]
    dev = [torch.from_numpy(b).cuda() for b in blobs]
    torch.cuda.synchronize()
    expect = [gpu_ctx.commit_and_generate_proof(b, 11 + i, cfg) for i, b in enumerate(blobs)]
    pipe = frieda_amd.ProofPipeline(0, depth=3)
    got = []
    for i, d in enumerate(dev):
        r = pipe.submit_device(d.data_ptr(), d.numel(), 11 + i, cfg)
        if r is not None:
            got.append(r)
    got += pipe.drain()
    pipe.close()
    assert len(got) == len(blobs)
    for (er, ep), (gr, gp) in zip(expect, got):
        assert er == gr and ep.serialize() == gp.serialize()
    o_root, o_proof = oracle.commit_and_generate_proof(blobs[0], 11, oracle.make_config(12, 4, 0, 20))
    assert got[0][0] == o_root and got[0][1].serialize() == o_proof.serialize()
    # protocol errors: finish without begin, begin twice
    with pytest.raises(frieda_amd.FriedaError):
        gpu_ctx.prove_finish()
    gpu_ctx.prove_begin_device(dev[0].data_ptr(), dev[0].numel(), 1, cfg)
    with pytest.raises(frieda_amd.FriedaError):
        gpu_ctx.prove_begin_device(dev[0].data_ptr(), dev[0].numel(), 1, cfg)
    gpu_ctx.prove_finish()


def test_cpp_api_harness(gpu_ctx):
    """The reference's unit tests transcribed to C++ over include/frieda.hpp (tests/cpp/test_api.cpp)."""
    import os
    import subprocess

    from conftest import GOLDEN, ROOT

    exe = os.path.join(ROOT, "tests", "cpp", "test_api.bin")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    r = subprocess.run([exe, os.path.join(GOLDEN, "blob")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr


def test_cpp_bench_harness(gpu_ctx):
    """The reference's criterion benches restated in C++ over include/frieda.hpp (tests/cpp/bench_api.cpp: groups commit, generate_proof,
    commit_and_generate_proof, verify_proof on the five bench inputs): runs, every proof verifies, 20 result lines."""
    import subprocess

    from conftest import GOLDEN, ROOT

    exe = os.path.join(ROOT, "tests", "cpp", "bench_api.bin")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    r = subprocess.run([exe, os.path.join(GOLDEN, "blob"), "0.02"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok: every proof verified" in r.stdout, r.stdout + r.stderr
    assert sum("time:" in ln for ln in r.stdout.splitlines()) == 20


@pytest.mark.parametrize("n_slots,mode", [(1, "plain"), (1, "rccl"), (2, "stub"), (3, "stub"), (8, "stub")])
def test_cpp_multi_gpu_entry_points(gpu_ctx, n_slots, mode):
    """frieda_multi_create / frieda_commit_many / frieda_prove_many from C++ (tests/cpp/test_api.cpp multi_mode): the no-exchange
    path, the real one-rank RCCL collective (FRIEDA_MULTI_FORCE_RCCL=1), and the N > 1 gather layout against the RCCL test
    double (this box has one GPU and real RCCL refuses a device listed twice).  8 slots = the target node's shape: 16 contexts,
    8 worker threads, an 8-way rank-major gather, every slot with a multi-call run of equal-length blobs; each mode also re-runs
    with the batch policy's options changed (results must not move) and checks the NUMA placement list."""
    import subprocess

    from conftest import GOLDEN, ROOT

    exe = os.path.join(ROOT, "tests", "cpp", "test_api.bin")
    env = dict(os.environ)
    env.pop("FRIEDA_RCCL_PATH", None)
    env.pop("FRIEDA_MULTI_FORCE_RCCL", None)
    env.setdefault("NCCL_SOCKET_IFNAME", "lo")  # RCCL's bootstrap over the loopback: the container's own interface may not resolve
    if mode == "rccl":
        env["FRIEDA_MULTI_FORCE_RCCL"] = "1"
    if mode == "stub":
        env["FRIEDA_RCCL_PATH"] = os.path.join(ROOT, "tests", "cpp", "librccl_stub.so")
    r = subprocess.run([exe, os.path.join(GOLDEN, "blob"), "multi", str(n_slots)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"rccl={0 if mode == 'plain' else 1}" in r.stdout


def _visible_gpus():
    import torch

    return torch.cuda.device_count()  # counts without initialising the GPU on this image


@pytest.mark.skipif(_visible_gpus() < 2, reason="needs a node with >= 2 visible GPUs (runs unprompted wherever there are)")
def test_cpp_multi_gpu_real_rccl():
    """frieda_commit_many / frieda_prove_many over every visible GPU with the real RCCL root gather (n > 1), from C++: ragged
    small blobs (the generic transform kernel's per-device LDS opt-in), the reference's fixture, runs of equal lengths."""
    import subprocess

    from conftest import GOLDEN, ROOT

    n = min(_visible_gpus(), 8)
    exe = os.path.join(ROOT, "tests", "cpp", "test_api.bin")
    env = dict(os.environ)
    env.setdefault("NCCL_SOCKET_IFNAME", "lo")  # one node: bootstrap over the loopback
    r = subprocess.run([exe, os.path.join(GOLDEN, "blob"), "multi_real", str(n)], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0 and "rccl=1" in r.stdout, r.stdout + r.stderr


@pytest.mark.skipif(_visible_gpus() < 2, reason="needs a node with >= 2 visible GPUs (runs unprompted wherever there are)")
def test_config4_eight_2p22_blobs_across_all_gpus_real_rccl(oracle, monkeypatch):
    """BASELINE.json configs[3] as written: 8 independent 2^22-domain blobs (generator seeds 100..107, benches/proof.rs:30-44 per
    blob), one per GPU round-robin over every visible device, roots gathered by the real RCCL all-gather: all 8 roots and all 8
    proofs byte-identical to the oracle's."""
    from concurrent.futures import ThreadPoolExecutor

    import frieda_amd

    n = min(_visible_gpus(), 8)
    blobs = [splitmix64_bytes(100 + i, blob_len_for(22)).tobytes() for i in range(8)]
    seeds = [len(b) for b in blobs]
    cfg = _cfg(frieda_amd, 20, 4, 0, 20)
    ocfg = oracle.make_config(20, 4, 0, 20)
    with ThreadPoolExecutor(max_workers=8) as ex:
        expected = list(ex.map(lambda a: oracle.commit_and_generate_proof(a[0], a[1], ocfg), zip(blobs, seeds)))
    if "NCCL_SOCKET_IFNAME" not in os.environ:
        monkeypatch.setenv("NCCL_SOCKET_IFNAME", "lo")  # one node: bootstrap over the loopback
    mc = frieda_amd.MultiContext(list(range(n)))
    assert mc.device_count == n and mc.uses_rccl
    assert mc.commit_many(blobs, 4) == [r for r, _ in expected]
    got = mc.prove_many(blobs, seeds, cfg)
    assert [r for r, _ in got] == [r for r, _ in expected]
    assert [p.serialize() for _, p in got] == [p.serialize() for _, p in expected]
    assert mc.gather_count == 2
    mc.close()


def test_many_entry_points_retry_with_smaller_calls_when_memory_runs_out(gpu_ctx, oracle):
    """frieda_prove_many / frieda_commit_many on a device that cannot hold the batch policy's calls.  A test
    limit on the workspace plays the smaller device: the first cut (6 blobs per call) and the second (3) are refused with
    FRIEDA_ERR_NOMEM, the third (1 per call) fits — the results are those of the unconstrained run; a limit below ONE blob's
    workspace fails loudly; release_workspace hands the memory back and the handle keeps working."""
    import frieda_amd

    L = gpu_ctx._L
    blobs = [splitmix64_bytes(900 + i, 61440).tobytes() for i in range(12)]  # 2^16-domain proofs, one length: one run
    seeds = list(range(12))
    cfg = _cfg(frieda_amd, 8, 4, 0, 10)
    ocfg = oracle.make_config(8, 4, 0, 10)
    expected = [oracle.commit_and_generate_proof(b, s, ocfg) for b, s in zip(blobs, seeds)]
    ws_prove = L.frieda_workspace_bytes(61440, 4, 0, 1)
    ws_commit = L.frieda_workspace_bytes(61440, 4, 0, 0)
    assert ws_prove > ws_commit > 0
    mc = frieda_amd.MultiContext([0])
    first = C.c_void_p(L.frieda_multi_ctx(mc._h, 0))
    assert L.frieda_ctx_test_set_arena_limit(first, int(2.5 * ws_prove)) == 0
    got = mc.prove_many(blobs, seeds, cfg)
    assert [r for r, _ in got] == [r for r, _ in expected]
    assert [p.serialize() for _, p in got] == [p.serialize() for _, p in expected]
    assert L.frieda_ctx_test_set_arena_limit(first, int(2.5 * ws_commit)) == 0
    assert mc.commit_many(blobs, 4) == [r for r, _ in expected]
    # below one blob's workspace nothing can be cut smaller: the error comes back, with the device named
    assert L.frieda_ctx_test_set_arena_limit(first, ws_commit // 2) == 0
    with pytest.raises(frieda_amd.FriedaError) as ei:
        mc.commit_many(blobs, 4)
    assert ei.value.status == 4 and "device 0" in str(ei.value)  # FRIEDA_ERR_NOMEM
    with pytest.raises(frieda_amd.FriedaError):
        mc.prove_many(blobs, seeds, cfg)
    # the handle stays usable; releasing the workspaces is not destroying it
    assert L.frieda_ctx_test_set_arena_limit(first, 0) == 0
    mc.release_workspace()
    assert mc.commit_many(blobs[:3], 4) == [r for r, _ in expected[:3]]
    mc.close()


def test_batch_budget_is_a_share_of_the_device(gpu_ctx):
    """the batch policy's budget is clamped to the device the context sits on — the default to 16 % of its memory, an
    explicit FRIEDA_BATCH_BUDGET_MB to 45 % — so two calls in flight always fit; creating a context leaves last_error empty."""
    import torch

    L = gpu_ctx._L
    total = torch.cuda.get_device_properties(0).total_memory
    length = 15 << 20  # a 2^24-domain proof: ~2.7 GB of workspace
    ws = L.frieda_workspace_bytes(length, 4, 0, 1)

    def largest_call(ctx_handle, count):
        calls = (C.c_uint32 * 4096)()
        n = C.c_uint32()
        assert L.frieda_batch_plan(ctx_handle, length, 4, 0, 1, count, 2, calls, 4096, C.byref(n)) == 0
        assert sum(calls[: n.value]) == count
        return max(calls[: n.value])

    ctx = type(gpu_ctx)(0)
    try:
        assert L.frieda_last_error(ctx._h) == b"" and isinstance(L.frieda_ctx_notes(ctx._h), bytes)
        assert largest_call(ctx._h, 4000) * ws <= 0.16 * total + ws
        ctx.set_option("FRIEDA_BATCH_BUDGET_MB", 262144)  # 256 GiB asked for
        assert largest_call(ctx._h, 4000) * ws <= 0.45 * total
        assert largest_call(None, 4000) == 16  # without a context: the documented default, sixteen 2^24-domain proofs per call
    finally:
        ctx.close()


def test_multi_context_python_and_rccl_failure_is_loud(gpu_ctx, oracle, monkeypatch):
    import frieda_amd

    blobs = [splitmix64_bytes(500 + i, 900 + 333 * i).tobytes() for i in range(5)]
    cfg = _cfg(frieda_amd, 8, 4, 0, 10)
    mc = frieda_amd.MultiContext([0])
    assert mc.device_count == 1 and not mc.uses_rccl
    assert mc.commit_many(blobs, 4) == [oracle.commit(b, 4) for b in blobs]
    got = mc.prove_many(blobs, list(range(5)), cfg)
    for i, (root, proof) in enumerate(got):
        o_root, o_proof = oracle.commit_and_generate_proof(blobs[i], i, oracle.make_config(8, 4, 0, 10))
        assert root == o_root and proof.serialize() == o_proof.serialize()
    assert mc.prove_many([], None, cfg) == [] and mc.commit_many([], 4) == []
    mc.close()
    # an RCCL that cannot be loaded fails the creation of a multi-device handle instead of falling back to anything
    monkeypatch.setenv("FRIEDA_RCCL_PATH", "/nonexistent/librccl.so")
    with pytest.raises(frieda_amd.FriedaError):
        frieda_amd.MultiContext([0, 0])
    with pytest.raises(frieda_amd.FriedaError):
        frieda_amd.MultiContext([])
    with pytest.raises(frieda_amd.FriedaError):
        frieda_amd.MultiContext([99])


def test_many_entry_points_without_the_upload_ring(gpu_ctx, oracle, monkeypatch):
    """FRIEDA_MULTI_NO_PREFETCH=1: the units read the host blobs at begin (batches through the pointer table, the lone blob through
    prove_begin / a batch of one) instead of the upload ring.  A run of four, a lone blob and a run of two on one device: roots and
    proofs byte-identical to the oracle's and to those of a handle that uploads ahead; one device gathers nothing."""
    import frieda_amd

    lengths = [3000, 3000, 3000, 3000, 1024, 3000, 3000]
    blobs = [splitmix64_bytes(700 + i, n).tobytes() for i, n in enumerate(lengths)]
    seeds = list(range(7))
    cfg = _cfg(frieda_amd, 8, 4, 0, 10)
    ocfg = oracle.make_config(8, 4, 0, 10)
    expected = [oracle.commit_and_generate_proof(b, s, ocfg) for b, s in zip(blobs, seeds)]
    exp_roots = [r for r, _ in expected]
    exp_proofs = [p.serialize() for _, p in expected]
    assert exp_roots == [oracle.commit(b, 4) for b in blobs]

    def run():
        mc = frieda_amd.MultiContext([0])  # (the variable is read when the handle is created)
        try:
            roots = mc.commit_many(blobs, 4)
            got = mc.prove_many(blobs, seeds, cfg)
            assert mc.gather_count == 0
            return roots, [r for r, _ in got], [p.serialize() for _, p in got]
        finally:
            mc.close()

    monkeypatch.setenv("FRIEDA_MULTI_NO_PREFETCH", "1")
    direct = run()
    assert direct[0] == exp_roots
    assert direct[1] == exp_roots and direct[2] == exp_proofs
    monkeypatch.delenv("FRIEDA_MULTI_NO_PREFETCH")
    assert run() == direct


def test_panics_map_to_status(gpu_ctx):
    import frieda_amd

    with pytest.raises(frieda_amd.FriedaPanic):
        gpu_ctx.generate_proof(b"tiny", None, _cfg(frieda_amd, 8, 4, 0, 4))


@pytest.mark.parametrize("B", [-1, 0xFFFFFFFF, 0xFFFFFFFE, 29, 1 << 31])
def test_huge_or_negative_blowup_is_refused(gpu_ctx, B):
    """log_blowup_factor arrives unchecked (ctypes turns -1 into 0xFFFFFFFF): L + B must not wrap into a small domain."""
    import frieda_amd

    data = splitmix64_bytes(3, 16)  # L = 2: B = 0xFFFFFFFF would wrap L + B to 1
    Bc = B & 0xFFFFFFFF
    with pytest.raises(frieda_amd.FriedaError):
        gpu_ctx.commit(data.tobytes(), Bc)
    buf = (C.c_uint8 * 64)(*data.tolist(), *([0] * 48))
    roots = (C.c_uint8 * 64)()
    assert gpu_ctx._L.frieda_commit_batch(gpu_ctx._h, buf, 16, 16, 2, Bc, roots) == 1  # FRIEDA_ERR_ARG
    cfg = _cfg(frieda_amd, 4, Bc, 0, 5)
    with pytest.raises(frieda_amd.FriedaError):
        gpu_ctx.commit_and_generate_proof(data.tobytes(), None, cfg)
    with pytest.raises(frieda_amd.FriedaError):
        gpu_ctx.prove_begin(data.tobytes(), None, cfg)
    with pytest.raises(frieda_amd.FriedaError):
        gpu_ctx.commit_and_generate_proof_batch([data.tobytes()] * 2, None, cfg)
    # log_last_layer_degree_bound is bounded before it is added to B, too
    with pytest.raises(frieda_amd.FriedaError):
        gpu_ctx.commit_and_generate_proof(data.tobytes(), None, _cfg(frieda_amd, 4, 4, 0xFFFFFFFC, 5))
    # the context is still usable
    assert len(gpu_ctx.commit(data.tobytes(), 4)) == 32


def test_proof_in_flight_blocks_every_workspace_user(gpu_ctx, oracle):
    """Between prove_begin and prove_finish the job's offsets point into the arena and its transcript summary sits in the pinned
    block: every other entry point that (re)allocates or writes either must refuse, and the proof must come out unharmed."""
    import torch

    import frieda_amd

    cfg = _cfg(frieda_amd, 10, 4, 0, 12)
    blob = splitmix64_bytes(77, 20000).tobytes()
    big = splitmix64_bytes(78, 400000)  # a larger call would have re-allocated the arena
    d_big = torch.from_numpy(big).cuda()
    d_root = torch.zeros(32, dtype=torch.uint8, device="cuda")
    cols = DevBuf.from_array(gpu_ctx, rand_m31(np.random.default_rng(1), (4, 64)))
    out = DevBuf(gpu_ctx, 32 * 64)
    gpu_ctx.prove_begin(blob, 5, cfg)
    L, h = gpu_ctx._L, gpu_ctx._h
    with pytest.raises(frieda_amd.FriedaError, match="in flight"):
        gpu_ctx.commit(big.tobytes(), 4)
    with pytest.raises(frieda_amd.FriedaError, match="in flight"):
        gpu_ctx.commit_device(d_big.data_ptr(), big.size, 4, d_root.data_ptr())
    with pytest.raises(frieda_amd.FriedaError, match="in flight"):
        gpu_ctx.commit_batch([big.tobytes()] * 2, 4)
    with pytest.raises(frieda_amd.FriedaError, match="in flight"):
        gpu_ctx.prove_begin(blob, 5, cfg)
    assert L.frieda_merkle_root(h, cols.ptr, 6, out.ptr) == 1
    digest = (C.c_uint8 * 32)()
    nonce = C.c_uint64()
    assert L.frieda_grind(h, digest, 4, C.byref(nonce)) == 1
    assert L.frieda_reconstruct_device(h, cols.ptr, 6, 10, 0, 100, out.ptr) == 1
    idx = (C.c_uint32 * 1)(0)
    assert L.frieda_circle_interpolate_cells(h, cols.ptr, idx, 1, 4, 6, 6, 10, out.ptr) == 1
    assert L.frieda_ctx_release_workspace(h) == 1
    root, proof = gpu_ctx.prove_finish()
    o_root, o_proof = oracle.commit_and_generate_proof(blob, 5, oracle.make_config(10, 4, 0, 12))
    assert root == o_root and proof.serialize() == o_proof.serialize()
    # and everything works again afterwards
    assert gpu_ctx.commit(big.tobytes(), 4) == oracle.commit(big.tobytes(), 4)


# ------------------------------------------------------------------------------------------------
# full sizes: properties that do not need the oracle at size
# ------------------------------------------------------------------------------------------------
def test_config3_commit_2p22_matches_oracle(gpu_ctx, oracle):
    """BASELINE.json configs[2]: 2^22-domain commit(); the oracle needs ~10 s here, still affordable once."""
    data = splitmix64_bytes(1, blob_len_for(22)).tobytes()
    assert gpu_ctx.commit(data, 4) == oracle.commit(data, 4)


def test_config3_prove_2p22_matches_oracle(gpu_ctx, oracle):
    """BASELINE.json configs[2]/[3]: the whole 2^22-domain proof (17 inner layers, every root, nonce, openings) byte-identical to
    the oracle's, on the blob bench.py gives rank 0 (generator seed 100, seed = Some(len), benches/proof.rs:5-23 config)."""
    import frieda_amd

    data = splitmix64_bytes(100, blob_len_for(22))
    o_root, o_proof = oracle.commit_and_generate_proof(data, data.size, oracle.make_config(20, 4, 0, 20))
    g_root, g_proof = gpu_ctx.commit_and_generate_proof(data, data.size, _cfg(frieda_amd, 20, 4, 0, 20))
    assert g_root == o_root and g_proof.n_inner_layers == 17
    assert g_proof.serialize() == o_proof.serialize()


def test_config4_eight_2p22_blobs_match_the_oracle(gpu_ctx, oracle):
    """BASELINE.json configs[3] at N = 1: the batch of 8 independent 2^22-domain blobs (generator seeds 100..107, SURVEY.md §8d
    config 4) through the sharding helpers (batch.commit_batch / prove_batch — world size 1 here, the same code the ranks run)
    and through the C ABI's multi-GPU entry (frieda_commit_many / frieda_prove_many, one device slot): all 8 roots and all 8
    proofs byte-identical to the oracle's (computed on 8 host threads)."""
    from concurrent.futures import ThreadPoolExecutor

    import frieda_amd
    from frieda_amd import batch

    blobs = [splitmix64_bytes(100 + i, blob_len_for(22)).tobytes() for i in range(8)]
    seeds = [len(b) for b in blobs]  # benches/proof.rs:23
    cfg = _cfg(frieda_amd, 20, 4, 0, 20)
    ocfg = oracle.make_config(20, 4, 0, 20)
    with ThreadPoolExecutor(max_workers=8) as ex:
        expected = list(ex.map(lambda a: oracle.commit_and_generate_proof(a[0], a[1], ocfg), zip(blobs, seeds)))
    exp_roots = [r for r, _ in expected]
    exp_proofs = [p.serialize() for _, p in expected]
    assert len(set(exp_roots)) == 8
    # sharding helpers
    assert batch.commit_batch(blobs, 4) == exp_roots
    roots, proofs = batch.prove_batch(blobs, seeds, cfg)
    assert roots == exp_roots
    assert [proofs[i].serialize() for i in range(8)] == exp_proofs
    del proofs
    # C ABI multi entry
    mc = frieda_amd.MultiContext([0])
    assert mc.commit_many(blobs, 4) == exp_roots
    got = mc.prove_many(blobs, seeds, cfg)
    assert [r for r, _ in got] == exp_roots
    assert [p.serialize() for _, p in got] == exp_proofs
    assert all(frieda_amd.verify(p, s) for (_, p), s in zip(got, seeds))
    mc.close()


def test_config5_prove_2p24_matches_oracle(gpu_ctx, oracle):
    """BASELINE.json configs[4], the bench workload itself: the 2^24-domain proof of bench.py's rank-0 blob is byte-identical
    to the oracle's (about half a minute of single-thread CPU for the oracle)."""
    import frieda_amd

    data = splitmix64_bytes(100, blob_len_for(24))
    g_root, g_proof = gpu_ctx.commit_and_generate_proof(data, data.size, _cfg(frieda_amd, 20, 4, 0, 20))
    o_root, o_proof = oracle.commit_and_generate_proof(data, data.size, oracle.make_config(20, 4, 0, 20))
    assert g_root == o_root and g_proof.n_inner_layers == 19
    assert g_proof.serialize() == o_proof.serialize()
    assert frieda_amd.verify(g_proof, data.size)


@pytest.mark.parametrize("n", [22, 24])
def test_full_size_prove_verify_and_tie(gpu_ctx, n):
    """configs[2]/[4]: prove -> verify round trip, first FRI root == commit() root (src/proof.rs:126-135), the last
    layer passes stwo's degree assertion (else FriedaPanic), tampering is rejected."""
    import frieda_amd

    data = splitmix64_bytes(100, blob_len_for(n))
    cfg = _cfg(frieda_amd, 20, 4, 0, 20)
    seed = data.size
    commitment, proof = gpu_ctx.commit_and_generate_proof(data, seed, cfg)
    assert commitment == gpu_ctx.commit(data, 4)
    assert proof.n_inner_layers == n - 1 - 4
    assert frieda_amd.verify(proof, seed)
    assert not frieda_amd.verify(proof, seed + 1)
    p = proof.clone()
    e = p.evaluations
    e[3, 2] ^= 1
    p.evaluations = e
    assert not frieda_amd.verify(p, seed)
    # serialisation round trip keeps the proof valid
    assert frieda_amd.verify(frieda_amd.Proof.deserialize(proof.serialize()), seed)


def test_large_domains_beyond_the_baseline_sizes(gpu_ctx):
    """2^26 prove -> verify + tie, and commit() at FRIEDA_MAX_LOG_DOMAIN = 2^28 (index arithmetic beyond 2^24; ~45 GB and
    ~12 GB of workspace).  The 2^28 root is checked against a second, independent device computation: Level B encode +
    single-layer Merkle kernels instead of the fused path."""
    import ctypes as C

    import frieda_amd

    data = splitmix64_bytes(7, blob_len_for(26))
    cfg = _cfg(frieda_amd, 16, 4, 0, 20)
    commitment, proof = gpu_ctx.commit_and_generate_proof(data, 5, cfg)
    assert proof.n_inner_layers == 26 - 1 - 4
    assert commitment == gpu_ctx.commit(data, 4)
    assert frieda_amd.verify(proof, 5) and not frieda_amd.verify(proof, 6)
    del proof

    n = 28
    data = splitmix64_bytes(8, blob_len_for(n))
    root = gpu_ctx.commit(data, 4)
    L_ = gpu_ctx._L
    d_in = DevBuf.from_array(gpu_ctx, data)
    d_coef, d_ev = DevBuf(gpu_ctx, 16 << (n - 4)), DevBuf(gpu_ctx, 16 << n)
    _check(gpu_ctx, L_.frieda_unpack30(gpu_ctx._h, d_in.ptr, data.size, d_coef.ptr, 4 << (n - 4)))
    _check(gpu_ctx, L_.frieda_circle_evaluate(gpu_ctx._h, d_coef.ptr, 4, n - 4, n, d_ev.ptr))
    # layer-by-layer tree with the trait-granular kernels, ping-ponging two buffers
    bufs = [DevBuf(gpu_ctx, 32 << n), DevBuf(gpu_ctx, 32 << (n - 1))]
    cols = (C.c_void_p * 4)(*[C.c_void_p(d_ev.ptr.value + (c << (n + 2))) for c in range(4)])
    _check(gpu_ctx, L_.frieda_merkle_commit_layer(gpu_ctx._h, n, None, cols, 4, bufs[0].ptr))
    cur = 0
    for l in range(n - 1, -1, -1):
        _check(gpu_ctx, L_.frieda_merkle_commit_layer(gpu_ctx._h, l, bufs[cur].ptr, None, 0, bufs[1 - cur].ptr))
        cur = 1 - cur
    assert bytes(bufs[cur].to_array(np.uint8, (32,))) == root


def test_full_size_encode_linearity(gpu_ctx):
    """RS encode is linear: E(a) + E(b) == E(a + b) on a 2^22 domain (coefficients drawn below 2^30 so that sums stay
    canonical through the codec-free Level B entry point)."""
    n, L = 22, 18
    rng = np.random.default_rng(9)
    a = rand_m31(rng, (4, 1 << L))
    b = rand_m31(rng, (4, 1 << L))
    s = ((a.astype(np.uint64) + b) % P).astype(np.uint32)
    outs = []
    for x in (a, b, s):
        d_c, d_o = DevBuf.from_array(gpu_ctx, x), DevBuf(gpu_ctx, 16 << n)
        _check(gpu_ctx, gpu_ctx._L.frieda_circle_evaluate(gpu_ctx._h, d_c.ptr, 4, L, n, d_o.ptr))
        outs.append(d_o.to_array(np.uint32, (4, 1 << n)).astype(np.uint64))
    assert np.array_equal((outs[0] + outs[1]) % P, outs[2])


# ------------------------------------------------------------------------------------------------
# reconstruction side
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,n", [(0, 1), (1, 1), (1, 2), (2, 2), (0, 3), (3, 3), (2, 6), (7, 11), (12, 16), (13, 17), (16, 20), (14, 14)])
def test_circle_interpolate_blocks(gpu_ctx, oracle, L, n):
    """Every aligned 1/2^B block of the codeword gives back the coefficients; bit-exact against the oracle's restatement of
    stwo's interpolate (block 0 with L == n is CpuBackend::interpolate itself)."""
    rng = np.random.default_rng(700 + 31 * n + L)
    ncols = 4 if n < 20 else 2
    coef = rand_m31(rng, (ncols, 1 << L))
    ev = oracle.circle_evaluate(coef, n)
    _, itw = oracle.precompute_twiddles(n)
    blocks = sorted(set([0, (1 << (n - L)) - 1, (1 << (n - L)) // 2, 1 % (1 << (n - L))]))
    for k in blocks:
        blk = np.ascontiguousarray(ev[:, k << L : (k + 1) << L])
        exp = oracle.circle_interpolate_block(blk, n, k, itw)
        assert np.array_equal(exp, coef)
        d_b, d_c = DevBuf.from_array(gpu_ctx, blk), DevBuf(gpu_ctx, 4 * ncols << L)
        _check(gpu_ctx, gpu_ctx._L.frieda_circle_interpolate(gpu_ctx._h, d_b.ptr, ncols, L, n, k, d_c.ptr))
        assert np.array_equal(d_c.to_array(np.uint32, (ncols, 1 << L)), coef), f"block {k}"


@pytest.mark.parametrize("L,n,ncols", [(12, 12, 1), (12, 13, 3), (13, 13, 4), (14, 15, 2), (15, 19, 5), (16, 16, 4), (17, 18, 1), (18, 18, 8), (19, 20, 4),
                                       (20, 20, 2), (21, 22, 4), (22, 22, 1), (23, 23, 2), (24, 24, 4), (20, 24, 4), (24, 25, 1)])
def test_circle_interpolate_pass_plans(gpu_ctx, oracle, L, n, ncols):
    """Every plan of the inverse transform from 12 layers on: the contiguous 12-layer pass, strided passes of 8 and 4 layers
    (intt_tile12_kernel<3,0> / <2,4> / <1,8>) and the generic kernel for the L mod 4 layers left, 1 .. 8 columns (groups of 4, 3, 2, 1
    per workgroup), first / last / a middle block.  Truth: the coefficients that were encoded (oracle encode up to 2^20, the device's own
    parity-tested encode above that); and an unaligned source (word offset 1) takes the generic kernel to the same answer."""
    rng = np.random.default_rng(5100 + 31 * n + L)
    coef = rand_m31(rng, (ncols, 1 << L))
    if n <= 20:
        ev = oracle.circle_evaluate(coef, n)
    else:
        d_c0, d_ev = DevBuf.from_array(gpu_ctx, coef), DevBuf(gpu_ctx, 4 * ncols << n)
        _check(gpu_ctx, gpu_ctx._L.frieda_circle_evaluate(gpu_ctx._h, d_c0.ptr, ncols, L, n, d_ev.ptr))
        ev = d_ev.to_array(np.uint32, (ncols, 1 << n))
        d_c0.free(), d_ev.free()
    nb = 1 << (n - L)
    for k in sorted(set([0, nb - 1, nb // 2])):
        blk = np.ascontiguousarray(ev[:, k << L : (k + 1) << L])
        d_b, d_c = DevBuf.from_array(gpu_ctx, blk), DevBuf(gpu_ctx, 4 * ncols << L)
        _check(gpu_ctx, gpu_ctx._L.frieda_circle_interpolate(gpu_ctx._h, d_b.ptr, ncols, L, n, k, d_c.ptr))
        assert np.array_equal(d_c.to_array(np.uint32, (ncols, 1 << L)), coef), f"block {k}"
    if ncols == 1 and L <= 22:
        import ctypes as C

        shifted = np.concatenate([np.zeros(1, np.uint32), blk.ravel()])
        d_s = DevBuf.from_array(gpu_ctx, shifted)
        _check(gpu_ctx, gpu_ctx._L.frieda_circle_interpolate(gpu_ctx._h, C.c_void_p(d_s.ptr.value + 4), 1, L, n, k, d_c.ptr))
        assert np.array_equal(d_c.to_array(np.uint32, (1, 1 << L)), coef)


@pytest.mark.parametrize("n_bytes", [1, 3, 4, 15, 16, 58, 119, 120, 1000, 4097, 65536])
def test_pack30(gpu_ctx, oracle, n_bytes):
    data = splitmix64_bytes(13, n_bytes)
    felts = oracle.bytes_to_felt_le(data)
    assert oracle.felts_to_bytes(felts, n_bytes) == data.tobytes()
    d_f, d_o = DevBuf.from_array(gpu_ctx, felts), DevBuf(gpu_ctx, n_bytes + 8)
    _check(gpu_ctx, gpu_ctx._L.frieda_pack30(gpu_ctx._h, d_f.ptr, felts.size, d_o.ptr, n_bytes))
    assert d_o.to_array(np.uint8, (n_bytes,)).tobytes() == data.tobytes()


@pytest.mark.parametrize("n_bytes,B", [(58, 4), (1024, 4), (70001, 2), (262146, 4), (3932160, 4)])
def test_encode_erase_reconstruct_round_trip(gpu_ctx, n_bytes, B):
    """encode -> keep one 1/2^B block (erase everything else) -> reconstruct the original bytes, for every block position
    tried; at 2^22 this is the size-independent round-trip property."""
    import ctypes as C

    data = splitmix64_bytes(17, n_bytes)
    L_ = gpu_ctx._L
    nf, npad, lg = C.c_size_t(), C.c_size_t(), C.c_uint32()
    L_.frieda_codec_shape(n_bytes, C.byref(nf), C.byref(npad), C.byref(lg))
    L, n = lg.value, lg.value + B
    d_in = DevBuf.from_array(gpu_ctx, data)
    d_coef, d_ev = DevBuf(gpu_ctx, 4 * npad.value), DevBuf(gpu_ctx, 16 << n)
    _check(gpu_ctx, L_.frieda_unpack30(gpu_ctx._h, d_in.ptr, n_bytes, d_coef.ptr, npad.value))
    _check(gpu_ctx, L_.frieda_circle_evaluate(gpu_ctx._h, d_coef.ptr, 4, L, n, d_ev.ptr))
    ev = d_ev.to_array(np.uint32, (4, 1 << n))
    for k in sorted(set([0, 1, (1 << B) - 1, (1 << B) // 2])):
        blk = np.ascontiguousarray(ev[:, k << L : (k + 1) << L])
        d_b, d_o = DevBuf.from_array(gpu_ctx, blk), DevBuf(gpu_ctx, n_bytes + 8)
        _check(gpu_ctx, L_.frieda_reconstruct_device(gpu_ctx._h, d_b.ptr, L, n, k, n_bytes, d_o.ptr))
        assert d_o.to_array(np.uint8, (n_bytes,)).tobytes() == data.tobytes(), f"block {k}"


@pytest.mark.parametrize("L,n,m", [(1, 2, 1), (3, 5, 1), (3, 5, 3), (4, 8, 2), (6, 10, 3), (8, 12, 4), (8, 9, 2), (10, 14, 5), (12, 16, 4), (16, 20, 8), (14, 18, 13),
                                   (0, 1, 0), (1, 1, 0), (2, 2, 0), (1, 3, 0), (3, 5, 0), (6, 10, 0), (8, 12, 0)])  # m == 0: single sampled points
def test_circle_interpolate_scattered_cells(gpu_ctx, oracle, L, n, m):
    """Any 2^(L-m) distinct cells of 2^m consecutive (bit-reversed) entries give back the coefficients: bit-exact against the
    oracle's fo_reconstruct_cells and against the coefficients themselves; bad arguments are rejected."""
    rng = np.random.default_rng(900 + 100 * L + 10 * n + m)
    ncols = 4
    coef = rand_m31(rng, (ncols, 1 << L))
    ev = oracle.circle_evaluate(coef, n)
    R = 1 << (L - m)
    for trial in range(2 if m else 8):
        idx = rng.choice(1 << (n - m), size=R, replace=False).astype(np.uint32)
        cells = np.ascontiguousarray(np.stack([ev[:, int(c) << m : (int(c) + 1) << m] for c in idx]))  # [R, ncols, 2^m]
        d_cells, d_c = DevBuf.from_array(gpu_ctx, cells), DevBuf(gpu_ctx, 4 * ncols << L)
        rc = gpu_ctx._L.frieda_circle_interpolate_cells(gpu_ctx._h, d_cells.ptr, idx.ctypes.data, R, ncols, m, L, n, d_c.ptr)
        if L <= 12:
            try:
                assert np.array_equal(oracle.reconstruct_cells(cells, idx, n, L), coef)
            except ValueError:
                # single points (m == 0) can form a singular system (tests/test_oracle_golden.py): both sides must say so
                assert m == 0 and rc == 1
                continue
        assert rc == 0
        assert np.array_equal(d_c.to_array(np.uint32, (ncols, 1 << L)), coef), (trial, idx[:4])
    L_ = gpu_ctx._L
    bad = idx.copy()
    if R > 1:
        bad[1] = bad[0]  # repeated cell
        assert L_.frieda_circle_interpolate_cells(gpu_ctx._h, d_cells.ptr, bad.ctypes.data, R, ncols, m, L, n, d_c.ptr) != 0
    bad = idx.copy()
    bad[0] = 1 << (n - m)  # out of range
    assert L_.frieda_circle_interpolate_cells(gpu_ctx._h, d_cells.ptr, bad.ctypes.data, R, ncols, m, L, n, d_c.ptr) != 0
    assert L_.frieda_circle_interpolate_cells(gpu_ctx._h, d_cells.ptr, idx.ctypes.data, R + 1, ncols, m, L, n, d_c.ptr) != 0


@pytest.mark.parametrize("L,n,m", [(3, 5, 0), (3, 6, 0), (4, 8, 0), (2, 2, 0), (5, 9, 1), (8, 12, 0)])
def test_circle_interpolate_cells_over_determined(gpu_ctx, oracle, L, n, m):
    """frieda_circle_interpolate_cells_any: a few cells more than needed, in any order, duplicates tolerated — the call picks an
    independent subset, so the point sets that are singular as drawn (a few % at these tiny domains, m == 0) still reconstruct."""
    rng = np.random.default_rng(4100 + 100 * L + 10 * n + m)
    ncols = 4
    coef = rand_m31(rng, (ncols, 1 << L))
    ev = oracle.circle_evaluate(coef, n)
    R = 1 << (L - m)
    total = 1 << (n - m)
    saw_singular_prefix = 0
    for trial in range(40 if L <= 4 else 4):
        n_avail = min(total, R + 4)
        idx = rng.choice(total, size=n_avail, replace=False).astype(np.uint32)
        if trial % 3 == 0 and n_avail > R:
            idx[-1] = idx[0]  # a repeated cell among the spares
        cells = np.ascontiguousarray(np.stack([ev[:, int(c) << m : (int(c) + 1) << m] for c in idx]))
        d_cells, d_c = DevBuf.from_array(gpu_ctx, cells), DevBuf(gpu_ctx, 4 * ncols << L)
        used = (C.c_uint32 * R)()
        _check(gpu_ctx, gpu_ctx._L.frieda_circle_interpolate_cells_any(gpu_ctx._h, d_cells.ptr, idx.ctypes.data, n_avail, ncols, m, L, n, d_c.ptr, used))
        assert np.array_equal(d_c.to_array(np.uint32, (ncols, 1 << L)), coef), (trial, idx)
        u = list(used)
        assert len(set(int(idx[k]) for k in u)) == R
        # the oracle on exactly the subset the product used gives the same coefficients
        assert np.array_equal(oracle.reconstruct_cells(cells[u][:, :1], idx[u], n, L), coef[:1])
        # was the first-R prefix singular by itself?  (then the exact-count entry refuses it and the over-determined one recovered)
        rc = gpu_ctx._L.frieda_circle_interpolate_cells(gpu_ctx._h, d_cells.ptr, idx.ctypes.data, R, ncols, m, L, n, d_c.ptr)
        saw_singular_prefix += rc != 0
    # rank-deficient offers are refused: one cell repeated n_avail times; fewer cells than needed
    same = np.full(R + 2, idx[0], dtype=np.uint32)
    assert gpu_ctx._L.frieda_circle_interpolate_cells_any(gpu_ctx._h, d_cells.ptr, same.ctypes.data, min(R + 2, n_avail), ncols, m, L, n, d_c.ptr, None) == (1 if R > 1 else 0)
    if R > 1:
        assert gpu_ctx._L.frieda_circle_interpolate_cells_any(gpu_ctx._h, d_cells.ptr, idx.ctypes.data, R - 1, ncols, m, L, n, d_c.ptr, None) == 1
    if (L, n, m) == (3, 5, 0):
        # the case this entry exists for, deterministically: these 8 points of the 32-point domain form a singular system
        # (found by search with the oracle); the exact-count entry refuses them, two spare points repair it
        sing = np.array([1, 3, 4, 8, 11, 14, 16, 27], dtype=np.uint32)
        with pytest.raises(ValueError):
            oracle.reconstruct_cells(np.ascontiguousarray(ev[:, sing].T.reshape(-1, ncols, 1)), sing, n, L)
        offer = np.concatenate([sing, np.array([2, 30], dtype=np.uint32)])
        cells = np.ascontiguousarray(ev[:, offer].T.reshape(-1, ncols, 1))
        d_cells = DevBuf.from_array(gpu_ctx, cells)
        assert gpu_ctx._L.frieda_circle_interpolate_cells(gpu_ctx._h, d_cells.ptr, offer.ctypes.data, R, ncols, m, L, n, d_c.ptr) == 1
        used = (C.c_uint32 * R)()
        _check(gpu_ctx, gpu_ctx._L.frieda_circle_interpolate_cells_any(gpu_ctx._h, d_cells.ptr, offer.ctypes.data, 10, ncols, m, L, n, d_c.ptr, used))
        assert np.array_equal(d_c.to_array(np.uint32, (ncols, 1 << L)), coef) and max(used) >= 8


@pytest.mark.parametrize("L,n,m,with_oracle", [(10, 14, 1, True), (10, 12, 1, False), (12, 16, 2, False), (13, 17, 1, False), (15, 19, 3, False),
                                               (9, 13, 0, True), (11, 15, 0, False), (12, 12, 0, False)])  # m == 0: single sampled points
def test_circle_interpolate_many_cells_device_solve(gpu_ctx, oracle, L, n, m, with_oracle):
    """More than 256 cells (512 .. 4096): the cell matrix is inverted on the device by a blocked Gauss-Jordan with row pivoting.
    The coefficients come back exactly; at 512 cells also against the oracle's fo_reconstruct_cells (cubic on the host)."""
    rng = np.random.default_rng(1900 + 100 * L + 10 * n + m)
    ncols = 4
    coef = rand_m31(rng, (ncols, 1 << L))
    ev = oracle.circle_evaluate(coef, n)
    R = 1 << (L - m)
    assert R > 256
    for trial in range(2):
        if trial == 0:
            idx = rng.choice(1 << (n - m), size=R, replace=False).astype(np.uint32)
        else:  # clustered cells: runs of neighbours share most of their twiddle path (zero pivots inside a panel are likelier)
            if (1 << (n - m)) // 8 < R // 8 + 1:
                continue
            base = rng.choice((1 << (n - m)) // 8, size=R // 8, replace=False).astype(np.uint32) * 8
            idx = (base[:, None] + np.arange(8, dtype=np.uint32)[None, :]).ravel()[rng.permutation(R)].astype(np.uint32)
        cells = np.ascontiguousarray(np.stack([ev[:, int(c) << m : (int(c) + 1) << m] for c in idx]))  # [R, ncols, 2^m]
        if with_oracle and trial == 0:
            assert np.array_equal(oracle.reconstruct_cells(cells[:, :1], idx, n, L), coef[:1])
        d_cells, d_c = DevBuf.from_array(gpu_ctx, cells), DevBuf(gpu_ctx, 4 * ncols << L)
        _check(gpu_ctx, gpu_ctx._L.frieda_circle_interpolate_cells(gpu_ctx._h, d_cells.ptr, idx.ctypes.data, R, ncols, m, L, n, d_c.ptr))
        assert np.array_equal(d_c.to_array(np.uint32, (ncols, 1 << L)), coef), (trial, idx[:4])
    bad = idx.copy()
    bad[R - 1] = bad[3]  # repeated cell
    assert gpu_ctx._L.frieda_circle_interpolate_cells(gpu_ctx._h, d_cells.ptr, bad.ctypes.data, R, ncols, m, L, n, d_c.ptr) != 0
    # more cells than the solver takes
    assert gpu_ctx._L.frieda_circle_interpolate_cells(gpu_ctx._h, d_cells.ptr, idx.ctypes.data, 8192, ncols, 1, 14, 18, d_c.ptr) != 0


@pytest.mark.parametrize("n_bytes,B,log_cell_below", [(58, 4, 1), (1024, 4, 3), (70001, 2, 6), (262146, 4, 8), (3932160, 4, 8), (3932160, 4, 12), (983040, 4, 10),
                                                      (1024, 4, 7), (15360, 4, 10)])  # the last two: single sampled points (m == 0)
def test_encode_sample_cells_reconstruct_round_trip(gpu_ctx, n_bytes, B, log_cell_below):
    """encode -> keep 2^j random cells scattered over the whole codeword (a sampling client's view) -> the original bytes."""
    import ctypes as C

    data = splitmix64_bytes(19, n_bytes)
    L_ = gpu_ctx._L
    nf, npad, lg = C.c_size_t(), C.c_size_t(), C.c_uint32()
    L_.frieda_codec_shape(n_bytes, C.byref(nf), C.byref(npad), C.byref(lg))
    L, n = lg.value, lg.value + B
    j = min(log_cell_below, L) if L >= 2 else 0
    m = L - j
    d_in = DevBuf.from_array(gpu_ctx, data)
    d_coef, d_ev = DevBuf(gpu_ctx, 4 * npad.value), DevBuf(gpu_ctx, 16 << n)
    _check(gpu_ctx, L_.frieda_unpack30(gpu_ctx._h, d_in.ptr, n_bytes, d_coef.ptr, npad.value))
    _check(gpu_ctx, L_.frieda_circle_evaluate(gpu_ctx._h, d_coef.ptr, 4, L, n, d_ev.ptr))
    ev = d_ev.to_array(np.uint32, (4, 1 << n))
    rng = np.random.default_rng(n_bytes)
    idx = rng.choice(1 << (n - m), size=1 << j, replace=False).astype(np.uint32)
    cells = np.ascontiguousarray(np.stack([ev[:, int(c) << m : (int(c) + 1) << m] for c in idx]))
    d_cells, d_o = DevBuf.from_array(gpu_ctx, cells), DevBuf(gpu_ctx, n_bytes + 8)
    _check(gpu_ctx, L_.frieda_reconstruct_cells_device(gpu_ctx._h, d_cells.ptr, idx.ctypes.data, 1 << j, m, L, n, n_bytes, d_o.ptr))
    assert d_o.to_array(np.uint8, (n_bytes,)).tobytes() == data.tobytes()


def test_python_reconstruction_helpers(gpu_ctx, oracle):
    """Context.reconstruct_from_block / reconstruct_from_cells (host arrays in, bytes out) on the oracle's own codeword."""
    data = splitmix64_bytes(23, 5000).tobytes()
    coef, L = oracle.polynomial_from_bytes(data)
    n = L + 4
    ev = oracle.circle_evaluate(coef, n)
    assert gpu_ctx.reconstruct_from_block(np.ascontiguousarray(ev[:, 5 << L : 6 << L]), n, 5, len(data)) == data
    m = L - 4
    rng = np.random.default_rng(3)
    idx = rng.choice(1 << (n - m), size=16, replace=False).astype(np.uint32)
    cells = np.ascontiguousarray(np.stack([ev[:, int(c) << m : (int(c) + 1) << m] for c in idx]))
    assert gpu_ctx.reconstruct_from_cells(cells, idx, L, n, len(data)) == data


# ---- batches of small blobs: every kernel handles the whole batch; results = separate calls ----
@pytest.mark.parametrize("length,count,seeded", [(1024, 1, True), (1024, 7, False), (4096, 33, True), (16384, 16, True), (65536, 5, True),
                                                 (262144, 3, False), (58, 4, True), (16, 3, True)])
def test_batched_proofs_equal_separate_proofs(gpu_ctx, oracle, length, count, seeded):
    import frieda_amd

    cfg = _cfg(frieda_amd, 10, 4, 0, 20)
    blobs = [splitmix64_bytes(7000 + 13 * i + length, length).tobytes() for i in range(count)]
    seeds = [1000 + i for i in range(count)] if seeded else None
    got = gpu_ctx.commit_and_generate_proof_batch(blobs, seeds, cfg)
    assert len(got) == count
    for i, (root, proof) in enumerate(got):
        er, ep = gpu_ctx.commit_and_generate_proof(blobs[i], seeds[i] if seeded else None, cfg)
        assert root == er and proof.serialize() == ep.serialize()
        if length >= 58:
            assert frieda_amd.verify(proof, seeds[i] if seeded else None)
        else:  # a 2^5 domain: the restated verifier hits one of stwo's assertions (the oracle does the same)
            with pytest.raises(frieda_amd.FriedaPanic):
                frieda_amd.verify(proof, seeds[i])
            with pytest.raises(RuntimeError):
                oracle.verify(oracle.commit_and_generate_proof(blobs[i], seeds[i], oracle.make_config(10, 4, 0, 20))[1], seeds[i])
    # the oracle on the first and last blob
    for i in {0, count - 1}:
        o_root, o_proof = oracle.commit_and_generate_proof(blobs[i], seeds[i] if seeded else None, oracle.make_config(10, 4, 0, 20))
        assert got[i][0] == o_root and got[i][1].serialize() == o_proof.serialize()
    roots = gpu_ctx.commit_batch(blobs, 4)
    assert roots == [g[0] for g in got]


def test_batched_proofs_other_configs_and_device_input(gpu_ctx, oracle):
    import torch

    import frieda_amd

    # last-layer degree bound 2, blowup 2, fewer queries; strided device-resident input
    cfg = _cfg(frieda_amd, 6, 2, 2, 9)
    length, stride, count = 3000, 3072, 6
    host = np.zeros(stride * count, dtype=np.uint8)
    blobs = []
    for i in range(count):
        b = splitmix64_bytes(8100 + i, length)
        host[i * stride : i * stride + length] = b
        host[i * stride + length : (i + 1) * stride] = 0xA5  # padding between blobs must be ignored
        blobs.append(b.tobytes())
    dev = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    seeds = [5 * i + 1 for i in range(count)]
    got = gpu_ctx.commit_and_generate_proof_batch_device(dev.data_ptr(), stride, length, count, seeds, cfg)
    for i, (root, proof) in enumerate(got):
        o_root, o_proof = oracle.commit_and_generate_proof(blobs[i], seeds[i], oracle.make_config(6, 2, 2, 9))
        assert root == o_root and proof.serialize() == o_proof.serialize()
    assert gpu_ctx.commit_batch_device(dev.data_ptr(), stride, length, count, 2) == [oracle.commit(b, 2) for b in blobs]
    # a batch whose grind needs more than the first chunk for some blob: 26 bits of work
    cfg26 = _cfg(frieda_amd, 24, 4, 0, 4)
    got = gpu_ctx.commit_and_generate_proof_batch(blobs[:3], None, cfg26)
    for b, (root, proof) in zip(blobs[:3], got):
        er, ep = gpu_ctx.commit_and_generate_proof(b, None, cfg26)
        assert root == er and proof.serialize() == ep.serialize() and frieda_amd.verify(proof, None)


def test_batch_argument_errors(gpu_ctx):
    import frieda_amd

    cfg = _cfg(frieda_amd, 4, 4, 0, 5)
    with pytest.raises(ValueError):
        gpu_ctx.commit_and_generate_proof_batch([b"abc", b"abcd"], None, cfg)
    assert gpu_ctx.commit_and_generate_proof_batch([], None, cfg) == []
    buf = (C.c_uint8 * 64)()
    with pytest.raises(frieda_amd.FriedaError):  # stride smaller than the blob length
        gpu_ctx._prove_batch(gpu_ctx._L.frieda_commit_and_generate_proof_batch, buf, 16, 32, 2, None, cfg)
    # last layer of 2^12 points: the single-proof API falls back to the host channel, a batch is refused
    big_last = _cfg(frieda_amd, 4, 4, 8, 5)
    blob = splitmix64_bytes(1, 65536).tobytes()
    gpu_ctx.commit_and_generate_proof(blob, None, big_last)
    with pytest.raises(frieda_amd.FriedaError):
        gpu_ctx.commit_and_generate_proof_batch([blob, blob], None, big_last)
    # the context is usable afterwards
    assert len(gpu_ctx.commit_and_generate_proof_batch([blob, blob], None, cfg)) == 2


def test_two_batches_in_flight(gpu_ctx):
    """frieda_prove_batch_begin / _finish on two contexts: same proofs as the one-call form; count mismatch is refused."""
    import torch

    import frieda_amd

    cfg = _cfg(frieda_amd, 8, 4, 0, 12)
    length, count = 2048, 9
    host = np.concatenate([splitmix64_bytes(9100 + i, length) for i in range(2 * count)])
    dev = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    other = frieda_amd.Context(0)
    seeds_a, seeds_b = list(range(count)), list(range(100, 100 + count))
    gpu_ctx.prove_batch_begin_device(dev.data_ptr(), length, length, count, seeds_a, cfg)
    other.prove_batch_begin_device(dev.data_ptr() + count * length, length, length, count, seeds_b, cfg)
    with pytest.raises(frieda_amd.FriedaError):
        gpu_ctx.prove_batch_finish(count + 1)
    # the mismatch left the batch in flight
    got_a = gpu_ctx.prove_batch_finish(count)
    got_b = other.prove_batch_finish(count)
    exp_a = gpu_ctx.commit_and_generate_proof_batch_device(dev.data_ptr(), length, length, count, seeds_a, cfg)
    exp_b = gpu_ctx.commit_and_generate_proof_batch_device(dev.data_ptr() + count * length, length, length, count, seeds_b, cfg)
    for got, exp in ((got_a, exp_a), (got_b, exp_b)):
        assert [(r, p.serialize()) for r, p in got] == [(r, p.serialize()) for r, p in exp]
    with pytest.raises(frieda_amd.FriedaError):
        gpu_ctx.prove_batch_finish(count)  # nothing in flight
    other.close()


@pytest.mark.parametrize("length,count", [(2048, 37), (61440, 9), (700, 3)])
def test_batch_policy_stream_equals_separate_calls(gpu_ctx, oracle, length, count):
    """BatchPipeline.run_stream_device: a stream of equal-length device blobs cut into calls by the library's batch policy
    (frieda_batch_plan) — whatever the cut (default budget, a 1 MB budget = one blob per call, four calls per context), the roots and
    proofs are those of separate calls and the oracle's."""
    import torch

    import frieda_amd

    cfg = _cfg(frieda_amd, 8, 4, 0, 12)
    ocfg = oracle.make_config(8, 4, 0, 12)
    blobs = [splitmix64_bytes(9700 + i, length) for i in range(count)]
    dev = torch.from_numpy(np.concatenate(blobs)).cuda()
    torch.cuda.synchronize()
    seeds = [None if count < 4 else 40 + i for i in range(count)]
    seeds = None if count < 4 else seeds
    expect = [oracle.commit_and_generate_proof(b.tobytes(), None if seeds is None else seeds[i], ocfg) for i, b in enumerate(blobs)]
    want = [(bytes(r), p.serialize()) for r, p in expect]
    pipe = frieda_amd.BatchPipeline(0, 2)
    try:
        cuts = []
        for opts in ({}, {"FRIEDA_BATCH_BUDGET_MB": 1}, {"FRIEDA_BATCH_BUDGET_MB": 0, "FRIEDA_BATCH_CALLS_PER_CTX": 4}):
            for k, v in opts.items():
                pipe.ctxs[0].set_option(k, v)
            cut = pipe.plan(length, count, cfg)
            assert sum(cut) == count
            cuts.append(cut)
            got = pipe.run_stream_device(dev.data_ptr(), length, length, count, seeds, cfg)
            assert [(r, p.serialize()) for r, p in got] == want
        if count >= 8:
            assert max(cuts[1]) < max(cuts[0]) and len(cuts[0]) == 2 and len(cuts[2]) > 2  # the options did change the cut
        if 2 * frieda_amd.workspace_bytes(length, 4) > (1 << 20) and count >= 4:
            assert max(cuts[1]) == 1  # 1 MB of workspace: one blob per call
    finally:
        pipe.close()


def test_batch_budget_option_range(gpu_ctx):
    import frieda_amd

    for name, bad in (("FRIEDA_BATCH_BUDGET_MB", -1), ("FRIEDA_BATCH_CALLS_PER_CTX", 0), ("FRIEDA_BATCH_CALLS_PER_CTX", 65), ("FRIEDA_UNPACK_TILES", 3),
                      ("FRIEDA_UNPACK_TILES", 7), ("FRIEDA_TEST_GRIND_FIRST_LOG", 10)):
        with pytest.raises(frieda_amd.FriedaError):
            gpu_ctx.set_option(name, bad)  # in-range-but-unsupported values are refused too; the grind hook is no longer an option
    gpu_ctx.set_option("FRIEDA_UNPACK_TILES", 4)
    assert gpu_ctx._L.frieda_ctx_test_set_grind_first_log(gpu_ctx._h, 5) != 0  # below the smallest window
    assert gpu_ctx._L.frieda_ctx_test_set_grind_first_log(gpu_ctx._h, 0) == 0


@pytest.mark.parametrize("iters", [1, 4, 8, 64])
def test_batched_grind_claim_sizes(oracle, iters):
    """The batched grind claims `FRIEDA_GRIND_ITERS / 4` units of 1024 nonces per atomic (one counter per blob, each on its own cache line):
    whatever the claim size — also when a claim reaches past the end of the range (test hook: 2^10-nonce first range, then doubling) — the
    nonce is the MINIMUM and the proofs are the oracle's."""
    import frieda_amd

    cfg = _cfg(frieda_amd, 14, 4, 0, 8)
    ocfg = oracle.make_config(14, 4, 0, 8)
    blobs = [splitmix64_bytes(9800 + i, 1200).tobytes() for i in range(7)]
    expect = [oracle.commit_and_generate_proof(b, 77 + i, ocfg) for i, b in enumerate(blobs)]
    ctx = frieda_amd.Context(0)
    try:
        ctx.set_option("FRIEDA_GRIND_ITERS", iters)
        for first_log in (0, 10):
            assert ctx._L.frieda_ctx_test_set_grind_first_log(ctx._h, first_log) == 0
            got = ctx.commit_and_generate_proof_batch(blobs, [77 + i for i in range(len(blobs))], cfg)
            assert [(bytes(r), p.serialize()) for r, p in expect] == [(r, p.serialize()) for r, p in got]
            r, p = ctx.commit_and_generate_proof(blobs[0], 77, cfg)
            assert p.serialize() == expect[0][1].serialize()
        with pytest.raises(frieda_amd.FriedaError):
            ctx.set_option("FRIEDA_GRIND_ITERS", 65)
    finally:
        ctx.close()


def test_sharded_batch_helpers_use_the_batched_kernels(oracle):
    """frieda_amd.batch (the multi-GPU sharding layer) on one rank: equal-length shards go through the batched kernels, ragged
    ones through the C ABI's multi entry (frieda_commit_many / frieda_prove_many, two proofs in flight); both give the oracle's
    roots and proofs.  The single-process form over the node's devices (commit_many_on_node / prove_many_on_node) likewise."""
    import frieda_amd
    from frieda_amd import batch

    cfg = _cfg(frieda_amd, 8, 4, 0, 10)
    ocfg = oracle.make_config(8, 4, 0, 10)
    equal = [splitmix64_bytes(9300 + i, 1500).tobytes() for i in range(5)]
    ragged = equal[:2] + [splitmix64_bytes(9400, 700).tobytes()]
    for blobs in (equal, ragged):
        seeds = list(range(len(blobs)))
        assert batch.commit_batch(blobs, 4) == [oracle.commit(b, 4) for b in blobs]
        roots, proofs = batch.prove_batch(blobs, seeds, cfg)
        for i, b in enumerate(blobs):
            o_root, o_proof = oracle.commit_and_generate_proof(b, seeds[i], ocfg)
            assert roots[i] == o_root and proofs[i].serialize() == o_proof.serialize()
    assert batch.commit_many_on_node(ragged, 4, devices=[0]) == [oracle.commit(b, 4) for b in ragged]
    got = batch.prove_many_on_node(ragged, [7, 8, 9], cfg, devices=[0])
    for (root, proof), b, sd in zip(got, ragged, [7, 8, 9]):
        o_root, o_proof = oracle.commit_and_generate_proof(b, sd, ocfg)
        assert root == o_root and proof.serialize() == o_proof.serialize()


def test_whole_proof_with_26_bit_proof_of_work(gpu_ctx, oracle):
    """pow_bits above the 24 the other cases stop at (PcsConfig::pow_bits is a free u32, src/proof.rs:108-116): the reference's 1 KiB bench
    input with a 26-bit proof of work — nonce 36 547 975, six seconds of the oracle's sequential scan — whole proof byte-identical."""
    import frieda_amd

    data = pattern_bytes(1024).tobytes()
    o_root, o_proof = oracle.commit_and_generate_proof(data, 1, oracle.make_config(26, 4, 0, 20))
    assert o_proof.c.proof_of_work == 36547975
    r, p = gpu_ctx.commit_and_generate_proof(data, 1, _cfg(frieda_amd, 26, 4, 0, 20))
    assert r == o_root and p.serialize() == o_proof.serialize() and frieda_amd.verify(p, 1)


def test_grind_retry_loop(gpu_ctx, oracle, monkeypatch):
    """The first grind range normally holds the nonce with probability 1 - e^-16; a test hook shortens it so that the host's
    retry loop (next range, doubled) runs — single proofs and batches, where some blobs finish rounds before others."""
    import frieda_amd

    cfg = _cfg(frieda_amd, 18, 4, 0, 8)
    blobs = [splitmix64_bytes(9500 + i, 900).tobytes() for i in range(6)]
    expect = [oracle.commit_and_generate_proof(b, i, oracle.make_config(18, 4, 0, 8)) for i, b in enumerate(blobs)]
    assert len({p.c.proof_of_work for _, p in expect}) > 1
    _check(gpu_ctx, gpu_ctx._L.frieda_ctx_test_set_grind_first_log(gpu_ctx._h, 10))  # 1024 nonces, then 2048, 4096, ... (this context only)
    try:
        got = gpu_ctx.commit_and_generate_proof_batch(blobs, list(range(len(blobs))), cfg)
        for (er, ep), (gr, gp) in zip(expect, got):
            assert er == gr and ep.serialize() == gp.serialize()
        r, p = gpu_ctx.commit_and_generate_proof(blobs[0], 0, cfg)
        assert r == expect[0][0] and p.serialize() == expect[0][1].serialize()
    finally:
        gpu_ctx._L.frieda_ctx_test_set_grind_first_log(gpu_ctx._h, 0)


def test_release_workspace(gpu_ctx):
    import frieda_amd

    cfg = _cfg(frieda_amd, 6, 4, 0, 8)
    blobs = [splitmix64_bytes(9600 + i, 5000).tobytes() for i in range(3)]
    before = gpu_ctx.commit_and_generate_proof_batch(blobs, None, cfg)
    gpu_ctx.release_workspace()
    gpu_ctx.release_workspace()  # idempotent
    after = gpu_ctx.commit_and_generate_proof_batch(blobs, None, cfg)
    assert [(r, p.serialize()) for r, p in before] == [(r, p.serialize()) for r, p in after]
    assert gpu_ctx.commit(blobs[0], 4) == before[0][0]


@pytest.mark.parametrize("nq", [64, 65, 300])
def test_many_queries_with_duplicate_draws(gpu_ctx, oracle, nq):
    """Up to 300 queries over a 2^9 .. 2^17 domain: repeated draws are deduplicated (Queries::generate), most Merkle nodes of the
    small trees are opened; single proofs and a batch equal the oracle's."""
    import frieda_amd

    cfg = _cfg(frieda_amd, 5, 3, 1, nq)
    ocfg = oracle.make_config(5, 3, 1, nq)
    blobs = [splitmix64_bytes(9700 + i, 200).tobytes() for i in range(3)] + [splitmix64_bytes(9800, 40000).tobytes()]
    for blob in (blobs[0], blobs[3]):
        o_root, o_proof = oracle.commit_and_generate_proof(blob, 7, ocfg)
        r1, p1 = gpu_ctx.commit_and_generate_proof(blob, 7, cfg)
        assert r1 == o_root and p1.serialize() == o_proof.serialize()
    got = gpu_ctx.commit_and_generate_proof_batch(blobs[:3], [1, 2, 3], cfg)
    for i, (ra, pa) in enumerate(got):
        o_root, o_proof = oracle.commit_and_generate_proof(blobs[i], i + 1, ocfg)
        assert ra == o_root and pa.serialize() == o_proof.serialize()


def test_openings_device_path_host_path_and_fallbacks(gpu_ctx, oracle, monkeypatch):
    """The openings are normally produced by the decommit kernel (one launch behind the grind).  The host planner + gather
    launch remains as the fallback: forced by FRIEDA_HOST_DECOMMIT, taken for more than 1024 queries, and taken when the
    kernel reports that its tables do not fit (n * unique queries > its LDS capacity).  All of them equal the oracle."""
    import frieda_amd

    cases = [("pattern:5000", 8, (10, 4, 1, 300)), ("pattern:120", 1, (4, 1, 0, 5)), ("pattern:70000", 3, (8, 4, 0, 20))]
    for spec, seed, cfg in cases:
        data = resolve_input(spec, None)
        o_root, o_proof = oracle.commit_and_generate_proof(data, seed, oracle.make_config(*cfg))
        for host in (False, True):
            gpu_ctx.set_option("FRIEDA_HOST_DECOMMIT", int(host))
            r, p = gpu_ctx.commit_and_generate_proof(data, seed, _cfg(frieda_amd, *cfg))
            assert r == o_root and p.serialize() == o_proof.serialize(), (spec, host)
    # batch through the forced host path
    gpu_ctx.set_option("FRIEDA_HOST_DECOMMIT", 1)
    cfg = _cfg(frieda_amd, 6, 4, 0, 20)
    blobs = [splitmix64_bytes(9900 + i, 3000).tobytes() for i in range(5)]
    got = gpu_ctx.commit_and_generate_proof_batch(blobs, [1, 2, 3, 4, 5], cfg)
    for i, (ra, pa) in enumerate(got):
        o_root, o_proof = oracle.commit_and_generate_proof(blobs[i], i + 1, oracle.make_config(6, 4, 0, 20))
        assert ra == o_root and pa.serialize() == o_proof.serialize()
    gpu_ctx.set_option("FRIEDA_HOST_DECOMMIT", 0)
    # 1000 queries on a 2^14 domain: ~970 unique, 14 * 970 table slots > the kernel's capacity -> it reports overflow, host plans
    # 1100 queries: above the kernel's limit, host plans from the start
    data = splitmix64_bytes(9950, 15000).tobytes()
    for nq in (1000, 1100):
        o_root, o_proof = oracle.commit_and_generate_proof(data, 5, oracle.make_config(5, 4, 0, nq))
        r, p = gpu_ctx.commit_and_generate_proof(data, 5, _cfg(frieda_amd, 5, 4, 0, nq))
        assert r == o_root and p.serialize() == o_proof.serialize(), nq
        assert frieda_amd.verify(p, 5)



def test_randomised_parity_short(gpu_ctx):
    """Fifteen seconds of tools/fuzz_parity.py: random blob sizes (0 B .. 8 MB), blow-ups, last-layer bounds, query counts, proof-of-work bits and
    seeds, single proofs and batches, every proof byte-compared with the oracle's."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("fuzz_parity", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "fuzz_parity.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    n_single, n_batch, _, n_big = mod.run(15.0, 20261003, gpu_ctx)
    assert n_single > 20 and n_big >= 1  # the first case of a run is a 0.4 - 8 MB blob (strided encode passes)
