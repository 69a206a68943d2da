"""GPU: the transform kernels of the encode's fast plan (frieda_amd/csrc/ntt.hip: ntt_tile12_kernel<3, 0>, <2, 4>, <1, 8> and
ntt_tile12_rep_kernel, which runs its first radix-16 stage on the registers it loaded) — bit-exact against the oracle on the smallest
shapes that reach each of them, through frieda_circle_evaluate (every output word) and through commit / commit_and_generate_proof.

    kernels                 L    n    what else the shape has
    <3,0> alone             12   16
    <1,8> + <3,0>           13   16   three zero-padded layers executed as butterflies (source words beyond 2^L read as zero)
    <1,8> + <3,0>           16   17
    <2,4> + <3,0>           17   20   three zero-padded layers
    <2,4> + <3,0>           20   21   (the rep kernel with FRIEDA_NTT_REP = 1)
    rep kernel + <3,0>      17   21   three zero-padded layers; a batch of two blobs (1024 workgroups), or one blob with FRIEDA_NTT_REP = 1

A launch below 512 tiles gives every workgroup ONE column (FRIEDA_NTT_CPW_SMALL), so the column loop of ntt_tile12_kernel only runs with
that option at 4: every evaluate case runs on such a context too, with 1, 2, 3 and 4 columns (3: an odd count above one).
"""
import ctypes as C

import numpy as np
import pytest

from conftest import splitmix64_bytes
from util import DevBuf, GuardedBuf

pytestmark = pytest.mark.gpu

P = 2**31 - 1
SHAPES = [(12, 16), (13, 16), (16, 17), (17, 20), (20, 21), (17, 21)]
_expected = {}


def exact_len(L):
    return (4 << L) * 30 // 8


def coefficients(L, n):
    return np.random.default_rng(7000 + 32 * L + n).integers(0, P, (4, 1 << L), dtype=np.uint32)


def expected(oracle, L, n):
    """the oracle's evaluation of the four columns of coefficients(L, n), computed once per shape and never modified"""
    if (L, n) not in _expected:
        tw, _ = oracle.precompute_twiddles(n)
        coef = coefficients(L, n)
        exp = np.concatenate([oracle.circle_evaluate(coef[c : c + 1], n, tw) for c in range(4)])
        exp.setflags(write=False)
        _expected[(L, n)] = exp
    return _expected[(L, n)]


@pytest.fixture(scope="module")
def wide_ctx():
    """four columns per workgroup in small launches too, and the rep kernel wherever the shape allows"""
    import frieda_amd

    ctx = frieda_amd.Context(0)
    ctx.set_option("FRIEDA_NTT_CPW_SMALL", 4)
    ctx.set_option("FRIEDA_NTT_REP", 1)
    yield ctx
    ctx.close()


def evaluate(ctx, coef, L, n, out=None):
    from frieda_amd.api import _check

    ncols = coef.shape[0]
    d_c = DevBuf.from_array(ctx, coef)
    d_o = out if out is not None else DevBuf(ctx, 4 * ncols << n)
    _check(ctx._L.frieda_circle_evaluate(ctx._h, d_c.ptr, ncols, L, n, d_o.ptr), ctx._h)
    return d_o


@pytest.mark.parametrize("ncols", [1, 2, 3, 4])
@pytest.mark.parametrize("L,n", SHAPES, ids=[f"L{L}-n{n}" for L, n in SHAPES])
def test_evaluate_every_word(gpu_ctx, wide_ctx, oracle, L, n, ncols):
    exp = expected(oracle, L, n)[:ncols]
    coef = coefficients(L, n)[:ncols]
    for name, ctx in (("default", gpu_ctx), ("cpw_small=4,rep=1", wide_ctx)):
        got = evaluate(ctx, coef, L, n).to_array(np.uint32, (ncols, 1 << n))
        assert np.array_equal(got, exp), (name, L, n, ncols, int(np.count_nonzero(got != exp)))


@pytest.mark.parametrize("L,n,offset", [(16, 17, 48), (17, 21, 4096 + 16)], ids=["L16-n17", "L17-n21-rep"])
def test_output_at_an_offset_inside_poison(wide_ctx, oracle, L, n, offset):
    """the evaluation lands at an offset pointer (16-byte aligned: the fast kernels' condition) inside one poisoned allocation; every
    byte around it keeps its poison"""
    exp = expected(oracle, L, n)
    out = GuardedBuf(wide_ctx, 16 << n, offset=offset)
    evaluate(wide_ctx, coefficients(L, n), L, n, out=out)
    assert np.array_equal(out.payload(np.uint32, (4, 1 << n)), exp)
    out.assert_zones_intact("evaluation")


COMMIT_SHAPES = [(12, 4), (13, 3), (16, 1), (17, 3), (20, 1), (17, 4)]


@pytest.mark.parametrize("L,B", COMMIT_SHAPES, ids=[f"L{L}-B{B}" for L, B in COMMIT_SHAPES])
def test_commit_root(gpu_ctx, wide_ctx, oracle, L, B):
    data = splitmix64_bytes(7100 + 8 * L + B, exact_len(L) - 4321).tobytes()
    lgs, nf, npad = C.c_uint32(), C.c_size_t(), C.c_size_t()
    gpu_ctx._L.frieda_codec_shape(len(data), C.byref(nf), C.byref(npad), C.byref(lgs))
    assert lgs.value == L
    want = oracle.commit(data, B)
    assert gpu_ctx.commit(data, B) == want
    assert wide_ctx.commit(data, B) == want


@pytest.mark.parametrize("L,B", [(13, 3), (16, 1), (17, 3)], ids=["L13-B3", "L16-B1", "L17-B3"])
def test_whole_proof(gpu_ctx, oracle, L, B):
    import frieda_amd

    data = splitmix64_bytes(7200 + 8 * L + B, exact_len(L) - 999).tobytes()
    cfg = frieda_amd.PcsConfig(frieda_amd.FriConfig(B, 0, 20), 6)
    o_root, o_proof = oracle.commit_and_generate_proof(data, 5, oracle.make_config(6, B, 0, 20))
    root, proof = gpu_ctx.commit_and_generate_proof(data, 5, cfg)
    assert root == o_root and proof.serialize() == o_proof.serialize()


def test_rep_kernel_batch_of_two_and_forced_on_one(gpu_ctx, wide_ctx, oracle):
    """L = 17, n = 21: two blobs in one call are 1024 workgroups of the rep kernel (the default rule); one blob takes it with
    FRIEDA_NTT_REP = 1.  Roots and whole proofs."""
    import frieda_amd

    L, B = 17, 4
    blobs = [splitmix64_bytes(7300 + i, exact_len(L) - 77).tobytes() for i in range(2)]
    cfg = frieda_amd.PcsConfig(frieda_amd.FriConfig(B, 0, 20), 6)
    want = [oracle.commit_and_generate_proof(b, 11 + i, oracle.make_config(6, B, 0, 20)) for i, b in enumerate(blobs)]
    got = gpu_ctx.commit_and_generate_proof_batch(blobs, [11, 12], cfg)
    for (r, p), (o_r, o_p) in zip(got, want):
        assert r == o_r and p.serialize() == o_p.serialize()
    assert gpu_ctx.commit_batch(blobs, B) == [w[0] for w in want]
    r, p = wide_ctx.commit_and_generate_proof(blobs[0], 11, cfg)
    assert r == want[0][0] and p.serialize() == want[0][1].serialize()
    assert wide_ctx.commit(blobs[0], B) == want[0][0]
