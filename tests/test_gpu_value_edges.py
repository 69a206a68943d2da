"""GPU: the field kernels on value-edge inputs (tests/edge_values.py), through the C ABI against the oracle — bit-exact, and every
output word canonical (< P: a P where 0 is meant is the classic miss of a lazily reduced butterfly).

The kernels here carry their own arithmetic instead of field.h's checked primitives (ntt.hip radix16_group, the mirrored inverse passes
and the three-product accumulators of intt.hip, the fused fold of tree.hip, polyops.hip's 64-bit partial sums, erasure.hip's line
products, the 30-bit codec).  Uniform words meet a sum that lands on P or a difference of exactly 0 once in ~2^31 operations; the
families meet them in every butterfly.  tests/test_edge_values_host.py checks the oracle itself against Python integers on the same
inputs.  Shapes are the smallest that reach each kernel (dispatch: ntt.hip evaluate_plan, intt.hip circle_interpolate_block, tree.hip
encode_and_first_tree and build_tree).  Two kernels are reached only from Level A and only in launches a lone 2^16 proof does not make:
ntt_last_tree_kernel (a batch of 16 blobs) and tree5rs_fold_circle_kernel (prove_seeds under FRIEDA_SEEDS_FOLD_GROUP); their tests
assert the kernel's name in the context's timing report, so they cannot pass without running it.

Beyond the issue's lists: the coefficient family onehot_first_pmax (a codeword that is P - 1 everywhere) is added to the scattered
reconstruction cases — with single-point cells it fills cells_combine_kernel's accumulators with (P - 1) * v products, which the named
families do not."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import edge_values as EV
from edge_values import ALPHAS, BLOBS, EVAL_POINTS, FAMILIES, FOLD_INPUTS, P, SPARSE_TARGETS
from util import DevBuf, blob_len_for

pytestmark = pytest.mark.gpu

ALL = list(FAMILIES)
REDUCED = ["pmax", "alt", "edge_rich"]  # the family list of the shapes at 2^20 and above
ACCEPTED, REJECTED = 1, 0


def _check(ctx, rc):
    from frieda_amd.api import _check as chk

    chk(rc, ctx._h)


def assert_same(got, exp, what=None):
    assert int(got.max(initial=0)) < P, f"non-canonical word in the output: {what}"
    assert np.array_equal(got, exp), what


def _oracle_cols(fn, n_items):
    """oracle work per column on a few host threads (the C oracle releases the GIL)"""
    with ThreadPoolExecutor(max_workers=6) as ex:
        return list(ex.map(fn, range(n_items)))


_CACHE = {}


def cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
        if isinstance(_CACHE[key], np.ndarray):
            _CACHE[key].setflags(write=False)
    return _CACHE[key]


def oracle_evaluate(oracle, coef, n):
    tw = cached(("tw", n), lambda: oracle.precompute_twiddles(n))[0]
    if n < 16:
        return oracle.circle_evaluate(coef, n, tw)
    return np.concatenate(_oracle_cols(lambda c: oracle.circle_evaluate(coef[c : c + 1], n, tw), coef.shape[0]))


def oracle_interpolate(oracle, block, n, k):
    itw = cached(("tw", n), lambda: oracle.precompute_twiddles(n))[1]
    if block.shape[1] < (1 << 16):
        return oracle.circle_interpolate_block(block, n, k, itw)
    return np.concatenate(_oracle_cols(lambda c: oracle.circle_interpolate_block(block[c : c + 1], n, k, itw), block.shape[0]))


def codeword(oracle, family, ncols, L, n):
    """(coefficients, the oracle's evaluation of them): computed once per (family, shape)"""
    coef = cached(("coef", family, ncols, L), lambda: FAMILIES[family]((ncols, 1 << L), seed=L))
    return coef, cached(("ev", family, ncols, L, n), lambda: oracle_evaluate(oracle, coef, n))


def gpu_evaluate(ctx, coef, L, n, offset=0):
    """frieda_circle_evaluate with both buffers `offset` bytes past their allocation"""
    ncols = coef.shape[0]
    d_c, d_o = DevBuf(ctx, coef.nbytes + offset), DevBuf(ctx, (4 * ncols << n) + offset)
    pc, po = C.c_void_p(d_c.ptr.value + offset), C.c_void_p(d_o.ptr.value + offset)
    c = np.ascontiguousarray(coef)
    _check(ctx, ctx._L.frieda_dev_upload(ctx._h, pc, c.ctypes.data, c.nbytes))
    _check(ctx, ctx._L.frieda_circle_evaluate(ctx._h, pc, ncols, L, n, po))
    out = np.zeros((ncols, 1 << n), dtype=np.uint32)
    _check(ctx, ctx._L.frieda_dev_download(ctx._h, out.ctypes.data, po, out.nbytes))
    d_c.free(), d_o.free()
    return out


# ------------------------------------------------------------------------------------------------
# a. forward transform
# ------------------------------------------------------------------------------------------------
# (0,4): ntt_broadcast; (3,3), (5,9): ntt_tile_kernel; (12,12), (12,16): ntt_tile12_kernel<3,0>; (16,16), (16,18): + <1,8>
FWD_SMALL = [(0, 4), (3, 3), (5, 9), (12, 12), (12, 16), (16, 16), (16, 18)]


@pytest.mark.parametrize("L,n", FWD_SMALL, ids=lambda v: str(v))
@pytest.mark.parametrize("family", ALL)
def test_evaluate(gpu_ctx, oracle, family, L, n):
    coef, exp = codeword(oracle, family, 4, L, n)
    assert_same(gpu_evaluate(gpu_ctx, coef, L, n), exp)


@pytest.mark.parametrize("L,n", FWD_SMALL, ids=lambda v: str(v))
def test_evaluate_one_column(gpu_ctx, oracle, L, n):
    coef, exp = codeword(oracle, "edge_rich", 1, L, n)
    assert_same(gpu_evaluate(gpu_ctx, coef, L, n), exp)


@pytest.mark.parametrize("family", REDUCED)
def test_evaluate_2p20_strided_eight_layer_pass(gpu_ctx, oracle, family):
    """(20,20), 2 columns: ntt_tile12_kernel<2,4> over layers 19 .. 12, then <3,0>"""
    coef, exp = codeword(oracle, family, 2, 20, 20)
    assert_same(gpu_evaluate(gpu_ctx, coef, 20, 20), exp)


@pytest.mark.parametrize("family", REDUCED)
def test_evaluate_2p21_replicated_source_pass(oracle, family):
    """(20,21), 2 columns, FRIEDA_NTT_REP = 1: ntt_tile12_rep_kernel reads the coefficient vector for both high blocks"""
    import frieda_amd

    coef, exp = codeword(oracle, family, 2, 20, 21)
    ctx = frieda_amd.Context(0)
    try:
        ctx.set_option("FRIEDA_NTT_REP", 1)
        assert_same(gpu_evaluate(ctx, coef, 20, 21), exp)
    finally:
        ctx.close()


@pytest.mark.parametrize("family", ALL)
def test_evaluate_generic_kernel_at_a_tile12_size(gpu_ctx, oracle, family):
    """(12,13) with both pointers 4 bytes past a 16-byte boundary: ntt_tile_kernel runs all 12 layers"""
    coef, exp = codeword(oracle, family, 4, 12, 13)
    assert_same(gpu_evaluate(gpu_ctx, coef, 12, 13, offset=4), exp)


@pytest.mark.parametrize("n", [5, 12, 16])
@pytest.mark.parametrize("target", SPARSE_TARGETS)
def test_evaluate_onto_a_sparse_target(gpu_ctx, oracle, target, n):
    """coefficients = interpolate(E) for an evaluation vector E that is mostly 0: every zero of E is a last-layer butterfly whose
    v + t is exactly P or whose v - t is exactly 0"""
    E = FAMILIES[target]((4, 1 << n))
    coef = cached(("sparse", target, n), lambda: oracle_interpolate(oracle, E, n, 0))
    assert_same(gpu_evaluate(gpu_ctx, coef, n, n), E)


# ------------------------------------------------------------------------------------------------
# b. inverse transform
# ------------------------------------------------------------------------------------------------
def gpu_interpolate(ctx, block, L, n, k):
    ncols = block.shape[0]
    d_b, d_c = DevBuf.from_array(ctx, block), DevBuf(ctx, 4 * ncols << L)
    _check(ctx, ctx._L.frieda_circle_interpolate(ctx._h, d_b.ptr, ncols, L, n, k, d_c.ptr))
    out = d_c.to_array(np.uint32, (ncols, 1 << L))
    d_b.free(), d_c.free()
    return out


def check_interpolate(ctx, oracle, family, L, n, k, ncols):
    # the block of a codeword whose coefficients are the family: the coefficients come back (zeros at the scaled last pass's output)
    coef, ev = codeword(oracle, family, ncols, L, n)
    block = np.ascontiguousarray(ev[:, k << L : (k + 1) << L])
    assert_same(gpu_interpolate(ctx, block, L, n, k), coef, "codeword block")
    # the family as the block itself: the operation is defined for any words
    exp = cached(("interp", family, ncols, L, n, k), lambda: oracle_interpolate(oracle, coef, n, k))
    assert_same(gpu_interpolate(ctx, coef, L, n, k), exp, "family-valued block")


# (3,5), (5,5): intt_tile_kernel; (12,12), (12,14): intt_tile12_kernel<3,0> with the scale; (13,13): + one generic layer;
# (16,18): + <1,8>; (20,20): + <2,4>
INV_SHAPES = [(3, 5, 0), (5, 5, 0), (12, 12, 0), (12, 14, 3), (13, 13, 0), (16, 18, 0)]


@pytest.mark.parametrize("L,n,k", INV_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("family", ALL)
def test_interpolate(gpu_ctx, oracle, family, L, n, k):
    check_interpolate(gpu_ctx, oracle, family, L, n, k, 4)


@pytest.mark.parametrize("family", REDUCED + ["zeros"])
def test_interpolate_2p20(gpu_ctx, oracle, family):
    check_interpolate(gpu_ctx, oracle, family, 20, 20, 0, 2)


@pytest.mark.parametrize("L,n,k", [(12, 14, 3), (16, 18, 0)], ids=lambda v: str(v))
def test_interpolate_generic_passes(oracle, L, n, k):
    """FRIEDA_INTT_GENERIC = 1: intt_tile_kernel for every layer of a shape the fast passes would take"""
    import frieda_amd

    ctx = frieda_amd.Context(0)
    try:
        ctx.set_option("FRIEDA_INTT_GENERIC", 1)
        for family in ALL:
            check_interpolate(ctx, oracle, family, L, n, k, 4)
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------
# c. folds
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 6, 12, 16])
@pytest.mark.parametrize("family", FOLD_INPUTS)
def test_fold_circle_into_line(gpu_ctx, oracle, family, n):
    half = (4, 1 << (n - 1))
    src = FOLD_INPUTS[family]((4, 1 << n), seed=n)
    d_s = DevBuf.from_array(gpu_ctx, src)
    for an in ALPHAS:
        alpha = EV.alpha_array(an)
        for dst0 in (EV.zeros(half), EV.pmax(half), EV.edge_rich(half, n)):  # pmax: dst * alpha^2 at its largest
            exp = oracle.fold_circle_into_line(src, alpha, dst0.copy())
            d_d = DevBuf.from_array(gpu_ctx, dst0)
            _check(gpu_ctx, gpu_ctx._L.frieda_fold_circle_into_line(gpu_ctx._h, d_d.ptr, d_s.ptr, n, alpha.ctypes.data))
            assert_same(d_d.to_array(np.uint32, half), exp, (an, int(dst0[0, 0])))
            d_d.free()
    d_s.free()


@pytest.mark.parametrize("n,m", [(2, 1), (6, 5), (6, 1), (12, 11), (16, 9)], ids=lambda v: str(v))
@pytest.mark.parametrize("family", FOLD_INPUTS)
def test_fold_line(gpu_ctx, oracle, family, n, m):
    src = FOLD_INPUTS[family]((4, 1 << m), seed=m)
    d_s, d_d = DevBuf.from_array(gpu_ctx, src), DevBuf(gpu_ctx, 16 << (m - 1))
    for an in ALPHAS:
        alpha = EV.alpha_array(an)
        exp = oracle.fold_line(src, n, alpha)
        _check(gpu_ctx, gpu_ctx._L.frieda_fold_line(gpu_ctx._h, d_s.ptr, m, n, alpha.ctypes.data, d_d.ptr))
        assert_same(d_d.to_array(np.uint32, (4, 1 << (m - 1))), exp, an)
    d_s.free(), d_d.free()


@pytest.mark.parametrize("no_cp", [0, 1])
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("L,n", [(12, 14), (14, 14)], ids=lambda v: str(v))
@pytest.mark.parametrize("family", ["zeros", "pmax", "edge_rich"])
def test_evaluate_fold2(oracle, family, L, n, accumulate, no_cp):
    """the one-pass form (ntt_last_fold_cp_kernel side by side, ntt_last_fold_kernel with FRIEDA_NTT_NO_CP = 1) against the oracle's
    three operations, for every pair (alpha0, alpha1) of ALPHAS; with `accumulate` line 1 starts from edge-rich contents"""
    import frieda_amd

    coef, ev = codeword(oracle, family, 4, L, n)
    start = cached(("fold2 start", n), lambda: EV.edge_rich((4, 1 << (n - 1)), 77))
    ctx = frieda_amd.Context(0)
    try:
        ctx.set_option("FRIEDA_NTT_NO_CP", no_cp)
        d_c, d_e = DevBuf.from_array(ctx, coef), DevBuf(ctx, 16 << n)
        d_1, d_2 = DevBuf(ctx, 16 << (n - 1)), DevBuf(ctx, 16 << (n - 2))
        for a0n in ALPHAS:
            a0 = EV.alpha_array(a0n)
            l1 = cached(("fold2 l1", family, L, n, accumulate, a0n),
                        lambda: oracle.fold_circle_into_line(ev, a0, start.copy() if accumulate else None))
            for a1n in ALPHAS:
                a1 = EV.alpha_array(a1n)
                l2 = cached(("fold2 l2", family, L, n, accumulate, a0n, a1n), lambda: oracle.fold_line(l1, n, a1))
                _check(ctx, ctx._L.frieda_dev_upload(ctx._h, d_1.ptr, start.ctypes.data, start.nbytes))
                _check(ctx, ctx._L.frieda_circle_evaluate_fold2(ctx._h, d_c.ptr, L, n, d_e.ptr, a0.ctypes.data, accumulate, d_1.ptr,
                                                               a1.ctypes.data, d_2.ptr))
                assert_same(d_1.to_array(np.uint32, (4, 1 << (n - 1))), l1, ("line 1", a0n, a1n))
                assert_same(d_2.to_array(np.uint32, (4, 1 << (n - 2))), l2, ("line 2", a0n, a1n))
            assert_same(d_e.to_array(np.uint32, (4, 1 << n)), ev, ("evaluation", a0n))
        d_c.free(), d_e.free(), d_1.free(), d_2.free()
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------
# d. fri_decompose
# ------------------------------------------------------------------------------------------------
DECOMPOSE = [(s, f) for s in (1, 5, 12, 13, 17) for f in ("pmax", "halves", "halves_swapped", "alt", "zeros")]
DECOMPOSE += [(22, f) for f in ("pmax", "halves", "halves_swapped")]  # 2^21 words of P - 1 per partial-sum chain: the 64-bit sums' largest values


@pytest.mark.parametrize("log_size,family", DECOMPOSE, ids=lambda v: str(v))
def test_fri_decompose(gpu_ctx, oracle, log_size, family):
    size = 1 << log_size
    ev = FAMILIES[family]((4, size))
    d_e, d_g = DevBuf.from_array(gpu_ctx, ev), DevBuf(gpu_ctx, 16 << log_size)
    lam = np.full(4, 0xFFFFFFFF, dtype=np.uint32)
    _check(gpu_ctx, gpu_ctx._L.frieda_fri_decompose(gpu_ctx._h, d_e.ptr, log_size, d_g.ptr, lam.ctypes.data))
    g = d_g.to_array(np.uint32, (4, size))
    d_e.free(), d_g.free()
    og, olam = oracle.fri_decompose(ev)
    assert_same(lam, olam, "lambda")
    assert_same(g, og, "g")
    # closed forms, in Python integers: lambda = (sum of the first half - sum of the second half) / size
    half_sum = (size // 2) * (P - 1)
    want = {"pmax": 0, "zeros": 0, "halves": -half_sum, "halves_swapped": half_sum}.get(family)
    if want is not None:
        want = want * pow(size % P, P - 2, P) % P
        assert lam.tolist() == [want] * 4
        if family in ("halves", "halves_swapped"):  # g = ev -+ lambda is one constant
            assert want == {"halves": (P + 1) // 2, "halves_swapped": (P - 1) // 2}[family]
            assert np.all(g == (P - want) % P if family == "halves" else g == want)
        else:
            assert np.array_equal(g, ev)


# ------------------------------------------------------------------------------------------------
# e. eval_at_point
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncols,log_coef", [(4, 2), (3, 5), (4, 9), (4, 12), (4, 13), (1, 17)], ids=lambda v: str(v))
@pytest.mark.parametrize("family", ["pmax", "alt", "onehot_last_pmax", "onehot_middle_1", "edge_rich"])
def test_eval_at_point(gpu_ctx, oracle, family, ncols, log_coef):
    coef = FAMILIES[family]((ncols, 1 << log_coef), seed=log_coef)
    d = DevBuf.from_array(gpu_ctx, coef)
    for name, (px, py) in EVAL_POINTS.items():
        px, py = np.array(px, dtype=np.uint32), np.array(py, dtype=np.uint32)
        out = np.full((ncols, 4), 0xFFFFFFFF, dtype=np.uint32)
        _check(gpu_ctx, gpu_ctx._L.frieda_circle_eval_at_point(gpu_ctx._h, d.ptr, ncols, log_coef, px.ctypes.data, py.ctypes.data, out.ctypes.data))
        exp = np.stack([oracle.circle_eval_at_point(coef[c], px, py) for c in range(ncols)])
        assert_same(out, exp, name)
    d.free()


# ------------------------------------------------------------------------------------------------
# f. scattered reconstruction
# ------------------------------------------------------------------------------------------------
SCATTER_FAMILIES = ["pmax", "alt", "edge_rich", "zeros", "onehot_first_pmax"]  # the last: every sample is P - 1 (module docstring)


def sample_cells(oracle, family, L, n, m, n_cells, seed):
    coef, ev = codeword(oracle, family, 4, L, n)
    idx = np.random.default_rng(seed).permutation(1 << (n - m))[:n_cells].astype(np.uint32)
    cells = np.ascontiguousarray(np.stack([ev[:, int(c) << m : (int(c) + 1) << m] for c in idx]))  # [R, 4, 2^m]
    return coef, cells, idx


# (6,10,0): 64 single points; (8,12,2): 64 cells of 4 — the host inverts the cell matrix, cells_combine_kernel combines;
# (10,14,1): 512 cells — the device's blocked elimination, then cells_combine_kernel over 512 products per word
@pytest.mark.parametrize("L,n,m", [(6, 10, 0), (8, 12, 2), (10, 14, 1)], ids=lambda v: str(v))
@pytest.mark.parametrize("family", SCATTER_FAMILIES)
def test_interpolate_cells_dense_solve(gpu_ctx, oracle, family, L, n, m):
    R = 1 << (L - m)
    coef, cells, idx = sample_cells(oracle, family, L, n, m, R, 1000 + L)
    if L <= 8:  # these positions determine the polynomial (the oracle's solve refuses a singular set), and its solve agrees
        assert np.array_equal(oracle.reconstruct_cells(cells[:, :1], idx, n, L), coef[:1])
    d_cells, d_c = DevBuf.from_array(gpu_ctx, cells), DevBuf.from_array(gpu_ctx, np.full((4, 1 << L), 0xEEEEEEEE, dtype=np.uint32))
    _check(gpu_ctx, gpu_ctx._L.frieda_circle_interpolate_cells(gpu_ctx._h, d_cells.ptr, idx.ctypes.data, R, 4, m, L, n, d_c.ptr))
    assert_same(d_c.to_array(np.uint32, (4, 1 << L)), coef)
    d_cells.free(), d_c.free()


@pytest.mark.parametrize("L,n,m", [(5, 9, 1), (8, 12, 0)], ids=lambda v: str(v))
@pytest.mark.parametrize("family", SCATTER_FAMILIES)
def test_interpolate_cells_any(gpu_ctx, oracle, family, L, n, m):
    R = 1 << (L - m)
    coef, cells, idx = sample_cells(oracle, family, L, n, m, R + 4, 2000 + L)
    d_cells, d_c = DevBuf.from_array(gpu_ctx, cells), DevBuf.from_array(gpu_ctx, np.full((4, 1 << L), 0xEEEEEEEE, dtype=np.uint32))
    used = (C.c_uint32 * R)()
    _check(gpu_ctx, gpu_ctx._L.frieda_circle_interpolate_cells_any(gpu_ctx._h, d_cells.ptr, idx.ctypes.data, R + 4, 4, m, L, n, d_c.ptr, used))
    assert_same(d_c.to_array(np.uint32, (4, 1 << L)), coef)
    d_cells.free(), d_c.free()
    u = list(used)
    assert len(set(int(idx[k]) for k in u)) == R
    assert np.array_equal(oracle.reconstruct_cells(cells[u][:, :1], idx[u], n, L), coef[:1])


@pytest.mark.parametrize("L,n,extra", [(6, 10, 40), (10, 14, 2)], ids=lambda v: str(v))
@pytest.mark.parametrize("family", SCATTER_FAMILIES)
def test_interpolate_points_both_routes(oracle, family, L, n, extra):
    """single sampled points through the line-by-line locator and through the product tree (FRIEDA_ERASURE_TREE_MIN_LOG); the all-zero
    codeword is consistent with the zero polynomial and must not be reported as inconsistent"""
    import frieda_amd

    n_pts = (1 << L) + extra
    coef, cells, idx = sample_cells(oracle, family, L, n, 0, n_pts, 3000 + L)
    if n <= 10:
        assert np.array_equal(oracle.reconstruct_points(np.ascontiguousarray(cells[:, :, 0]), idx, n, L), coef)
    ctx = frieda_amd.Context(0)
    try:
        d_cells, d_c = DevBuf.from_array(ctx, cells), DevBuf(ctx, 16 << L)
        for route, min_log in (("lines", 32), ("tree", 6)):
            ctx.set_option("FRIEDA_ERASURE_TREE_MIN_LOG", min_log)
            poison = np.full((4, 1 << L), 0xEEEEEEEE, dtype=np.uint32)
            _check(ctx, ctx._L.frieda_dev_upload(ctx._h, d_c.ptr, poison.ctypes.data, poison.nbytes))
            rc = ctx._L.frieda_circle_interpolate_points(ctx._h, d_cells.ptr, idx.ctypes.data, n_pts, 4, 0, L, n, d_c.ptr)
            assert rc == 0, (route, ctx._L.frieda_last_error(ctx._h))
            assert_same(d_c.to_array(np.uint32, (4, 1 << L)), coef, route)
        d_cells.free(), d_c.free()
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------
# g. codec
# ------------------------------------------------------------------------------------------------
UNPACK_LENGTHS = [0, 1, 3, 4, 14, 15, 16, 29, 30, 31, 58, 60, 61, 119, 1000, 1024, 4097, 65536, 262146]  # test_unpack30's (1, 4, 15 among them)


@pytest.mark.parametrize("blob", BLOBS)
def test_unpack30(gpu_ctx, oracle, blob):
    for n_bytes in UNPACK_LENGTHS:
        data = np.frombuffer(BLOBS[blob](n_bytes), dtype=np.uint8)
        coef, _ = oracle.polynomial_from_bytes(data)
        d_in = DevBuf.from_array(gpu_ctx, data if n_bytes else np.zeros(4, np.uint8))
        d_out = DevBuf.from_array(gpu_ctx, np.full(coef.size, 0xEEEEEEEE, dtype=np.uint32))
        _check(gpu_ctx, gpu_ctx._L.frieda_unpack30(gpu_ctx._h, d_in.ptr, n_bytes, d_out.ptr, coef.size))
        assert_same(d_out.to_array(np.uint32, (coef.size,)), coef.ravel(), n_bytes)
        d_in.free(), d_out.free()


PACK_FELTS = {"pmax": lambda n: EV.pmax(n), "edge_rich": lambda n: EV.edge_rich(n, 9), "2p30": lambda n: np.full(n, 2**30, dtype=np.uint32)}


@pytest.mark.parametrize("felts", PACK_FELTS)
def test_pack30_keeps_the_low_30_bits(gpu_ctx, oracle, felts):
    """felts with bit 30 set: the oracle's packer keeps bits 0 .. 29 (pack30_kernel's 0x3fffffff mask), byte for byte, also where the
    last byte holds part of a felt"""
    f = PACK_FELTS[felts](4096)
    d_f = DevBuf.from_array(gpu_ctx, f)
    for n_bytes in (15360, 15359, 4097, 1001, 15, 7, 4, 1):
        d_o = DevBuf.from_array(gpu_ctx, np.full(n_bytes + 8, 0xEE, dtype=np.uint8))
        _check(gpu_ctx, gpu_ctx._L.frieda_pack30(gpu_ctx._h, d_f.ptr, f.size, d_o.ptr, n_bytes))
        assert d_o.to_array(np.uint8, (n_bytes,)).tobytes() == oracle.felts_to_bytes(f, n_bytes), n_bytes
        d_o.free()
    d_f.free()


# ------------------------------------------------------------------------------------------------
# h. whole proofs
# ------------------------------------------------------------------------------------------------
def _cfg(nq, blowup, last, pow_bits):
    import frieda_amd

    return frieda_amd.PcsConfig(frieda_amd.FriConfig(blowup, last, nq), pow_bits)


# 1 KiB: the fused small-domain first launch; 30 000 B at blowup 2^2, last-layer bound 2: nine inner layers; blob_len_for(16): a lone
# 2^16 proof is ntt_tile12<1,8>, <3,0>, a separate leaf launch and the nine-level fold + tree kernel, whose fold is field.h's
# qm_fold_pair.  It does NOT reach ntt_last_tree_kernel (encode_and_first_tree, tree.hip: the fusion needs 256 tiles in the launch, a
# lone 2^16 blob has 16, and proofs take it only under FRIEDA_ENCODE_TREE_FUSION_PROVE) nor tree5rs_fold_circle_kernel, the fold copy
# with the unreduced f0 (build_tree: prove_seeds with FRIEDA_SEEDS_FOLD_GROUP > 0 and a register-subtree launch, level A + log2(seeds)
# >= 18).  The three tests below the first reach those two at this blob length.
PROOF_SHAPES = {"1KiB": (1024, (4, 4, 0, 20)), "30000B": (30000, (4, 2, 2, 8)), "2p16": (blob_len_for(16), (4, 4, 0, 20))}  # (pow, blowup, last, nq)
SEED = 5


def oracle_proof(oracle, blob, shape, seed=SEED):
    """(root, serialised proof) of the oracle, computed once per (blob, shape, seed)"""
    n_bytes, (pow_bits, blowup, last, nq) = PROOF_SHAPES[shape]

    def run():
        root, proof = oracle.commit_and_generate_proof(BLOBS[blob](n_bytes), seed, oracle.make_config(pow_bits, blowup, last, nq))
        assert oracle.verify(proof, seed)
        return root, proof.serialize()

    return cached(("proof", blob, shape, seed), run)


def kernels_of(ctx, fn):
    """fn()'s result and the names of the kernel launches it made (the context's per-kernel timing report)"""
    ctx.set_kernel_timing(True)
    try:
        out = fn()
        names = {k["name"] for k in ctx.kernel_timing_report()}
    finally:
        ctx.set_kernel_timing(False)
    return out, names


def _bump_evaluation(proof):
    """the same proof with its second evaluation word incremented.  Wire image, in 32-bit words: head 2, config 4,
    L 1, nonce 2, the count of evaluations at word 9, their words from 10 on"""
    import frieda_amd

    w = np.frombuffer(proof.serialize(), dtype="<u4").copy()
    assert w[9] >= 1
    w[11] = (int(w[11]) + 1) % P
    return frieda_amd.Proof.deserialize(w.tobytes())


@pytest.mark.parametrize("shape", PROOF_SHAPES)
@pytest.mark.parametrize("blob", BLOBS)
def test_commit_prove_verify(gpu_ctx, oracle, blob, shape):
    import frieda_amd

    n_bytes, (pow_bits, blowup, last, nq) = PROOF_SHAPES[shape]
    data = BLOBS[blob](n_bytes)
    o_root, o_image = oracle_proof(oracle, blob, shape)
    assert gpu_ctx.commit(data, blowup) == oracle.commit(data, blowup) == o_root
    proofs = []
    for host_channel in (False, True):
        gpu_ctx.set_host_channel(host_channel)
        try:
            g_root, g_proof = gpu_ctx.commit_and_generate_proof(data, SEED, _cfg(nq, blowup, last, pow_bits))
        finally:
            gpu_ctx.set_host_channel(False)
        assert g_root == o_root and g_proof.serialize() == o_image, f"host_channel={host_channel}"
        proofs.append(g_proof)
    assert frieda_amd.verify(proofs[0], SEED)
    bad = _bump_evaluation(proofs[0])
    assert bad.serialize() != proofs[0].serialize() and not frieda_amd.verify(bad, SEED)
    assert list(gpu_ctx.verify_many([proofs[0], bad, proofs[1]], [SEED] * 3)) == [ACCEPTED, REJECTED, ACCEPTED]


def test_commit_batch_2p16_fused_encode_and_tree(gpu_ctx, oracle):
    """16 blobs of blob_len_for(16), four of each of BLOBS, committed in one launch: 16 tiles each, 256 in all, the smallest launch
    whose last transform pass is ntt_last_tree_kernel (radix16_group, leaf hashing and six node levels in one kernel; nothing kept)"""
    kinds = list(BLOBS) * 4
    roots, names = kernels_of(gpu_ctx, lambda: gpu_ctx.commit_batch([BLOBS[k](blob_len_for(16)) for k in kinds], 4))
    assert "ntt_last_tree7" in names, names
    assert roots == [oracle_proof(oracle, k, "2p16")[0] for k in kinds]


def test_prove_batch_2p16_fused_encode_and_tree(oracle):
    """the same 16 blobs proved in one call with FRIEDA_ENCODE_TREE_FUSION_PROVE = 1: ntt_last_tree_kernel in its every-level-kept
    form, which also writes the evaluation the folds and the openings read"""
    import frieda_amd

    kinds = list(BLOBS) * 4
    ctx = frieda_amd.Context(0)
    try:
        ctx.set_option("FRIEDA_ENCODE_TREE_FUSION_PROVE", 1)
        blobs = [BLOBS[k](blob_len_for(16)) for k in kinds]
        got, names = kernels_of(ctx, lambda: ctx.commit_and_generate_proof_batch(blobs, [SEED] * 16, _cfg(20, 4, 0, 4)))
    finally:
        ctx.close()
    assert "ntt_last_tree7" in names, names
    for i, (k, (root, proof)) in enumerate(zip(kinds, got)):
        assert (root, proof.serialize()) == oracle_proof(oracle, k, "2p16"), (i, k)


@pytest.mark.parametrize("blob", BLOBS)
def test_prove_seeds_2p16_seed_looped_fold(gpu_ctx, oracle, blob):
    """blob_len_for(16) under 8 seeds with FRIEDA_SEEDS_FOLD_GROUP set: level A of the first fold is 2^15 nodes, 15 + log2(8) = 18, the
    smallest register-subtree launch, so the fold is tree5rs_fold_circle_kernel — its own copy of qm_fold_pair with f0 = x + y kept
    unreduced and x + (P - y) reduced with the twiddle product.  Groups of 3 (does not divide 8: a short last group) and 8.  Directed
    pair coverage here is what the blobs give: on the all-zero blob every pair is x == y == 0, so f0 = 0 and x + (P - y) is exactly P."""
    import frieda_amd

    data = BLOBS[blob](blob_len_for(16))
    cfg = _cfg(20, 4, 0, 4)
    seeds = list(range(SEED, SEED + 8))
    want = [gpu_ctx.commit_and_generate_proof(data, s, cfg)[1].serialize() for s in seeds]
    assert want[0] == oracle_proof(oracle, blob, "2p16")[1]
    assert want[7] == oracle_proof(oracle, blob, "2p16", seeds[7])[1]
    ctx = frieda_amd.Context(0)
    try:
        enc = ctx.encode(data, 4)
        try:
            assert enc.commitment == oracle_proof(oracle, blob, "2p16")[0]
            for group in (3, 8):
                ctx.set_option("FRIEDA_SEEDS_FOLD_GROUP", group)
                got, names = kernels_of(ctx, lambda: ctx.prove_seeds(enc, seeds, cfg))
                assert "tree5s_fold_circle" in names, names
                assert [p.serialize() for p in got] == want, f"group {group}"
        finally:
            enc.close()
    finally:
        ctx.close()


@pytest.mark.parametrize("blob", BLOBS)
def test_1kib_seeds_and_reconstruction(gpu_ctx, oracle, blob):
    """one 1 KiB blob under many seeds: prove_seeds equals separate proofs, and the pooled verified samples (the all-zero blob: every
    value 0, many equal leaves) rebuild the blob — equal values are neither duplicates nor conflicts"""
    data = BLOBS[blob](1024)
    cfg = _cfg(20, 4, 0, 4)
    seeds = list(range(1, 17))
    root, proofs = gpu_ctx.commit_and_generate_proofs_for_seeds(data, seeds, cfg)
    assert root == oracle.commit(data, 4) and len(proofs) == 16
    for s, p in zip(seeds[:8], proofs[:8]):
        r1, p1 = gpu_ctx.commit_and_generate_proof(data, s, cfg)
        assert r1 == root and p1.serialize() == p.serialize(), s
    assert oracle_proof(oracle, blob, "1KiB", seeds[0])[1] == proofs[0].serialize()
    assert list(gpu_ctx.verify_many(proofs, seeds, expected_commitment=root)) == [ACCEPTED] * 16
    out, st, n_points = gpu_ctx.reconstruct_from_proofs(proofs, seeds, root, len(data))  # 2^7 coefficients per column: 130 points needed
    assert out == data and set(st) == {ACCEPTED} and n_points >= 130
    out, st, n_pairs = gpu_ctx.reconstruct_from_proof_pairs(proofs[:8], seeds[:8], root, len(data))
    assert out == data and set(st) == {ACCEPTED} and n_pairs >= 130
