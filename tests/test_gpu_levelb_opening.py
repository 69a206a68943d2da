"""GPU tests of the Level B openings: frieda_dev_gather / _hashes / _device against numpy indexing and frieda_dev_at*, frieda_merkle_decommit
(both routes, both forms, both tree layouts) against stwo's decommit walk (test_levelb_opening_symbols.stwo_decommit_walk), and the
composition: every layer of a Level A proof rebuilt and opened through Level B calls only, byte for byte."""
import ctypes as C

import numpy as np
import pytest

from test_levelb_opening_symbols import hash_bound, stwo_decommit_walk
from util import DevBuf, blob_len_for, resolve_input

pytestmark = pytest.mark.gpu
P = (1 << 31) - 1
ERR_ARG = 1


def _check(ctx, rc):
    from frieda_amd.api import _check as chk

    chk(rc, ctx._h)


def rand_m31(rng, shape):
    return rng.integers(0, P, shape, dtype=np.uint32)


def _indices(rng, length, n):
    idx = rng.integers(0, length, n, dtype=np.uint64)  # unsorted, repeats
    idx[: min(n, 4)] = [0, length - 1, 0, length - 1][: min(n, 4)]
    return idx


# ---- gather ----
@pytest.mark.parametrize("ncols", [1, 4])
@pytest.mark.parametrize("n", [1, 37, 4096, 1 << 20])
def test_dev_gather_equals_numpy_indexing(gpu_ctx, ncols, n):
    rng = np.random.default_rng(n + ncols)
    length = 1 << 18
    cols = rand_m31(rng, (ncols, length))
    d = DevBuf.from_array(gpu_ctx, cols)
    idx = _indices(rng, length, n)
    got = gpu_ctx.dev_gather(d.ptr, length, ncols, idx)
    assert got.shape == (n, ncols)
    assert np.array_equal(got, cols[:, idx].T)
    L_ = gpu_ctx._L
    for r in list(range(min(n, 4))) + list(rng.integers(0, n, 6)):
        i = int(idx[r])
        if ncols == 1:
            v = C.c_uint32()
            _check(gpu_ctx, L_.frieda_dev_at(gpu_ctx._h, d.ptr, i, C.byref(v)))
            assert got[r, 0] == v.value
        else:
            q = (C.c_uint32 * 4)()
            _check(gpu_ctx, L_.frieda_dev_at_secure(gpu_ctx._h, d.ptr, length, i, q))
            assert list(got[r]) == list(q)


def test_dev_gather_refuses_an_out_of_range_index(gpu_ctx):
    rng = np.random.default_rng(3)
    cols = rand_m31(rng, (4, 1024))
    d = DevBuf.from_array(gpu_ctx, cols)
    L_ = gpu_ctx._L
    for ncols in (1, 4):
        idx = np.array([5, 1023, 1024, 2], dtype=np.uint64)
        out = np.full((4, ncols), 0xABCDEF01, dtype=np.uint32)
        assert L_.frieda_dev_gather(gpu_ctx._h, d.ptr, 1024, ncols, idx.ctypes.data, 4, out.ctypes.data) == ERR_ARG
        assert (out == 0xABCDEF01).all()
    assert L_.frieda_dev_gather(gpu_ctx._h, d.ptr, 1024, 4, None, 0, None) == 0  # n = 0: no-op


def test_dev_gather_hashes_equal_the_stored_layer(gpu_ctx):
    rng = np.random.default_rng(4)
    m = 12
    d_c = DevBuf.from_array(gpu_ctx, rand_m31(rng, (4, 1 << m)))
    d_t, ptrs = _commit_tree(gpu_ctx, d_c, m)
    buf = d_t.to_array(np.uint8, (32 * ((2 << m) - 1),))
    for layer in (m, m - 3, 1, 0):
        off = gpu_ctx._L.frieda_merkle_layer_offset(m, layer)
        idx = _indices(rng, 1 << layer, 300)
        got = gpu_ctx.dev_gather_hashes(ptrs[layer], 1 << layer, idx)
        assert got == b"".join(bytes(buf[off + 32 * int(i) : off + 32 * int(i) + 32]) for i in idx)
    out = np.full(64, 7, dtype=np.uint8)
    bad = np.array([1, 1 << m], dtype=np.uint64)
    assert gpu_ctx._L.frieda_dev_gather_hashes(gpu_ctx._h, ptrs[m], 1 << m, bad.ctypes.data, 2, out.ctypes.data) == ERR_ARG
    assert (out == 7).all()


# ---- decommit ----
def _commit_tree(ctx, d_cols, m):
    d = DevBuf(ctx, 32 * ((2 << m) - 1))
    _check(ctx, ctx._L.frieda_merkle_commit(ctx._h, d_cols.ptr, m, d.ptr))
    return d, [d.ptr.value + ctx._L.frieda_merkle_layer_offset(m, j) for j in range(m + 1)]


def _layer_trees(ctx, d_cols, ncols, stride, m):
    """the same tree shape built layer by layer with frieda_merkle_commit_layer into separate buffers"""
    bufs = [None] * (m + 1)
    cols = (C.c_void_p * ncols)(*[d_cols.ptr.value + 4 * c * stride for c in range(ncols)])
    bufs[m] = DevBuf(ctx, 32 << m)
    _check(ctx, ctx._L.frieda_merkle_commit_layer(ctx._h, m, None, cols, ncols, bufs[m].ptr))
    for j in range(m - 1, -1, -1):
        bufs[j] = DevBuf(ctx, 32 << j)
        _check(ctx, ctx._L.frieda_merkle_commit_layer(ctx._h, j, bufs[j + 1].ptr, None, 0, bufs[j].ptr))
    return bufs, [b.ptr.value for b in bufs]


def _expected_hashes(ctx, ptrs, walk):
    """the walk's (layer, node) list as bytes, read per layer with frieda_dev_gather_hashes (checked against the stored layers above)"""
    if not walk:
        return b""
    walk = np.array(walk, dtype=np.int64)
    out = np.zeros((len(walk), 32), dtype=np.uint8)
    for layer in np.unique(walk[:, 0]):
        sel = np.nonzero(walk[:, 0] == layer)[0]
        got = ctx.dev_gather_hashes(ptrs[layer], 1 << int(layer), walk[sel, 1].astype(np.uint64))
        out[sel] = np.frombuffer(got, dtype=np.uint8).reshape(-1, 32)
    return out.tobytes()


def _positions(kind, m, rng):
    N = 1 << m
    if kind == "single":
        return np.array([int(rng.integers(0, N))], dtype=np.uint32)
    if kind == "all":
        return np.arange(N, dtype=np.uint32)
    if kind == "pairs":
        p = np.unique(rng.integers(0, max(N // 2, 1), 8))
        return np.unique(np.concatenate([2 * p, 2 * p + 1])).astype(np.uint32)[: N]
    if kind == "rand20":
        return np.sort(rng.choice(N, min(N, 20), replace=False)).astype(np.uint32)
    if kind == "rand65536":
        return np.sort(rng.choice(N, min(N, 1 << 16), replace=False)).astype(np.uint32)
    if kind == "ends":
        return np.unique(np.array([0, N - 1], dtype=np.uint32))
    raise ValueError(kind)


def _set_small_max(ctx, v):
    ctx.set_option("FRIEDA_OPEN_SMALL_MAX", v)


@pytest.fixture(scope="module")
def trees(gpu_ctx):
    cache = {}

    def get(m):
        if m not in cache:
            cache.clear()  # one large tree at a time (2^24 leaves: 1 GiB of hashes)
            rng = np.random.default_rng(1000 + m)
            cols = rand_m31(rng, (4, 1 << m))
            d_c = DevBuf.from_array(gpu_ctx, cols)
            d_t, ptrs = _commit_tree(gpu_ctx, d_c, m)
            cache[m] = (cols, d_c, d_t, ptrs)
        return cache[m]

    yield get
    cache.clear()


@pytest.mark.parametrize("m", [0, 1, 5, 12, 20, 24])
@pytest.mark.parametrize("kind", ["single", "all", "pairs", "rand20", "rand65536", "ends"])
def test_merkle_decommit_equals_the_stwo_walk(gpu_ctx, trees, m, kind):
    cols, d_c, d_t, ptrs = trees(m)
    rng = np.random.default_rng(m * 7 + len(kind))
    pos = _positions(kind, m, rng)
    vals, hashes = gpu_ctx.merkle_decommit(ptrs, m, d_c.ptr, 4, 1 << m, pos)
    assert np.array_equal(vals, cols[:, pos].T)
    if kind == "all":
        assert hashes == b""  # every leaf opened: an empty witness
    else:
        assert hashes == _expected_hashes(gpu_ctx, ptrs, stwo_decommit_walk(pos.tolist(), m))
    assert len(hashes) // 32 <= hash_bound(pos.size, m)
    if pos.size <= 512:  # the same list through the multi-block route: identical bytes
        _set_small_max(gpu_ctx, 0)
        try:
            v2, h2 = gpu_ctx.merkle_decommit(ptrs, m, d_c.ptr, 4, 1 << m, pos)
        finally:
            _set_small_max(gpu_ctx, 512)
        assert np.array_equal(v2, vals) and h2 == hashes


@pytest.mark.parametrize("ncols,m", [(1, 10), (3, 13), (4, 11), (3, 0)])
def test_merkle_decommit_of_layer_by_layer_trees(gpu_ctx, ncols, m):
    rng = np.random.default_rng(50 + ncols * m)
    stride = (1 << m) + 64  # columns need not be packed
    cols = rand_m31(rng, (ncols, stride))
    d_c = DevBuf.from_array(gpu_ctx, cols)
    bufs, ptrs = _layer_trees(gpu_ctx, d_c, ncols, stride, m)
    for n in (1, 20, 600, 1 << m):
        pos = np.sort(rng.choice(1 << m, min(n, 1 << m), replace=False)).astype(np.uint32)
        vals, hashes = gpu_ctx.merkle_decommit(ptrs, m, d_c.ptr, ncols, stride, pos)
        assert np.array_equal(vals, cols[:, pos].T)
        assert hashes == _expected_hashes(gpu_ctx, ptrs, stwo_decommit_walk(pos.tolist(), m))
    if ncols == 4:  # the same columns committed in one call: the same bytes
        packed = DevBuf.from_array(gpu_ctx, np.ascontiguousarray(cols[:, : 1 << m]))
        d_t, ptrs2 = _commit_tree(gpu_ctx, packed, m)
        pos = np.sort(rng.choice(1 << m, 37, replace=False)).astype(np.uint32)
        assert gpu_ctx.merkle_decommit(ptrs2, m, packed.ptr, 4, 1 << m, pos)[1] == gpu_ctx.merkle_decommit(ptrs, m, d_c.ptr, 4, stride, pos)[1]


def test_merkle_decommit_refusals(gpu_ctx, trees):
    cols, d_c, d_t, ptrs = trees(12)
    L_ = gpu_ctx._L
    layers = (C.c_void_p * 13)(*ptrs)
    vals = np.zeros((8, 4), dtype=np.uint32)
    hashes = np.full(32 * 200, 9, dtype=np.uint8)
    n = C.c_size_t(12345)

    def call(pos, cap=200, out=hashes):
        pos = np.array(pos, dtype=np.uint32)
        return L_.frieda_merkle_decommit(gpu_ctx._h, layers, 12, d_c.ptr, 4, 1 << 12, pos.ctypes.data, pos.size, vals.ctypes.data,
                                         None if out is None else out.ctypes.data, cap, C.byref(n))

    for bad in ([5, 3], [3, 3], [1, 4096], [0, 1, 2, 5000]):
        assert call(bad) == ERR_ARG
    assert (hashes == 9).all()
    pos = [3, 700, 2000, 4000]
    need = len(stwo_decommit_walk(pos, 12))
    assert call(pos, cap=need - 1) == ERR_ARG and n.value == need
    assert call(pos, cap=0, out=None) == ERR_ARG and n.value == need  # size query
    assert call(pos, cap=need) == 0 and n.value == need
    assert hashes[: 32 * need].tobytes() == _expected_hashes(gpu_ctx, ptrs, stwo_decommit_walk(pos, 12))


def test_async_forms_equal_the_synchronous_ones(gpu_ctx, trees):
    m = 20
    cols, d_c, d_t, ptrs = trees(m)
    L_ = gpu_ctx._L
    rng = np.random.default_rng(77)
    layers = (C.c_void_p * (m + 1))(*ptrs)
    for npos in (1, 20, 512, 513, 5000, 1 << 16):
        pos = np.sort(rng.choice(1 << m, npos, replace=False)).astype(np.uint32)
        vals, hashes = gpu_ctx.merkle_decommit(ptrs, m, d_c.ptr, 4, 1 << m, pos)
        d_pos = DevBuf.from_array(gpu_ctx, pos)
        d_vals, d_h, d_n = DevBuf(gpu_ctx, 16 * npos), DevBuf(gpu_ctx, 32 * npos * m), DevBuf(gpu_ctx, 4)
        _check(gpu_ctx, L_.frieda_merkle_decommit_device(gpu_ctx._h, layers, m, d_c.ptr, 4, 1 << m, d_pos.ptr, npos, d_vals.ptr, d_h.ptr, d_n.ptr))
        cnt = int(d_n.to_array(np.uint32, (1,))[0])
        assert cnt == len(hashes) // 32
        assert np.array_equal(d_vals.to_array(np.uint32, (npos, 4)), vals)
        assert d_h.to_array(np.uint8, (32 * cnt,)).tobytes() == hashes
        idx = _indices(rng, 1 << m, npos)
        d_idx, d_out = DevBuf.from_array(gpu_ctx, idx), DevBuf(gpu_ctx, 16 * npos)
        _check(gpu_ctx, L_.frieda_dev_gather_device(gpu_ctx._h, d_c.ptr, 1 << m, 4, d_idx.ptr, npos, d_out.ptr))
        assert np.array_equal(d_out.to_array(np.uint32, (npos, 4)), gpu_ctx.dev_gather(d_c.ptr, 1 << m, 4, idx))
    # malformed positions on the device: the count word says so and no hash is written
    for npos in (20, 2000):
        pos = np.sort(rng.choice(1 << m, npos, replace=False)).astype(np.uint32)
        pos[npos // 2] = pos[npos // 2 - 1]
        d_pos = DevBuf.from_array(gpu_ctx, pos)
        d_vals, d_h, d_n = DevBuf(gpu_ctx, 16 * npos), DevBuf.from_array(gpu_ctx, np.zeros(32 * npos * m, np.uint8)), DevBuf(gpu_ctx, 4)
        _check(gpu_ctx, L_.frieda_merkle_decommit_device(gpu_ctx._h, layers, m, d_c.ptr, 4, 1 << m, d_pos.ptr, npos, d_vals.ptr, d_h.ptr, d_n.ptr))
        assert int(d_n.to_array(np.uint32, (1,))[0]) == 0xFFFFFFFF
        assert not d_h.to_array(np.uint8, (32 * npos * m,)).any()


# ---- composition: a Level A proof's openings, rebuilt through Level B only ----
COMPOSE_CASES = [
    ("pattern:1024", None, (20, 4, 0, 20)),
    ("pattern:4096", 4096, (20, 4, 1, 20)),
    ("pattern:300", 9, (8, 2, 1, 12)),
    ("pattern:2000", 3, (6, 1, 2, 7)),
    ("pattern:5000", 8, (10, 4, 1, 300)),
    ("pattern:777", None, (6, 5, 2, 64)),
    ("blob", None, (20, 4, 1, 20)),
    ("domain:20", 5, (20, 4, 0, 20)),
    ("domain:22", None, (20, 4, 0, 20)),
    ("domain:24", 11, (20, 4, 0, 20)),
]


def _decommitment_positions(q, li):
    pairs = np.unique(q >> (li + 1))
    return np.unique(np.concatenate([2 * pairs, 2 * pairs + 1])).astype(np.uint32)


@pytest.mark.parametrize("spec,seed,cfg", COMPOSE_CASES, ids=lambda v: str(v)[:24])
def test_level_b_reproduces_a_proofs_openings(gpu_ctx, blob, spec, seed, cfg):
    import frieda_amd

    pow_bits, B, last, nq = cfg
    if spec.startswith("domain:"):
        data = np.frombuffer(resolve_input("pattern:%d" % blob_len_for(int(spec[7:]), B), blob), dtype=np.uint8)
    else:
        data = np.frombuffer(resolve_input(spec, blob), dtype=np.uint8)
    root, proof = gpu_ctx.commit_and_generate_proof(data.tobytes(), seed, frieda_amd.PcsConfig(frieda_amd.FriConfig(B, last, nq), pow_bits))
    alphas = [np.array(a, dtype=np.uint32) for a in gpu_ctx.last_transcript()["alphas"]]
    ok, q = frieda_amd.verify_samples(proof, seed)
    assert ok
    q = np.asarray(q, dtype=np.int64)
    L_ = gpu_ctx._L
    n_felts, npad, lg = C.c_size_t(), C.c_size_t(), C.c_uint32()
    L_.frieda_codec_shape(data.size, C.byref(n_felts), C.byref(npad), C.byref(lg))
    L, n = lg.value, lg.value + B
    n_layers = proof.n_inner_layers + 1
    assert len(alphas) >= n_layers
    # the layers, with Level B calls only
    d_in = DevBuf.from_array(gpu_ctx, data)
    d_coef = DevBuf(gpu_ctx, 4 * npad.value)
    _check(gpu_ctx, L_.frieda_unpack30(gpu_ctx._h, d_in.ptr, data.size, d_coef.ptr, npad.value))
    d_in.free()
    layer = DevBuf(gpu_ctx, 16 << n)
    _check(gpu_ctx, L_.frieda_circle_evaluate(gpu_ctx._h, d_coef.ptr, 4, L, n, layer.ptr))
    d_coef.free()
    for li in range(n_layers):
        m = n - li
        d_t, ptrs = _commit_tree(gpu_ctx, layer, m)
        r = np.zeros(32, dtype=np.uint8)
        _check(gpu_ctx, L_.frieda_dev_download(gpu_ctx._h, r.ctypes.data, C.c_void_p(ptrs[0]), 32))
        root_li = r.tobytes()
        lp = proof.layer(li)
        assert root_li == lp["commitment"], f"layer {li} root"
        if li == 0:
            assert root_li == root
            ev = gpu_ctx.dev_gather(layer.ptr, 1 << m, 4, q.astype(np.uint64))
            assert np.array_equal(ev, proof.evaluations)
        dpos = _decommitment_positions(q, li)
        vals, hashes = gpu_ctx.merkle_decommit(ptrs, m, layer.ptr, 4, 1 << m, dpos)
        assert hashes == b"".join(lp["hash_witness"]), f"layer {li} hash witness"
        queried = set(np.unique(q >> li).tolist())
        wit = np.array([p for p in dpos.tolist() if p not in queried], dtype=np.uint64)
        assert np.array_equal(gpu_ctx.dev_gather(layer.ptr, 1 << m, 4, wit).reshape(-1, 4), lp["fri_witness"]), f"layer {li} fri witness"
        assert np.array_equal(vals[np.isin(dpos, wit)], lp["fri_witness"])
        d_t.free()
        # fold into the next layer
        nxt = DevBuf.from_array(gpu_ctx, np.zeros((4, 1 << (m - 1)), np.uint32))
        a = np.ascontiguousarray(alphas[li])
        if li == 0:
            _check(gpu_ctx, L_.frieda_fold_circle_into_line(gpu_ctx._h, nxt.ptr, layer.ptr, n, a.ctypes.data))
        else:
            _check(gpu_ctx, L_.frieda_fold_line(gpu_ctx._h, layer.ptr, m, n, a.ctypes.data, nxt.ptr))
        layer.free()
        layer = nxt
