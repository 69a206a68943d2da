"""GPU: the four frieda_rebuild_encoded_* calls — each its reconstruct twin plus handles.  On the same arguments the new call must give
the twin's return code, status bytes, n_used and bytes, and its handles must be indistinguishable from frieda_encode of the original
bytes (encoded_util.facts).  The provider's side of every case is the library's own openers over lone frieda_encode handles; the
image-rule cases are built from the CPU oracle (arbitrary coefficient columns -> circle_evaluate -> merkle_commit)."""
import ctypes as C
import os

import numpy as np
import pytest

import cells_util as U
from frieda_amd.api import codec_log_size
import encoded_util as E
import workspace_rows as W
from cells_util import ACCEPTED, ERR_ARG, POISON, REJECTED
from conftest import GOLDEN, splitmix64_bytes

pytestmark = pytest.mark.gpu

# (L, log_blowup_factor, log_cell, blob bytes, FRIEDA_ERASURE_TREE_MIN_LOG or None): the smallest shape the point route takes; cells of 1, 8
# and 64 entries; the fixture by cells and by single points (the product-tree route at the default threshold); a small shape sent down the
# product-tree route by the lowered threshold
SHAPES = [
    (1, 1, 0, 16, None),
    (7, 4, 0, 1024, None),
    (7, 4, 3, 1024, None),
    (11, 4, 6, 20000, None),
    (11, 5, 1, 20000, None),
    (15, 4, 6, "blob", None),
    (15, 4, 0, "blob", None),
    (7, 4, 0, 1024, 6),
]
IDS = ["L%d-B%d-c%d%s" % (s[0], s[1], s[2], "-tree" if s[4] else "") for s in SHAPES]


def blobs_of(length, count):
    if length == "blob":
        with open(os.path.join(GOLDEN, "blob"), "rb") as f:
            base = np.frombuffer(f.read(), dtype=np.uint8)
        return [np.roll(base, 131 * b).tobytes() for b in range(count)]
    return [splitmix64_bytes(8000 + 17 * b + length, length).tobytes() for b in range(count)]


def need_of(L, c):
    return (1 << (L - c)) + 1 if c else (1 << L) + 2


def offers(L, n, c, seed):
    """[(label, distinct indices, repeats)]: exactly the needed number, and need + 37 with repeats (as many spare distinct cells as the
    domain has, up to 30, then 7 repeats)"""
    need, total = need_of(L, c), 1 << (n - c)
    rng = np.random.default_rng(seed)
    perm = rng.permutation(total).astype(np.uint32)
    spare = min(30, total - need)
    return [("exact", perm[:need], perm[:0]), ("plus37", perm[: need + spare], perm[: 37 - spare])]


def chunks(idx, size=1000):
    s = np.sort(idx)
    cut = max(1, min(size, (len(s) + 2) // 3))  # at least three bundles where there are three cells
    return [s[i : i + cut] for i in range(0, len(s), cut)]


def offer_bundles(distinct, reps, need):
    """the offer as bundles: the needed cells in three chunks, then the spare cells as a bundle of their own, then the repeats as one.
    -> (bundles, number of the first bundle the rebuild can do without, or None)"""
    base = chunks(distinct[:need])
    extra = [np.sort(x) for x in (distinct[need:], reps) if len(x)]
    return base + extra, (len(base) if extra else None)


def reject_bundle(bundles, b, values, witness, wfirst, k=1, blob=0):
    """copies of (values, witness) with bundle b's piece of `blob` damaged: one bit of its witness where it has one, else one word of its
    first cell (values [cells, 4, 2^c] for k = 1, [stripes, k, 4, 2^c] for a block; the witness laid out as the openers return it)"""
    v, w = values.copy(), witness.copy()
    W = int(wfirst[b + 1]) - int(wfirst[b])
    if W:
        w[k * int(wfirst[b]) + blob * W + W // 2, 5] ^= 0x10
    else:
        first = sum(len(x) for x in bundles[:b])
        if k == 1:
            v[first, 2, 0] ^= 1
        else:
            v[first, blob, 2, 0] ^= 1
    return v, w


class Ctx:
    """the context of a case: the shared one, with the erasure threshold lowered for the case that asks for it"""

    def __init__(self, gpu_ctx, min_log):
        self.ctx, self.min_log = gpu_ctx, min_log

    def __enter__(self):
        if self.min_log:
            self.ctx.set_option("FRIEDA_ERASURE_TREE_MIN_LOG", self.min_log)
        return self.ctx

    def __exit__(self, *a):
        if self.min_log:
            self.ctx.set_option("FRIEDA_ERASURE_TREE_MIN_LOG", 15)  # the default, for the tests that follow on this context


def compare(ctx, twin, new, args, datas, blowup, want_rc=0, prove=True):
    """twin(*args) against new(*args): return code, status bytes, n_used and bytes equal; on FRIEDA_OK the handles equal H0 of `datas`"""
    t = E.call(twin, *args)
    g = E.call(new, *args)
    try:
        assert g[0] == t[0] == want_rc, (g[0], t[0], ctx._L.frieda_last_error(ctx._h))
        assert g[2].tobytes() == t[2].tobytes() and g[3] == t[3]
        assert g[1] == t[1]
        if want_rc == 0:
            assert (g[1] if isinstance(g[1], list) else [g[1]]) == list(datas)
            assert len(g[4]) == len(datas)
            for b, e in enumerate(g[4]):
                E.assert_same(E.facts(ctx, e, prove), E.facts_of_bytes(ctx, datas[b], blowup, prove), "blob %d" % b)
        else:
            assert g[4] is None
        return g
    finally:
        E.close_all(g[4])


@pytest.mark.parametrize("L,blowup,c,length,min_log", SHAPES, ids=IDS)
def test_rebuild_from_cells_and_cell_bundles(gpu_ctx, L, blowup, c, length, min_log):
    data = blobs_of(length, 1)[0]
    n = L + blowup
    need = need_of(L, c)
    with Ctx(gpu_ctx, min_log) as ctx:
        enc = ctx.encode(data, blowup)
        try:
            assert enc.shape == (L, n)
            root = enc.commitment
            for label, distinct, reps in offers(L, n, c, 40 + n + c):
                idx = np.concatenate([distinct, reps])
                values, paths = enc.open_cells(ctx, c, idx)
                compare(ctx, ctx.reconstruct_from_opened_cells, ctx.rebuild_encoded_from_opened_cells, (root, blowup, len(data), c, idx, values, paths), [data], blowup)
                bundles, spare_b = offer_bundles(distinct, reps, need)
                bv, bw, bwf = enc.open_cell_bundles(ctx, c, bundles)
                bargs = (root, blowup, len(data), c, bundles, bv, bw, bwf)
                compare(ctx, ctx.reconstruct_from_cell_bundles, ctx.rebuild_encoded_from_cell_bundles, bargs, [data], blowup)
                if label == "plus37":
                    # a whole rejected bundle beside enough accepted ones: the twin's statuses and count, a good handle
                    vb, wb = reject_bundle(bundles, spare_b, bv, bw, bwf)
                    g = compare(ctx, ctx.reconstruct_from_cell_bundles, ctx.rebuild_encoded_from_cell_bundles, (root, blowup, len(data), c, bundles, vb, wb, bwf), [data],
                                blowup)
                    assert np.flatnonzero(g[2] != ACCEPTED).tolist() == [spare_b] and g[2][spare_b] == REJECTED and g[3] == need
                    continue
                # --- from here on: the exact offer, damaged ---
                # one corrupted cell: too few remain; the twin's statuses, no handle
                t = need // 2
                vbad = values.copy()
                vbad[t, 1, 0] ^= 2
                g = compare(ctx, ctx.reconstruct_from_opened_cells, ctx.rebuild_encoded_from_opened_cells, (root, blowup, len(data), c, idx, vbad, paths), [data], blowup,
                            want_rc=ERR_ARG)
                assert np.flatnonzero(g[2] != ACCEPTED).tolist() == [t] and g[3] == need - 1
                # a whole rejected bundle: too few remain
                wbad = bw.copy()
                if len(wbad):
                    wbad[0, 0] ^= 1
                    g = compare(ctx, ctx.reconstruct_from_cell_bundles, ctx.rebuild_encoded_from_cell_bundles, (root, blowup, len(data), c, bundles, bv, wbad, bwf), [data],
                                blowup, want_rc=ERR_ARG)
                    assert g[2][0] == REJECTED and (g[2][1:] == ACCEPTED).all()
                # out_bytes = NULL still gives the handle
                r = ctx.rebuild_encoded_from_opened_cells(root, blowup, len(data), c, idx, values, paths, want_bytes=False)
                try:
                    assert r[0] is None and r[2] == need and (r[1] == ACCEPTED).all()
                    E.assert_same(E.facts(ctx, r[3]), E.facts_of_bytes(ctx, data, blowup))
                finally:
                    r[3].close()
                # a wrong len inside the same L, both ways: whatever the twin answers (a shorter blob does not commit; a longer one commits
                # to the zero-extended bytes only when the padding agrees)
                for other in (len(data) - 1, len(data) + 1):
                    if codec_log_size(other) != L:
                        continue
                    t_ = E.call(ctx.reconstruct_from_opened_cells, root, blowup, other, c, idx, values, paths)
                    g_ = E.call(ctx.rebuild_encoded_from_opened_cells, root, blowup, other, c, idx, values, paths)
                    try:
                        assert g_[0] == t_[0] and g_[1] == t_[1] and g_[2].tobytes() == t_[2].tobytes() and g_[3] == t_[3], other
                        if g_[0] == 0:
                            # the handle of the (zero-extended) rebuilt bytes
                            E.assert_same(E.facts(ctx, g_[4][0], False), E.facts_of_bytes(ctx, g_[1], blowup, False))
                        else:
                            assert b"commit" in ctx._L.frieda_last_error(ctx._h)
                    finally:
                        E.close_all(g_[4])
            # enough cells remain beside a corrupted one: a good handle
            label, distinct, reps = offers(L, n, c, 40 + n + c)[1]
            if len(distinct) > need:
                values, paths = enc.open_cells(ctx, c, distinct)
                values[0, 2, 0] ^= 1
                g = compare(ctx, ctx.reconstruct_from_opened_cells, ctx.rebuild_encoded_from_opened_cells, (root, blowup, len(data), c, distinct, values, paths), [data],
                            blowup)
                assert g[2][0] == REJECTED and g[3] == len(distinct) - 1
        finally:
            enc.close()


BLOCKS = [(s, 3) for s in SHAPES] + [((7, 4, 3, 1024, None), 16), ((7, 4, 0, 1024, None), 16)]


@pytest.mark.parametrize("shape,k", BLOCKS, ids=["%s-K%d" % (IDS[SHAPES.index(s)], k) for s, k in BLOCKS])
def test_rebuild_blocks_from_stripes_and_stripe_bundles(gpu_ctx, shape, k):
    import frieda_amd

    L, blowup, c, length, min_log = shape
    datas = blobs_of(length, k)
    n = L + blowup
    need = need_of(L, c)
    prove = k <= 3
    with Ctx(gpu_ctx, min_log) as ctx:
        encs = [ctx.encode(d, blowup) for d in datas]
        try:
            coms = [e.commitment for e in encs]
            for label, distinct, reps in offers(L, n, c, 70 + n + c + k):
                idx = np.concatenate([distinct, reps])
                values, paths = frieda_amd.open_stripes(ctx, encs, c, idx)
                sargs = (coms, blowup, len(datas[0]), c, idx, values, paths)
                compare(ctx, ctx.reconstruct_blobs_from_opened_stripes, ctx.rebuild_encoded_blobs_from_opened_stripes, sargs, datas, blowup, prove=prove)
                bundles, spare_b = offer_bundles(distinct, reps, need)
                bv, bw, bwf = frieda_amd.open_stripe_bundles(ctx, encs, c, bundles)
                bargs = (coms, blowup, len(datas[0]), c, bundles, bv, bw, bwf)
                compare(ctx, ctx.reconstruct_blobs_from_stripe_bundles, ctx.rebuild_encoded_blobs_from_stripe_bundles, bargs, datas, blowup, prove=prove)
                if label == "plus37":
                    # a stripe with one blob's cell corrupted is not used: enough remain where the offer had spares
                    if len(distinct) > need:
                        vbad = values.copy()
                        vbad[1, k - 1, 0, 0] ^= 4
                        g = compare(ctx, ctx.reconstruct_blobs_from_opened_stripes, ctx.rebuild_encoded_blobs_from_opened_stripes,
                                    (coms, blowup, len(datas[0]), c, idx, vbad, paths), datas, blowup, prove=False)
                        assert g[2][1, k - 1] == REJECTED and (g[2][1, : k - 1] == ACCEPTED).all()
                    # a stripe bundle with one blob's piece rejected is not used (the statuses are ANDed per bundle before pooling); enough
                    # stripes remain in the others: the twin's statuses and count, good handles
                    vb, wb = reject_bundle(bundles, spare_b, bv, bw, bwf, k=k, blob=k - 1)
                    g = compare(ctx, ctx.reconstruct_blobs_from_stripe_bundles, ctx.rebuild_encoded_blobs_from_stripe_bundles,
                                (coms, blowup, len(datas[0]), c, bundles, vb, wb, bwf), datas, blowup, prove=False)
                    assert np.argwhere(g[2] != ACCEPTED).tolist() == [[spare_b, k - 1]] and g[2][spare_b, k - 1] == REJECTED and g[3] == need
                    continue
                vbad = values.copy()
                vbad[need // 2, k // 2, 3, 0] ^= 1
                g = compare(ctx, ctx.reconstruct_blobs_from_opened_stripes, ctx.rebuild_encoded_blobs_from_opened_stripes,
                            (coms, blowup, len(datas[0]), c, idx, vbad, paths), datas, blowup, want_rc=ERR_ARG)
                assert g[3] == need - 1 and (g[2] != ACCEPTED).sum() == 1
                if len(bw):
                    wbad = bw.copy()
                    wbad[len(wbad) - 1, 31] ^= 0x80  # the last blob's piece of the last bundle
                    g = compare(ctx, ctx.reconstruct_blobs_from_stripe_bundles, ctx.rebuild_encoded_blobs_from_stripe_bundles,
                                (coms, blowup, len(datas[0]), c, bundles, bv, wbad, bwf), datas, blowup, want_rc=ERR_ARG)
                    assert (g[2] == REJECTED).sum() == 1
                r = ctx.rebuild_encoded_blobs_from_stripe_bundles(coms, blowup, len(datas[0]), c, bundles, bv, bw, bwf, want_bytes=False)
                try:
                    assert r[0] is None and r[2] == need
                    for b in (0, k - 1):
                        E.assert_same(E.facts(ctx, r[3][b], False), E.facts_of_bytes(ctx, datas[b], blowup, False))
                finally:
                    E.close_all(r[3])
                # commitments swapped: the twin's answer, and its words
                if k >= 2:
                    swapped = [coms[1], coms[0]] + coms[2:]
                    t_ = E.call(ctx.reconstruct_blobs_from_opened_stripes, swapped, blowup, len(datas[0]), c, idx, values, paths)
                    twin_err = ctx._L.frieda_last_error(ctx._h)
                    g_ = E.call(ctx.rebuild_encoded_blobs_from_opened_stripes, swapped, blowup, len(datas[0]), c, idx, values, paths)
                    assert g_[0] == t_[0] == ERR_ARG and g_[4] is None and g_[2].tobytes() == t_[2].tobytes()
                    assert ctx._L.frieda_last_error(ctx._h) == twin_err
        finally:
            E.close_all(encs)


# ---- raw calls: what the Python wrappers hide (NULL handles, untouched out_bytes) ----
def raw_cells(ctx, root, blowup, length, c, idx, values, paths):
    buf = np.full(length + 64, POISON, dtype=np.uint8)
    status = np.zeros(len(idx), dtype=np.uint8)
    used = C.c_size_t(0)
    enc = C.c_void_p(0xDEAD0)
    idx = np.ascontiguousarray(idx, dtype=np.uint32)
    rc = ctx._L.frieda_rebuild_encoded_from_opened_cells(ctx._h, (C.c_uint8 * 32)(*root), blowup, length, c, idx.ctypes.data, len(idx), values.ctypes.data,
                                                         paths.ctypes.data, buf.ctypes.data, status.ctypes.data, C.byref(used), C.byref(enc))
    return rc, buf, status, used.value, enc.value


def raw_stripes(ctx, coms, blowup, length, c, idx, values, paths):
    k = len(coms)
    buf = np.full(length * k + 64, POISON, dtype=np.uint8)
    status = np.zeros(len(idx) * k, dtype=np.uint8)
    used = C.c_size_t(0)
    encs = (C.c_void_p * k)(*([0xDEAD0] * k))
    idx = np.ascontiguousarray(idx, dtype=np.uint32)
    com = np.frombuffer(b"".join(coms), dtype=np.uint8).copy()
    rc = ctx._L.frieda_rebuild_encoded_blobs_from_opened_stripes(ctx._h, com.ctypes.data, k, blowup, length, c, idx.ctypes.data, len(idx), values.ctypes.data,
                                                                 paths.ctypes.data, buf.ctypes.data, status.ctypes.data, C.byref(used), encs)
    return rc, buf, status, used.value, [e for e in encs]


def test_errors_give_null_handles_and_leave_out_bytes_untouched(gpu_ctx):
    import frieda_amd

    L, blowup, c, k = 7, 4, 3, 3
    n, need = L + blowup, need_of(7, 3)
    datas = blobs_of(1024, k)
    encs = [gpu_ctx.encode(d, blowup) for d in datas]
    try:
        coms = [e.commitment for e in encs]
        idx = np.random.default_rng(5).permutation(1 << (n - c))[:need].astype(np.uint32)
        v1, p1 = encs[0].open_cells(gpu_ctx, c, idx)
        vs, ps = frieda_amd.open_stripes(gpu_ctx, encs, c, idx)
        # too few cells / stripes
        rc, buf, st, used, enc = raw_cells(gpu_ctx, coms[0], blowup, 1024, c, idx[:-1], v1[:-1], p1[:-1])
        assert rc == ERR_ARG and enc is None and (buf == POISON).all() and used == need - 1 and (st == ACCEPTED).all()
        rc, buf, st, used, es = raw_stripes(gpu_ctx, coms, blowup, 1024, c, idx[:-1], vs[:-1], ps[:-1])
        assert rc == ERR_ARG and es == [None] * k and (buf == POISON).all() and used == need - 1
        # a wrong len: does not commit
        rc, buf, st, used, enc = raw_cells(gpu_ctx, coms[0], blowup, 1023, c, idx, v1, p1)
        assert rc == ERR_ARG and enc is None and (buf == POISON).all() and used == need
        # argument errors: n_blobs out of range, a NULL handle array
        rc = gpu_ctx._L.frieda_rebuild_encoded_from_opened_cells(gpu_ctx._h, (C.c_uint8 * 32)(*coms[0]), blowup, 1024, c, idx.ctypes.data, need, v1.ctypes.data,
                                                                 p1.ctypes.data, None, None, None, None)
        assert rc == ERR_ARG
        # a proof in flight
        ctx = frieda_amd.Context(0)
        try:
            ctx.prove_begin(datas[0], 1, E.pcs(blowup))
            rc, buf, st, used, enc = raw_cells(ctx, coms[0], blowup, 1024, c, idx, v1, p1)
            assert rc == ERR_ARG and enc is None and (buf == POISON).all()
            ctx.prove_finish()
        finally:
            ctx.close()
        # and the good call through the same wrapper: the bytes, the red zone behind them, a handle
        rc, buf, st, used, enc = raw_cells(gpu_ctx, coms[0], blowup, 1024, c, idx, v1, p1)
        assert rc == 0 and enc and buf[:1024].tobytes() == datas[0] and (buf[1024:] == POISON).all()
        gpu_ctx._L.frieda_encoded_free(C.c_void_p(enc))
    finally:
        E.close_all(encs)


# ---- the image rule end to end ----
def mutated_columns(oracle, data, L):
    """[(label, coefficient columns [4, 2^L])]: the blob's polynomial with ONE word moved into each forbidden region"""
    coef, L_ = oracle.polynomial_from_bytes(data)
    assert L_ == L
    coef = np.asarray(coef, dtype=np.uint32).reshape(4, 1 << L)
    K = 1 << L
    F = (8 * len(data) + 29) // 30
    last_bits = 8 * len(data) - 30 * (F - 1)
    assert F < 4 * K and last_bits < 30 and (coef.reshape(-1)[F:] == 0).all()
    out = []
    for label, k, v in [("word 3 = 2^30 + 5", 3, (1 << 30) + 5), ("a bit above the blob's last", F - 1, int(coef.reshape(-1)[F - 1]) | (1 << last_bits)),
                        ("first padding word = 1", F, 1), ("last word of column 3 = 7", 4 * K - 1, 7)]:
        m = coef.copy()
        m[k // K, k % K] = v
        out.append((label, m))
    return out


def test_a_committed_polynomial_that_is_no_blob_image_is_refused(gpu_ctx, oracle):
    """A committer publishes the root of a polynomial that is no blob's image.  Its cells verify; commit(pack30(coef)) is another root, so
    the twins answer FRIEDA_ERR_ARG — and so must the calls that compare the root of evaluate(coef) instead: that root IS the commitment."""
    L, blowup, c, k = 7, 4, 3, 3
    n, need = L + blowup, need_of(7, 3)
    datas = blobs_of(1024, k)
    honest = []
    for d in datas:
        coef, _ = oracle.polynomial_from_bytes(d)
        ev = oracle.circle_evaluate(np.asarray(coef, dtype=np.uint32).reshape(4, 1 << L), n)
        honest.append((ev, oracle.merkle_commit(ev)))
    idx = np.random.default_rng(9).permutation(1 << (n - c))[: need + 3].astype(np.uint32)
    # the honest block first: the oracle's cells rebuild, with handles (the construction of this test is sound)
    cells = [U.open_oracle(ev, layers, c, idx) for ev, layers in honest]
    coms = [layers[0][0].tobytes() for _, layers in honest]
    sv = np.ascontiguousarray(np.stack([v for v, _ in cells], axis=1))
    sp = np.ascontiguousarray(np.stack([p for _, p in cells], axis=1))
    g = E.call(gpu_ctx.rebuild_encoded_blobs_from_opened_stripes, coms, blowup, 1024, c, idx, sv, sp)
    assert g[0] == 0 and g[1] == datas
    E.close_all(g[4])
    for label, cols in mutated_columns(oracle, datas[1], L):
        ev = oracle.circle_evaluate(cols, n)
        layers = oracle.merkle_commit(ev)
        root = layers[0][0].tobytes()
        values, paths = U.open_oracle(ev, layers, c, idx)
        assert U.independent_status(root, n, c, idx, values, paths).all(), label
        args = (root, blowup, 1024, c, idx, values, paths)
        t = E.call(gpu_ctx.reconstruct_from_opened_cells, *args)
        assert t[0] == ERR_ARG and (t[2] == ACCEPTED).all() and t[3] == len(idx), label
        g = E.call(gpu_ctx.rebuild_encoded_from_opened_cells, *args)
        assert g[0] == ERR_ARG and g[4] is None and (g[2] == ACCEPTED).all() and g[3] == len(idx), label
        assert b"does not commit" in gpu_ctx._L.frieda_last_error(gpu_ctx._h), label
        # in a block: blob 1 of three is the bad one
        bsv, bsp, bcoms = sv.copy(), sp.copy(), list(coms)
        bsv[:, 1], bsp[:, 1], bcoms[1] = values, paths, root
        t = E.call(gpu_ctx.reconstruct_blobs_from_opened_stripes, bcoms, blowup, 1024, c, idx, bsv, bsp)
        assert t[0] == ERR_ARG and (t[2] == ACCEPTED).all(), label
        g = E.call(gpu_ctx.rebuild_encoded_blobs_from_opened_stripes, bcoms, blowup, 1024, c, idx, bsv, bsp)
        assert g[0] == ERR_ARG and g[4] is None and (g[2] == ACCEPTED).all() and g[3] == t[3], label
        assert b"blob 1 does not commit" in gpu_ctx._L.frieda_last_error(gpu_ctx._h), label


@pytest.mark.parametrize("word", [0x00000000, 0xFFFFFFFF, 0x7FFFFFFF])
def test_same_outputs_on_a_sticky_poisoned_context(gpu_ctx, word):
    import frieda_amd

    L, blowup, c, k = 7, 4, 3, 3
    n, need = L + blowup, need_of(7, 3)
    datas = blobs_of(1024, k)
    ctx = frieda_amd.Context(0)
    try:
        W.poison(ctx, word)
        encs = [ctx.encode(d, blowup) for d in datas]
        try:
            coms = [e.commitment for e in encs]
            idx = np.random.default_rng(word & 0xFF).permutation(1 << (n - c))[: need + 2].astype(np.uint32)
            v1, p1 = encs[0].open_cells(ctx, c, idx)
            compare(ctx, ctx.reconstruct_from_opened_cells, ctx.rebuild_encoded_from_opened_cells, (coms[0], blowup, 1024, c, idx, v1, p1), datas[:1], blowup)
            vs, ps = frieda_amd.open_stripes(ctx, encs, c, idx)
            compare(ctx, ctx.reconstruct_blobs_from_opened_stripes, ctx.rebuild_encoded_blobs_from_opened_stripes, (coms, blowup, 1024, c, idx, vs, ps), datas, blowup)
            # (the reference facts above come from this poisoned context's lone encodes; against an unpoisoned context as well)
            g = E.call(ctx.rebuild_encoded_blobs_from_opened_stripes, coms, blowup, 1024, c, idx, vs, ps)
            try:
                for b in range(k):
                    E.assert_same(E.facts(gpu_ctx, g[4][b]), E.facts(gpu_ctx, encs[b]))
            finally:
                E.close_all(g[4])
        finally:
            E.close_all(encs)
    finally:
        ctx.close()


def test_handles_outlive_the_workspace_and_the_context(gpu_ctx):
    """the documented lifetime of frieda_encoded: a handle from a rebuild works after release_workspace() and after the context that built
    it is closed, opening through a second context"""
    import frieda_amd

    L, blowup, c, k = 7, 4, 3, 3
    n, need = L + blowup, need_of(7, 3)
    datas = blobs_of(1024, k)
    ctx = frieda_amd.Context(0)
    try:
        encs = [ctx.encode(d, blowup) for d in datas]
        coms = [e.commitment for e in encs]
        idx = np.random.default_rng(3).permutation(1 << (n - c))[:need].astype(np.uint32)
        vs, ps = frieda_amd.open_stripes(ctx, encs, c, idx)
        E.close_all(encs)
        _, _, used, made = ctx.rebuild_encoded_blobs_from_opened_stripes(coms, blowup, 1024, c, idx, vs, ps)
        v1, p1 = made[0].open_cells(ctx, c, idx)
        _, _, _, one = ctx.rebuild_encoded_from_opened_cells(coms[0], blowup, 1024, c, idx, v1, p1, want_bytes=False)
        ctx.release_workspace()
        for b in range(k):
            E.assert_same(E.facts(ctx, made[b]), E.facts_of_bytes(gpu_ctx, datas[b], blowup))
    finally:
        ctx.close()
    try:
        made[1].close()  # one of the block goes first; the others keep the allocation
        for b in (0, 2):
            E.assert_same(E.facts(gpu_ctx, made[b]), E.facts_of_bytes(gpu_ctx, datas[b], blowup))
        E.assert_same(E.facts(gpu_ctx, one), E.facts_of_bytes(gpu_ctx, datas[0], blowup))
    finally:
        E.close_all(made + [one])
