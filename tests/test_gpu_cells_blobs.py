"""The cells of a block on the GPU: frieda_open_cells_blobs against the CPU oracle's codewords and trees (one call over blobs encoded
under different options), frieda_verify_cells_blobs_many against the host verifier and the independent check,
frieda_circle_interpolate_points at the column counts a block needs, frieda_reconstruct_blobs_from_opened_stripes end to end.

Shapes are the smallest at which each branch exists: 2^12 trees with and without their two lowest node levels beside a general-route
blob in one call, the fused small route beside the general one at 2^11, log_cell on both sides of the 16-byte copy (2) and of the
one-cell-per-workgroup reduction (10), pair counts off the wave size (65, 300), several verify passes, blob counts that are no power of
two (3, 5) and the 1024-column bound (256 blobs of a 2^5 domain)."""
import ctypes as C

import numpy as np
import pytest

import cells_util as U
import test_cells_blobs_host as H
from cells_util import ACCEPTED, ERR_ARG, POISON, REJECTED
from util import DevBuf

pytestmark = pytest.mark.gpu

GUARD = 64
P = U.P31


def blob_of(length, blowup, seed):
    data, ev, layers, n, L = U.codeword(length, blowup, seed=seed)
    return data, ev, layers


def table(commitments):
    return np.frombuffer(b"".join(commitments), dtype=np.uint8).copy()


# ---- open -------------------------------------------------------------------------------------------------------------------------------
def encode_each(specs):
    """specs: [(blob, options, blowup)] — every blob on a context of its own, with that context's options: [(ctx, enc)]"""
    import frieda_amd

    out = []
    for (data, _, layers), options, blowup in specs:
        ctx = frieda_amd.Context(0)
        for name, value in options.items():
            ctx.set_option(name, value)
        enc = ctx.encode(data, blowup)
        assert enc.commitment == layers[0][0].tobytes()
        out.append((ctx, enc))
    return out


def close_all(pairs):
    for ctx, enc in pairs:
        enc.close()
        ctx.close()


def check_open(ctx, encs, blobs, n, log_cells, counts):
    import frieda_amd

    k = len(blobs)
    for c in log_cells:
        for count in counts:
            if count < k:
                bidx, idx = np.full(count, k - 1, dtype=np.uint32), U.cell_list(n, c, count, seed=count)
            else:
                bidx, idx = H.pair_list(n, c, count, k=k, seed=count)
            values, paths = frieda_amd.open_cells_blobs(ctx, encs, c, bidx, idx)
            want_v, want_p = H.open_pairs(blobs, c, bidx, idx)
            assert values.shape == want_v.shape and paths.shape == want_p.shape
            assert values.tobytes() == want_v.tobytes(), (c, count)
            assert paths.tobytes() == want_p.tobytes(), (c, count, np.flatnonzero((paths != want_p).any(axis=2).any(axis=1)))


def test_open_one_call_over_blobs_encoded_under_different_options(gpu_ctx):
    """skip_log is per blob: a 2^12 tree without its two lowest node levels, one with them, and a general-route blob, in one call"""
    blobs = [blob_of(3000, 4, 501), blob_of(3000, 4, 502), blob_of(24000, 1, 503)]
    n = 12
    assert all(bl[1].shape[1] == 1 << n for bl in blobs)
    options = [{"FRIEDA_TREE_SKIP_LOG": 10, "FRIEDA_TREE_SKIP_LONE_LOG": 10}, {"FRIEDA_TREE_SKIP_LOG": 40, "FRIEDA_TREE_SKIP_LONE_LOG": 40}, {}]
    made = encode_each(list(zip(blobs, options, [4, 4, 1])))
    try:
        encs = [e for _, e in made]
        check_open(gpu_ctx, encs, blobs, n, (0, 1, 2, 3, 6, 10), (1, 65))
        # refused with the outputs untouched: no cells is a no-op; a blob number or a cell out of range; a NULL handle
        L_ = gpu_ctx._L
        handles = (C.c_void_p * 3)(*[e._handle() for e in encs])
        v = np.full((2, 4, 1), 0xA5A5A5A5, dtype=np.uint32)
        p = np.full((2, n, 32), POISON, dtype=np.uint8)
        ok_b, ok_i = np.array([0, 2], dtype=np.uint32), np.array([0, 5], dtype=np.uint32)
        assert L_.frieda_open_cells_blobs(gpu_ctx._h, handles, 3, 0, None, None, 0, None, None) == 0
        for bb, ii, c in ((np.array([0, 3], np.uint32), ok_i, 0), (ok_b, np.array([0, 1 << n], np.uint32), 0), (ok_b, ok_i, n + 1)):
            assert L_.frieda_open_cells_blobs(gpu_ctx._h, handles, 3, c, bb.ctypes.data, ii.ctypes.data, 2, v.ctypes.data, p.ctypes.data) == ERR_ARG
        holed = (C.c_void_p * 3)(encs[0]._handle(), None, encs[2]._handle())
        assert L_.frieda_open_cells_blobs(gpu_ctx._h, holed, 3, 0, ok_b.ctypes.data, ok_i.ctypes.data, 2, v.ctypes.data, p.ctypes.data) == ERR_ARG
        assert L_.frieda_open_cells_blobs(gpu_ctx._h, handles, 0, 0, ok_b.ctypes.data, ok_i.ctypes.data, 2, v.ctypes.data, p.ctypes.data) == ERR_ARG
        assert (v == 0xA5A5A5A5).all() and (p == POISON).all()
    finally:
        close_all(made)


def test_open_fused_and_general_small_route_in_one_call(gpu_ctx):
    blobs = [blob_of(1024, 4, 511), blob_of(1024, 4, 512)]
    n = 11
    made = encode_each(list(zip(blobs, [{}, {"FRIEDA_NO_SMALL_FUSED": 1}], [4, 4])))
    other = blob_of(3000, 4, 501)
    try:
        encs = [e for _, e in made]
        check_open(gpu_ctx, encs, blobs, n, (0, 1, 2, 3, 6, 10), (1, 65))
        # blobs of different log_domain in one call: refused, outputs untouched
        enc12 = gpu_ctx.encode(other[0], 4)
        try:
            handles = (C.c_void_p * 2)(encs[0]._handle(), enc12._handle())
            v = np.full((2, 4, 1), 0xA5A5A5A5, dtype=np.uint32)
            p = np.full((2, 12, 32), POISON, dtype=np.uint8)
            bb, ii = np.array([0, 1], dtype=np.uint32), np.array([0, 1], dtype=np.uint32)
            assert gpu_ctx._L.frieda_open_cells_blobs(gpu_ctx._h, handles, 2, 0, bb.ctypes.data, ii.ctypes.data, 2, v.ctypes.data, p.ctypes.data) == ERR_ARG
            assert b"log_domain" in gpu_ctx._L.frieda_last_error(gpu_ctx._h)
            assert (v == 0xA5A5A5A5).all() and (p == POISON).all()
        finally:
            enc12.close()
    finally:
        close_all(made)


def test_open_beside_a_prove_seeds_job(gpu_ctx):
    """the blobs are only read: another context opens their cells while a prove_seeds job is in flight; the context with the job refuses"""
    import frieda_amd

    blobs = [blob_of(1024, 4, 511), blob_of(1024, 4, 512)]
    cfg = frieda_amd.PcsConfig(frieda_amd.FriConfig(4, 0, 8), 4)
    other = frieda_amd.Context(0)
    encs = [gpu_ctx.encode(bl[0], 4) for bl in blobs]
    try:
        bidx, idx = H.pair_list(11, 3, 17, k=2)
        want_v, want_p = H.open_pairs(blobs, 3, bidx, idx)
        gpu_ctx.prove_seeds_begin(encs[1], [1, 2, 3], cfg)
        try:
            values, paths = frieda_amd.open_cells_blobs(other, encs, 3, bidx, idx)
            with pytest.raises(frieda_amd.FriedaError) as e:
                frieda_amd.open_cells_blobs(gpu_ctx, encs, 3, bidx, idx)
            assert e.value.status == ERR_ARG and "in flight" in str(e.value)
        finally:
            proofs = gpu_ctx.prove_seeds_finish()
        assert values.tobytes() == want_v.tobytes() and paths.tobytes() == want_p.tobytes()
        assert all(frieda_amd.verify(p, s) for p, s in zip(proofs, [1, 2, 3]))
    finally:
        for e in encs:
            e.close()
        other.close()


# ---- verify -----------------------------------------------------------------------------------------------------------------------------
def raw_verify_many(ctx, commitments, n, c, bidx, idx, values, paths, n_blobs=None):
    bidx = np.ascontiguousarray(bidx, dtype=np.uint32)
    idx = np.ascontiguousarray(idx, dtype=np.uint32)
    values = np.ascontiguousarray(values, dtype=np.uint32)
    paths = np.ascontiguousarray(paths, dtype=np.uint8)
    status = np.full(max(1, len(idx)), POISON, dtype=np.uint8)
    com = table(commitments)
    rc = ctx._L.frieda_verify_cells_blobs_many(ctx._h, com.ctypes.data, len(commitments) if n_blobs is None else n_blobs, n, c, bidx.ctypes.data,
                                               idx.ctypes.data, len(idx), values.ctypes.data, paths.ctypes.data if paths.size else None, status.ctypes.data)
    return rc, status[: len(idx)]


def three_way(ctx, coms, n, c, bidx, idx, values, paths, label=None):
    """device == host == independent; returns the status"""
    want = H.independent_pairs(coms, n, c, bidx, idx, values, paths)
    rc, host = H.raw_verify(coms, n, c, bidx, idx, values, paths)
    assert rc == 0, label
    rc, st = raw_verify_many(ctx, coms, n, c, bidx, idx, values, paths)
    assert rc == 0, (label, ctx._L.frieda_last_error(ctx._h))
    assert st.tolist() == host.tolist() == want.tolist(), label
    return want


@pytest.mark.parametrize("n,c", [(n, c) for n in (11, 12) for c in (0, 1, 3, 6)])
def test_verify_blobs_many_on_the_mutation_matrix(gpu_ctx, n, c):
    blobs = H.block(n, 4)
    coms = H.commitments_of(blobs)
    bidx, idx = H.pair_list(n, c, 9)
    values, paths = H.open_pairs(blobs, c, bidx, idx)
    assert three_way(gpu_ctx, coms, n, c, bidx, idx, values, paths, "intact").all()
    for label, t, b2, i2, v2, p2 in H.pair_mutations(n, c, bidx, idx, values, paths):
        want = three_way(gpu_ctx, coms, n, c, b2, i2, v2, p2, label)
        assert np.flatnonzero(want != ACCEPTED).tolist() == [t], label
    # bad arguments leave the status untouched
    bad = bidx.copy()
    bad[-1] = H.K
    rc, st = raw_verify_many(gpu_ctx, coms, n, c, bad, idx, values, paths)
    assert rc == ERR_ARG and (st == POISON).all()
    bad = idx.copy()
    bad[-1] = 1 << (n - c)
    rc, st = raw_verify_many(gpu_ctx, coms, n, c, bidx, bad, values, paths)
    assert rc == ERR_ARG and (st == POISON).all()
    rc, st = raw_verify_many(gpu_ctx, coms, n, c, np.zeros(9, np.uint32), idx, values, paths, n_blobs=0)
    assert rc == ERR_ARG and (st == POISON).all()


def flipped_pairs(n, c, k, count, flips, seed):
    """`count` pairs over k blobs with `flips` single-bit flips, each in another pair: values, paths, in-range index bits and the blob
    number in turn"""
    blobs = H.block(n, 4, k=k)
    rng = np.random.default_rng(seed)
    bidx = rng.integers(0, k, size=count).astype(np.uint32)
    idx = rng.integers(0, 1 << (n - c), size=count).astype(np.uint32)
    values, paths = H.open_pairs(blobs, c, bidx, idx)
    for j, t in enumerate(rng.choice(count, size=flips, replace=False)):
        kind = j % 4
        if kind == 0:
            w = values[t].reshape(-1)
            w[int(rng.integers(0, w.size))] ^= np.uint32(1 << int(rng.integers(0, 32)))
        elif kind == 1:
            p = paths[t].reshape(-1)
            p[int(rng.integers(0, p.size))] ^= np.uint8(1 << int(rng.integers(0, 8)))
        elif kind == 2:
            idx[t] ^= np.uint32(1 << int(rng.integers(0, n - c)))
        else:
            bidx[t] = (int(bidx[t]) + 1 + int(rng.integers(0, k - 1))) % k
    return H.commitments_of(blobs), bidx, idx, values, paths


@pytest.mark.parametrize("pass_bytes", [0, 40000])
def test_verify_blobs_many_on_random_bit_flips(gpu_ctx, pass_bytes):
    """300 pairs over 5 blobs at log_domain 12, log_cell 3, 200 of them with one flipped bit; 40000 bytes per pass: 94 cells, four passes"""
    n, c = 12, 3
    coms, bidx, idx, values, paths = flipped_pairs(n, c, 5, 300, 200, seed=2025)
    want = H.independent_pairs(coms, n, c, bidx, idx, values, paths)
    assert 0 < want.sum() < 300 and 95 <= want.sum() <= 110  # the untouched pairs, and the rare flip that lands on an identical value
    if pass_bytes:
        assert 300 * (8 + (16 << c) + 32 * (n - c)) > 3 * pass_bytes
    assert gpu_ctx._L.frieda_ctx_test_set_verify_pass_bytes(gpu_ctx._h, pass_bytes) == 0
    try:
        got = three_way(gpu_ctx, coms, n, c, bidx, idx, values, paths)
    finally:
        gpu_ctx._L.frieda_ctx_test_set_verify_pass_bytes(gpu_ctx._h, 0)
    assert got.tolist() == want.tolist()


@pytest.mark.parametrize("c", [0, 1, 6, 10])
@pytest.mark.parametrize("count", [1, 65, 300])
def test_verify_blobs_many_pair_counts(gpu_ctx, c, count):
    """The oracle-side accepted count is checked first to lie strictly between 0 and the pair count.  One pair can only give 0 or 1: that
    count runs twice, an untouched pair (accepted) and a flipped one (rejected), so both values are seen."""
    n, k = 12, 5
    runs = [(count + 2) // 3] if count > 1 else [0, 1]
    seen = 0
    for flips in runs:
        coms, bidx, idx, values, paths = flipped_pairs(n, c, k, count, flips, seed=count + c)
        want = H.independent_pairs(coms, n, c, bidx, idx, values, paths)
        if count > 1:
            assert 0 < want.sum() < count
        seen += int(want.sum())
        st = gpu_ctx.verify_cells_blobs_many(coms, n, c, bidx, idx, values, paths)
        rc, host = H.raw_verify(coms, n, c, bidx, idx, values, paths)
        assert rc == 0 and st.tolist() == host.tolist() == want.tolist()
    if count == 1:
        assert seen == 1


# ---- wide columns on the point reconstruction -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,n,m,ncols", [(4, 5, 1, 12), (4, 5, 1, 256), (4, 5, 1, 1024), (7, 11, 3, 20), (7, 11, 0, 20)])
def test_interpolate_points_at_block_column_counts(gpu_ctx, oracle, L, n, m, ncols):
    """frieda_circle_interpolate_points has only run at 1 to 5 columns; a block of K blobs is 4 K.  Random coefficient columns, evaluated
    by frieda_circle_evaluate (checked against the oracle's transform), sampled in cells, interpolated back."""
    rng = np.random.default_rng(12000 + 100 * L + ncols + m)
    coef = rng.integers(0, P, (ncols, 1 << L), dtype=np.uint32)
    d_coef, d_ev = DevBuf.from_array(gpu_ctx, coef), DevBuf(gpu_ctx, 4 * ncols << n)
    assert gpu_ctx._L.frieda_circle_evaluate(gpu_ctx._h, d_coef.ptr, ncols, L, n, d_ev.ptr) == 0
    ev = d_ev.to_array(np.uint32, (ncols, 1 << n))
    assert np.array_equal(ev, oracle.circle_evaluate(coef, n))
    need = (1 << (L - m)) + 1 if m else (1 << L) + 2
    n_cells = need + 2  # two spare cells: they only serve the check against the re-encoded result
    idx = rng.permutation(1 << (n - m))[:n_cells].astype(np.uint32)
    cells = np.ascontiguousarray(np.stack([ev[:, int(c) << m : (int(c) + 1) << m] for c in idx]))  # [cells, ncols, 2^m]
    d_cells, d_c = DevBuf.from_array(gpu_ctx, cells), DevBuf(gpu_ctx, 4 * ncols << L)
    for count in (need, n_cells):
        poison = np.full((ncols, 1 << L), 0xEEEEEEEE, dtype=np.uint32)
        assert gpu_ctx._L.frieda_dev_upload(gpu_ctx._h, d_c.ptr, poison.ctypes.data, poison.nbytes) == 0
        rc = gpu_ctx._L.frieda_circle_interpolate_points(gpu_ctx._h, d_cells.ptr, idx.ctypes.data, count, ncols, m, L, n, d_c.ptr)
        assert rc == 0, gpu_ctx._L.frieda_last_error(gpu_ctx._h)
        got = d_c.to_array(np.uint32, (ncols, 1 << L))
        assert np.array_equal(got, coef), np.flatnonzero((got != coef).any(axis=1))[:8]
    # one corrupted word in the last column of a spare cell is reported
    cells[-1, ncols - 1, 0] = (int(cells[-1, ncols - 1, 0]) + 1) % P
    d_bad = DevBuf.from_array(gpu_ctx, cells)
    assert gpu_ctx._L.frieda_circle_interpolate_points(gpu_ctx._h, d_bad.ptr, idx.ctypes.data, n_cells, ncols, m, L, n, d_c.ptr) == ERR_ARG
    assert b"not values of one polynomial" in gpu_ctx._L.frieda_last_error(gpu_ctx._h)


# ---- stripes ----------------------------------------------------------------------------------------------------------------------------
def raw_stripes(ctx, commitments, blowup, length, c, stripes, values, paths, n_blobs=None):
    """frieda_reconstruct_blobs_from_opened_stripes into poison-filled buffers between red zones: (rc, [bytes] or None, status [S, K], used)"""
    k = len(commitments)
    stripes = np.ascontiguousarray(stripes, dtype=np.uint32)
    values = np.ascontiguousarray(values, dtype=np.uint32)
    paths = np.ascontiguousarray(paths, dtype=np.uint8)
    s = len(stripes)
    buf = np.full(k * length + 2 * GUARD, POISON, dtype=np.uint8)
    status = np.full(s * k + GUARD, POISON, dtype=np.uint8)
    used = C.c_size_t(12345)
    com = table(commitments)
    rc = ctx._L.frieda_reconstruct_blobs_from_opened_stripes(ctx._h, com.ctypes.data, k if n_blobs is None else n_blobs, blowup, length, c,
                                                             stripes.ctypes.data, s, values.ctypes.data, paths.ctypes.data if paths.size else None,
                                                             buf.ctypes.data + GUARD, status.ctypes.data, C.byref(used))
    assert (buf[:GUARD] == POISON).all() and (buf[GUARD + k * length:] == POISON).all(), "red zone around out_bytes"
    assert (status[s * k:] == POISON).all(), "red zone behind out_status"
    body = buf[GUARD:GUARD + k * length]
    if rc != 0:
        assert (body == POISON).all(), "out_bytes written by a failed call"
    out = [body[b * length:(b + 1) * length].tobytes() for b in range(k)] if rc == 0 else None
    return rc, out, status[: s * k].reshape(s, k), used.value


def open_stripes_oracle(blobs, c, stripes):
    """values [S, K, 4, 2^c], paths [S, K, n - c, 32] from the oracle's codewords and trees"""
    per = [U.open_oracle(bl[1], bl[2], c, stripes) for bl in blobs]
    return np.ascontiguousarray(np.stack([v for v, _ in per], axis=1)), np.ascontiguousarray(np.stack([p for _, p in per], axis=1))


STRIPE_CASES = [(11, 4, k, c) for k in (3, 5) for c in (0, 3, 6)] + [(12, 4, 3, 6)] + [(5, 1, k, 1) for k in (64, 256)]


@pytest.mark.parametrize("multi_pass", [False, True])
@pytest.mark.parametrize("n,blowup,k,c", STRIPE_CASES)
def test_reconstruct_blobs_from_opened_stripes(gpu_ctx, n, blowup, k, c, multi_pass):
    blobs = H.block(n, blowup, k=k)
    coms = H.commitments_of(blobs)
    length, L = len(blobs[0][0]), n - blowup
    need = (1 << (L - c)) + 1 if c else (1 << L) + 2
    if (n, k) == (5, 256):
        assert need == 9 and 4 * k == 1024
    rng = np.random.default_rng(400 + n + c + k)
    pick = rng.choice(1 << (n - c), size=need + 1, replace=False).astype(np.uint32)
    values, paths = open_stripes_oracle(blobs, c, pick)
    flat_b, flat_i = np.tile(np.arange(k, dtype=np.uint32), need + 1), np.repeat(pick, k)
    assert H.independent_pairs(coms, n, c, flat_b, flat_i, values.reshape(-1, 4, 1 << c), paths.reshape(-1, n - c, 32)).all()
    idx, v, p = pick[:need], values[:need], paths[:need]
    want_data = [bl[0] for bl in blobs]
    pass_bytes = 0
    if multi_pass:  # a third of the needed stripes per pass: at least three passes, cut at stripe boundaries
        per = max(1, need // 3)
        pass_bytes = per * k * (8 + (16 << c) + 32 * (n - c))
        assert -(-need // per) >= 3
    assert gpu_ctx._L.frieda_ctx_test_set_verify_pass_bytes(gpu_ctx._h, pass_bytes) == 0
    try:
        # exactly the minimum number of distinct stripes
        rc, out, st, used = raw_stripes(gpu_ctx, coms, blowup, length, c, idx, v, p)
        assert rc == 0, gpu_ctx._L.frieda_last_error(gpu_ctx._h)
        assert out == want_data and used == need and (st == ACCEPTED).all()

        # one cell of one blob corrupted: the whole stripe is dropped; too few, one status byte names the cell, the output keeps its poison
        t, b = int(rng.integers(0, need)), int(rng.integers(0, k))
        vbad = values.copy()
        vbad[t, b, 1, 0] ^= 2
        rc, out, st, used = raw_stripes(gpu_ctx, coms, blowup, length, c, idx, vbad[:need], p)
        assert rc == ERR_ARG and used == need - 1
        assert np.argwhere(st != ACCEPTED).tolist() == [[t, b]] and st[t, b] == REJECTED

        # one spare stripe added: enough again, and the damaged stripe is neither counted nor used (the bytes are right)
        rc, out, st, used = raw_stripes(gpu_ctx, coms, blowup, length, c, pick, vbad, paths)
        assert rc == 0 and out == want_data and used == need
        assert np.argwhere(st != ACCEPTED).tolist() == [[t, b]]

        # a repeated stripe does not count twice
        rep = np.concatenate([idx[:-1], idx[:1]])
        rc, out, st, used = raw_stripes(gpu_ctx, coms, blowup, length, c, rep, np.concatenate([v[:-1], v[:1]]), np.concatenate([p[:-1], p[:1]]))
        assert rc == ERR_ARG and used == need - 1 and (st == ACCEPTED).all()

        # a wrong len (same polynomial size; blob 0's last byte is not zero, so its shorter form commits elsewhere): every cell
        # verifies, the commitment check fails and names the blob
        assert want_data[0][-1] != 0
        rc, out, st, used = raw_stripes(gpu_ctx, coms, blowup, length - 1, c, idx, v, p)
        assert rc == ERR_ARG and used == need and (st == ACCEPTED).all()
        err = gpu_ctx._L.frieda_last_error(gpu_ctx._h)
        assert b"commit" in err and b"blob 0" in err

        # one commitment of the block swapped for another blob's: all of that blob's cells are rejected, so no stripe is used
        swapped = list(coms)
        swapped[k - 1] = coms[0]
        rc, out, st, used = raw_stripes(gpu_ctx, swapped, blowup, length, c, idx, v, p)
        assert rc == ERR_ARG and used == 0
        assert (st[:, k - 1] == REJECTED).all() and (st[:, : k - 1] == ACCEPTED).all()
    finally:
        gpu_ctx._L.frieda_ctx_test_set_verify_pass_bytes(gpu_ctx._h, 0)


def test_reconstruct_stripes_argument_errors(gpu_ctx):
    n, blowup, c, k = 11, 4, 3, 3
    blobs = H.block(n, blowup, k=k)
    coms = H.commitments_of(blobs)
    length = len(blobs[0][0])
    idx = np.arange(17, dtype=np.uint32)
    values, paths = open_stripes_oracle(blobs, c, idx)
    # 257 blobs: refused before anything is read (the table passed is that long all the same)
    rc, out, st, used = raw_stripes(gpu_ctx, coms, blowup, length, c, idx, values, paths, n_blobs=0)
    assert rc == ERR_ARG and (st == POISON).all() and used == 0
    many = coms + [coms[0]] * 254
    com = table(many)
    status = np.full(17 * 257, POISON, dtype=np.uint8)
    out = np.full(257 * length, POISON, dtype=np.uint8)
    v257, p257 = np.zeros((17, 257, 4, 1 << c), np.uint32), np.zeros((17, 257, n - c, 32), np.uint8)
    used = C.c_size_t(7)
    rc = gpu_ctx._L.frieda_reconstruct_blobs_from_opened_stripes(gpu_ctx._h, com.ctypes.data, 257, blowup, length, c, idx.ctypes.data, 17, v257.ctypes.data,
                                                                 p257.ctypes.data, out.ctypes.data, status.ctypes.data, C.byref(used))
    assert rc == ERR_ARG and b"n_blobs" in gpu_ctx._L.frieda_last_error(gpu_ctx._h)
    assert (status == POISON).all() and (out == POISON).all()
    # a stripe out of range; no stripes at all is "too few"
    bad = idx.copy()
    bad[3] = 1 << (n - c)
    rc, out, st, used = raw_stripes(gpu_ctx, coms, blowup, length, c, bad, values, paths)
    assert rc == ERR_ARG and (st == POISON).all()
    rc, out, st, used = raw_stripes(gpu_ctx, coms, blowup, length, c, idx[:0], values[:1], paths[:1])
    assert rc == ERR_ARG and used == 0 and b"needed" in gpu_ctx._L.frieda_last_error(gpu_ctx._h)


def test_one_blob_is_the_single_blob_call(gpu_ctx):
    """K = 1: the bytes, statuses and count of frieda_reconstruct_from_opened_cells on the same input (one cell rejected, one spare)"""
    from test_gpu_cells import raw_reconstruct

    n, blowup, c = 11, 4, 3
    data, ev, layers = H.block(n, blowup, k=1)[0]
    root = layers[0][0].tobytes()
    need = (1 << (n - blowup - c)) + 1
    pick = np.random.default_rng(8).choice(1 << (n - c), size=need + 1, replace=False).astype(np.uint32)
    values, paths = U.open_oracle(ev, layers, c, pick)
    values[4, 2, 1] ^= 1
    for count in (need + 1, need):
        rc1, out1, st1, used1 = raw_reconstruct(gpu_ctx, root, blowup, len(data), c, pick[:count], values[:count], paths[:count])
        rc2, out2, st2, used2 = raw_stripes(gpu_ctx, [root], blowup, len(data), c, pick[:count], values[:count, None], paths[:count, None])
        assert (rc1, used1, st1.tolist()) == (rc2, used2, st2[:, 0].tolist())
        assert rc1 == (0 if count == need + 1 else ERR_ARG)
        if rc1 == 0:
            assert out2 == [out1] == [data]


def test_stripes_python_surface(gpu_ctx):
    import frieda_amd

    n, blowup, c, k = 11, 4, 3, 3
    blobs = H.block(n, blowup, k=k)
    coms = H.commitments_of(blobs)
    length = len(blobs[0][0])
    encs = [gpu_ctx.encode(bl[0], blowup) for bl in blobs]
    try:
        stripes = np.random.default_rng(4).permutation(1 << (n - c))[: (1 << (n - blowup - c)) + 1].astype(np.uint32)
        values, paths = frieda_amd.open_stripes(gpu_ctx, encs, c, stripes)
    finally:
        for e in encs:
            e.close()
    assert values.shape == (len(stripes), k, 4, 1 << c) and paths.shape == (len(stripes), k, n - c, 32)
    want_v, want_p = open_stripes_oracle(blobs, c, stripes)
    assert values.tobytes() == want_v.tobytes() and paths.tobytes() == want_p.tobytes()
    out, st, used = gpu_ctx.reconstruct_blobs_from_opened_stripes(coms, blowup, length, c, stripes, values, paths)
    assert out == [bl[0] for bl in blobs] and used == len(stripes) and st.shape == (len(stripes), k) and (st == ACCEPTED).all()
    with pytest.raises(frieda_amd.FriedaError) as e:
        gpu_ctx.reconstruct_blobs_from_opened_stripes(coms, blowup, length, c, stripes[:-1], values[:-1], paths[:-1])
    assert e.value.status == ERR_ARG and e.value.n_stripes_used == len(stripes) - 1
    assert e.value.cell_status.shape == (len(stripes) - 1, k) and (e.value.cell_status == ACCEPTED).all()
