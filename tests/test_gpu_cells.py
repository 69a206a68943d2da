"""Authenticated cells on the GPU: frieda_open_cells against the CPU oracle's codeword and tree for every layout frieda_encode can leave,
frieda_verify_cells_many against the host verifier and the independent check, frieda_reconstruct_from_opened_cells end to end.

Shapes are the smallest at which each branch exists: the one-leaf-pair domain, the fused small-domain route and the general route at
2^11, a 2^12 tree with and without its two lowest node levels, log_cell on both sides of the 16-byte copy (2) and of the
one-cell-per-workgroup reduction (10), cell counts off the wave size (65, 300), several verify passes."""
import ctypes as C
import os

import numpy as np
import pytest

import cells_util as U
from cells_util import ACCEPTED, ERR_ARG, HOST_CASES, POISON, REJECTED
from conftest import GOLDEN, splitmix64_bytes

pytestmark = pytest.mark.gpu

GUARD = 64


def oracle_commit(data, blowup):
    from oracle import oracle as O

    O.build()
    return O.commit(data, blowup)


# ---- open -------------------------------------------------------------------------------------------------------------------------------
OPEN_SHAPES = {
    "smallest": (1, 1, {}),
    "1k": (1024, 4, {}),
    "d12_levels_skipped": (3000, 4, {"FRIEDA_TREE_SKIP_LOG": 10, "FRIEDA_TREE_SKIP_LONE_LOG": 10}),
    "d12_full_tree": (3000, 4, {"FRIEDA_TREE_SKIP_LOG": 40, "FRIEDA_TREE_SKIP_LONE_LOG": 40}),
    "1k_general_route": (1024, 4, {"FRIEDA_NO_SMALL_FUSED": 1}),
}


@pytest.mark.parametrize("shape", sorted(OPEN_SHAPES))
def test_open_cells_equal_the_oracle(shape):
    import frieda_amd

    length, blowup, options = OPEN_SHAPES[shape]
    data, ev, layers, n, L = U.codeword(length, blowup)
    root = layers[0][0].tobytes()
    assert root == oracle_commit(data, blowup)
    ctx = frieda_amd.Context(0)
    try:
        for name, value in options.items():
            ctx.set_option(name, value)
        enc = ctx.encode(data, blowup)
        assert enc.commitment == root == ctx.commit(data, blowup)
        assert enc.shape == (L, n)
        for c in (0, 1, 2, 3, 6, 10):
            if c > n:
                continue
            for count in (1, 65):
                idx = U.cell_list(n, c, count, seed=count)
                values, paths = enc.open_cells(ctx, c, idx)
                want_v, want_p = U.open_oracle(ev, layers, c, idx)
                assert values.shape == want_v.shape and paths.shape == want_p.shape
                assert values.tobytes() == want_v.tobytes(), (c, count)
                assert paths.tobytes() == want_p.tobytes(), (c, count, np.flatnonzero((paths != want_p).any(axis=2).any(axis=0)))
        # no cells: a no-op; bad arguments: refused with the outputs untouched
        L_ = ctx._L
        assert L_.frieda_open_cells(ctx._h, enc._handle(), 0, None, 0, None, None) == 0
        v = np.full((2, 4, 1), 0xA5A5A5A5, dtype=np.uint32)
        p = np.full((2, n, 32), POISON, dtype=np.uint8)
        bad = np.array([0, 1 << n], dtype=np.uint32)
        assert L_.frieda_open_cells(ctx._h, enc._handle(), 0, bad.ctypes.data, 2, v.ctypes.data, p.ctypes.data) == ERR_ARG
        assert L_.frieda_open_cells(ctx._h, enc._handle(), n + 1, bad.ctypes.data, 1, v.ctypes.data, p.ctypes.data) == ERR_ARG
        assert (v == 0xA5A5A5A5).all() and (p == POISON).all()
        enc.close()
    finally:
        ctx.close()


def test_open_cells_beside_a_prove_seeds_job(gpu_ctx):
    """the blob is only read: another context opens cells while a prove_seeds job is in flight; the context with the job refuses"""
    import frieda_amd

    data, ev, layers, n, L = U.codeword(1024, 4)
    cfg = frieda_amd.PcsConfig(frieda_amd.FriConfig(4, 0, 8), 4)
    other = frieda_amd.Context(0)
    enc = gpu_ctx.encode(data, 4)
    try:
        idx = U.cell_list(n, 3, 17)
        want_v, want_p = U.open_oracle(ev, layers, 3, idx)
        gpu_ctx.prove_seeds_begin(enc, [1, 2, 3], cfg)
        try:
            values, paths = enc.open_cells(other, 3, idx)
            with pytest.raises(frieda_amd.FriedaError) as e:
                enc.open_cells(gpu_ctx, 3, idx)
            assert e.value.status == ERR_ARG and "in flight" in str(e.value)
        finally:
            proofs = gpu_ctx.prove_seeds_finish()
        assert values.tobytes() == want_v.tobytes() and paths.tobytes() == want_p.tobytes()
        assert all(frieda_amd.verify(p, s) for p, s in zip(proofs, [1, 2, 3]))
    finally:
        enc.close()
        other.close()


# ---- verify -----------------------------------------------------------------------------------------------------------------------------
def raw_verify_many(ctx, commitment, n, c, idx, values, paths):
    idx = np.ascontiguousarray(idx, dtype=np.uint32)
    values = np.ascontiguousarray(values, dtype=np.uint32)
    paths = np.ascontiguousarray(paths, dtype=np.uint8)
    status = np.full(max(1, len(idx)), POISON, dtype=np.uint8)
    com = (C.c_uint8 * 32)(*bytes(commitment))
    rc = ctx._L.frieda_verify_cells_many(ctx._h, com, n, c, idx.ctypes.data, len(idx), values.ctypes.data, paths.ctypes.data if paths.size else None,
                                         status.ctypes.data)
    return rc, status[: len(idx)]


def host_status(commitment, n, c, idx, values, paths):
    import frieda_amd

    return frieda_amd.verify_cells(commitment, n, c, idx, values, paths)


@pytest.mark.parametrize("n,b,c", HOST_CASES)
def test_verify_many_on_the_mutation_matrix(gpu_ctx, n, b, c):
    _, ev, layers, _, _ = U.case(n, b)
    root = layers[0][0].tobytes()
    idx = U.cell_list(n, c, 9)
    values, paths = U.open_oracle(ev, layers, c, idx)
    runs = [("intact", None, idx, values, paths)] + U.mutations(n, c, idx, values, paths)
    for label, t, i2, v2, p2 in runs:
        want = U.independent_status(root, n, c, i2, v2, p2)
        assert want.sum() == len(idx) - (0 if t is None else 1), label
        host = host_status(root, n, c, i2, v2, p2)
        rc, st = raw_verify_many(gpu_ctx, root, n, c, i2, v2, p2)
        assert rc == 0, label
        assert st.tolist() == host.tolist() == want.tolist(), (label, t)
    # a wrong commitment rejects all; bad arguments leave the status untouched
    wrong = bytearray(root)
    wrong[5] ^= 1
    rc, st = raw_verify_many(gpu_ctx, bytes(wrong), n, c, idx, values, paths)
    assert rc == 0 and (st == REJECTED).all()
    bad = idx.copy()
    bad[-1] = 1 << (n - c)
    rc, st = raw_verify_many(gpu_ctx, root, n, c, bad, values, paths)
    assert rc == ERR_ARG and (st == POISON).all()
    rc, st = raw_verify_many(gpu_ctx, root, n, 11, np.zeros(len(idx), np.uint32), values, paths)
    assert rc == ERR_ARG and (st == POISON).all()


def flipped_call(n, c, count, flips, seed):
    """a `count`-cell call with `flips` single-bit flips, each in another cell: values, paths and in-range index bits in turn"""
    _, ev, layers, _, _ = U.case(n, 4)
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, 1 << (n - c), size=count).astype(np.uint32)
    values, paths = U.open_oracle(ev, layers, c, idx)
    for j, t in enumerate(rng.choice(count, size=flips, replace=False)):
        kind = j % 3
        if kind == 0:
            w = values[t].reshape(-1)
            w[int(rng.integers(0, w.size))] ^= np.uint32(1 << int(rng.integers(0, 32)))
        elif kind == 1:
            p = paths[t].reshape(-1)
            p[int(rng.integers(0, p.size))] ^= np.uint8(1 << int(rng.integers(0, 8)))
        else:
            idx[t] ^= np.uint32(1 << int(rng.integers(0, n - c)))
    return layers[0][0].tobytes(), idx, values, paths


@pytest.mark.parametrize("pass_bytes", [0, 40000])
def test_verify_many_on_random_bit_flips(gpu_ctx, pass_bytes):
    """300 cells at log_domain 12, log_cell 3, 200 of them with one flipped bit; 40000 bytes per pass: 95 cells, four passes"""
    n, c = 12, 3
    root, idx, values, paths = flipped_call(n, c, 300, 200, seed=2024)
    want = U.independent_status(root, n, c, idx, values, paths)
    assert 95 <= want.sum() <= 110  # the untouched cells, and the rare flip that lands on an identical value
    host = host_status(root, n, c, idx, values, paths)
    if pass_bytes:
        assert 300 * (4 + (16 << c) + 32 * (n - c)) > 3 * pass_bytes
    assert gpu_ctx._L.frieda_ctx_test_set_verify_pass_bytes(gpu_ctx._h, pass_bytes) == 0
    try:
        rc, st = raw_verify_many(gpu_ctx, root, n, c, idx, values, paths)
    finally:
        gpu_ctx._L.frieda_ctx_test_set_verify_pass_bytes(gpu_ctx._h, 0)
    assert rc == 0
    assert st.tolist() == host.tolist() == want.tolist()


@pytest.mark.parametrize("c", [0, 1, 6, 10])
@pytest.mark.parametrize("count", [1, 65, 300])
def test_verify_many_cell_counts(gpu_ctx, c, count):
    n = 12
    root, idx, values, paths = flipped_call(n, c, count, (count + 2) // 3, seed=count + c)
    want = U.independent_status(root, n, c, idx, values, paths)
    host = host_status(root, n, c, idx, values, paths)
    st = gpu_ctx.verify_cells_many(root, n, c, idx, values, paths)
    assert st.tolist() == host.tolist() == want.tolist()
    assert want.sum() < count


# ---- reconstruct ------------------------------------------------------------------------------------------------------------------------
def raw_reconstruct(ctx, commitment, blowup, length, c, idx, values, paths):
    """frieda_reconstruct_from_opened_cells into a poison-filled buffer between two red zones: (rc, bytes or None, status, n_used)"""
    idx = np.ascontiguousarray(idx, dtype=np.uint32)
    values = np.ascontiguousarray(values, dtype=np.uint32)
    paths = np.ascontiguousarray(paths, dtype=np.uint8)
    buf = np.full(length + 2 * GUARD, POISON, dtype=np.uint8)
    status = np.full(len(idx) + GUARD, POISON, dtype=np.uint8)
    used = C.c_size_t(12345)
    com = (C.c_uint8 * 32)(*bytes(commitment))
    rc = ctx._L.frieda_reconstruct_from_opened_cells(ctx._h, com, blowup, length, c, idx.ctypes.data, len(idx), values.ctypes.data, paths.ctypes.data,
                                                     buf.ctypes.data + GUARD, status.ctypes.data, C.byref(used))
    assert (buf[:GUARD] == POISON).all() and (buf[GUARD + length:] == POISON).all(), "red zone around out_bytes"
    assert (status[len(idx):] == POISON).all(), "red zone behind out_status"
    body = buf[GUARD:GUARD + length]
    if rc != 0:
        assert (body == POISON).all(), "out_bytes written by a failed call"
    return rc, (body.tobytes() if rc == 0 else None), status[: len(idx)], used.value


def reconstruct_case(which):
    if which == "blob":
        with open(os.path.join(GOLDEN, "blob"), "rb") as f:
            data = f.read()
        return (data,) + _blob_codeword()
    data, ev, layers, n, L = U.case(which, 4)
    return data, ev, layers, n, L


_blob_cache = []


def _blob_codeword():
    from oracle import oracle as O

    if not _blob_cache:
        O.build()
        with open(os.path.join(GOLDEN, "blob"), "rb") as f:
            data = f.read()
        coef, L = O.polynomial_from_bytes(data)
        ev = O.circle_evaluate(coef, L + 4)
        _blob_cache.append((ev, O.merkle_commit(ev), L + 4, L))
    return _blob_cache[0]


RECONSTRUCT_CASES = [(n, c) for n in (11, 12) for c in (0, 3, 6)] + [("blob", 6)]


@pytest.mark.parametrize("which,c", RECONSTRUCT_CASES)
def test_reconstruct_from_opened_cells(gpu_ctx, which, c):
    data, ev, layers, n, L = reconstruct_case(which)
    if which == "blob":
        assert (L, n) == (15, 19)
    root = layers[0][0].tobytes()
    need = (1 << (L - c)) + 1 if c else (1 << L) + 2
    if which == "blob":
        assert need == 513
    rng = np.random.default_rng(300 + n + c)
    pick = rng.choice(1 << (n - c), size=need + 1, replace=False).astype(np.uint32)
    idx, spare = pick[:need], pick[need:]
    values, paths = U.open_oracle(ev, layers, c, pick)
    assert U.independent_status(root, n, c, pick, values, paths).all()
    v, p = values[:need], paths[:need]

    # exactly the minimum number of distinct cells
    rc, out, st, used = raw_reconstruct(gpu_ctx, root, 4, len(data), c, idx, v, p)
    assert rc == 0, gpu_ctx._L.frieda_last_error(gpu_ctx._h)
    assert out == data and used == need and (st == ACCEPTED).all()

    # one of them corrupted: too few, the status names it, the output keeps its poison
    t = int(rng.integers(0, need))
    vbad = values.copy()
    vbad[t, 1, 0] ^= 2
    rc, out, st, used = raw_reconstruct(gpu_ctx, root, 4, len(data), c, idx, vbad[:need], p)
    assert rc == ERR_ARG and used == need - 1
    assert np.flatnonzero(st != ACCEPTED).tolist() == [t] and st[t] == REJECTED

    # one spare cell added: enough again, and the rejected cell is not counted (nor used: the bytes are right)
    rc, out, st, used = raw_reconstruct(gpu_ctx, root, 4, len(data), c, pick, vbad, paths)
    assert rc == 0 and out == data and used == need
    assert np.flatnonzero(st != ACCEPTED).tolist() == [t]

    # repeated indices do not count twice
    rep = np.concatenate([idx[:-1], idx[:1]])
    rc, out, st, used = raw_reconstruct(gpu_ctx, root, 4, len(data), c, rep, np.concatenate([v[:-1], v[:1]]), np.concatenate([p[:-1], p[:1]]))
    assert rc == ERR_ARG and used == need - 1 and (st == ACCEPTED).all()

    # a wrong len (same polynomial size): every cell verifies, the commitment check fails
    assert oracle_commit(data[:-1], 4) != root
    rc, out, st, used = raw_reconstruct(gpu_ctx, root, 4, len(data) - 1, c, idx, v, p)
    assert rc == ERR_ARG and used == need and (st == ACCEPTED).all()
    assert b"commit" in gpu_ctx._L.frieda_last_error(gpu_ctx._h)


def test_reconstruct_python_surface(gpu_ctx):
    import frieda_amd

    data, ev, layers, n, L = U.case(11, 4)
    root = layers[0][0].tobytes()
    enc = gpu_ctx.encode(data, 4)
    try:
        idx = np.random.default_rng(4).permutation(1 << (n - 3))[: (1 << (L - 3)) + 1].astype(np.uint32)
        values, paths = enc.open_cells(gpu_ctx, 3, idx)
    finally:
        enc.close()
    out, st, used = gpu_ctx.reconstruct_from_opened_cells(root, 4, len(data), 3, idx, values, paths)
    assert out == data and used == len(idx) and (st == ACCEPTED).all()
    with pytest.raises(frieda_amd.FriedaError) as e:
        gpu_ctx.reconstruct_from_opened_cells(root, 4, len(data), 3, idx[:-1], values[:-1], paths[:-1])
    assert e.value.status == ERR_ARG and e.value.n_cells_used == len(idx) - 1 and (e.value.cell_status == ACCEPTED).all()
