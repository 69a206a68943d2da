"""GPU: frieda_verify_blobs_many — the proofs of a block against a table of commitments, on both launch shapes.

8 blobs of 1 KiB through encode_batch and prove_seeds_blobs under 2 seeds: 16 proofs, proof (b, s) at entry 2 b + s.  The reference of
every status is frieda_verify_many for that proof alone with expected_commitment = commitments[blob_index[i]]."""
import ctypes as C

import numpy as np
import pytest

from conftest import splitmix64_bytes
from test_gpu_verify_many import ACCEPTED, ERR_ARG, REJECTED, WRONG_COMMITMENT, _bump, mutate

pytestmark = pytest.mark.gpu

K, SEEDS = 8, [11, 12]


def _cfg():
    import frieda_amd

    return frieda_amd.PcsConfig(frieda_amd.FriConfig(4, 0, 20), 8)


@pytest.fixture(scope="module")
def block(gpu_ctx):
    """(commitments[K], proofs[2 K], seeds[2 K], blob_index[2 K])"""
    blobs = [splitmix64_bytes(70 + b, 1024).tobytes() for b in range(K)]
    encs = gpu_ctx.encode_batch(blobs, 4)
    try:
        coms = [e.commitment for e in encs]
        grid = gpu_ctx.prove_seeds_blobs(encs, SEEDS, _cfg())
    finally:
        for e in encs:
            e.close()
    assert len(set(coms)) == K
    proofs = [grid[b][s] for b in range(K) for s in range(2)]
    return coms, proofs, SEEDS * K, [b for b in range(K) for _ in range(2)]


@pytest.fixture(scope="module", params=[0, 1 << 31], ids=["one-kernel", "split"])
def ctx(request):
    import frieda_amd

    c = frieda_amd.Context(0)
    c.set_option("FRIEDA_VERIFY_DEVICE_MIN", 0)
    c.set_option("FRIEDA_VERIFY_SPLIT_MAX", request.param)
    yield c
    c.close()


def _alone(ctx, proofs, seeds, coms, bidx):
    """frieda_verify_many proof by proof, each with its own expected commitment"""
    return [int(ctx.verify_many([p], [s], expected_commitment=coms[b])[0]) for p, s, b in zip(proofs, seeds, bidx)]


def test_all_accepted_with_the_right_index(ctx, block):
    coms, proofs, seeds, bidx = block
    st, acc = ctx.verify_blobs_many(proofs, coms, bidx, seeds)
    assert list(st) == [ACCEPTED] * 16 == _alone(ctx, proofs, seeds, coms, bidx)
    assert acc.dtype == np.uint32 and list(acc) == [2] * K


def test_two_index_entries_swapped(ctx, block):
    coms, proofs, seeds, bidx = block
    swapped = list(bidx)
    swapped[3], swapped[10] = swapped[10], swapped[3]  # a proof of blob 1 names blob 5 and the other way round
    st, acc = ctx.verify_blobs_many(proofs, coms, swapped, seeds)
    assert [i for i, s in enumerate(st) if s != ACCEPTED] == [3, 10] and st[3] == st[10] == WRONG_COMMITMENT
    assert list(st) == _alone(ctx, proofs, seeds, coms, swapped)
    assert list(acc) == [1 if b in (1, 5) else 2 for b in range(K)]


def test_one_mutated_proof(ctx, block):
    coms, proofs, seeds, bidx = block
    ps = list(proofs)
    ps[7] = mutate(proofs[7], lambda d: _bump(d["inner"][2]["fri"], 1))
    st, acc = ctx.verify_blobs_many(ps, coms, bidx, seeds)
    assert st[7] == int(ctx.verify_many([ps[7]], [seeds[7]], expected_commitment=coms[3])[0]) == REJECTED
    assert list(st) == _alone(ctx, ps, seeds, coms, bidx)
    assert list(acc) == [1 if b == 3 else 2 for b in range(K)]
    # the count may be left out; a blob nobody names counts 0; proofs in any order
    order = [15, 0, 7, 6]
    st2, acc2 = ctx.verify_blobs_many([ps[i] for i in order], coms, [bidx[i] for i in order], [seeds[i] for i in order])
    assert list(st2) == [ACCEPTED, ACCEPTED, REJECTED, ACCEPTED] and list(acc2) == [1, 0, 0, 1, 0, 0, 0, 1]
    status = np.full(16, 0xEE, dtype=np.uint8)
    arr = (C.c_void_p * 16)(*[p._h.value if isinstance(p._h, C.c_void_p) else p._h for p in ps])
    rc = ctx._L.frieda_verify_blobs_many(ctx._h, arr, (C.c_uint64 * 16)(*seeds), 16, b"".join(coms), K, (C.c_uint32 * 16)(*bidx), status.ctypes.data, None)
    assert rc == 0 and status.tobytes() == st.tobytes()


def test_without_an_index_proof_i_belongs_to_commitment_i(ctx, block):
    coms, proofs, seeds, _ = block
    st, acc = ctx.verify_blobs_many(proofs[0::2], coms, None, seeds[0::2])
    assert list(st) == [ACCEPTED] * K and list(acc) == [1] * K
    rolled = coms[1:] + coms[:1]
    st, acc = ctx.verify_blobs_many(proofs[1::2], rolled, None, seeds[1::2])
    assert list(st) == [WRONG_COMMITMENT] * K and list(acc) == [0] * K


def test_bad_arguments_leave_the_outputs_untouched(ctx, block):
    coms, proofs, seeds, bidx = block
    L = ctx._L
    arr = (C.c_void_p * 16)(*[p._h.value if isinstance(p._h, C.c_void_p) else p._h for p in proofs])
    sd = (C.c_uint64 * 16)(*seeds)
    table = b"".join(coms)

    def call(c, count, tab, n_blobs, index):
        status = np.full(16, 0xEE, dtype=np.uint8)
        acc = np.full(K, 0xEEEEEEEE, dtype=np.uint32)
        ix = None if index is None else (C.c_uint32 * len(index))(*index)
        rc = L.frieda_verify_blobs_many(c._h, arr, sd, count, tab, n_blobs, ix, status.ctypes.data, acc.ctypes.data)
        assert set(status) == {0xEE} and set(acc) == {0xEEEEEEEE}
        return rc

    beyond = list(bidx)
    beyond[15] = K
    assert call(ctx, 16, table, K, beyond) == ERR_ARG          # an index >= n_blobs
    assert call(ctx, 16, table, K, None) == ERR_ARG            # no index and count != n_blobs
    assert call(ctx, 7, table, K, None) == ERR_ARG
    assert call(ctx, 16, table, 0, bidx) == ERR_ARG            # proofs but no blobs
    assert call(ctx, 16, table, 0, None) == ERR_ARG
    assert call(ctx, 16, None, K, bidx) == ERR_ARG             # no commitments
    data = splitmix64_bytes(70, 1024).tobytes()
    ctx.prove_begin(data, 5, _cfg())                           # a proof in flight on the context
    try:
        assert call(ctx, 16, table, K, bidx) == ERR_ARG
    finally:
        ctx.prove_finish()
    st, acc = ctx.verify_blobs_many(proofs, coms, bidx, seeds)
    assert list(st) == [ACCEPTED] * 16 and list(acc) == [2] * K
