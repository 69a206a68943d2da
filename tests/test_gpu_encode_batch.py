"""GPU: frieda_encode_batch — the handles of a block made in one call.  Handle b must be indistinguishable from frieda_encode of blob b
through every call that takes a handle (encoded_util.facts: commitment, shape, open_cells, open_cell_bundles, prove_seeds as bytes);
the roots must be frieda_commit_batch's; the handles are closed one by one in a scrambled order with the survivors still serving."""
import ctypes as C
import os

import numpy as np
import pytest

import encoded_util as E
import workspace_rows as W
from cells_util import ERR_ARG
from conftest import GOLDEN, splitmix64_bytes

pytestmark = pytest.mark.gpu

# (blob bytes, log_blowup_factor): the smallest the prover takes (L = 1, n = 2); the fused small route; its upper border n = 15; the
# general route from n = 16; 64 KiB; the 2^15-coefficient fixture ("blob": tests/golden/blob)
SHAPES = [(16, 1), (1024, 4), (20000, 4), (20000, 5), (65536, 4), ("blob", 4)]
COUNTS = [1, 2, 5, 17]


def blobs_of(length, count):
    if length == "blob":
        with open(os.path.join(GOLDEN, "blob"), "rb") as f:
            base = np.frombuffer(f.read(), dtype=np.uint8)
        return [np.roll(base, 977 * b).tobytes() for b in range(count)]
    return [splitmix64_bytes(5000 + 31 * b + length, length).tobytes() for b in range(count)]


def check_block(ctx, ref_ctx, blobs, blowup, stride=None, prove_all=True):
    """encode_batch on ctx; every handle against H0 (made on ref_ctx, default options); scrambled closes"""
    import frieda_amd

    encs = ctx.encode_batch(blobs, blowup, stride=stride)
    try:
        assert len(encs) == len(blobs)
        assert [e.commitment for e in encs] == ctx.commit_batch(blobs, blowup)
        for b, e in enumerate(encs):
            # (the proofs of every handle for small blocks, of the first, the last and a middle one for the larger)
            prove = prove_all or b in (0, len(encs) // 2, len(encs) - 1)
            E.assert_same(E.facts(ctx, e, prove), E.facts_of_bytes(ref_ctx, blobs[b], blowup, prove), "blob %d" % b)
        # a mixed table: stripes over handles of the batch and lone handles together
        n = encs[0].shape[1]
        ref = [ref_ctx.encode(bl, blowup) for bl in blobs]  # a lone handle of every blob
        try:
            stripes = np.array([0, (1 << (n - 1)) - 1, 1], dtype=np.uint32) % (1 << (n - 1))
            mixed = frieda_amd.open_stripes(ctx, list(encs) + ref[:2], 1, stripes)
            alone = frieda_amd.open_stripes(ref_ctx, ref + ref[:2], 1, stripes)
            assert mixed[0].tobytes() == alone[0].tobytes() and mixed[1].tobytes() == alone[1].tobytes()
            ends = np.array([0, (1 << n) - 1], dtype=np.uint32)
            want = [tuple(x.tobytes() for x in r.open_cells(ref_ctx, 0, ends)) for r in ref]
        finally:
            E.close_all(ref)
        # closed in a scrambled order: after every close the survivors still open the same cells, values and paths
        order = np.random.default_rng(len(blobs)).permutation(len(encs))
        alive = set(range(len(encs)))
        for b in order:
            encs[b].close()
            alive.discard(int(b))
            for a in sorted(alive)[:3]:
                v, p = encs[a].open_cells(ctx, 0, ends)
                assert (v.tobytes(), p.tobytes()) == want[a], (int(b), a)
                assert encs[a].commitment == E.facts_of_bytes(ref_ctx, blobs[a], blowup, False)["commitment"]
    finally:
        E.close_all(encs)


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("length,blowup", SHAPES)
def test_encode_batch_handles_equal_lone_handles(gpu_ctx, length, blowup, count):
    blobs = blobs_of(length, count)
    # a stride larger than len in one case per shape
    stride = len(blobs[0]) + 37 if count == 5 else None
    check_block(gpu_ctx, gpu_ctx, blobs, blowup, stride=stride, prove_all=count <= 5)


@pytest.mark.parametrize("count", [1, 3])
def test_encode_batch_under_low_skip_thresholds(gpu_ctx, count):
    """FRIEDA_TREE_SKIP_LOG = FRIEDA_TREE_SKIP_LONE_LOG = 10 on the context that encodes: the trees lose the two levels above their leaves,
    the handles say so, and every answer is still that of a handle built with the defaults"""
    import frieda_amd

    ctx = frieda_amd.Context(0)
    try:
        ctx.set_option("FRIEDA_TREE_SKIP_LOG", 10)
        ctx.set_option("FRIEDA_TREE_SKIP_LONE_LOG", 10)
        check_block(ctx, gpu_ctx, blobs_of("blob", count), 4)
        check_block(ctx, gpu_ctx, blobs_of(20000, count), 4)
    finally:
        ctx.close()


def raw_encode_batch(ctx, data, stride, length, count, blowup, null_data=False, null_out=False):
    buf = (C.c_uint8 * max(len(data), 1)).from_buffer_copy(data or b"\0")
    outs = (C.c_void_p * max(count, 4))(*([0xDEAD0] * max(count, 4)))
    rc = ctx._L.frieda_encode_batch(ctx._h, None if null_data else buf, stride, length, count, blowup, None if null_out else outs)
    return rc, list(outs)


def test_argument_errors_leave_out_encs_untouched(gpu_ctx):
    import frieda_amd

    data = b"".join(blobs_of(1024, 3))
    untouched = [0xDEAD0] * 4
    assert raw_encode_batch(gpu_ctx, data, 1024, 1024, 0, 4) == (ERR_ARG, untouched)  # count 0
    assert raw_encode_batch(gpu_ctx, data, 1024, 1024, 3, 4, null_data=True) == (ERR_ARG, untouched)
    assert raw_encode_batch(gpu_ctx, data, 1024, 1024, 3, 4, null_out=True)[0] == ERR_ARG
    assert raw_encode_batch(gpu_ctx, data, 1024, 1024, 3, 29) == (ERR_ARG, untouched)  # log_blowup_factor beyond FRIEDA_MAX_LOG_DOMAIN
    assert raw_encode_batch(gpu_ctx, data, 1024, 1024, 3, 0xFFFFFFFF) == (ERR_ARG, untouched)
    assert raw_encode_batch(gpu_ctx, data, 1023, 1024, 3, 4) == (ERR_ARG, untouched)  # stride below len
    rc, outs = raw_encode_batch(gpu_ctx, data, 1024, 1024, 65536, 4)  # count beyond 65535 (refused before the blobs are read)
    assert rc == ERR_ARG and set(outs) == {0xDEAD0}
    # a proof in flight on the context
    ctx = frieda_amd.Context(0)
    try:
        ctx.prove_begin(data[:1024], 1, E.pcs(4))
        assert raw_encode_batch(ctx, data, 1024, 1024, 3, 4) == (ERR_ARG, untouched)
        assert b"in flight" in ctx._L.frieda_last_error(ctx._h)
        ctx.prove_finish()
        rc, outs = raw_encode_batch(ctx, data, 1024, 1024, 3, 4)
        assert rc == 0 and outs[3] == 0xDEAD0 and all(outs[:3])
        for h in outs[:3]:
            ctx._L.frieda_encoded_free(C.c_void_p(h))
    finally:
        ctx.close()


def test_arena_limit_gives_nomem_and_leaves_the_context_usable(gpu_ctx):
    """the call is not cut into passes: a workspace that does not fit is FRIEDA_ERR_NOMEM, out_encs untouched, the context usable"""
    import frieda_amd

    ctx = frieda_amd.Context(0)
    try:
        blobs = blobs_of(65536, 5)
        assert ctx._L.frieda_ctx_test_set_arena_limit(ctx._h, 1 << 16) == 0
        rc, outs = raw_encode_batch(ctx, b"".join(blobs), 65536, 65536, 5, 4)
        assert rc == 4 and outs == [0xDEAD0] * 5, (rc, ctx._L.frieda_last_error(ctx._h))
        assert ctx._L.frieda_ctx_test_set_arena_limit(ctx._h, 0) == 0
        check_block(ctx, gpu_ctx, blobs[:2], 4)
    finally:
        ctx.close()


@pytest.mark.parametrize("word", [0x00000000, 0xFFFFFFFF, 0x7FFFFFFF])
def test_same_handles_on_a_sticky_poisoned_context(gpu_ctx, word):
    import frieda_amd

    ctx = frieda_amd.Context(0)
    try:
        W.poison(ctx, word)
        check_block(ctx, gpu_ctx, blobs_of(1024, 3), 4)
        check_block(ctx, gpu_ctx, blobs_of(20000, 3), 5)
    finally:
        ctx.close()
