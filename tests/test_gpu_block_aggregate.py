"""GPU: the aggregate handle of a block (frieda_aggregate_encoded, aggregate.hip): g = sum over k of rho^k * f_k.

The aggregate's evaluation, read back through frieda_open_cells over the whole domain, must equal the sum computed from the oracle's
codewords and the oracle channel's rho word for word, and its commitment the oracle's merkle_commit of those columns — for every blob
length of the grid at K = 3 and every K at one length, whatever slabs and tree-skip thresholds the handles come from.  K = 1 is the
blob itself.  The testing hook takes rho through every coordinate in {0, 1, P - 1} on value-edge blobs and both kernel routes.  The
inputs are only read, the bytes do not depend on what the workspace held, and the argument rules refuse what they must."""
import ctypes as C
import itertools

import numpy as np
import pytest

from block_util import P, aggregate_reference, oracle_rho
from conftest import splitmix64_bytes
from edge_values import BLOBS
from util import blob_len_for
from workspace_rows import WORDS, cfg_of, poison

pytestmark = pytest.mark.gpu

_EVALS = {}


def blob(length, seed):
    return splitmix64_bytes(0xB10C + 1000 * seed + length % 997, length).tobytes()


def oracle_eval(oracle, data, log_blowup):
    """the codeword of `data`: uint32 [4, 2^n], bit-reversed order"""
    key = (bytes(data), log_blowup)
    if key not in _EVALS:
        coef, L = oracle.polynomial_from_bytes(data)
        _EVALS[key] = oracle.circle_evaluate(coef, L + log_blowup)
    return _EVALS[key]


def read_eval(ctx, enc):
    """the handle's evaluation through frieda_open_cells over the whole domain: uint32 [4, 2^n]"""
    n = enc.shape[1]
    log_cell = min(n, 10)
    values, _ = enc.open_cells(ctx, log_cell, np.arange(1 << (n - log_cell), dtype=np.uint32))
    return np.ascontiguousarray(values.transpose(1, 0, 2).reshape(4, -1))


def check_aggregate(ctx, oracle, agg, blobs, log_blowup, rho=None):
    evals = [oracle_eval(oracle, d, log_blowup) for d in blobs]
    if rho is None:
        rho = oracle_rho(oracle, [oracle.merkle_commit(e)[0][0].tobytes() for e in evals])
    want = aggregate_reference(oracle, evals, rho)
    got = read_eval(ctx, agg)
    assert got.shape == want.shape
    assert np.array_equal(got, want), f"{int((got != want).sum())} words differ, first at {tuple(np.argwhere(got != want)[0])}"
    assert agg.commitment == oracle.merkle_commit(want)[0][0].tobytes()
    assert agg.aggregate_of == len(blobs)
    return want


GRID = [(length, 3, 4) for length in (1, 16, 100, 1024, 131072, blob_len_for(18))] + [(1024, k, 4) for k in (1, 2, 5, 17)] + [(1, 3, 1), (100, 3, 1)]


@pytest.mark.parametrize("length,k,log_blowup", GRID)
def test_aggregate_equals_the_sum_from_the_oracle(gpu_ctx, oracle, length, k, log_blowup):
    blobs = [blob(length, s) for s in range(k)]
    encs = gpu_ctx.encode_batch(blobs, log_blowup)
    try:
        roots = [e.commitment for e in encs]
        assert roots == [oracle.commit(d, log_blowup) for d in blobs]
        with gpu_ctx.aggregate_encoded(encs) as agg:
            assert agg.shape == encs[0].shape and agg.nbytes == encs[0].nbytes
            assert all(e.aggregate_of == 0 for e in encs)
            check_aggregate(gpu_ctx, oracle, agg, blobs, log_blowup)
            # the inputs were only read
            assert [e.commitment for e in encs] == roots
            assert np.array_equal(read_eval(gpu_ctx, encs[k - 1]), oracle_eval(oracle, blobs[k - 1], log_blowup))
    finally:
        for e in encs:
            e.close()


def test_one_blob_is_its_own_aggregate(gpu_ctx, oracle):
    data = blob(1024, 7)
    cfg = cfg_of(4, 4, 0, 20)
    with gpu_ctx.encode(data, 4) as enc, gpu_ctx.aggregate_encoded([enc]) as agg:
        assert agg.commitment == enc.commitment == oracle.commit(data, 4)
        assert agg.aggregate_of == 1 and enc.aggregate_of == 0
        assert np.array_equal(read_eval(gpu_ctx, agg), read_eval(gpu_ctx, enc))
        seeds = [3, 4, 2**64 - 1]
        assert [p.serialize() for p in gpu_ctx.prove_seeds(agg, seeds, cfg)] == [p.serialize() for p in gpu_ctx.prove_seeds(enc, seeds, cfg)]


def test_handles_of_any_mix_give_the_same_aggregate(gpu_ctx, oracle):
    """one slab, lone handles, a mix of both, and a repeated handle"""
    blobs = [blob(1024, s) for s in range(3)]
    slab = gpu_ctx.encode_batch(blobs, 4)
    lone = [gpu_ctx.encode(d, 4) for d in blobs]
    try:
        images = []
        for encs in (slab, lone, [slab[0], lone[1], slab[2]]):
            with gpu_ctx.aggregate_encoded(encs) as agg:
                images.append((agg.commitment, read_eval(gpu_ctx, agg).tobytes()))
        assert images[0] == images[1] == images[2]
        with gpu_ctx.aggregate_encoded([slab[0], slab[0], lone[1]]) as agg:
            check_aggregate(gpu_ctx, oracle, agg, [blobs[0], blobs[0], blobs[1]], 4)
    finally:
        for e in slab + lone:
            e.close()


def test_tree_skip_thresholds_do_not_matter_at_2_18(gpu_ctx, oracle):
    """2^18 leaves: a block's handles are built without the two levels above the leaves (FRIEDA_TREE_SKIP_LOG 18), a lone handle with them
    (FRIEDA_TREE_SKIP_LONE_LOG 23); the aggregate itself is built under either.  Evaluation, commitment and a proof from it are the same."""
    import frieda_amd

    length = blob_len_for(18)
    blobs = [blob(length, s) for s in range(2)]
    cfg = cfg_of(4, 4, 0, 20)
    skipping = frieda_amd.Context(0)
    slab = gpu_ctx.encode_batch(blobs, 4)
    lone = [gpu_ctx.encode(d, 4) for d in blobs]
    try:
        skipping.set_option("FRIEDA_TREE_SKIP_LONE_LOG", 18)
        results = []
        for ctx, encs in ((gpu_ctx, slab), (gpu_ctx, lone), (gpu_ctx, [slab[0], lone[1]]), (skipping, [lone[0], slab[1]])):
            with ctx.aggregate_encoded(encs) as agg:
                results.append((agg.commitment, read_eval(ctx, agg).tobytes(), ctx.prove_seeds(agg, [9], cfg)[0].serialize()))
        assert all(r == results[0] for r in results[1:])
        evals = [oracle_eval(oracle, d, 4) for d in blobs]
        want = aggregate_reference(oracle, evals, oracle_rho(oracle, [e.commitment for e in slab]))
        assert results[0][1] == want.tobytes() and results[0][0] == oracle.merkle_commit(want)[0][0].tobytes()
    finally:
        for e in slab + lone:
            e.close()
        skipping.close()


EDGE_RHOS = list(itertools.product((0, 1, P - 1), repeat=4))


def test_rho_through_the_hook_on_both_routes(oracle):
    """every coordinate of rho from {0, 1, P - 1}, on the value-edge blobs, through the one-thread chain and the split chain"""
    import frieda_amd

    length = 100
    names = sorted(BLOBS)
    blobs = [BLOBS[name](length) for name in names] + [blob(length, 1)]
    evals = [oracle_eval(oracle, d, 4) for d in blobs]
    routes = {}
    for mode, route in ((1, "one chain"), (2, "split")):
        ctx = frieda_amd.Context(0)
        ctx.set_option("FRIEDA_AGG_SPLIT", mode)
        routes[route] = ctx
    encs = routes["split"].encode_batch(blobs, 4)
    try:
        for rho in EDGE_RHOS:
            want = aggregate_reference(oracle, evals, rho)
            for route, ctx in routes.items():
                with ctx.aggregate_encoded(encs, rho=rho) as agg:
                    assert np.array_equal(read_eval(ctx, agg), want), (rho, route)
            if rho == (0, 0, 0, 0):
                assert np.array_equal(want, evals[0])
            if rho == (1, 0, 0, 0):
                assert np.array_equal(want, (sum(e.astype(np.uint64) for e in evals) % P).astype(np.uint32))
        # both routes under the drawn rho too, with their commitments
        images = []
        for ctx in routes.values():
            with ctx.aggregate_encoded(encs) as agg:
                check_aggregate(ctx, oracle, agg, blobs, 4)
                images.append((agg.commitment, read_eval(ctx, agg).tobytes()))
        assert images[0] == images[1]
        # the hook's own rule: four canonical words
        out = C.c_void_p()
        handles = (C.c_void_p * len(encs))(*[e._handle() for e in encs])
        ctx = routes["split"]
        assert ctx._L.frieda_test_aggregate_with_rho(ctx._h, handles, len(encs), (C.c_uint32 * 4)(0, P, 0, 0), C.byref(out)) == 1 and not out.value
        assert ctx._L.frieda_test_aggregate_with_rho(ctx._h, handles, len(encs), None, C.byref(out)) == 1 and not out.value
    finally:
        for e in encs:
            e.close()
        for ctx in routes.values():
            ctx.close()


def test_identical_bytes_on_a_poisoned_workspace(oracle):
    """a fresh context, then the arena and the pinned blocks filled with each word, then a context that poisons every allocation it makes"""
    import frieda_amd

    blobs = [blob(1024, s) for s in range(9)]  # (nine blobs: the split route)
    cfg = cfg_of(4, 4, 0, 20)

    def run(ctx):
        encs = ctx.encode_batch(blobs, 4)
        try:
            with ctx.aggregate_encoded(encs) as agg:
                return agg.commitment, read_eval(ctx, agg).tobytes(), ctx.prove_seeds(agg, [1], cfg)[0].serialize()
        finally:
            for e in encs:
                e.close()

    ctx = frieda_amd.Context(0)
    try:
        r0 = run(ctx)
        want = aggregate_reference(oracle, [oracle_eval(oracle, d, 4) for d in blobs], oracle_rho(oracle, [oracle.commit(d, 4) for d in blobs]))
        assert r0[1] == want.tobytes() and r0[0] == oracle.merkle_commit(want)[0][0].tobytes()
        for word in WORDS:
            assert poison(ctx, word)[0] > 0
            assert run(ctx) == r0, f"other bytes after the workspace was filled with {word:#010x}"
            other = frieda_amd.Context(0)
            try:
                assert poison(other, word) == [0, 0, 0, 0]
                assert run(other) == r0, f"other bytes when every new allocation is filled with {word:#010x}"
            finally:
                other.close()
    finally:
        ctx.close()


def test_argument_errors(gpu_ctx):
    import frieda_amd

    L = gpu_ctx._L
    a = gpu_ctx.encode(blob(1024, 0), 4)
    b = gpu_ctx.encode(blob(100, 0), 4)       # another length
    c = gpu_ctx.encode(blob(1024, 0), 3)      # another blow-up
    try:
        out = C.c_void_p()

        def call(handles, k):
            arr = (C.c_void_p * max(1, len(handles)))(*handles)
            rc = L.frieda_aggregate_encoded(gpu_ctx._h, arr, k, C.byref(out))
            assert not out.value
            return rc

        assert call([a._handle(), b._handle()], 2) == 1 and b"one length" in L.frieda_last_error(gpu_ctx._h)
        assert call([a._handle(), c._handle()], 2) == 1
        assert call([a._handle(), None], 2) == 1 and b"null" in L.frieda_last_error(gpu_ctx._h)
        assert call([a._handle()], 0) == 1
        assert call([a._handle()], 65536) == 1
        assert L.frieda_aggregate_encoded(gpu_ctx._h, None, 1, C.byref(out)) == 1
        assert L.frieda_aggregate_encoded(gpu_ctx._h, (C.c_void_p * 1)(a._handle()), 1, None) == 1
        # a job in flight
        cfg = cfg_of(4, 4, 0, 20)
        gpu_ctx.prove_seeds_begin(a, [1], cfg)
        assert call([a._handle()], 1) == 1 and b"in flight" in L.frieda_last_error(gpu_ctx._h)
        (proof,) = gpu_ctx.prove_seeds_finish()
        assert frieda_amd.verify(proof, 1)
        # and the context is as usable as before
        with gpu_ctx.aggregate_encoded([a, a]) as agg:
            assert agg.aggregate_of == 2
    finally:
        for e in (a, b, c):
            e.close()
