"""GPU: identical bytes whatever the workspace held before — the state a call starts from.

Every row of tests/workspace_rows.py (one per route of the library) runs on a fresh context (R0), then again after
frieda_ctx_test_poison has filled the arena, the pinned blocks and the twiddle generator's scratch with 0x00000000, 0xFFFFFFFF and
0x7FFFFFFF (P: not canonical, and zero to lazily reducing code), and once more per word on a context that has allocated nothing yet and
poisons every allocation it makes (the sticky mode: arena growth, new twiddle sets, pinned blocks, encoded blobs, pools, temporaries).
Everything the caller can see — output bytes, statuses, counts — must equal R0, and R0 equals the CPU oracle (the rows assert that
with the helpers of the ops' own parity tests).  A kernel that reads one word further than this call wrote, or a route on which the
zeroing launch does not run, gives other bytes under at least one of the words.

Reach is asserted: the R0 run must launch the kernels the row names (the context's timing report), and the poison must have filled at
least frieda_workspace_bytes of the row's shape (where that function applies; elsewhere more than nothing — rows of entry points that
plan no workspace say so and are checked to have none).  The second half is history beyond the arena: a larger call of another shape,
release_workspace, the twiddle cache toggled, refused calls of every kind, a rejected proof."""
import ctypes as C

import numpy as np
import pytest

import workspace_rows as W
from conftest import splitmix64_bytes
from test_gpu_value_edges import kernels_of
from util import blob_len_for
from workspace_rows import ROWS, WORDS, norm, poison, setup

pytestmark = pytest.mark.gpu


def last_error(ctx):
    return ctx._L.frieda_last_error(ctx._h)


def fresh(row):
    import frieda_amd

    ctx = frieda_amd.Context(0)
    setup(ctx, row)
    return ctx


@pytest.mark.parametrize("name", sorted(ROWS))
def test_row_gives_the_same_bytes_on_a_poisoned_workspace(oracle, name):
    row = ROWS[name]
    ctx = fresh(row)
    try:
        assert poison(ctx, 0xDEADBEEF, sticky=0) == [0, 0, 0, 0], "a context that has run nothing owns nothing"
        r0, names = kernels_of(ctx, lambda: norm(row.run(ctx, oracle)))
        assert set(row.kernels) <= names, f"{name} did not reach {sorted(set(row.kernels) - names)}: launched {sorted(names)}"
        for word in WORDS:
            err = last_error(ctx)  # (rows that end with a refused call leave its text: the hook neither sets nor clears it)
            filled = poison(ctx, word)
            if row.ws is not None:
                assert filled[0] >= ctx._L.frieda_workspace_bytes(*row.ws) > 0, (name, filled)
            elif row.arena:
                assert filled[0] > 0, (name, filled)
            else:
                assert filled[0] == 0, f"{name} is listed as planning no workspace, and has {filled[0]} bytes of it"
            assert last_error(ctx) == err, "poisoning is not an error"
            assert norm(row.run(ctx, oracle)) == r0, f"{name}: other bytes after the workspace was filled with {word:#010x}"
            other = fresh(row)
            try:
                assert poison(other, word) == [0, 0, 0, 0]
                assert norm(row.run(other, oracle)) == r0, f"{name}: other bytes when every new allocation is filled with {word:#010x}"
            finally:
                other.close()
    finally:
        ctx.close()


# ---- the hook itself -------------------------------------------------------------------------------------------------------------------
def test_poison_fills_what_it_reports_and_nothing_the_caller_sees(oracle):
    """the regions by size; sticky off again; the twiddle tables only when they are scratch; an encoded blob's commitment and proofs"""
    import frieda_amd

    ctx = frieda_amd.Context(0)
    try:
        data = W.BLOBS["ff_then_00"](blob_len_for(16))
        cfg = W.cfg_of(4, 4, 0, 20)
        with ctx.encode(data, 4) as enc:
            commitment = enc.commitment
            want = [p.serialize() for p in ctx.prove_seeds(enc, [5, 6], cfg)]
            filled = poison(ctx, 0xFFFFFFFF, sticky=0)
            assert filled[0] >= frieda_amd.seeds_workspace_bytes(len(data), cfg, 2) > 0 and filled[0] % (1 << 20) == 0
            assert filled[1] >= 4096 and filled[2] == 0, filled
            assert filled[3] >= 8192 and filled[3] % 8192 == 0, filled  # cached twiddle sets: 8 KiB of generator scratch each, the tables left alone
            assert last_error(ctx) == b"" and enc.commitment == commitment
            assert [p.serialize() for p in ctx.prove_seeds(enc, [5, 6], cfg)] == want
            ctx.set_twiddle_cache(False)
            assert poison(ctx, 0x7FFFFFFF, sticky=0)[3] >= filled[3] + 2 * (4 << 15), "the tables of the 2^16 domain are scratch without the cache"
            assert [p.serialize() for p in ctx.prove_seeds(enc, [5, 6], cfg)] == want
            ctx.set_twiddle_cache(True)
        small = W.BLOBS["ff_then_00"](1024)
        root = ctx.commit(small, 4)  # a lone small host blob: the pinned input block
        assert poison(ctx, 0, sticky=0)[2] == 7680
        assert ctx.commit(small, 4) == root == oracle.commit(small, 4)
        # refused while a proof is in flight, as every call that touches the workspace
        ctx.prove_begin(small, 1, cfg)
        out = (C.c_uint64 * 4)(7, 7, 7, 7)
        assert ctx._L.frieda_ctx_test_poison(ctx._h, 0, 1, out) == 1 and list(out) == [7, 7, 7, 7]
        assert b"in flight" in last_error(ctx)
        r, p = ctx.prove_finish()
        assert r == root and frieda_amd.verify(p, 1)
        assert ctx._L.frieda_ctx_test_poison(ctx._h, 0, 0, None) == 0  # the out-array is optional
    finally:
        ctx.close()


# ---- a call takes what its sizing function says ---------------------------------------------------------------------------------------------
MIB = 1 << 20


def _arena_after(call):
    """the arena of a context that has made this one call (the hook's region 0); data and handles come from another context"""
    import frieda_amd

    ctx = frieda_amd.Context(0)
    try:
        call(ctx)
        return poison(ctx, 0xDEADBEEF, sticky=0)[0]
    finally:
        ctx.close()


def _rounded(nbytes):
    """Ctx::ensure_arena's rule"""
    return (nbytes + MIB - 1) & ~(MIB - 1)


def test_a_call_takes_what_its_sizing_function_says(oracle):
    """The arena of a fresh context after ONE call equals the public sizing function's figure, rounded up to 1 MiB as ensure_arena does:
    one layout feeds the call and the function.  Device-resident data, as the functions assume; the handles of the seeds forms are
    encoded on another context (an encode's own arena would hide the call's).  No public function gives a plain batch's total (its
    shared tail — transcripts, grind counters, opening lists — is not the seeds forms' exact one): for it the per-blob figure bounds the
    arena from below, and the tail of three 2^12 jobs (about 0.5 MiB) plus the rounding from above."""
    import frieda_amd
    from util import DevBuf

    cfg = W.cfg_of(20, 4, 0, 20)
    small, big = W.BLOBS["ff_then_00"](blob_len_for(12)), W.BLOBS["ff_then_00"](blob_len_for(16))
    helper = frieda_amd.Context(0)
    try:
        stride = (len(small) + 255) & ~255
        three = np.zeros((3, stride), dtype=np.uint8)
        three[:, : len(small)] = np.frombuffer(small, dtype=np.uint8)
        d_three, d_big = DevBuf.from_array(helper, three), DevBuf.from_array(helper, np.frombuffer(big, dtype=np.uint8))
        want_small = oracle.commit_and_generate_proof(small, 7, oracle.make_config(20, 4, 0, 20))

        def lone(ctx):
            ctx.prove_begin_device(d_three.ptr, len(small), 7, cfg)
            root, proof = ctx.prove_finish()
            assert (root, proof.serialize()) == (want_small[0], want_small[1].serialize())

        ws = frieda_amd.workspace_bytes(len(small), 4, 0)
        assert _arena_after(lone) == _rounded(ws) > 0

        def batch(ctx):
            got = ctx.commit_and_generate_proof_batch_device(d_three.ptr, stride, len(small), 3, [7, 7, 7], cfg)
            assert [(r, p.serialize()) for r, p in got] == [(want_small[0], want_small[1].serialize())] * 3

        assert 3 * ws <= _arena_after(batch) < 3 * ws + 2 * MIB

        with helper.encode(big, 4) as enc:
            want = [p.serialize() for p in helper.prove_seeds(enc, [5, 6], cfg)]
            got = _arena_after(lambda ctx: [p.serialize() for p in ctx.prove_seeds(enc, [5, 6], cfg)] == want or pytest.fail("other proofs"))
            assert got == _rounded(frieda_amd.seeds_workspace_bytes(len(big), cfg, 2)) > 0
        encs = helper.encode_batch([small, small[::-1]], 4)
        try:
            want = [[p.serialize() for p in row] for row in helper.prove_seeds_blobs(encs, [5, 6], cfg)]
            got = _arena_after(lambda ctx: [[p.serialize() for p in row] for row in ctx.prove_seeds_blobs(encs, [5, 6], cfg)] == want or pytest.fail("other proofs"))
            assert got == _rounded(frieda_amd.seeds_blobs_workspace_bytes(len(small), cfg, 2, 2)) > 0
        finally:
            for e in encs:
                e.close()

        root_big = oracle.commit(big, 4)
        got = _arena_after(lambda ctx: ctx.commit_batch_device(d_big.ptr, len(big), len(big), 1, 4) == [root_big] or pytest.fail("other root"))
        assert got == _rounded(frieda_amd.workspace_bytes(len(big), 4, prove=False)) > 0
        d_three.free()
        d_big.free()
    finally:
        helper.close()


# ---- history beyond the arena ------------------------------------------------------------------------------------------------------------
PROBE = ("prove/general", "prove/small_fused", "interpolate_points/lines", "verify_cells_many", "reconstruct_from_proof_pairs", "open_cells/small_fused")


def probe(ctx, oracle):
    """the calls of a handful of rows, one after the other on one context with its default options (2^8 coefficients: the line route)"""
    return tuple(norm(ROWS[name].run(ctx, oracle)) for name in PROBE)


@pytest.fixture(scope="module")
def r0(oracle):
    import frieda_amd

    ctx = frieda_amd.Context(0)
    try:
        return probe(ctx, oracle)
    finally:
        ctx.close()


@pytest.fixture()
def ctx():
    import frieda_amd

    c = frieda_amd.Context(0)
    yield c
    c.close()


def test_after_a_larger_call_of_another_shape_and_blowup(ctx, oracle, r0):
    noise = splitmix64_bytes(3, blob_len_for(18)).tobytes()  # 2^16 coefficients per column at blowup 2^2: more workspace than any probe call
    cfg = W.cfg_of(4, 2, 1, 30)
    root, proof = ctx.commit_and_generate_proof(noise, 9, cfg)
    assert root == oracle.commit(noise, 2)
    ctx.commit_and_generate_proof_batch([noise[:100000], noise[100000:200000]], [1, 2], cfg)
    assert probe(ctx, oracle) == r0


def test_after_release_workspace(ctx, oracle, r0):
    assert probe(ctx, oracle) == r0
    ctx.release_workspace()
    assert poison(ctx, 0xFFFFFFFF, sticky=1) == [0, 0, 0, 0], "release_workspace hands everything back"
    assert probe(ctx, oracle) == r0
    ctx.release_workspace()
    assert probe(ctx, oracle) == r0


def test_after_toggling_the_twiddle_cache(ctx, oracle, r0):
    ctx.set_twiddle_cache(False)
    assert probe(ctx, oracle) == r0
    poison(ctx, 0x7FFFFFFF)  # (the tables are scratch now: filled too)
    assert probe(ctx, oracle) == r0
    ctx.set_twiddle_cache(True)
    assert probe(ctx, oracle) == r0
    ctx.set_twiddle_cache(False)
    ctx.set_twiddle_cache(True)
    assert probe(ctx, oracle) == r0


def test_after_refused_calls_of_every_kind(ctx, oracle, r0):
    import frieda_amd

    data = W.BLOBS["ff_then_00"](blob_len_for(16))
    cfg = W.cfg_of(4, 4, 0, 20)

    def refused(call, status):
        with pytest.raises(frieda_amd.FriedaError) as e:
            call()
        assert e.value.status == status, e.value

    assert probe(ctx, oracle) == r0
    refused(lambda: ctx.commit(data, 99), 1)  # an argument error
    refused(lambda: ctx.commit_and_generate_proof(data, 1, W.cfg_of(4, 4, 0, 0)), 1)
    assert probe(ctx, oracle) == r0
    ctx.release_workspace()
    assert ctx._L.frieda_ctx_test_set_arena_limit(ctx._h, ctx._L.frieda_workspace_bytes(len(data), 4, 0, 1) // 2) == 0
    try:
        refused(lambda: ctx.commit_and_generate_proof(data, 1, cfg), 4)  # FRIEDA_ERR_NOMEM, after the smaller calls before it were planned
    finally:
        assert ctx._L.frieda_ctx_test_set_arena_limit(ctx._h, 0) == 0
    assert probe(ctx, oracle) == r0
    refused(lambda: ctx.commit_and_generate_proof(data, 1, W.cfg_of(4, 4, 11, 20)), 1)  # a last layer the device channel does not take
    assert probe(ctx, oracle) == r0
    ctx.prove_begin(data, 1, cfg)
    refused(lambda: ctx.commit(data, 4), 1)  # a proof is in flight
    refused(lambda: ctx.encode(data, 4), 1)
    ctx.prove_finish()
    assert probe(ctx, oracle) == r0


def test_after_a_rejected_proof_in_verify_many(ctx, oracle, r0):
    from test_gpu_value_edges import _bump_evaluation

    _, root, seeds, proofs = W._kib_proofs(oracle)
    bad = [_bump_evaluation(p) for p in proofs[:4]]
    assert list(ctx.verify_many(bad, seeds[:4])) == [0, 0, 0, 0]
    st, pts = ctx.verify_pairs_many(bad + proofs[4:6], seeds[:6], expected_commitment=root)
    assert list(st) == [0, 0, 0, 0, 1, 1]
    assert probe(ctx, oracle) == r0


# ---- frieda_multi: the hook set through the slot's context reaches both of its contexts --------------------------------------------------
def test_multi_prove_many_and_commit_many_on_poisoned_slots(oracle):
    import frieda_amd
    from test_gpu_value_edges import oracle_proof

    kinds = list(W.BLOBS) * 2
    blobs = [W.BLOBS[k](blob_len_for(16)) for k in kinds]
    want = [oracle_proof(oracle, k, "2p16") for k in kinds]
    cfg = W.cfg_of(4, 4, 0, 20)
    mc = frieda_amd.MultiContext([0])
    try:
        slot = C.c_void_p(mc._L.frieda_multi_ctx(mc._h, 0))

        def check(what):
            got = mc.prove_many(blobs, [W.SEED] * len(blobs), cfg)
            assert [(r, p.serialize()) for r, p in got] == want, what
            assert mc.commit_many(blobs, 4) == [r for r, _ in want], what

        check("R0")
        for word in WORDS:
            out = (C.c_uint64 * 4)()
            assert mc._L.frieda_ctx_test_poison(slot, word, 1, out) == 0
            assert out[0] >= mc._L.frieda_workspace_bytes(len(blobs[0]), 4, 0, 1), "the slot's first context ran the calls before: it has their arena"
            check((word, "poisoned workspace"))
            mc.release_workspace()  # the next calls allocate afresh: both contexts of the slot under the sticky flag
            check((word, "poisoned new allocations"))
    finally:
        mc.close()
