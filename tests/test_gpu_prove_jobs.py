"""GPU: any list of (handle, seed) jobs in one call (Context.prove_jobs, frieda_prove_jobs), cut into passes.

got[j] must serialise to the bytes of the ordinary proof of the job's blob under the job's seed, in the caller's order.  The expected
bytes never come from the new call: they are the reference of test_gpu_prove_seeds_blobs (the oracle up to 2^13,
`commit_and_generate_proof_device` above), computed once per shape and shared with that file.

Shapes (B = 4, last = 0): 2^5 (the circle fold inside the tail is the only fold), 2^8 (tail), 2^11 and 2^13 (narrow multi-workgroup
launches), 2^18 (register-subtree launch: the only one that reaches the seed-looped kernel).

The list: four handles — 0 to 2 are the reference's blobs, 3 is blob 0 encoded again and named by no job — and nine unsorted jobs.  Blob
2 has five (groups of 2 and 4 end short, a group of 8 exceeds the run), blob 1 one, blob 0 three with one pair twice.
Every test runs once under its own SIGALRM limit."""
import ctypes as C

import pytest

import workspace_rows as W
from test_gpu_prove_seeds_blobs import CFG, K, SEEDS, _cfg, _close, _time_limit, _want, reference  # noqa: F401  (_time_limit: autouse here too)
from test_gpu_workspace_history import _rounded

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_NOMEM = 1, 4
LOGS = [5, 8, 11, 13, 18]
GROUPS = (0, 2, 4, 8)
BLOB_OF = [0, 1, 2, 0]  # the blob each handle encodes
JOBS = [(2, 11), (0, 13), (2, 2**64 - 1), (1, 11), (0, 11), (2, 13), (2, 0), (0, 11), (2, 11)]
JOBS11 = JOBS + [(3, 13), (1, 0)]
assert K == 3 and {s for _, s in JOBS11} <= set(SEEDS)


def _handles(ctx, blobs):
    return ctx.encode_batch(blobs, CFG[1]) + [ctx.encode(blobs[0], CFG[1])]


def _expect(want, jobs, blob_of=BLOB_OF):
    return [want[blob_of[b]][SEEDS.index(s)] for b, s in jobs]


def _ser(proofs):
    return [p.serialize() for p in proofs]


@pytest.mark.parametrize("host_decommit", [0, 1])
@pytest.mark.parametrize("log_domain", LOGS)
def test_list_equals_the_ordinary_proofs_on_every_route(oracle, log_domain, host_decommit):
    import frieda_amd

    ctx = frieda_amd.Context(0)
    try:
        blobs, want = reference(ctx, oracle, log_domain)
        encs = _handles(ctx, blobs)
        ctx.set_option("FRIEDA_HOST_DECOMMIT", host_decommit)
        expect = _expect(want, JOBS)
        for group in GROUPS:
            ctx.set_option("FRIEDA_SEEDS_FOLD_GROUP", group)
            got = _ser(ctx.prove_jobs(encs, JOBS, _cfg(*CFG)))
            assert len(got) == len(JOBS)
            for j, job in enumerate(JOBS):
                assert got[j] == expect[j], f"job {j} {job}, group {group}"
            assert got[4] == got[7] and got[0] == got[8]  # the repeated pairs
            ctx.prove_jobs_begin(encs, JOBS, _cfg(*CFG))
            assert _ser(ctx.prove_jobs_finish()) == expect, group
        _close(encs)
    finally:
        ctx.close()


@pytest.mark.parametrize("log_domain", [11, 18])
def test_relations_to_the_calls_that_exist(gpu_ctx, oracle, log_domain):
    import frieda_amd

    blobs, want = reference(gpu_ctx, oracle, log_domain)
    pcs = _cfg(*CFG)
    encs = gpu_ctx.encode_batch(blobs, CFG[1])
    try:
        for group in (0, 4):
            gpu_ctx.set_option("FRIEDA_SEEDS_FOLD_GROUP", group)
            # the rectangle's list
            rect = [(b, s) for b in range(K) for s in SEEDS]
            block = gpu_ctx.prove_seeds_blobs(encs, SEEDS, pcs)
            flat = [p.serialize() for row in block for p in row]
            assert _ser(frieda_amd.prove_jobs(gpu_ctx, encs, rect, pcs)) == flat == [x for row in want for x in row], group
            # one blob
            assert _ser(gpu_ctx.prove_jobs(encs[1:2], [(0, s) for s in SEEDS], pcs)) == _ser(gpu_ctx.prove_seeds(encs[1], SEEDS, pcs)) == want[1], group
            # one job
            assert _ser(gpu_ctx.prove_jobs(encs, [(2, SEEDS[2])], pcs)) == [want[2][2]], group
            # descending blob order == ascending, permuted back
            down = [(2, 11), (2, 13), (1, 0), (1, 11), (0, 13), (0, 2**64 - 1)]
            up = down[::-1]
            got_down, got_up = _ser(gpu_ctx.prove_jobs(encs, down, pcs)), _ser(gpu_ctx.prove_jobs(encs, up, pcs))
            assert got_down == got_up[::-1] == _expect(want, down), group
    finally:
        gpu_ctx.set_option("FRIEDA_SEEDS_FOLD_GROUP", 0)
        _close(encs)


@pytest.mark.parametrize("log_domain", [11, 18])
def test_handles_of_mixed_origin(gpu_ctx, oracle, log_domain):
    """handles 0 and 1 from one encode_batch, handles 2 and 3 from lone encodes"""
    blobs, want = reference(gpu_ctx, oracle, log_domain)
    pcs = _cfg(*CFG)
    pair = gpu_ctx.encode_batch(blobs[:2], CFG[1])
    lone = [gpu_ctx.encode(blobs[2], CFG[1]), gpu_ctx.encode(blobs[0], CFG[1])]
    try:
        for group in (0, 4):
            gpu_ctx.set_option("FRIEDA_SEEDS_FOLD_GROUP", group)
            assert _ser(gpu_ctx.prove_jobs(pair + lone, JOBS, pcs)) == _expect(want, JOBS), group
            # the same handle at two positions of the list
            twice = [lone[0], pair[0], lone[0], pair[1]]
            assert _ser(gpu_ctx.prove_jobs(twice, JOBS, pcs)) == _expect(want, JOBS, [2, 0, 2, 1]), group
    finally:
        gpu_ctx.set_option("FRIEDA_SEEDS_FOLD_GROUP", 0)
        _close(pair + lone)


@pytest.mark.parametrize("host_decommit", [0, 1])
def test_handles_encoded_under_different_skip_thresholds(oracle, host_decommit):
    """2^18: the trees of handles 0 and 2 lack the two levels above their leaves, those of handles 1 and 3 hold every level"""
    import frieda_amd

    ctx = frieda_amd.Context(0)
    try:
        blobs, want = reference(ctx, oracle, 18)
        pcs = _cfg(*CFG)

        def encode(data, skip):
            ctx.set_option("FRIEDA_TREE_SKIP_LOG", skip)
            ctx.set_option("FRIEDA_TREE_SKIP_LONE_LOG", skip)
            return ctx.encode(data, CFG[1])

        encs = [encode(blobs[0], 12), encode(blobs[1], 40), encode(blobs[2], 12), encode(blobs[0], 40)]
        for at_prove in (12, 40):
            ctx.set_option("FRIEDA_TREE_SKIP_LOG", at_prove)
            ctx.set_option("FRIEDA_TREE_SKIP_LONE_LOG", at_prove)
            ctx.set_option("FRIEDA_HOST_DECOMMIT", host_decommit)
            for group in (0, 4):
                ctx.set_option("FRIEDA_SEEDS_FOLD_GROUP", group)
                assert _ser(ctx.prove_jobs(encs, JOBS, pcs)) == _expect(want, JOBS), (at_prove, group)
                assert _ser(ctx.prove_jobs(encs, JOBS11, pcs)) == _expect(want, JOBS11), (at_prove, group)
        _close(encs)
    finally:
        ctx.close()


def _passes(jobs, n_blobs, per_pass):
    """the written rule: the jobs sorted by blob (stable), ceil(n / per_pass) passes of sizes equal to within one -> [(distinct blobs, jobs)]"""
    order = sorted(range(len(jobs)), key=lambda j: jobs[j][0])
    n_passes = -(-len(jobs) // per_pass)
    out, at = [], 0
    for i in range(n_passes):
        size = len(jobs) // n_passes + (1 if i < len(jobs) % n_passes else 0)
        out.append((len({jobs[j][0] for j in order[at:at + size]}), size))
        at += size
    assert at == len(jobs)
    return out


@pytest.mark.parametrize("group", [0, 4])
def test_passes(gpu_ctx, oracle, group):
    """2^13, the handles encoded on another context (an encode's own arena would hide the call's): the plan, the bytes and the arena under
    four limits"""
    import frieda_amd

    blobs, want = reference(gpu_ctx, oracle, 13)
    pcs = _cfg(*CFG)
    length = len(blobs[0])
    encs = _handles(gpu_ctx, blobs)
    ws = lambda kb, p: frieda_amd.prove_jobs_workspace_bytes(length, pcs, kb, p)
    four, one = ws(4, 4), ws(1, 1)
    assert 0 < one < ws(3, 3) < four
    try:
        for limit, per_pass in ((four, 4), (four - 1, 3), (one, 1)):
            for jobs in (JOBS, JOBS11):
                ctx = frieda_amd.Context(0)
                try:
                    ctx.set_option("FRIEDA_SEEDS_FOLD_GROUP", group)
                    assert ctx._L.frieda_ctx_test_set_arena_limit(ctx._h, limit) == 0
                    n_passes = -(-len(jobs) // per_pass)
                    assert frieda_amd.prove_jobs_plan(length, pcs, 4, len(jobs), ctx=ctx) == (per_pass, n_passes)
                    if per_pass == 4:
                        assert n_passes == 3
                    assert _ser(ctx.prove_jobs(encs, jobs, pcs)) == _expect(want, jobs), (limit, len(jobs))
                    largest = max(ws(kb, p) for kb, p in _passes(jobs, 4, per_pass))
                    assert largest <= limit
                    assert W.poison(ctx, 0xDEADBEEF, sticky=0)[0] == _rounded(largest), (limit, len(jobs))
                finally:
                    ctx.close()
        # not even one job fits: the error reaches the caller, no proof comes back, and the context works once the limit is lifted
        ctx = frieda_amd.Context(0)
        try:
            ctx.set_option("FRIEDA_SEEDS_FOLD_GROUP", group)
            assert ctx._L.frieda_ctx_test_set_arena_limit(ctx._h, one - 1) == 0
            assert frieda_amd.prove_jobs_plan(length, pcs, 4, len(JOBS), ctx=ctx) == (1, len(JOBS))
            n_blobs, n_jobs, handles, bidx, seeds = ctx._jobs_arrays(encs, JOBS)
            outs = (C.c_void_p * n_jobs)(*([1] * n_jobs))
            assert ctx._L.frieda_prove_jobs(ctx._h, handles, n_blobs, bidx, seeds, n_jobs, pcs._c(), outs) == ERR_NOMEM
            assert [outs[j] for j in range(n_jobs)] == [None] * n_jobs
            assert ctx._L.frieda_ctx_test_set_arena_limit(ctx._h, 0) == 0
            assert _ser(ctx.prove_jobs(encs, JOBS, pcs)) == _expect(want, JOBS)
            phases = ctx.last_prove_phases()
            assert 0 < phases["enqueued"] <= phases["device_done"] <= phases["assembled"]
        finally:
            ctx.close()
    finally:
        _close(encs)


def test_begin_and_finish_are_one_pass_and_only_read_the_handles(gpu_ctx, oracle):
    import frieda_amd

    log_domain = 13
    blobs, want = reference(gpu_ctx, oracle, log_domain)
    pcs = _cfg(*CFG)
    length = len(blobs[0])
    other = frieda_amd.Context(0)
    encs = _handles(gpu_ctx, blobs)
    try:
        cells = [0, 5, (1 << (log_domain - 2)) - 1]
        before = [(e.commitment, [a.tobytes() for a in e.open_cells(gpu_ctx, 2, cells)]) for e in encs]
        assert [c for c, _ in before] == [oracle.commit(blobs[b], CFG[1]) for b in BLOB_OF]
        # a list above the limit: NOMEM from _begin, no passes, the context usable afterwards
        ws = frieda_amd.prove_jobs_workspace_bytes(length, pcs, 4, len(JOBS))
        assert other._L.frieda_ctx_test_set_arena_limit(other._h, ws - 1) == 0
        with pytest.raises(frieda_amd.FriedaError) as ei:
            other.prove_jobs_begin(encs, JOBS, pcs)
        assert ei.value.status == ERR_NOMEM
        assert _ser(other.prove_jobs(encs, JOBS, pcs)) == _expect(want, JOBS)  # (the synchronous form cuts the same list into passes)
        assert other._L.frieda_ctx_test_set_arena_limit(other._h, ws) == 0
        other.prove_jobs_begin(encs, JOBS, pcs)  # the planned size is enough
        assert _ser(other.prove_jobs_finish()) == _expect(want, JOBS)
        assert other._L.frieda_ctx_test_set_arena_limit(other._h, 0) == 0
        # two contexts in flight from the same handles with different lists
        gpu_ctx.prove_jobs_begin(encs, JOBS, pcs)
        other.prove_jobs_begin(encs, JOBS11[::-1], pcs)
        assert _ser(other.prove_jobs_finish()) == _expect(want, JOBS11[::-1])
        assert _ser(gpu_ctx.prove_jobs_finish()) == _expect(want, JOBS)
        assert [(e.commitment, [a.tobytes() for a in e.open_cells(other, 2, cells)]) for e in encs] == before
    finally:
        _close(encs)
        other.close()


def test_statuses(oracle, blob):
    import frieda_amd
    from frieda_amd.api import _check
    from test_gpu_prove_seeds_blobs import HOST_CASE
    from util import resolve_input

    ctx = frieda_amd.Context(0)
    try:
        blobs, want = reference(ctx, oracle, 8)
        other_len, _ = reference(ctx, oracle, 11)
        pcs = _cfg(*CFG)
        encs = _handles(ctx, blobs)
        longer = ctx.encode(other_len[0], CFG[1])  # another length
        wider = ctx.encode(blobs[0], 3)  # the same length, another blow-up
        L, h = ctx._L, ctx._h
        n_blobs, n_jobs, good, bidx, seeds = ctx._jobs_arrays(encs, JOBS)
        outs = (C.c_void_p * 65536)()

        def table(es):
            return (C.c_void_p * len(es))(*[e._handle() if e is not None else None for e in es])

        def refused(call, status=ERR_ARG):
            with pytest.raises(frieda_amd.FriedaError) as ei:
                call()
            assert ei.value.status == status, ei.value
            assert _ser(ctx.prove_jobs(encs, JOBS[:4], pcs)) == _expect(want, JOBS[:4])  # the context works afterwards

        for fn, tail in ((L.frieda_prove_jobs, (outs,)), (L.frieda_prove_jobs_begin, ())):
            refused(lambda: _check(fn(h, None, n_blobs, bidx, seeds, n_jobs, pcs._c(), *tail), h))  # a null list
            refused(lambda: _check(fn(h, table([encs[0], None, encs[2], encs[3]]), n_blobs, bidx, seeds, n_jobs, pcs._c(), *tail), h))  # a null handle
            refused(lambda: _check(fn(h, good, n_blobs, None, seeds, n_jobs, pcs._c(), *tail), h))  # null blob_index
            refused(lambda: _check(fn(h, good, n_blobs, bidx, None, n_jobs, pcs._c(), *tail), h))  # null seeds
            refused(lambda: _check(fn(h, good, 0, bidx, seeds, n_jobs, pcs._c(), *tail), h))  # n_blobs 0
            refused(lambda: _check(fn(h, good, n_blobs, bidx, seeds, 0, pcs._c(), *tail), h))  # n_jobs 0
            refused(lambda: _check(fn(h, good, 2, bidx, seeds, n_jobs, pcs._c(), *tail), h))  # an index equal to n_blobs
        refused(lambda: _check(L.frieda_prove_jobs(h, good, n_blobs, bidx, seeds, n_jobs, pcs._c(), None), h))  # null out_proofs
        refused(lambda: _check(L.frieda_prove_jobs_finish(h, None), h))
        many_idx = (C.c_uint32 * 65536)()
        many_seeds = (C.c_uint64 * 65536)(*range(65536))
        refused(lambda: _check(L.frieda_prove_jobs_begin(h, good, n_blobs, many_idx, many_seeds, 65536, pcs._c()), h))  # only a pass has the cap
        refused(lambda: ctx.prove_jobs([encs[0], longer], JOBS[1:2], pcs))  # two lengths
        refused(lambda: ctx.prove_jobs([encs[0], wider], JOBS[1:2], pcs))  # two blow-ups
        refused(lambda: ctx.prove_jobs(encs, JOBS, _cfg(CFG[0], 3, CFG[2], CFG[3])))  # cfg's blow-up is not the handles'
        refused(lambda: ctx.prove_jobs(encs, JOBS, _cfg(CFG[0], 4, 11, CFG[3])))  # the rules of prove_seeds_begin
        refused(lambda: ctx.prove_jobs(encs, JOBS, _cfg(CFG[0], 4, 0, 0)))
        refused(lambda: ctx.prove_jobs_finish())  # nothing in flight
        # a begin, of either form, while a job is in flight
        ctx.prove_jobs_begin(encs, JOBS, pcs)
        for call in (lambda: ctx.prove_jobs_begin(encs, JOBS, pcs), lambda: ctx.prove_jobs(encs, JOBS, pcs), lambda: ctx.prove_seeds_begin(encs[0], SEEDS, pcs)):
            with pytest.raises(frieda_amd.FriedaError) as ei:
                call()
            assert ei.value.status == ERR_ARG
        assert _ser(ctx.prove_jobs_finish()) == _expect(want, JOBS)
        # the host-channel policy: two jobs refused, one job accepted
        ctx.set_host_channel(True)
        try:
            for call in (lambda: ctx.prove_jobs(encs, JOBS[:2], pcs), lambda: ctx.prove_jobs_begin(encs, JOBS[:2], pcs)):
                with pytest.raises(frieda_amd.FriedaError) as ei:
                    call()
                assert ei.value.status == ERR_ARG
            assert _ser(ctx.prove_jobs(encs, JOBS[:1], pcs)) == _expect(want, JOBS[:1])
            ctx.prove_jobs_begin(encs, JOBS[:1], pcs)
            assert _ser(ctx.prove_jobs_finish()) == _expect(want, JOBS[:1])
        finally:
            ctx.set_host_channel(False)
        # ... and a shape whose last layer needs the host channel under either policy
        spec, seed, cfg = HOST_CASE
        data = resolve_input(spec, blob)
        enc = ctx.encode(data, cfg[1])
        try:
            lone = ctx.commit_and_generate_proof(data, seed, _cfg(*cfg))[1].serialize()
            assert _ser(ctx.prove_jobs([enc], [(0, seed)], _cfg(*cfg))) == [lone]
            with pytest.raises(frieda_amd.FriedaError) as ei:
                ctx.prove_jobs([enc, enc], [(0, seed), (1, seed)], _cfg(*cfg))
            assert ei.value.status == ERR_ARG
        finally:
            enc.close()
        assert _ser(ctx.prove_jobs(encs, JOBS, pcs)) == _expect(want, JOBS)
        _close(encs + [longer, wider])
    finally:
        ctx.close()


@pytest.mark.parametrize("log_domain", [10, 18])
def test_same_bytes_on_a_poisoned_context_and_a_callers_stream(oracle, log_domain):
    import torch

    import frieda_amd

    stream = torch.cuda.Stream()
    pcs = _cfg(*CFG)
    for make in (lambda: frieda_amd.Context(0), lambda: frieda_amd.Context(0, stream=stream.cuda_stream)):
        ctx = make()
        try:
            blobs, want = reference(ctx, oracle, log_domain)
            encs = _handles(ctx, blobs)
            expect = _expect(want, JOBS)
            for word in (None, 0x00000000, 0xFFFFFFFF, 0x7FFFFFFF):
                if word is not None:
                    W.poison(ctx, word)  # the sticky mode: every later allocation of the context is filled too
                for group in (0, 4):
                    ctx.set_option("FRIEDA_SEEDS_FOLD_GROUP", group)
                    assert _ser(ctx.prove_jobs(encs, JOBS, pcs)) == expect, (word, group)
            _close(encs)
        finally:
            ctx.close()


def test_every_proof_verifies_under_its_own_seed_only(gpu_ctx, oracle):
    import frieda_amd

    blobs, _ = reference(gpu_ctx, oracle, 11)
    jobs = [(2, 21), (0, 22), (2, 23), (1, 24), (3, 25), (2, 26), (0, 27)]
    encs = _handles(gpu_ctx, blobs)
    try:
        proofs = gpu_ctx.prove_jobs(encs, jobs, _cfg(*CFG))
        roots = [e.commitment for e in encs]
    finally:
        _close(encs)
    assert len(set(roots)) == K and roots[3] == roots[0]
    for j, (p, (b, seed)) in enumerate(zip(proofs, jobs)):
        assert p.layer(0)["commitment"] == roots[b], j
        assert frieda_amd.verify(p, seed), j
        assert not frieda_amd.verify(p, jobs[(j + 1) % len(jobs)][1]), j
