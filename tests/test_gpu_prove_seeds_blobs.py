"""GPU: a block of encoded blobs proved under one seed list in one call (Context.prove_seeds_blobs, frieda_prove_seeds_blobs).

proofs[b][s] must serialise to the bytes of the ordinary proof of blob b under seeds[s].  The expected bytes never come from the new
call: the oracle gives them for domains up to 2^13, `commit_and_generate_proof_device` per (blob, seed) above.  A reference is computed
once per shape and shared by the tests of this file.

Shapes (B = 4, last = 0): 2^5 (the circle fold inside the tail is the only fold), 2^8 and 2^10 (tail), 2^11 and 2^13 (narrow
multi-workgroup launches), 2^18 (register-subtree launch and the seed-looped kernel), and one PROVE_CASES shape with B != 4, last != 0.
Every test runs once under its own SIGALRM limit."""
import ctypes as C
import signal

import numpy as np
import pytest

import workspace_rows as W
from conftest import splitmix64_bytes
from test_gpu_parity import PROVE_CASES
from util import DevBuf, blob_len_for, resolve_input

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_NOMEM = 1, 4
TAIL_LOG = 11
K = 3
SEEDS = [11, 2**64 - 1, 13, 11, 0]  # S = 5, one seed repeated: groups of 2 and 4 do not divide 5, a group of 8 exceeds it
CFG = (8, 4, 0, 20)  # pow_bits, B, last, queries
LOGS = [5, 8, 10, 11, 13, 18]
GROUPS = (0, 2, 4, 8)
ODD_CASE = next(c for c in PROVE_CASES if c[2][1] != 4 and c[2][2] != 0 and c[2][1] + c[2][2] <= TAIL_LOG)  # ("pattern:300", 9, (8, 2, 1, 12))
HOST_CASE = next(c for c in PROVE_CASES if c[2][1] + c[2][2] > TAIL_LOG)


@pytest.fixture(autouse=True)
def _time_limit(request):
    """one run per test, ended by SIGALRM after its limit"""
    limit = getattr(request.function, "time_limit", 120)

    def on_alarm(signum, frame):
        raise TimeoutError(f"{request.node.name}: over its {limit} s limit")

    old = signal.signal(signal.SIGALRM, on_alarm)
    signal.alarm(limit)
    try:
        yield
    finally:
        signal.alarm(0)
        signal.signal(signal.SIGALRM, old)


def _cfg(pow_bits, B, last, nq):
    import frieda_amd

    return frieda_amd.PcsConfig(frieda_amd.FriConfig(B, last, nq), pow_bits)


def _ser(block):
    return [[p.serialize() for p in row] for row in block]


_REF = {}


def reference(ctx, oracle, log_domain):
    """(blobs, want) of a shape, computed once: K distinct blobs that exactly fill a 2^log_domain domain, want[b][s] = the ordinary
    proof of blob b under SEEDS[s], from code the block call does not run"""
    if log_domain not in _REF:
        length = blob_len_for(log_domain)
        blobs = [splitmix64_bytes(9100 + 16 * log_domain + b, length).tobytes() for b in range(K)]
        _REF[log_domain] = (blobs, _want(ctx, oracle, blobs, SEEDS, CFG, log_domain <= 13))
    return _REF[log_domain]


def _want(ctx, oracle, blobs, seeds, cfg, from_oracle):
    pcs = _cfg(*cfg)
    want = []
    for data in blobs:
        by_seed = {}
        if from_oracle:
            for s in set(seeds):
                by_seed[s] = oracle.commit_and_generate_proof(data, s, oracle.make_config(*cfg))[1].serialize()
        else:
            d = DevBuf.from_array(ctx, np.frombuffer(data, dtype=np.uint8))
            try:
                for s in set(seeds):
                    by_seed[s] = ctx.commit_and_generate_proof_device(d.ptr, len(data), s, pcs)[1].serialize()
            finally:
                d.free()
        want.append([by_seed[s] for s in seeds])
    return want


def _close(encs):
    for e in encs:
        e.close()


@pytest.mark.parametrize("host_decommit", [0, 1])
@pytest.mark.parametrize("log_domain", LOGS)
def test_block_equals_the_ordinary_proofs_on_every_route(oracle, log_domain, host_decommit):
    """K = 3 distinct blobs x S = 5 seeds; route A and the seed groups 2, 4 (the straddling case: a group must end with its blob) and 8"""
    import frieda_amd

    ctx = frieda_amd.Context(0)
    try:
        blobs, want = reference(ctx, oracle, log_domain)
        encs = ctx.encode_batch(blobs, CFG[1])
        ctx.set_option("FRIEDA_HOST_DECOMMIT", host_decommit)
        for group in GROUPS:
            ctx.set_option("FRIEDA_SEEDS_FOLD_GROUP", group)
            got = _ser(ctx.prove_seeds_blobs(encs, SEEDS, _cfg(*CFG)))
            assert len(got) == K and all(len(r) == len(SEEDS) for r in got)
            for b in range(K):
                for s in range(len(SEEDS)):
                    assert got[b][s] == want[b][s], f"blob {b}, seed index {s}, group {group}"
            assert got[1][0] == got[1][3]  # the repeated seed
        _close(encs)
    finally:
        ctx.close()


def test_block_of_a_shape_with_another_blowup_and_last_layer(gpu_ctx, oracle, blob):
    spec, _, cfg = ODD_CASE
    base = resolve_input(spec, blob)
    blobs = [bytes((x + 37 * b) & 0xFF for x in base) for b in range(K)]
    want = _want(gpu_ctx, oracle, blobs, SEEDS, cfg, True)
    encs = gpu_ctx.encode_batch(blobs, cfg[1])
    try:
        for group in (0, 4):
            gpu_ctx.set_option("FRIEDA_SEEDS_FOLD_GROUP", group)
            assert _ser(gpu_ctx.prove_seeds_blobs(encs, SEEDS, _cfg(*cfg))) == want, group
    finally:
        gpu_ctx.set_option("FRIEDA_SEEDS_FOLD_GROUP", 0)
        _close(encs)


@pytest.mark.parametrize("log_domain", [11, 18])
def test_handles_of_mixed_origin_and_a_handle_listed_twice(gpu_ctx, oracle, log_domain):
    """handles 0 and 1 from one encode_batch, handle 2 from a lone encode; then the same handle twice in the list"""
    import frieda_amd

    blobs, want = reference(gpu_ctx, oracle, log_domain)
    pcs = _cfg(*CFG)
    pair = gpu_ctx.encode_batch(blobs[:2], CFG[1])
    lone = gpu_ctx.encode(blobs[2], CFG[1])
    try:
        for group in (0, 4):
            gpu_ctx.set_option("FRIEDA_SEEDS_FOLD_GROUP", group)
            assert _ser(gpu_ctx.prove_seeds_blobs(pair + [lone], SEEDS, pcs)) == want, group
            assert _ser(frieda_amd.prove_seeds_blobs(gpu_ctx, [lone, pair[0], lone, pair[1]], SEEDS, pcs)) == [want[2], want[0], want[2], want[1]], group
    finally:
        gpu_ctx.set_option("FRIEDA_SEEDS_FOLD_GROUP", 0)
        _close(pair + [lone])


@pytest.mark.parametrize("host_decommit", [0, 1])
def test_handles_encoded_under_different_skip_thresholds(oracle, host_decommit):
    """2^18: handle 0's tree lacks the two levels above its leaves, handle 1's holds every level; both ways round in the list, and the
    skipping handle listed twice (the host fallback completes a tree once per distinct blob)"""
    import frieda_amd

    log_domain = 18
    ctx = frieda_amd.Context(0)
    try:
        blobs, want = reference(ctx, oracle, log_domain)
        pcs = _cfg(*CFG)

        def encode(data, skip):
            ctx.set_option("FRIEDA_TREE_SKIP_LOG", skip)
            ctx.set_option("FRIEDA_TREE_SKIP_LONE_LOG", skip)
            return ctx.encode(data, CFG[1])

        skipping, full = encode(blobs[0], 12), encode(blobs[1], 40)
        for at_prove in (12, 40):
            ctx.set_option("FRIEDA_TREE_SKIP_LOG", at_prove)
            ctx.set_option("FRIEDA_TREE_SKIP_LONE_LOG", at_prove)
            ctx.set_option("FRIEDA_HOST_DECOMMIT", host_decommit)
            for group in (0, 4):
                ctx.set_option("FRIEDA_SEEDS_FOLD_GROUP", group)
                assert _ser(ctx.prove_seeds_blobs([skipping, full], SEEDS, pcs)) == want[:2], (at_prove, group)
                assert _ser(ctx.prove_seeds_blobs([full, skipping, skipping], SEEDS, pcs)) == [want[1], want[0], want[0]], (at_prove, group)
        _close([skipping, full])
    finally:
        ctx.close()


@pytest.mark.parametrize("log_domain", [8, 13])
def test_one_blob_and_one_seed(gpu_ctx, oracle, log_domain):
    blobs, want = reference(gpu_ctx, oracle, log_domain)
    pcs = _cfg(*CFG)
    encs = gpu_ctx.encode_batch(blobs, CFG[1])
    try:
        one = gpu_ctx.prove_seeds_blobs(encs[1:2], SEEDS, pcs)  # K = 1 is prove_seeds
        assert _ser(one) == [want[1]] == [[p.serialize() for p in gpu_ctx.prove_seeds(encs[1], SEEDS, pcs)]]
        col = gpu_ctx.prove_seeds_blobs(encs, SEEDS[1:2], pcs)  # S = 1: three lone proofs
        assert _ser(col) == [[want[b][1]] for b in range(K)]
        assert _ser(gpu_ctx.prove_seeds_blobs(encs[2:], SEEDS[2:3], pcs)) == [[want[2][2]]]
    finally:
        _close(encs)


def test_host_channel_one_job_works_more_are_refused(gpu_ctx, blob):
    import frieda_amd

    spec, seed, cfg = HOST_CASE
    data = resolve_input(spec, blob)
    pcs = _cfg(*cfg)
    want = gpu_ctx.commit_and_generate_proof(data, seed, pcs)[1].serialize()
    enc = gpu_ctx.encode(data, cfg[1])
    try:
        for host_channel in (False, True):
            gpu_ctx.set_host_channel(host_channel)
            try:
                assert _ser(gpu_ctx.prove_seeds_blobs([enc], [seed], pcs)) == [[want]], host_channel  # K = S = 1, both policies
                for encs, seeds in (([enc, enc], [seed]), ([enc], [seed, seed + 1]), ([enc, enc], [seed, seed + 1])):
                    with pytest.raises(frieda_amd.FriedaError) as ei:
                        gpu_ctx.prove_seeds_blobs(encs, seeds, pcs)
                    assert ei.value.status == ERR_ARG
            finally:
                gpu_ctx.set_host_channel(False)
    finally:
        enc.close()


def test_host_channel_policy_refuses_a_block_of_a_small_shape(gpu_ctx, oracle):
    import frieda_amd

    blobs, want = reference(gpu_ctx, oracle, 8)
    pcs = _cfg(*CFG)
    encs = gpu_ctx.encode_batch(blobs, CFG[1])
    gpu_ctx.set_host_channel(True)
    try:
        assert _ser(gpu_ctx.prove_seeds_blobs(encs[:1], SEEDS[:1], pcs)) == [[want[0][0]]]
        with pytest.raises(frieda_amd.FriedaError) as ei:
            gpu_ctx.prove_seeds_blobs(encs, SEEDS, pcs)
        assert ei.value.status == ERR_ARG
    finally:
        gpu_ctx.set_host_channel(False)
        _close(encs)
    # the refusal left nothing in flight
    encs = gpu_ctx.encode_batch(blobs, CFG[1])
    try:
        assert _ser(gpu_ctx.prove_seeds_blobs(encs, SEEDS, pcs)) == want
    finally:
        _close(encs)


def test_handles_are_only_read(gpu_ctx, oracle):
    """commitments and opened cells before == after; a second context proves from the same handles, both jobs in flight at once"""
    import frieda_amd

    log_domain = 13
    blobs, want = reference(gpu_ctx, oracle, log_domain)
    pcs = _cfg(*CFG)
    other = frieda_amd.Context(0)
    encs = gpu_ctx.encode_batch(blobs, CFG[1])
    try:
        cells = [0, 5, (1 << (log_domain - 2)) - 1]
        before = [(e.commitment, [a.tobytes() for a in e.open_cells(gpu_ctx, 2, cells)]) for e in encs]
        assert [c for c, _ in before] == [oracle.commit(d, CFG[1]) for d in blobs]
        gpu_ctx.prove_seeds_blobs_begin(encs, SEEDS, pcs)
        other.prove_seeds_blobs_begin(encs[::-1], SEEDS, pcs)
        assert _ser(other.prove_seeds_blobs_finish()) == want[::-1]
        assert _ser(gpu_ctx.prove_seeds_blobs_finish()) == want
        assert [(e.commitment, [a.tobytes() for a in e.open_cells(other, 2, cells)]) for e in encs] == before
        assert _ser(other.prove_seeds_blobs(encs, SEEDS, pcs)) == want
    finally:
        _close(encs)
        other.close()


def test_every_proof_verifies_under_its_own_seed_only(gpu_ctx, oracle):
    import frieda_amd

    blobs, _ = reference(gpu_ctx, oracle, 11)
    seeds = [21, 22, 23, 24, 25]
    encs = gpu_ctx.encode_batch(blobs, CFG[1])
    try:
        block = gpu_ctx.prove_seeds_blobs(encs, seeds, _cfg(*CFG))
        roots = [e.commitment for e in encs]
    finally:
        _close(encs)
    assert len(set(roots)) == K
    for b, row in enumerate(block):
        for s, p in enumerate(row):
            assert p.layer(0)["commitment"] == roots[b], (b, s)
            assert frieda_amd.verify(p, seeds[s]), (b, s)
            assert not frieda_amd.verify(p, seeds[(s + 1) % len(seeds)]), (b, s)


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
            encs = ctx.encode_batch(blobs, CFG[1])
            for word in (None, 0x00000000, 0xFFFFFFFF, 0x7FFFFFFF):
                if word is not None:
                    W.poison(ctx, word)  # the sticky mode: every later allocation of the context is filled too
                for group, host_decommit in ((0, 0), (4, 0), (4, 1)):
                    ctx.set_option("FRIEDA_SEEDS_FOLD_GROUP", group)
                    ctx.set_option("FRIEDA_HOST_DECOMMIT", host_decommit)
                    assert _ser(ctx.prove_seeds_blobs(encs, SEEDS, pcs)) == want, (word, group, host_decommit)
            _close(encs)
        finally:
            ctx.close()


def test_statuses_and_the_two_finishes(oracle):
    import frieda_amd
    from frieda_amd.api import _check

    ctx = frieda_amd.Context(0)
    try:
        blobs, want = reference(ctx, oracle, 10)
        other_len, _ = reference(ctx, oracle, 11)
        pcs = _cfg(*CFG)
        encs = ctx.encode_batch(blobs, CFG[1])
        longer = ctx.encode(other_len[0], CFG[1])  # another length
        wider = ctx.encode(blobs[0], 3)  # the same length, another blow-up
        L, h = ctx._L, ctx._h
        seeds = (C.c_uint64 * len(SEEDS))(*SEEDS)
        outs = (C.c_void_p * 65536)()

        def table(es):
            return (C.c_void_p * len(es))(*[e._handle() if e is not None else None for e in es])

        def refused(call, status=ERR_ARG):
            with pytest.raises(frieda_amd.FriedaError) as ei:
                call()
            assert ei.value.status == status, ei.value
            assert _ser(ctx.prove_seeds_blobs(encs[:2], SEEDS[:2], pcs)) == [w[:2] for w in want[:2]]  # the context works afterwards

        good = table(encs)
        refused(lambda: _check(L.frieda_prove_seeds_blobs(h, None, K, seeds, 5, pcs._c(), outs), h))  # a null list
        refused(lambda: _check(L.frieda_prove_seeds_blobs(h, table([encs[0], None, encs[2]]), K, seeds, 5, pcs._c(), outs), h))  # a null handle
        refused(lambda: _check(L.frieda_prove_seeds_blobs(h, good, K, None, 5, pcs._c(), outs), h))  # null seeds
        refused(lambda: _check(L.frieda_prove_seeds_blobs(h, good, K, seeds, 5, pcs._c(), None), h))  # null out_proofs
        refused(lambda: _check(L.frieda_prove_seeds_blobs(h, good, 0, seeds, 5, pcs._c(), outs), h))  # n_blobs 0
        refused(lambda: _check(L.frieda_prove_seeds_blobs(h, good, K, seeds, 0, pcs._c(), outs), h))  # n_seeds 0
        many = table([encs[0]] * 256)
        many_seeds = (C.c_uint64 * 256)(*range(256))
        refused(lambda: _check(L.frieda_prove_seeds_blobs(h, many, 256, many_seeds, 256, pcs._c(), outs), h))  # K * S = 65536
        refused(lambda: ctx.prove_seeds_blobs([encs[0], longer], SEEDS, pcs))  # two lengths
        refused(lambda: ctx.prove_seeds_blobs([encs[0], wider], SEEDS, pcs))  # two blow-ups
        refused(lambda: ctx.prove_seeds_blobs(encs, SEEDS, _cfg(CFG[0], 3, CFG[2], CFG[3])))  # cfg's blow-up is not the handles'
        refused(lambda: ctx.prove_seeds_blobs(encs, SEEDS, _cfg(CFG[0], 4, 11, CFG[3])))  # the rules of prove_seeds_begin
        refused(lambda: ctx.prove_seeds_blobs(encs, SEEDS, _cfg(CFG[0], 4, 0, 0)))
        refused(lambda: ctx.prove_seeds_blobs_finish())  # nothing in flight
        # a second begin while a job is in flight: what prove_seeds_begin returns there
        ctx.prove_seeds_begin(encs[0], SEEDS, pcs)
        with pytest.raises(frieda_amd.FriedaError) as ei:
            ctx.prove_seeds_begin(encs[0], SEEDS, pcs)
        in_flight_status = ei.value.status
        with pytest.raises(frieda_amd.FriedaError) as ei:
            ctx.prove_seeds_blobs_begin(encs, SEEDS, pcs)
        assert ei.value.status == in_flight_status == ERR_ARG
        # ... and the job of prove_seeds_begin is finished by the block finish: the finishes are one function, as prove_seeds_finish
        # completes a batch begun by another entry point
        ctx._seeds_blobs_in_flight = (1, len(SEEDS))
        assert _ser(ctx.prove_seeds_blobs_finish()) == [want[0]]
        ctx.prove_seeds_blobs_begin(encs, SEEDS, pcs)
        with pytest.raises(frieda_amd.FriedaError) as ei:
            ctx.prove_seeds_blobs_begin(encs, SEEDS, pcs)
        assert ei.value.status == ERR_ARG
        ctx._seeds_in_flight = K * len(SEEDS)
        flat = [p.serialize() for p in ctx.prove_seeds_finish()]  # the other way round: blob-major
        assert flat == [x for row in want for x in row]
        ctx._seeds_blobs_in_flight = (0, 0)
        _close(encs + [longer, wider])
    finally:
        ctx.close()


def test_memory_is_the_planned_size_and_a_refused_call_leaves_the_context_usable(oracle):
    import frieda_amd

    ctx = frieda_amd.Context(0)
    try:
        blobs, want = reference(ctx, oracle, 13)
        pcs = _cfg(*CFG)
        length = len(blobs[0])
        encs = ctx.encode_batch(blobs, CFG[1])
        ws = frieda_amd.seeds_blobs_workspace_bytes(length, pcs, K, len(SEEDS))
        smaller = frieda_amd.seeds_blobs_workspace_bytes(length, pcs, K, 2)
        assert 0 < smaller < ws
        assert ctx._L.frieda_ctx_test_set_arena_limit(ctx._h, ws - 1) == 0
        try:
            with pytest.raises(frieda_amd.FriedaError) as ei:
                ctx.prove_seeds_blobs(encs, SEEDS, pcs)
            assert ei.value.status == ERR_NOMEM
            assert _ser(ctx.prove_seeds_blobs(encs, SEEDS[:2], pcs)) == [w[:2] for w in want]  # the next, smaller call
            assert ctx._L.frieda_ctx_test_set_arena_limit(ctx._h, ws) == 0
            assert _ser(ctx.prove_seeds_blobs(encs, SEEDS, pcs)) == want  # the planned size is enough
            phases = ctx.last_prove_phases()
            assert 0 < phases["enqueued"] <= phases["device_done"] <= phases["assembled"]
        finally:
            assert ctx._L.frieda_ctx_test_set_arena_limit(ctx._h, 0) == 0
        _close(encs)
    finally:
        ctx.close()
