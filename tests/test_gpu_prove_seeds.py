"""GPU: one blob proved under many seeds (Context.encode + Context.prove_seeds): every proof byte-identical to the ordinary proof of the
same blob under that seed — against the oracle, against Level A at size, across the two fold routes, the two decommit routes and
differing tree-skip thresholds —, the handle's independence of the context's workspace, the documented statuses, the small fused
shapes, the provider / client sampling loop and the memory claim.  Every test runs once under its own time limit."""
import ctypes as C
import signal

import numpy as np
import pytest

from conftest import splitmix64_bytes
from test_gpu_parity import PROVE_CASES
from test_gpu_small_fused import CASES as SMALL_CASES
from test_gpu_small_fused import _len_for as small_len_for
from util import DevBuf, blob_len_for, resolve_input

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_NOMEM = 1, 4
TAIL_LOG = 11  # the device channel's last layer holds at most 2^11 points


@pytest.fixture(autouse=True)
def _time_limit(request):
    """one run per test, ended by SIGALRM after its limit (default 300 s; @pytest.mark.parametrize cases share their test's limit)"""
    limit = getattr(request.function, "time_limit", 300)

    def on_alarm(signum, frame):
        raise TimeoutError(f"{request.node.name}: over its {limit} s limit")

    old = signal.signal(signal.SIGALRM, on_alarm)
    signal.alarm(limit)
    try:
        yield
    finally:
        signal.alarm(0)
        signal.signal(signal.SIGALRM, old)


def time_limit(seconds):
    def deco(f):
        f.time_limit = seconds
        return f

    return deco


def _cfg(pow_bits, B, last, nq):
    import frieda_amd

    return frieda_amd.PcsConfig(frieda_amd.FriConfig(B, last, nq), pow_bits)


def _status(excinfo):
    return excinfo.value.status


DEVICE_CASES = [c for c in PROVE_CASES if c[2][1] + c[2][2] <= TAIL_LOG]
HOST_CASES = [c for c in PROVE_CASES if c[2][1] + c[2][2] > TAIL_LOG]


def test_case_split_is_not_vacuous():
    assert len(DEVICE_CASES) >= 14 and [c[0] for c in HOST_CASES] == ["pattern:40000"]


@pytest.mark.parametrize("spec,seed,cfg", DEVICE_CASES, ids=lambda v: str(v)[:28])
def test_bytes_equal_the_oracle(gpu_ctx, oracle, blob, spec, seed, cfg):
    import frieda_amd

    data = resolve_input(spec, blob)
    seeds = [seed if seed is not None else 0, 1, 2**64 - 1, 12345, 1]
    want = {s: oracle.commit_and_generate_proof(data, s, oracle.make_config(*cfg)) for s in set(seeds)}
    pcs = _cfg(*cfg)
    enc = gpu_ctx.encode(data, cfg[1])
    try:
        assert enc.commitment == oracle.commit(data, cfg[1]) == want[seeds[0]][0]
        proofs = gpu_ctx.prove_seeds(enc, seeds, pcs)
    finally:
        enc.close()
    assert len(proofs) == len(seeds)
    for s, p in zip(seeds, proofs):
        assert p.serialize() == want[s][1].serialize(), f"seed {s}"
    assert proofs[1].serialize() == proofs[4].serialize()  # the repeated seed
    if proofs[0].n_inner_layers > 0:
        for i, (s, p) in enumerate(zip(seeds, proofs)):
            other = next(o for o in seeds if o != s)
            assert frieda_amd.verify(p, s), f"proof {i} under its own seed"
            assert not frieda_amd.verify(p, other), f"proof {i} under seed {other}"
    # the one-call convenience: the same bytes and the commitment
    root, again = gpu_ctx.commit_and_generate_proofs_for_seeds(data, seeds[:2], pcs)
    assert root == want[seeds[0]][0] and [p.serialize() for p in again] == [want[s][1].serialize() for s in seeds[:2]]


@pytest.mark.parametrize("spec,seed,cfg", HOST_CASES, ids=lambda v: str(v)[:28])
def test_host_channel_case_one_seed_both_policies_two_seeds_refused(gpu_ctx, oracle, blob, spec, seed, cfg):
    import frieda_amd

    data = resolve_input(spec, blob)
    o_root, o_proof = oracle.commit_and_generate_proof(data, seed, oracle.make_config(*cfg))
    pcs = _cfg(*cfg)
    enc = gpu_ctx.encode(data, cfg[1])
    try:
        assert enc.commitment == o_root
        for host_channel in (False, True):
            gpu_ctx.set_host_channel(host_channel)
            try:
                (p,) = gpu_ctx.prove_seeds(enc, [seed], pcs)
                assert p.serialize() == o_proof.serialize(), f"host_channel={host_channel}"
                with pytest.raises(frieda_amd.FriedaError) as ei:
                    gpu_ctx.prove_seeds(enc, [seed, seed + 1], pcs)
                assert _status(ei) == ERR_ARG
            finally:
                gpu_ctx.set_host_channel(False)
        # a case that fits the device tail, under the host-channel policy: one seed works, two are refused
        small_cfg = (10, 4, 0, 16)
        enc2 = gpu_ctx.encode(data, 4)
        gpu_ctx.set_host_channel(True)
        try:
            (p,) = gpu_ctx.prove_seeds(enc2, [3], _cfg(*small_cfg))
            assert p.serialize() == oracle.commit_and_generate_proof(data, 3, oracle.make_config(*small_cfg))[1].serialize()
            with pytest.raises(frieda_amd.FriedaError) as ei:
                gpu_ctx.prove_seeds(enc2, [3, 4], _cfg(*small_cfg))
            assert _status(ei) == ERR_ARG
        finally:
            gpu_ctx.set_host_channel(False)
            enc2.close()
    finally:
        enc.close()


def _level_a(ctx, d_blob, length, seeds, pcs):
    return [ctx.commit_and_generate_proof_device(d_blob.ptr, length, s, pcs) for s in seeds]


@time_limit(600)
@pytest.mark.parametrize("log_domain", [20, 22, 24])
def test_bytes_equal_level_a_at_size(gpu_ctx, oracle, log_domain):
    length = blob_len_for(log_domain)
    data = splitmix64_bytes(808 + log_domain, length)
    d_blob = DevBuf.from_array(gpu_ctx, data)
    pcs = _cfg(20, 4, 0, 20)
    seeds = [7, 2**63 + 5, 0, 99, 7, 31337]
    try:
        ref = _level_a(gpu_ctx, d_blob, length, seeds, pcs)
        enc = gpu_ctx.encode_device(d_blob.ptr, length, 4)
        try:
            assert enc.commitment == ref[0][0]
            got = gpu_ctx.prove_seeds(enc, seeds, pcs)
        finally:
            enc.close()
        for i, (g, (_, r)) in enumerate(zip(got, ref)):
            assert g.serialize() == r.serialize(), f"seed index {i}"
        if log_domain == 20:
            o_root, o_proof = oracle.commit_and_generate_proof(data.tobytes(), seeds[0], oracle.make_config(20, 4, 0, 20))
            assert o_root == ref[0][0] and got[0].serialize() == o_proof.serialize()
    finally:
        d_blob.free()


ROUTE_SEEDS = [11, 12, 13, 14, 15, 16]  # 6 seeds: a group of 4 does not divide them


@time_limit(600)
@pytest.mark.parametrize("log_domain", [13, 18, 21])
def test_routes_decommit_forms_and_skip_thresholds_agree(gpu_ctx, log_domain):
    """Route A, route B with groups of 2, 4 (not a divisor of 6) and 8 (more than the seeds); device and host decommit; the encoded tree
    and the inner trees built under different skip thresholds, both ways round, and a handle encoded under one setting proved under
    another.  2^18 and 2^21 reach the seed-looped kernel (register-subtree launches); 2^13 is a shape in which route B must fall back."""
    import frieda_amd

    length = blob_len_for(log_domain)
    data = splitmix64_bytes(4242 + log_domain, length)
    pcs = _cfg(12, 4, 0, 20)
    d_ref = DevBuf.from_array(gpu_ctx, data)
    try:
        want = [p.serialize() for _, p in _level_a(gpu_ctx, d_ref, length, ROUTE_SEEDS, pcs)]
    finally:
        d_ref.free()
    ctx = frieda_amd.Context(0)
    d_blob = DevBuf.from_array(ctx, data)
    try:
        def run(enc, seeds=ROUTE_SEEDS):
            return [p.serialize() for p in ctx.prove_seeds(enc, seeds, pcs)]

        enc = ctx.encode_device(d_blob.ptr, length, 4)
        for group in (0, 2, 4, 8):
            ctx.set_option("FRIEDA_SEEDS_FOLD_GROUP", group)
            for host_decommit in (0, 1):
                ctx.set_option("FRIEDA_HOST_DECOMMIT", host_decommit)
                assert run(enc) == want, f"group {group}, host_decommit {host_decommit}"
        ctx.set_option("FRIEDA_SEEDS_FOLD_GROUP", 0)
        enc.close()
        lo = 12 if log_domain > 13 else 10
        # (skip_log, skip_lone_log) at encode -> at prove.  The encoded tree uses the lone threshold max(lone, skip), the inner trees of a
        # call of several seeds `skip`: full first tree + skipping inner trees, skipping first tree + full inner trees, and a handle
        # encoded under one setting proved under the other
        for at_encode, at_prove in [((lo, 40), (lo, 40)), ((lo, lo), (40, 40)), ((40, 40), (lo, lo)), ((lo, lo), (lo, lo))]:
            ctx.set_option("FRIEDA_TREE_SKIP_LOG", at_encode[0])
            ctx.set_option("FRIEDA_TREE_SKIP_LONE_LOG", at_encode[1])
            enc = ctx.encode_device(d_blob.ptr, length, 4)
            ctx.set_option("FRIEDA_TREE_SKIP_LOG", at_prove[0])
            ctx.set_option("FRIEDA_TREE_SKIP_LONE_LOG", at_prove[1])
            for group in (0, 4):
                ctx.set_option("FRIEDA_SEEDS_FOLD_GROUP", group)
                for host_decommit in (0, 1):
                    ctx.set_option("FRIEDA_HOST_DECOMMIT", host_decommit)
                    assert run(enc) == want, f"thresholds {at_encode} -> {at_prove}, group {group}, host_decommit {host_decommit}"
                    assert run(enc, ROUTE_SEEDS[:1]) == want[:1], f"one seed, thresholds {at_encode} -> {at_prove}"
            enc.close()
    finally:
        d_blob.free()
        ctx.close()


@time_limit(600)
def test_handle_is_independent_of_the_workspace(gpu_ctx, oracle):
    import frieda_amd

    pcs = _cfg(10, 4, 0, 20)
    data_a = splitmix64_bytes(1, blob_len_for(16)).tobytes()
    data_b = splitmix64_bytes(2, blob_len_for(14)).tobytes()
    seeds = [5, 6, 7]
    ctx = frieda_amd.Context(0)
    other = frieda_amd.Context(0)
    try:
        want_a = [ctx.commit_and_generate_proof(data_a, s, pcs)[1].serialize() for s in seeds]
        want_b = [ctx.commit_and_generate_proof(data_b, s, pcs)[1].serialize() for s in seeds]
        enc_a = ctx.encode(data_a, 4)
        enc_b = ctx.encode(data_b, 4)  # two handles alive at once
        # unrelated work on the same context: a commit and a batch proof of other blobs (a larger workspace: the arena is reallocated)
        noise = splitmix64_bytes(3, blob_len_for(18)).tobytes()
        assert ctx.commit(noise, 4) == oracle.commit(noise, 4)
        ctx.commit_and_generate_proof_batch([noise, noise[::-1]], [1, 2], pcs)
        ctx.release_workspace()
        assert [p.serialize() for p in ctx.prove_seeds(enc_a, seeds, pcs)] == want_a
        assert [p.serialize() for p in ctx.prove_seeds(enc_b, seeds, pcs)] == want_b
        assert enc_a.commitment == oracle.commit(data_a, 4) and enc_b.commitment == oracle.commit(data_b, 4)
        # a second context proves from the same handle, both in flight at once
        ctx.prove_seeds_begin(enc_a, seeds, pcs)
        other.prove_seeds_begin(enc_a, seeds[::-1], pcs)
        assert [p.serialize() for p in other.prove_seeds_finish()] == want_a[::-1]
        assert [p.serialize() for p in ctx.prove_seeds_finish()] == want_a

        # ---- the documented statuses; the context works after each ----
        def refused(call, status=ERR_ARG):
            with pytest.raises(frieda_amd.FriedaError) as ei:
                call()
            assert _status(ei) == status, ei.value
            assert [p.serialize() for p in ctx.prove_seeds(enc_a, seeds[:1], pcs)] == want_a[:1]

        refused(lambda: ctx.prove_seeds(enc_a, seeds, _cfg(10, 3, 0, 20)))  # not the blow-up it was encoded with
        refused(lambda: ctx.prove_seeds(enc_a, [], pcs))  # n_seeds == 0
        refused(lambda: ctx.prove_seeds(enc_a, [1] * 65536, pcs))
        refused(lambda: frieda_amd.api._check(ctx._L.frieda_prove_seeds_begin(ctx._h, enc_a._handle(), None, 2, pcs._c()), ctx._h))  # null seeds
        refused(lambda: frieda_amd.api._check(ctx._L.frieda_prove_seeds_begin(ctx._h, None, (C.c_uint64 * 1)(1), 1, pcs._c()), ctx._h))
        refused(lambda: ctx.prove_seeds_finish())  # finish without begin
        refused(lambda: ctx.prove_seeds(enc_a, seeds, _cfg(10, 4, 0, 0)))  # the batch entry points' argument rules
        refused(lambda: ctx.prove_seeds(enc_a, seeds, _cfg(10, 4, 11, 20)))
        ctx.prove_seeds_begin(enc_a, seeds, pcs)
        with pytest.raises(frieda_amd.FriedaError) as ei:  # begin while a job is in flight
            ctx.prove_seeds_begin(enc_a, seeds, pcs)
        assert _status(ei) == ERR_ARG
        with pytest.raises(frieda_amd.FriedaError) as ei:  # so is encoding: it would resize the workspace the job lives in
            ctx.encode(data_b, 4)
        assert _status(ei) == ERR_ARG
        ctx._seeds_in_flight = len(seeds)
        assert [p.serialize() for p in ctx.prove_seeds_finish()] == want_a
        # memory: a call the device cannot hold is FRIEDA_ERR_NOMEM, sized by seeds_workspace_bytes — one seed fewer than the limit fits
        ws3 = frieda_amd.seeds_workspace_bytes(len(data_a), pcs, 3)
        ws2 = frieda_amd.seeds_workspace_bytes(len(data_a), pcs, 2)
        assert ctx._L.frieda_ctx_test_set_arena_limit(ctx._h, ws3 - 1) == 0
        try:
            refused(lambda: ctx.prove_seeds(enc_a, seeds, pcs), ERR_NOMEM)
            assert ws2 < ws3
            assert [p.serialize() for p in ctx.prove_seeds(enc_a, seeds[:2], pcs)] == want_a[:2]
        finally:
            assert ctx._L.frieda_ctx_test_set_arena_limit(ctx._h, 0) == 0
        assert [p.serialize() for p in ctx.prove_seeds(enc_a, seeds, pcs)] == want_a
        enc_a.close()
        enc_b.close()
        with pytest.raises(ValueError):
            ctx.prove_seeds(enc_a, seeds, pcs)  # a closed handle never reaches the library
    finally:
        ctx.close()
        other.close()


SMALL_PROVABLE = [p for p in SMALL_CASES if p.values[0] >= 1 and p.values[0] + p.values[1] >= 2]


@pytest.mark.parametrize("kind", ["exact", "ragged", "short"])
@pytest.mark.parametrize("L,B", SMALL_PROVABLE)
def test_small_fused_shapes_equal_the_batch_path(gpu_ctx, L, B, kind):
    """The length classes of the fused small-domain path, 33 seeds: equal to the batch path given 33 copies of the blob."""
    length = small_len_for(L, kind)
    data = splitmix64_bytes(7000 + 16 * L + B, length).tobytes()
    pcs = _cfg(6, B, 0, 20)
    seeds = [1000 + 3 * i for i in range(33)]
    want = gpu_ctx.commit_and_generate_proof_batch([data] * 33, seeds, pcs)
    enc = gpu_ctx.encode(data, B)
    try:
        got = gpu_ctx.prove_seeds(enc, seeds, pcs)
        assert enc.commitment == want[0][0]
    finally:
        enc.close()
    assert [p.serialize() for p in got] == [p.serialize() for _, p in want]


def test_small_case_list_is_not_vacuous():
    assert len(SMALL_PROVABLE) >= 60


@time_limit(900)
@pytest.mark.parametrize("spec,B,nq", [("pattern:1024", 4, 20), ("pattern:4096", 4, 20), ("blob", 4, 300), ("pattern:300", 2, 12)])
def test_das_loop_encode_once_prove_seeds_pool_reconstruct(gpu_ctx, blob, spec, B, nq):
    """The loop a provider and its sampling clients run (test_das_loop_prove_verify_pool_reconstruct's flow and parameter sets) with ONE
    encode and prove_seeds in chunks of 64 client seeds in place of one full proof per seed."""
    import frieda_amd
    from test_gpu_reconstruct_points import _encode_on_device

    data = resolve_input(spec, blob)
    ev, L, n = _encode_on_device(gpu_ctx, data, B)
    cfg = frieda_amd.PcsConfig(frieda_amd.FriConfig(B, 0, nq), 8)
    root = gpu_ctx.commit(data, B)
    need = (1 << L) + 2
    # a chunk of 64 proofs opens at most 64 * nq new positions and, while under half of the 2^n >= 4 * 2^L domain is pooled, at least a
    # few: ten times the collision-free count of chunks is far beyond what the pool can need — the loop ends or the test fails
    max_chunks = 10 * (need + 64 * nq - 1) // (64 * nq) + 10
    pool = {}
    chunks = 0
    enc = gpu_ctx.encode(data, B)  # (the provider: once per blob)
    try:
        assert enc.commitment == root
        while len(pool) < need:
            assert chunks < max_chunks, "the pool does not fill"
            seeds = list(range(1 + 64 * chunks, 65 + 64 * chunks))  # (64 clients' seeds)
            chunks += 1
            proofs = gpu_ctx.prove_seeds(enc, seeds, cfg)
            assert len(proofs) == 64
            for seed, proof in zip(seeds, proofs):
                ok, positions = frieda_amd.verify_samples(proof, seed)  # (the client's side)
                assert ok and frieda_amd.verify(proof, seed)
                assert proof.layer(0)["commitment"] == root
                evals = proof.evaluations
                assert len(positions) == len(evals) and np.all(np.diff(positions.astype(np.int64)) > 0) and positions.max() < (1 << n)
                assert np.array_equal(ev[:, positions].T, evals), "a returned position does not hold the proof's evaluation"
                for p, v in zip(positions.tolist(), evals):
                    pool[p] = v
            if chunks == 1:  # a wrong seed is a rejected proof and yields no positions
                bad_ok, bad_pos = frieda_amd.verify_samples(proofs[0], seeds[1])
                assert not bad_ok and bad_pos is None
    finally:
        enc.close()
    assert chunks >= 1 and len(pool) >= need
    idx = np.array(sorted(pool), dtype=np.uint32)
    cells = np.ascontiguousarray(np.stack([pool[int(p)] for p in idx]).astype(np.uint32).reshape(-1, 4, 1))
    assert gpu_ctx.reconstruct_from_points(cells, idx, L, n, len(data)) == bytes(data)


def _up256(b):
    return (b + 255) & ~255


@time_limit(600)
def test_memory_stays_within_the_plan(gpu_ctx):
    """2^22 domain, 8 seeds on a fresh context: the device memory the call takes stays within seeds_workspace_bytes (the workspace is
    allocated in whole MiB, and the driver hands memory out in 2 MiB pages: that much slack and no more), and the handle holds
    evaluations + first tree + root, each from a 256-byte boundary."""
    import torch

    import frieda_amd

    log_domain, n_seeds = 22, 8
    length = blob_len_for(log_domain)
    data = splitmix64_bytes(2222, length)
    pcs = _cfg(20, 4, 0, 20)
    ctx = frieda_amd.Context(0)
    d_blob = DevBuf.from_array(ctx, data)
    try:
        # once through the whole path first: what the runtime allocates on first use (code objects, its own pools) is not the call's
        warm = ctx.encode_device(d_blob.ptr, length, 4)
        ctx.prove_seeds(warm, [0], pcs)
        warm.close()
        ctx.release_workspace()
        torch.cuda.synchronize()
        free0, _ = torch.cuda.mem_get_info(0)
        enc = ctx.encode_device(d_blob.ptr, length, 4)
        expect = _up256(16 << log_domain) + _up256((64 << log_domain) - 64 + 32) + _up256(32)
        assert enc.nbytes == expect
        ctx.release_workspace()  # the coefficients' workspace and the twiddles go; the handle stays
        free1, _ = torch.cuda.mem_get_info(0)
        assert expect <= free0 - free1 <= expect + (4 << 20), (free0 - free1, expect)  # (two pages of slack)
        ctx.prove_seeds(enc, [1], pcs)  # twiddles of this size are back in the cache, and a workspace smaller than the one measured
        free2, _ = torch.cuda.mem_get_info(0)
        seeds = list(range(n_seeds))
        proofs = ctx.prove_seeds(enc, seeds, pcs)
        free3, _ = torch.cuda.mem_get_info(0)
        ws1 = frieda_amd.seeds_workspace_bytes(length, pcs, 1)
        ws = frieda_amd.seeds_workspace_bytes(length, pcs, n_seeds)
        grown = free2 - free3  # the one-seed workspace was freed, the eight-seed one allocated
        print(f"arena growth {grown} B for {n_seeds} seeds; plan {ws} B ({ws1} B for one seed)")
        assert grown > 0
        assert grown + ws1 <= ws + (1 << 20) + (2 << 20) + (1 << 20), (grown, ws1, ws)
        assert ws + expect < n_seeds * frieda_amd.workspace_bytes(length, 4, 0, True)
        want = ctx.commit_and_generate_proof_device(d_blob.ptr, length, seeds[3], pcs)[1].serialize()
        assert proofs[3].serialize() == want
        enc.close()
        free4, _ = torch.cuda.mem_get_info(0)
        assert free4 - free3 >= expect - (2 << 20)  # closing the handle gives its memory back
    finally:
        d_blob.free()
        ctx.close()
