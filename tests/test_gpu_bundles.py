"""Cell bundles on the GPU: frieda_open_cell_bundles against the CPU oracle's codeword and tree for every layout frieda_encode can leave,
frieda_verify_cell_bundles_many against the host verifier status for status, frieda_reconstruct_from_cell_bundles end to end.

Shapes are the smallest at which each branch exists: the open shapes of tests/test_gpu_cells.py (the 2^12 tree with and without its two
lowest node levels exercises the re-hash at log_cell <= 2), log_cell on both sides of the 16-byte copy and of the one-cell-per-workgroup
reduction, bundles off the wave size (1, 2, 64, 65, 300), the cap (1024) and one more, several verify passes."""
import ctypes as C

import numpy as np
import pytest

import bundles_util as B
import cells_util as U
import stripe_bundles_util as S
import workspace_rows as W
from bundles_util import ACCEPTED, MALFORMED, REJECTED
from cells_util import ERR_ARG, HOST_CASES, POISON
from test_gpu_cells import OPEN_SHAPES, oracle_commit

pytestmark = pytest.mark.gpu

GUARD = 64


# ---- open -------------------------------------------------------------------------------------------------------------------------------
def raw_open(ctx, enc, c, bundles, n_values_words, cap=None, query=False):
    """frieda_open_cell_bundles into poison-filled buffers between red zones: (rc, values words, witness [H, 32], witness_first)"""
    idx = np.ascontiguousarray(np.concatenate(bundles), dtype=np.uint32)
    first = np.concatenate([[0], np.cumsum([len(b) for b in bundles])]).astype(np.uint32)
    nb = len(bundles)
    want_hashes = sum(len(B.merge_walk(enc.shape[1] - c, b)) for b in bundles) if cap is None else cap
    values = np.full(n_values_words + 2 * GUARD, 0xA5A5A5A5, dtype=np.uint32)
    witness = np.full(32 * want_hashes + 2 * GUARD, POISON, dtype=np.uint8)
    wfirst = np.full(nb + 1 + GUARD, 0x1234567812345678, dtype=np.uint64)
    rc = ctx._L.frieda_open_cell_bundles(ctx._h, enc._handle(), c, idx.ctypes.data, first.ctypes.data, nb, None if query else values.ctypes.data + 4 * GUARD,
                                         None if query else witness.ctypes.data + GUARD, want_hashes, wfirst.ctypes.data)
    assert (values[:GUARD] == 0xA5A5A5A5).all() and (values[GUARD + n_values_words:] == 0xA5A5A5A5).all(), "red zone around out_values"
    assert (witness[:GUARD] == POISON).all() and (witness[GUARD + 32 * want_hashes:] == POISON).all(), "red zone around out_witness"
    assert (wfirst[nb + 1:] == 0x1234567812345678).all(), "red zone behind out_witness_first"
    return rc, values[GUARD:GUARD + n_values_words], witness[GUARD:GUARD + 32 * want_hashes].reshape(-1, 32), wfirst[: nb + 1]


@pytest.mark.parametrize("shape", sorted(OPEN_SHAPES))
def test_open_cell_bundles_equal_the_oracle(shape):
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
        assert enc.commitment == root and enc.shape == (L, n)
        for c in (0, 1, 2, 3, 6, 10):
            if c > n:
                continue
            total = 1 << (n - c)
            five = [B.pick(n, c, min(k, total), seed=70 + j) for j, k in enumerate((1, 2, 64, 65, 300))]
            for bundles in ([B.pick(n, c, min(65, total), seed=69)], five):
                want = B.build_call(ev, layers, c, bundles)
                words = want.values.size
                rc, v, w, wf = raw_open(ctx, enc, c, bundles, words)
                assert rc == 0, ctx._L.frieda_last_error(ctx._h)
                assert v.tobytes() == want.values.tobytes(), (c, len(bundles))
                assert wf.tolist() == want.wfirst.tolist(), (c, len(bundles))
                assert w.tobytes() == want.witness.tobytes(), (c, len(bundles), np.flatnonzero((w != want.witness).any(axis=1))[:8])
                for b, idx in enumerate(bundles):
                    assert B.witness_count(n, c, idx) == (0, int(wf[b + 1] - wf[b]))
                # the size query: out_witness == NULL fills out_witness_first only
                rc, v, w, wf = raw_open(ctx, enc, c, bundles, words, query=True)
                assert rc == 0 and wf.tolist() == want.wfirst.tolist()
                assert (v == 0xA5A5A5A5).all() and (w == POISON).all()
                # cap_hashes one too small: refused, outputs untouched
                if int(want.wfirst[-1]):
                    rc, v, w, wf = raw_open(ctx, enc, c, bundles, words, cap=int(want.wfirst[-1]) - 1)
                    assert rc == ERR_ARG and (v == 0xA5A5A5A5).all() and (w == POISON).all() and (wf == 0x1234567812345678).all()
            # the Python surface gives the same arrays
            v, w, wf = enc.open_cell_bundles(ctx, c, five)
            want = B.build_call(ev, layers, c, five)
            assert v.tobytes() == want.values.tobytes() and w.tobytes() == want.witness.tobytes() and wf.tolist() == want.wfirst.tolist()
        # a malformed bundle refuses the whole call and is named; no bundles: a no-op
        good = B.pick(n, 0, min(5, 1 << n), seed=1)
        for bad in (good[::-1].copy(), np.array([0, 1 << n], np.uint32), np.zeros(0, np.uint32), np.array([1, 1], np.uint32)):
            rc, v, w, wf = raw_open(ctx, enc, 0, [good, bad], 4 * (len(good) + len(bad)), cap=64)
            assert rc == ERR_ARG and (v == 0xA5A5A5A5).all() and (w == POISON).all() and (wf == 0x1234567812345678).all()
            assert b"bundle 1" in ctx._L.frieda_last_error(ctx._h)
        assert ctx._L.frieda_open_cell_bundles(ctx._h, enc._handle(), 0, None, None, 0, None, None, 0, None) == 0
        enc.close()
    finally:
        ctx.close()


def test_open_cell_bundles_beside_a_prove_seeds_job(gpu_ctx):
    """the blob is only read: another context opens bundles while a prove_seeds job is in flight; the context with the job refuses"""
    import frieda_amd

    data, ev, layers, n, L = U.codeword(1024, 4)
    cfg = frieda_amd.PcsConfig(frieda_amd.FriConfig(4, 0, 8), 4)
    other = frieda_amd.Context(0)
    enc = gpu_ctx.encode(data, 4)
    try:
        bundles = [B.pick(n, 3, 17, seed=1), B.pick(n, 3, 5, seed=2)]
        want = B.build_call(ev, layers, 3, bundles)
        gpu_ctx.prove_seeds_begin(enc, [1, 2, 3], cfg)
        try:
            v, w, wf = enc.open_cell_bundles(other, 3, bundles)
            with pytest.raises(frieda_amd.FriedaError) as e:
                enc.open_cell_bundles(gpu_ctx, 3, bundles)
            assert e.value.status == ERR_ARG and "in flight" in str(e.value)
        finally:
            proofs = gpu_ctx.prove_seeds_finish()
        assert v.tobytes() == want.values.tobytes() and w.tobytes() == want.witness.tobytes() and wf.tolist() == want.wfirst.tolist()
        assert all(frieda_amd.verify(p, s) for p, s in zip(proofs, [1, 2, 3]))
    finally:
        enc.close()
        other.close()


# ---- verify -----------------------------------------------------------------------------------------------------------------------------
def both(ctx, call):
    """(host statuses, device statuses) of one call; both calls must succeed"""
    rc_h, host = B.raw_verify(call)
    rc_d, dev = B.raw_verify(call, ctx)
    assert rc_h == 0 and rc_d == 0, (rc_h, rc_d, ctx._L.frieda_last_error(ctx._h))
    return host.tolist(), dev.tolist()


@pytest.mark.parametrize("n,b,c", HOST_CASES)
def test_verify_many_on_every_shape_and_the_mutation_matrix(gpu_ctx, n, b, c):
    labels, call = B.shapes_call(n, b, c)
    host, dev = both(gpu_ctx, call)
    assert dev == host == [ACCEPTED] * len(labels), [l for l, s in zip(labels, dev) if s != ACCEPTED]
    small = B.small_call(n, b, c)
    for label, hit, must, mutated in B.mutations(small):
        host, dev = both(gpu_ctx, mutated)
        assert dev == host, (label, hit)
        B.check_mutation(label, hit, must, host, len(small.bundles))
    wrong = bytearray(call.commitment)
    wrong[5] ^= 1
    host, dev = both(gpu_ctx, call.replace(commitment=bytes(wrong)))
    assert dev == host == [REJECTED] * len(labels)


def test_verify_many_sizes_1_and_300_in_one_pass_and_the_cap(gpu_ctx):
    n, c = 12, 0
    _, ev, layers, _, _ = U.case(n, 4)
    sizes = (1, 300, 1, 1024, 1025, 300, 1)
    call = B.build_call(ev, layers, c, [B.pick(n, c, k, seed=80 + j) for j, k in enumerate(sizes)])
    host, dev = both(gpu_ctx, call)
    assert dev == host == [MALFORMED if k > 1024 else ACCEPTED for k in sizes]
    # the same with one word of the cap bundle's last cell changed
    v = call.values.copy()
    v[int(call.first[4]) - 1, 3, 0] ^= 1
    host, dev = both(gpu_ctx, call.replace(values=v))
    assert dev == host == [ACCEPTED, ACCEPTED, ACCEPTED, REJECTED, MALFORMED, ACCEPTED, ACCEPTED]
    # bad call structure: refused, status untouched
    first = call.first.copy()
    rc, st = B.raw_verify(call.replace(wfirst=call.wfirst[::-1].copy()), gpu_ctx)
    assert rc == ERR_ARG and (st == POISON).all()
    rc, st = B.raw_verify(call.replace(n=29), gpu_ctx)
    assert rc == ERR_ARG and (st == POISON).all()
    assert first[0] == 0


def flipped_call(n, c, sizes, flips, seed):
    """bundles of `sizes` cells with `flips` single-bit flips over indices, values and witness in turn"""
    _, ev, layers, _, _ = U.case(n, 4)
    rng = np.random.default_rng(seed)
    call = B.build_call(ev, layers, c, [B.pick(n, c, k, seed=seed + j) for j, k in enumerate(sizes)])
    idx = np.concatenate(call.bundles)
    values, witness = call.values.copy(), call.witness.copy()
    for j in range(flips):
        kind = j % 3
        if kind == 0:
            w = values.reshape(-1)
            w[int(rng.integers(0, w.size))] ^= np.uint32(1 << int(rng.integers(0, 32)))
        elif kind == 1:
            p = witness.reshape(-1)
            p[int(rng.integers(0, p.size))] ^= np.uint8(1 << int(rng.integers(0, 8)))
        else:
            idx[int(rng.integers(0, idx.size))] ^= np.uint32(1 << int(rng.integers(0, n - c)))
    first = call.first
    return call.replace(bundles=[idx[first[b]:first[b + 1]] for b in range(len(sizes))], values=values, witness=witness)


def staged_bytes(call):
    """what each bundle of a call stages in a pass (bundles_pass.h): its table row, its indices, its values and its witness"""
    vb = 16 << call.c
    return [12 + len(i) * (4 + vb) + 32 * int(w1 - w0) for i, w0, w1 in zip(call.bundles, call.wfirst[:-1], call.wfirst[1:])]


def pass_cuts(staged, pass_bytes):
    """the passes of bundles that stage `staged` bytes each, by the rule of bundles_pass.h written out again: bundles in order while their
    sum stays within pass_bytes, one bundle always admitted"""
    cuts, first = [], 0
    while first < len(staged):
        end, total = first + 1, staged[first]
        while end < len(staged) and total + staged[end] <= pass_bytes:
            total += staged[end]
            end += 1
        cuts.append(list(range(first, end)))
        first = end
    return cuts


@pytest.mark.parametrize("pass_bytes", [0, 30000])
def test_verify_many_on_random_bit_flips_in_four_passes(gpu_ctx, pass_bytes):
    """120 bundles of 1 .. 9 cells at log_domain 12, log_cell 3, 200 flipped bits; 30000 bytes per pass: at least four passes"""
    n, c = 12, 3
    sizes = [1 + (j * 7) % 9 for j in range(120)]
    call = flipped_call(n, c, sizes, 200, seed=2025)
    want = B.independent_status(call)
    assert 10 <= (want == ACCEPTED).sum() <= 80 and (want == MALFORMED).any() and (want == REJECTED).any()
    if pass_bytes:
        staged = sum(12 + len(i) * (4 + (16 << c)) + 32 * int(w1 - w0) for i, w0, w1, s in zip(call.bundles, call.wfirst[:-1], call.wfirst[1:], want) if s != MALFORMED)
        assert staged > 3 * pass_bytes
    assert gpu_ctx._L.frieda_ctx_test_set_verify_pass_bytes(gpu_ctx._h, pass_bytes) == 0
    try:
        host, dev = both(gpu_ctx, call)
    finally:
        gpu_ctx._L.frieda_ctx_test_set_verify_pass_bytes(gpu_ctx._h, 0)
    assert dev == host == want.tolist()


def test_pass_cuts_beside_a_malformed_and_behind_a_rejected_bundle(gpu_ctx):
    """8 bundles of 3 .. 7 cells at log_domain 12, log_cell 3 with 4 flipped bits, twice the largest bundle per pass: at least three passes,
    a MALFORMED bundle (never staged) between the bundles of two passes, a REJECTED bundle as the last of a pass.  The same arrays through
    the single-blob driver, the stripe driver with one blob and the host verifier: identical status bytes."""
    n, c = 12, 3
    call = flipped_call(n, c, [5, 6, 7, 4, 5, 6, 7, 3], 4, seed=38)
    want = B.independent_status(call)
    assert {ACCEPTED, REJECTED, MALFORMED} == set(want.tolist())
    good = [b for b, s in enumerate(want) if s != MALFORMED]
    staged = [staged_bytes(call)[b] for b in good]
    pass_bytes = 2 * max(staged)
    passes = [[good[g] for g in p] for p in pass_cuts(staged, pass_bytes)]
    assert len(passes) >= 3
    assert any(a[-1] + 1 < z[0] for a, z in zip(passes[:-1], passes[1:])), "no malformed bundle between two passes"
    assert any(want[p[-1]] == REJECTED for p in passes), "no rejected bundle at the end of a pass"
    assert gpu_ctx._L.frieda_ctx_test_set_verify_pass_bytes(gpu_ctx._h, pass_bytes) == 0
    try:
        host, dev = both(gpu_ctx, call)
        rc, block = S.raw_verify(S.assemble([call]), gpu_ctx)
    finally:
        gpu_ctx._L.frieda_ctx_test_set_verify_pass_bytes(gpu_ctx._h, 0)
    assert rc == 0, gpu_ctx._L.frieda_last_error(gpu_ctx._h)
    assert dev == host == block[:, 0].tolist() == want.tolist()


def test_same_bytes_on_a_poisoned_workspace_and_a_callers_stream():
    """open, verify and rebuild on a private and on a caller's stream, on a fresh context and after frieda_ctx_test_poison has filled the
    arena and the pinned blocks with 0x00000000, 0xFFFFFFFF and 0x7FFFFFFF: the same bytes every time"""
    import torch

    import frieda_amd

    n, c = 12, 1
    call = flipped_call(n, c, [1, 65, 300, 2, 64], 3, seed=11)
    _, host = B.raw_verify(call)
    data, ev, layers, n2, L2 = U.case(11, 4)
    perm = np.random.default_rng(21).permutation(1 << (n2 - 3)).astype(np.uint32)
    bundles = [np.sort(perm[:9]), np.sort(perm[9:18]), np.sort(perm[18:19])]
    want = B.build_call(ev, layers, 3, bundles)
    stream = torch.cuda.Stream()
    for ctx in (frieda_amd.Context(0), frieda_amd.Context(0, stream=stream.cuda_stream)):
        try:
            enc = ctx.encode(data, 4)
            for word in (None, 0x00000000, 0xFFFFFFFF, 0x7FFFFFFF):
                if word is not None:
                    W.poison(ctx, word)
                rc, dev = B.raw_verify(call, ctx)
                assert rc == 0 and dev.tolist() == host.tolist(), word
                v, w, wf = enc.open_cell_bundles(ctx, 3, bundles)
                assert v.tobytes() == want.values.tobytes() and w.tobytes() == want.witness.tobytes() and wf.tolist() == want.wfirst.tolist(), word
                rc, out, st, used = raw_reconstruct(ctx, want, 4, len(data))
                assert rc == 0 and out == data and used == 19 and (st == ACCEPTED).all(), word
            enc.close()
        finally:
            ctx.close()


# ---- reconstruct ------------------------------------------------------------------------------------------------------------------------
def raw_reconstruct(ctx, call, blowup, length):
    """frieda_reconstruct_from_cell_bundles into a poison-filled buffer between two red zones: (rc, bytes or None, status, n_used)"""
    idx = np.ascontiguousarray(np.concatenate(call.bundles), dtype=np.uint32)
    first = np.ascontiguousarray(call.first, dtype=np.uint32)
    values = np.ascontiguousarray(call.values, dtype=np.uint32)
    witness = np.ascontiguousarray(call.witness, dtype=np.uint8)
    wfirst = np.ascontiguousarray(call.wfirst, dtype=np.uint64)
    nb = len(call.bundles)
    buf = np.full(length + 2 * GUARD, POISON, dtype=np.uint8)
    status = np.full(nb + GUARD, POISON, dtype=np.uint8)
    used = C.c_size_t(12345)
    com = (C.c_uint8 * 32)(*call.commitment)
    rc = ctx._L.frieda_reconstruct_from_cell_bundles(ctx._h, com, blowup, length, call.c, idx.ctypes.data, first.ctypes.data, nb, values.ctypes.data,
                                                     witness.ctypes.data, wfirst.ctypes.data, buf.ctypes.data + GUARD, status.ctypes.data, C.byref(used))
    assert (buf[:GUARD] == POISON).all() and (buf[GUARD + length:] == POISON).all(), "red zone around out_bytes"
    assert (status[nb:] == POISON).all(), "red zone behind out_status"
    body = buf[GUARD:GUARD + length]
    if rc != 0:
        assert (body == POISON).all(), "out_bytes written by a failed call"
    return rc, (body.tobytes() if rc == 0 else None), status[:nb], used.value


@pytest.mark.parametrize("multi_pass", [False, True])
@pytest.mark.parametrize("c,sizes,extra", [(3, (5, 6, 7), 6), (0, (64, 65, 1), 70)])
def test_reconstruct_from_cell_bundles(gpu_ctx, c, sizes, extra, multi_pass):
    """the 1024-byte blob at blowup 4 (2^7 coefficients, 2^11 domain): 17 distinct cells at log_cell 3, 130 points at log_cell 0;
    multi_pass: one byte less per pass than the first two bundles stage, so no pass holds both"""
    data, ev, layers, n, L = U.case(11, 4)
    assert (L, n) == (7, 11) and len(data) == 1024
    need = (1 << (L - c)) + 1 if c else (1 << L) + 2
    assert sum(sizes) >= need
    rng = np.random.default_rng(500 + c)
    perm = rng.permutation(1 << (n - c)).astype(np.uint32)
    cuts = np.concatenate([[0], np.cumsum(sizes)])
    bundles = [np.sort(perm[a:z]) for a, z in zip(cuts[:-1], cuts[1:])]
    # the fourth bundle: new cells and two that the first bundle already holds
    fourth = np.sort(np.concatenate([perm[cuts[-1]:cuts[-1] + extra], bundles[0][:2]]))
    call = B.build_call(ev, layers, c, bundles)
    pass_bytes = sum(staged_bytes(call)[:2]) - 1 if multi_pass else 0
    assert gpu_ctx._L.frieda_ctx_test_set_verify_pass_bytes(gpu_ctx._h, pass_bytes) == 0
    try:
        rc, out, st, used = raw_reconstruct(gpu_ctx, call, 4, len(data))
        assert rc == 0 and out == data and used == sum(sizes) and (st == ACCEPTED).all(), gpu_ctx._L.frieda_last_error(gpu_ctx._h)

        # one bundle corrupted: too few, the statuses name it, the output keeps its poison
        t = 1
        v = call.values.copy()
        v[int(call.first[t]), 1, 0] ^= 2
        bad = call.replace(values=v)
        rc, out, st, used = raw_reconstruct(gpu_ctx, bad, 4, len(data))
        assert rc == ERR_ARG and st.tolist() == [ACCEPTED, REJECTED, ACCEPTED] and used == sum(sizes) - sizes[t]
        assert sum(sizes) - sizes[t] < need

        # a fourth good bundle: enough again; its overlap with the first bundle is counted once, the rejected bundle is not used
        four = B.build_call(ev, layers, c, bundles + [fourth])
        v4 = four.values.copy()
        v4[int(four.first[t]), 1, 0] ^= 2
        rc, out, st, used = raw_reconstruct(gpu_ctx, four.replace(values=v4), 4, len(data))
        distinct = len(set(np.concatenate([bundles[0], bundles[2], fourth]).tolist()))
        assert distinct == sum(sizes) - sizes[t] + extra >= need
        assert rc == 0 and out == data and used == distinct and st.tolist() == [ACCEPTED, REJECTED, ACCEPTED, ACCEPTED]

        # a wrong len (same polynomial size): every bundle verifies, the commitment check fails
        assert oracle_commit(data[:-1], 4) != call.commitment
        rc, out, st, used = raw_reconstruct(gpu_ctx, call, 4, len(data) - 1)
        assert rc == ERR_ARG and (st == ACCEPTED).all() and used == sum(sizes)
        assert b"commit" in gpu_ctx._L.frieda_last_error(gpu_ctx._h)
    finally:
        gpu_ctx._L.frieda_ctx_test_set_verify_pass_bytes(gpu_ctx._h, 0)


def test_python_surface(gpu_ctx):
    import frieda_amd

    data, ev, layers, n, L = U.case(11, 4)
    root = layers[0][0].tobytes()
    enc = gpu_ctx.encode(data, 4)
    try:
        perm = np.random.default_rng(4).permutation(1 << (n - 3)).astype(np.uint32)
        bundles = [np.sort(perm[:9]), np.sort(perm[9:17])]
        values, witness, wfirst = enc.open_cell_bundles(gpu_ctx, 3, bundles)
    finally:
        enc.close()
    assert gpu_ctx.verify_cell_bundles_many(root, n, 3, bundles, values, witness, wfirst).tolist() == [ACCEPTED, ACCEPTED]
    assert frieda_amd.verify_cell_bundles(root, n, 3, bundles, values, witness, wfirst).tolist() == [ACCEPTED, ACCEPTED]
    out, st, used = gpu_ctx.reconstruct_from_cell_bundles(root, 4, len(data), 3, bundles, values, witness, wfirst)
    assert out == data and used == 17 and (st == ACCEPTED).all()
    with pytest.raises(frieda_amd.FriedaError) as e:
        gpu_ctx.reconstruct_from_cell_bundles(root, 4, len(data), 3, bundles[:1], values[:9], witness[: int(wfirst[1])], wfirst[:2])
    assert e.value.status == ERR_ARG and e.value.n_cells_used == 9 and (e.value.bundle_status == ACCEPTED).all()
