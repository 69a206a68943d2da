"""Stripe bundles on the GPU: frieda_open_stripe_bundles against the CPU oracle's codewords and trees and against K calls of
frieda_open_cell_bundles, frieda_verify_stripe_bundles_many against the host verifier and the independent check piece for piece,
frieda_reconstruct_blobs_from_stripe_bundles end to end at the shapes of the stripe rebuild.

Shapes are the smallest at which each branch exists: domains 2^5, 2^11 and 2^12; log_cell on both sides of the 16-byte copy and of the
leaf walk (0, 3, 6, 10 and log_cell = log_domain); bundles off the wave size (1, 63, 64, 65, 300), every stripe of the domain (an empty
witness), the cap (1024) and one more; blob counts that are no power of two (3, 5), one blob, 64 and the 1024-column bound (256 blobs
of a 2^5 domain); several verify passes; trees with and without their two lowest node levels in one call."""
import ctypes as C

import numpy as np
import pytest

import bundles_util as B
import stripe_bundles_util as S
import test_cells_blobs_host as H
import workspace_rows as W
from bundles_util import ACCEPTED, MALFORMED, REJECTED
from cells_util import ERR_ARG, POISON
from test_gpu_cells_blobs import STRIPE_CASES, blob_of, close_all, encode_each

pytestmark = pytest.mark.gpu

GUARD = 64
VFILL, WFILL = 0xA5A5A5A5, 0x1234567812345678


# ---- open -------------------------------------------------------------------------------------------------------------------------------
def raw_open(ctx, encs, c, bundles, cap=None, query=False):
    """frieda_open_stripe_bundles into poison-filled buffers between red zones: (rc, values words, witness [K * H, 32], witness_first)"""
    k, n = len(encs), encs[0].shape[1]
    idx = np.ascontiguousarray(np.concatenate(bundles), dtype=np.uint32)
    first = np.concatenate([[0], np.cumsum([len(b) for b in bundles])]).astype(np.uint32)
    nb = len(bundles)
    words = (len(idx) * k * 4) << c
    want_hashes = k * sum(len(B.merge_walk(n - c, b)) for b in bundles) if cap is None else cap
    values = np.full(words + 2 * GUARD, VFILL, dtype=np.uint32)
    witness = np.full(32 * want_hashes + 2 * GUARD, POISON, dtype=np.uint8)
    wfirst = np.full(nb + 1 + GUARD, WFILL, dtype=np.uint64)
    handles = (C.c_void_p * k)(*[e._handle() for e in encs])
    rc = ctx._L.frieda_open_stripe_bundles(ctx._h, handles, k, c, idx.ctypes.data, first.ctypes.data, nb, None if query else values.ctypes.data + 4 * GUARD,
                                           None if query else witness.ctypes.data + GUARD, want_hashes, wfirst.ctypes.data)
    assert (values[:GUARD] == VFILL).all() and (values[GUARD + words:] == VFILL).all(), "red zone around out_values"
    assert (witness[:GUARD] == POISON).all() and (witness[GUARD + 32 * want_hashes:] == POISON).all(), "red zone around out_witness"
    assert (wfirst[nb + 1:] == WFILL).all(), "red zone behind out_witness_first"
    return rc, values[GUARD:GUARD + words], witness[GUARD:GUARD + 32 * want_hashes].reshape(-1, 32), wfirst[: nb + 1]


def check_open(ctx, encs, blobs, c, bundles):
    """values, witness and witness_first equal the oracle's laid out as the header pins it, and the pieces equal K single-blob calls"""
    want = S.build(blobs, c, bundles)
    rc, v, w, wf = raw_open(ctx, encs, c, bundles)
    assert rc == 0, ctx._L.frieda_last_error(ctx._h)
    assert v.tobytes() == want.values.tobytes(), (c, len(bundles))
    assert wf.tolist() == want.wfirst.tolist(), (c, len(bundles))
    assert w.tobytes() == want.witness.tobytes(), (c, len(bundles), np.flatnonzero((w != want.witness).any(axis=1))[:8])
    got = want.replace(values=v.reshape(want.values.shape), witness=w)
    for j, enc in enumerate(encs):
        v1, w1, wf1 = enc.open_cell_bundles(ctx, c, bundles)
        mine = got.blob_call(j)
        assert v1.tobytes() == mine.values.tobytes() and w1.tobytes() == mine.witness.tobytes() and wf1.tolist() == wf.tolist(), (c, j)
    # the size query: out_witness == NULL fills out_witness_first only
    rc, v, w, wf = raw_open(ctx, encs, c, bundles, query=True)
    assert rc == 0 and wf.tolist() == want.wfirst.tolist()
    assert (v == VFILL).all() and (w == POISON).all()
    # cap_hashes one too small (it counts against K * witness_first[n_bundles]): refused, outputs untouched
    if int(want.wfirst[-1]):
        rc, v, w, wf = raw_open(ctx, encs, c, bundles, cap=len(encs) * int(want.wfirst[-1]) - 1)
        assert rc == ERR_ARG and (v == VFILL).all() and (w == POISON).all() and (wf == WFILL).all()
    return want


def open_bundles(n, c):
    """sizes 1, 63, 64, 65 and 300 (as many as the domain has), and every stripe of the domain where the cap allows it"""
    total = 1 << (n - c)
    out = [B.pick(n, c, min(s, total), seed=70 + j) for j, s in enumerate((1, 63, 64, 65, 300))]
    if total <= B.MAX_BUNDLE_CELLS:
        out.append(np.arange(total, dtype=np.uint32))
    return out


@pytest.mark.parametrize("k", [3, 5])
@pytest.mark.parametrize("n", [11, 12])
def test_open_equals_the_oracle_and_k_single_blob_calls(gpu_ctx, n, k):
    blobs = H.block(n, 4, k=k)
    encs = [gpu_ctx.encode(bl[0], 4) for bl in blobs]
    try:
        assert [e.commitment for e in encs] == H.commitments_of(blobs)
        for c in (0, 3, 6):
            want = check_open(gpu_ctx, encs, blobs, c, open_bundles(n, c))
            if (1 << (n - c)) <= B.MAX_BUNDLE_CELLS:
                assert int(want.wfirst[-1]) == int(want.wfirst[-2]), "every stripe of the domain: an empty witness"
        # a malformed bundle refuses the whole call and is named; no bundles: a no-op
        good = B.pick(n, 0, 5, seed=1)
        for bad in (good[::-1].copy(), np.array([0, 1 << n], np.uint32), np.zeros(0, np.uint32), np.array([1, 1], np.uint32)):
            rc, v, w, wf = raw_open(gpu_ctx, encs, 0, [good, bad], cap=64 * k)
            assert rc == ERR_ARG and (v == VFILL).all() and (w == POISON).all() and (wf == WFILL).all()
            assert b"bundle 1" in gpu_ctx._L.frieda_last_error(gpu_ctx._h)
        handles = (C.c_void_p * k)(*[e._handle() for e in encs])
        assert gpu_ctx._L.frieda_open_stripe_bundles(gpu_ctx._h, handles, k, 0, None, None, 0, None, None, 0, None) == 0
        holed = (C.c_void_p * k)(*([encs[0]._handle(), None] + [e._handle() for e in encs[2:]]))
        first, one = np.array([0, 1], np.uint32), np.array([0], np.uint32)
        assert gpu_ctx._L.frieda_open_stripe_bundles(gpu_ctx._h, holed, k, 0, one.ctypes.data, first.ctypes.data, 1, None, None, 0, None) == ERR_ARG
        assert gpu_ctx._L.frieda_open_stripe_bundles(gpu_ctx._h, handles, 0, 0, one.ctypes.data, first.ctypes.data, 1, None, None, 0, None) == ERR_ARG
    finally:
        for e in encs:
            e.close()


@pytest.mark.parametrize("n,b,c,bundles", [(5, 1, 5, [[0]]), (12, 4, 10, [[0, 2], [1], [0, 1, 2, 3]])])
def test_open_at_the_largest_cells(gpu_ctx, n, b, c, bundles):
    """log_cell = log_domain (one cell: nothing to witness) and log_cell 10 on a 2^12 domain"""
    blobs = H.block(n, b, k=3)
    encs = [gpu_ctx.encode(bl[0], b) for bl in blobs]
    try:
        want = check_open(gpu_ctx, encs, blobs, c, [np.array(x, dtype=np.uint32) for x in bundles])
        if c == n:
            assert int(want.wfirst[-1]) == 0
    finally:
        for e in encs:
            e.close()


def test_open_over_blobs_encoded_under_different_skip_thresholds(gpu_ctx):
    """skip_log is per blob: a 2^12 tree without its two lowest node levels (the re-hash route, log_cell <= 2), one with them, and the
    first blob a second time, in one call"""
    two = [blob_of(3000, 4, 501), blob_of(3000, 4, 502)]
    options = [{"FRIEDA_TREE_SKIP_LOG": 10, "FRIEDA_TREE_SKIP_LONE_LOG": 10}, {"FRIEDA_TREE_SKIP_LOG": 40, "FRIEDA_TREE_SKIP_LONE_LOG": 40}]
    made = encode_each(list(zip(two, options, [4, 4])))
    try:
        encs = [made[0][1], made[1][1], made[0][1]]
        blobs = [two[0], two[1], two[0]]
        for c in (0, 1, 2, 3):
            check_open(gpu_ctx, encs, blobs, c, [B.pick(12, c, s, seed=90 + j) for j, s in enumerate((1, 65, 7))])
        # blobs of different log_domain in one call: refused
        enc11 = gpu_ctx.encode(H.block(11, 4, k=1)[0][0], 4)
        try:
            rc, v, w, wf = raw_open(gpu_ctx, [made[0][1], enc11], 0, [np.array([0, 1], np.uint32)], cap=64)
            assert rc == ERR_ARG and b"log_domain" in gpu_ctx._L.frieda_last_error(gpu_ctx._h)
            assert (v == VFILL).all() and (w == POISON).all() and (wf == WFILL).all()
        finally:
            enc11.close()
    finally:
        close_all(made)


def test_open_beside_a_prove_seeds_job_and_refused_in_flight(gpu_ctx):
    """the blobs are only read: another context opens stripe bundles while a prove_seeds job is in flight; the context with the job
    refuses all three context calls with FRIEDA_ERR_ARG"""
    import frieda_amd

    n, c = 11, 3
    blobs = H.block(n, 4, k=2)
    coms = H.commitments_of(blobs)
    cfg = frieda_amd.PcsConfig(frieda_amd.FriConfig(4, 0, 8), 4)
    other = frieda_amd.Context(0)
    encs = [gpu_ctx.encode(bl[0], 4) for bl in blobs]
    try:
        bundles = [B.pick(n, c, 17, seed=1), B.pick(n, c, 5, seed=2)]
        want = S.build(blobs, c, bundles)
        gpu_ctx.prove_seeds_begin(encs[1], [1, 2, 3], cfg)
        try:
            v, w, wf = frieda_amd.open_stripe_bundles(other, encs, c, bundles)
            for call in (lambda: frieda_amd.open_stripe_bundles(gpu_ctx, encs, c, bundles),
                         lambda: gpu_ctx.verify_stripe_bundles_many(coms, n, c, bundles, want.values, want.witness, want.wfirst),
                         lambda: gpu_ctx.reconstruct_blobs_from_stripe_bundles(coms, 4, len(blobs[0][0]), c, bundles, want.values, want.witness, want.wfirst)):
                with pytest.raises(frieda_amd.FriedaError) as e:
                    call()
                assert e.value.status == ERR_ARG and "in flight" in str(e.value)
        finally:
            proofs = gpu_ctx.prove_seeds_finish()
        assert v.tobytes() == want.values.tobytes() and w.tobytes() == want.witness.tobytes() and wf.tolist() == want.wfirst.tolist()
        assert all(frieda_amd.verify(p, s) for p, s in zip(proofs, [1, 2, 3]))
    finally:
        for e in encs:
            e.close()
        other.close()


# ---- verify -----------------------------------------------------------------------------------------------------------------------------
def three_way(ctx, call, want=None, label=None):
    """device == host == independent per piece; returns the status [n_bundles, K]"""
    want = S.independent(call) if want is None else want
    rc_h, host = S.raw_verify(call)
    rc_d, dev = S.raw_verify(call, ctx)
    assert rc_h == 0 and rc_d == 0, (label, rc_h, rc_d, ctx._L.frieda_last_error(ctx._h))
    assert dev.tolist() == host.tolist() == want.tolist(), label
    return want


def small_bundles(n, c):
    total = 1 << (n - c)
    return [B.pick(n, c, min(s, total), seed=40 + j) for j, s in enumerate((5, 2, 9))]


@pytest.mark.parametrize("n,c", [(n, c) for n in (11, 12) for c in (0, 3, 6)] + [(5, 1), (5, 5)])
def test_verify_three_way_on_the_mutation_matrix(gpu_ctx, n, c):
    k, j = 3, 1
    calls = S.blob_calls(H.block(n, 1 if n == 5 else 4, k=k), c, small_bundles(n, c))
    call = S.assemble(calls)
    assert (three_way(gpu_ctx, call, label="intact") == ACCEPTED).all()
    for label, hit, must, shared, mutated in S.mutations(calls, j):
        want = S.independent(mutated)
        S.check_mutation(label, hit, must, shared, j, want)
        three_way(gpu_ctx, mutated, want, label)
    coms = list(call.commitments)
    coms[2] = coms[0]
    want = three_way(gpu_ctx, call.replace(commitments=coms), label="commitment")
    assert (want[:, 2] == REJECTED).all() and (want[:, :2] == ACCEPTED).all()
    # bad call structure: refused, status untouched
    reversed_first = [call.replace(wfirst=call.wfirst[::-1].copy())] if int(call.wfirst[-1]) else []  # (an empty witness reads the same both ways)
    for bad in reversed_first + [call.replace(n=29), call.replace(c=n + 1)]:
        rc, st = S.raw_verify(bad, gpu_ctx)
        assert rc == ERR_ARG and (st == POISON).all()
    rc, st = S.raw_verify(call, gpu_ctx, n_blobs=0)
    assert rc == ERR_ARG and (st == POISON).all()


def flipped_call(n, blowup, c, k, sizes, flips, seed):
    """bundles of `sizes` stripes over k blobs with `flips` single-bit flips, in the values and in the witness in turn"""
    rng = np.random.default_rng(seed)
    call = S.build(H.block(n, blowup, k=k), c, [B.pick(n, c, s, seed=seed + j) for j, s in enumerate(sizes)])
    values, witness = call.values.copy(), call.witness.copy()
    for t in range(flips):
        if t % 2 == 0 or witness.size == 0:
            w = values.reshape(-1)
            w[int(rng.integers(0, w.size))] ^= np.uint32(1 << int(rng.integers(0, 32)))
        else:
            p = witness.reshape(-1)
            p[int(rng.integers(0, p.size))] ^= np.uint8(1 << int(rng.integers(0, 8)))
    return call.replace(values=values, witness=witness)


def staged_bytes(call):
    k, vb = call.k, 16 << call.c
    return [12 + 4 * len(i) + k * (len(i) * vb + 32 * int(w1 - w0)) for i, w0, w1 in zip(call.bundles, call.wfirst[:-1], call.wfirst[1:])]


@pytest.mark.parametrize("passes", [1, 4])
def test_verify_many_on_random_bit_flips(gpu_ctx, passes):
    """120 bundles of 1 .. 9 stripes over 3 blobs at log_domain 12, log_cell 3, 200 flipped bits in values and witness; in one pass and
    with a quarter of the staged bytes per pass: at least four passes"""
    call = flipped_call(12, 4, 3, 3, [1 + (t * 7) % 9 for t in range(120)], 200, seed=2025)
    want = S.independent(call)
    assert 0 < (want == REJECTED).sum() <= 200 and not (want == MALFORMED).any() and (want == ACCEPTED).sum() >= 160  # (360 bytes, a flip spoils one)
    pass_bytes = 0
    if passes > 1:
        pass_bytes = sum(staged_bytes(call)) // passes
        assert pass_bytes > max(staged_bytes(call))
    assert gpu_ctx._L.frieda_ctx_test_set_verify_pass_bytes(gpu_ctx._h, pass_bytes) == 0
    try:
        three_way(gpu_ctx, call, want)
    finally:
        gpu_ctx._L.frieda_ctx_test_set_verify_pass_bytes(gpu_ctx._h, 0)


@pytest.mark.parametrize("nb,k", [(1, 1), (1, 3), (65, 3), (300, 3), (1, 64), (65, 64)])
def test_verify_many_bundle_and_blob_counts(gpu_ctx, nb, k):
    """The oracle-side accepted count is checked first to lie strictly between 0 and the number of status bytes.  One byte can only be 0
    or 1: that shape runs twice, untouched (accepted) and with one flipped bit (rejected), so both values are seen."""
    n, blowup, c = (5, 1, 1) if k == 64 else (11, 4, 3)
    sizes = [1 + (t * 5) % 4 for t in range(nb)]
    seen = set()
    for flips in ([0, 1] if nb * k == 1 else [(nb * k + 2) // 3]):
        call = flipped_call(n, blowup, c, k, sizes, flips, seed=300 + nb + k)
        want = S.independent(call)
        if nb * k > 1:
            assert 0 < (want == ACCEPTED).sum() < nb * k
        three_way(gpu_ctx, call, want, (nb, k, flips))
        seen |= set(want.reshape(-1).tolist())
    assert seen == {ACCEPTED, REJECTED}


def test_verify_many_the_cap_and_one_more(gpu_ctx):
    """1024 stripes in one bundle are accepted (36 KB of LDS per wave), 1025 are malformed for every blob"""
    n, c, k = 12, 0, 3
    sizes = (1, 300, 1024, 1025, 64)
    call = S.build(H.block(n, 4, k=k), c, [B.pick(n, c, s, seed=80 + j) for j, s in enumerate(sizes)])
    rc_h, host = S.raw_verify(call)
    rc_d, dev = S.raw_verify(call, gpu_ctx)
    assert rc_h == 0 and rc_d == 0
    assert dev.tolist() == host.tolist() == [[MALFORMED if s > 1024 else ACCEPTED] * k for s in sizes]
    # one word of the cap bundle's last stripe changed in one blob
    v = call.values.copy()
    v[int(call.first[3]) - 1, 1, 3, 0] ^= 1
    want = [[ACCEPTED] * k, [ACCEPTED] * k, [ACCEPTED, REJECTED, ACCEPTED], [MALFORMED] * k, [ACCEPTED] * k]
    rc_h, host = S.raw_verify(call.replace(values=v))
    rc_d, dev = S.raw_verify(call.replace(values=v), gpu_ctx)
    assert rc_h == 0 and rc_d == 0 and dev.tolist() == host.tolist() == want


# ---- rebuild ----------------------------------------------------------------------------------------------------------------------------
def raw_reconstruct(ctx, call, blowup, length, n_blobs=None):
    """frieda_reconstruct_blobs_from_stripe_bundles into poison-filled buffers between red zones: (rc, [bytes] or None, status [n_bundles, K], used)"""
    com, idx, first, values, witness, wfirst = S.host_arrays(call)
    nb, k = len(call.bundles), call.k
    buf = np.full(k * length + 2 * GUARD, POISON, dtype=np.uint8)
    status = np.full(nb * k + GUARD, POISON, dtype=np.uint8)
    used = C.c_size_t(12345)
    rc = ctx._L.frieda_reconstruct_blobs_from_stripe_bundles(ctx._h, com.ctypes.data, k if n_blobs is None else n_blobs, blowup, length, call.c, idx.ctypes.data,
                                                             first.ctypes.data, nb, values.ctypes.data, witness.ctypes.data if witness.size else None,
                                                             wfirst.ctypes.data, buf.ctypes.data + GUARD, status.ctypes.data, C.byref(used))
    assert (buf[:GUARD] == POISON).all() and (buf[GUARD + k * length:] == POISON).all(), "red zone around out_bytes"
    assert (status[nb * k:] == POISON).all(), "red zone behind out_status"
    body = buf[GUARD:GUARD + k * length]
    if rc != 0:
        assert (body == POISON).all(), "out_bytes written by a failed call"
    out = [body[b * length:(b + 1) * length].tobytes() for b in range(k)] if rc == 0 else None
    return rc, out, status[: nb * k].reshape(nb, k), used.value


@pytest.mark.parametrize("multi_pass", [False, True])
@pytest.mark.parametrize("n,blowup,k,c", STRIPE_CASES)
def test_reconstruct_blobs_from_stripe_bundles(gpu_ctx, n, blowup, k, c, multi_pass):
    blobs = H.block(n, blowup, k=k)
    length, L = len(blobs[0][0]), n - blowup
    need = (1 << (L - c)) + 1 if c else (1 << L) + 2
    if (n, k) == (5, 256):
        assert need == 9 and 4 * k == 1024
    rng = np.random.default_rng(400 + n + c + k)
    perm = rng.permutation(1 << (n - c)).astype(np.uint32)
    cuts = [0, need // 3, 2 * (need // 3), need]
    three = [np.sort(perm[a:z]) for a, z in zip(cuts[:-1], cuts[1:])]  # exactly enough stripes, over three bundles
    spare = np.sort(perm[need:need + 2])
    want_data = [bl[0] for bl in blobs]
    full = S.build(blobs, c, three + [spare])
    assert (S.independent(full) == ACCEPTED).all() if k <= 5 else True
    t, jb = int(rng.integers(0, 2)), int(rng.integers(0, k))
    vbad = full.values.copy()
    vbad[int(full.first[3]) + t, jb, 1, 0] ^= 2
    damaged = full.replace(values=vbad)  # the fourth bundle: one corrupted word in one blob
    pass_bytes = 0
    if multi_pass:  # one byte less than the first two bundles stage: at least three passes, cut at bundle boundaries
        pass_bytes = sum(staged_bytes(full)[:2]) - 1
    assert gpu_ctx._L.frieda_ctx_test_set_verify_pass_bytes(gpu_ctx._h, pass_bytes) == 0
    try:
        # exactly the minimum number of distinct stripes, plus a bundle that one blob spoils: the whole bundle is left out
        rc, out, st, used = raw_reconstruct(gpu_ctx, damaged, blowup, length)
        assert rc == 0, gpu_ctx._L.frieda_last_error(gpu_ctx._h)
        assert out == want_data and used == need
        assert np.argwhere(st != ACCEPTED).tolist() == [[3, jb]] and st[3, jb] == REJECTED

        # all four bundles intact: every stripe counts
        rc, out, st, used = raw_reconstruct(gpu_ctx, full, blowup, length)
        assert rc == 0 and out == want_data and used == need + 2 and (st == ACCEPTED).all()

        # one stripe short: too few, the statuses are valid, the output keeps its poison
        rest = [three[2][:-1]] if len(three[2]) > 1 else []  # (a bundle of one stripe goes as a whole: an empty bundle is malformed)
        short = S.build(blobs, c, three[:2] + rest + [spare])
        last = len(short.bundles) - 1
        vs = short.values.copy()
        vs[int(short.first[last]) + t, jb, 1, 0] ^= 2
        rc, out, st, used = raw_reconstruct(gpu_ctx, short.replace(values=vs), blowup, length)
        assert rc == ERR_ARG and used == need - 1 and b"needed" in gpu_ctx._L.frieda_last_error(gpu_ctx._h)
        assert np.argwhere(st != ACCEPTED).tolist() == [[last, jb]]

        # stripes repeated across bundles count once
        rep = S.build(blobs, c, three[:2] + rest + [three[0]])
        rc, out, st, used = raw_reconstruct(gpu_ctx, rep, blowup, length)
        assert rc == ERR_ARG and used == need - 1 and (st == ACCEPTED).all()
        rep = S.build(blobs, c, three + [three[0]])
        rc, out, st, used = raw_reconstruct(gpu_ctx, rep, blowup, length)
        assert rc == 0 and out == want_data and used == need and (st == ACCEPTED).all()

        # a wrong len (same polynomial size; blob 0's last byte is not zero, so its shorter form commits elsewhere): every bundle
        # verifies, the commitment check fails and names the blob
        assert want_data[0][-1] != 0
        ok = S.build(blobs, c, three)
        rc, out, st, used = raw_reconstruct(gpu_ctx, ok, blowup, length - 1)
        assert rc == ERR_ARG and used == need and (st == ACCEPTED).all()
        err = gpu_ctx._L.frieda_last_error(gpu_ctx._h)
        assert b"commit" in err and b"blob 0" in err

        # one commitment of the block swapped for another blob's: that blob's piece of every bundle is rejected, so no bundle is used
        swapped = list(ok.commitments)
        swapped[k - 1] = ok.commitments[0]
        rc, out, st, used = raw_reconstruct(gpu_ctx, ok.replace(commitments=swapped), blowup, length)
        if k > 1:
            assert rc == ERR_ARG and used == 0
            assert (st[:, k - 1] == REJECTED).all() and (st[:, : k - 1] == ACCEPTED).all()
    finally:
        gpu_ctx._L.frieda_ctx_test_set_verify_pass_bytes(gpu_ctx._h, 0)


def test_reconstruct_argument_errors(gpu_ctx):
    n, blowup, c, k = 11, 4, 3, 3
    blobs = H.block(n, blowup, k=k)
    length = len(blobs[0][0])
    call = S.build(blobs, c, [np.arange(9, dtype=np.uint32), np.arange(9, 17, dtype=np.uint32)])
    for n_blobs in (0, 257):
        rc, out, st, used = raw_reconstruct(gpu_ctx, call, blowup, length, n_blobs=n_blobs)
        assert rc == ERR_ARG and (st == POISON).all() and used == 0 and b"n_blobs" in gpu_ctx._L.frieda_last_error(gpu_ctx._h)
    # a malformed bundle is a status, not an argument error: its row is 2, the other bundle does not suffice
    bad = call.replace(bundles=[call.bundles[0][::-1].copy(), call.bundles[1]])
    rc, out, st, used = raw_reconstruct(gpu_ctx, bad, blowup, length)
    assert rc == ERR_ARG and st.tolist() == [[MALFORMED] * k, [ACCEPTED] * k] and used == 8
    # no bundles at all is "too few"
    rc, out, st, used = raw_reconstruct(gpu_ctx, call.replace(bundles=[], wfirst=call.wfirst[:1]), blowup, length)
    assert rc == ERR_ARG and used == 0 and b"needed" in gpu_ctx._L.frieda_last_error(gpu_ctx._h)


# ---- other ------------------------------------------------------------------------------------------------------------------------------
def test_one_blob_is_the_single_blob_bundle_call(gpu_ctx):
    """K = 1: the bytes, statuses and rebuilt blob of frieda_open_cell_bundles, frieda_verify_cell_bundles_many and
    frieda_reconstruct_from_cell_bundles on the same input (one bundle rejected, one spare)"""
    import frieda_amd
    from test_gpu_bundles import raw_reconstruct as raw_one

    n, blowup, c = 11, 4, 3
    data, ev, layers = H.block(n, blowup, k=1)[0]
    need = (1 << (n - blowup - c)) + 1
    perm = np.random.default_rng(8).permutation(1 << (n - c)).astype(np.uint32)
    bundles = [np.sort(perm[:9]), np.sort(perm[9:need - 1]), np.sort(perm[need:need + 3]), np.sort(perm[need + 3:need + 12])]  # 9 + 7 < need <= 9 + 7 + 9
    enc = gpu_ctx.encode(data, blowup)
    try:
        v1, w1, wf1 = enc.open_cell_bundles(gpu_ctx, c, bundles)
        v, w, wf = frieda_amd.open_stripe_bundles(gpu_ctx, [enc], c, bundles)
    finally:
        enc.close()
    assert v.shape == (len(v1), 1, 4, 1 << c) and v.tobytes() == v1.tobytes() and w.tobytes() == w1.tobytes() and wf.tolist() == wf1.tolist()
    one = B.build_call(ev, layers, c, bundles)
    assert v1.tobytes() == one.values.tobytes() and w1.tobytes() == one.witness.tobytes()
    values = one.values.copy()
    values[int(one.first[2]), 2, 1] ^= 1  # the third bundle is rejected
    for count in (4, 3, 2):
        single = B.build_call(ev, layers, c, bundles[:count]).replace(values=values[: int(one.first[count])])
        block = S.assemble([single])
        rc_a, st_a = B.raw_verify(single, gpu_ctx)
        rc_b, st_b = S.raw_verify(block, gpu_ctx)
        assert rc_a == rc_b == 0 and st_a.tolist() == st_b[:, 0].tolist()
        rc1, out1, st1, used1 = raw_one(gpu_ctx, single, blowup, len(data))
        rc2, out2, st2, used2 = raw_reconstruct(gpu_ctx, block, blowup, len(data))
        assert (rc1, used1, st1.tolist()) == (rc2, used2, st2[:, 0].tolist()), count
        assert rc1 == (0 if count == 4 else ERR_ARG)
        if rc1 == 0:
            assert out2 == [out1] == [data]


def test_same_bytes_on_a_poisoned_workspace_and_a_callers_stream():
    """open, verify and rebuild on a private and on a caller's stream, on a fresh context and after frieda_ctx_test_poison has filled the
    arena and the pinned blocks with 0x00000000, 0xFFFFFFFF and 0x7FFFFFFF: the same bytes every time"""
    import torch

    import frieda_amd

    k = 3
    flipped = flipped_call(12, 4, 1, k, [1, 65, 300, 2, 64], 6, seed=11)
    _, host = S.raw_verify(flipped)
    assert (host == REJECTED).any() and (host == ACCEPTED).any()
    n, blowup, c = 11, 4, 3
    blobs = H.block(n, blowup, k=k)
    perm = np.random.default_rng(21).permutation(1 << (n - c)).astype(np.uint32)
    bundles = [np.sort(perm[:9]), np.sort(perm[9:18]), np.sort(perm[18:19])]
    want = S.build(blobs, c, bundles)
    data = [bl[0] for bl in blobs]
    stream = torch.cuda.Stream()
    for ctx in (frieda_amd.Context(0), frieda_amd.Context(0, stream=stream.cuda_stream)):
        try:
            encs = [ctx.encode(d, blowup) for d in data]
            for word in (None, 0x00000000, 0xFFFFFFFF, 0x7FFFFFFF):
                if word is not None:
                    W.poison(ctx, word)
                rc, dev = S.raw_verify(flipped, ctx)
                assert rc == 0 and dev.tolist() == host.tolist(), word
                v, w, wf = frieda_amd.open_stripe_bundles(ctx, encs, c, bundles)
                assert v.tobytes() == want.values.tobytes() and w.tobytes() == want.witness.tobytes() and wf.tolist() == want.wfirst.tolist(), word
                rc, out, st, used = raw_reconstruct(ctx, want, blowup, len(data[0]))
                assert rc == 0 and out == data and used == 19 and (st == ACCEPTED).all(), word
            for e in encs:
                e.close()
        finally:
            ctx.close()


def test_python_surface(gpu_ctx):
    import frieda_amd

    n, blowup, c, k = 11, 4, 3, 3
    blobs = H.block(n, blowup, k=k)
    coms = H.commitments_of(blobs)
    data = [bl[0] for bl in blobs]
    encs = [gpu_ctx.encode(d, blowup) for d in data]
    try:
        perm = np.random.default_rng(4).permutation(1 << (n - c)).astype(np.uint32)
        bundles = [np.sort(perm[:9]), np.sort(perm[9:17])]
        values, witness, wfirst = frieda_amd.open_stripe_bundles(gpu_ctx, encs, c, bundles)
    finally:
        for e in encs:
            e.close()
    assert values.shape == (17, k, 4, 1 << c) and witness.shape == (k * int(wfirst[-1]), 32)
    want = S.build(blobs, c, bundles)
    assert values.tobytes() == want.values.tobytes() and witness.tobytes() == want.witness.tobytes()
    ok = [[ACCEPTED] * k] * 2
    assert gpu_ctx.verify_stripe_bundles_many(coms, n, c, bundles, values, witness, wfirst).tolist() == ok
    assert frieda_amd.verify_stripe_bundles(coms, n, c, bundles, values, witness, wfirst).tolist() == ok
    out, st, used = gpu_ctx.reconstruct_blobs_from_stripe_bundles(coms, blowup, len(data[0]), c, bundles, values, witness, wfirst)
    assert out == data and used == 17 and st.tolist() == ok
    one = S.build(blobs, c, bundles[:1])
    with pytest.raises(frieda_amd.FriedaError) as e:
        gpu_ctx.reconstruct_blobs_from_stripe_bundles(coms, blowup, len(data[0]), c, bundles[:1], one.values, one.witness, one.wfirst)
    assert e.value.status == ERR_ARG and e.value.n_stripes_used == 9 and e.value.bundle_status.shape == (1, k) and (e.value.bundle_status == ACCEPTED).all()
