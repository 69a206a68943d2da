"""GPU: frieda_verify_pairs_many / frieda_reconstruct_from_proof_pairs — every point an accepted proof authenticates (both members of every
opened first-layer pair), pooled on the device and fed to the erasure-locator reconstruction.

The reference of every check is pairs_util.restate: the pair points written down from the proof's accessors (verify_samples for the
queried positions, layer(0)'s fri_witness for the siblings), and the codeword itself."""
import ctypes as C

import numpy as np
import pytest

from conftest import pattern_bytes, splitmix64_bytes
from pairs_util import ACCEPTED, ERR_ARG, INVARIANT, REJECTED, SENTINEL, WRONG_COMMITMENT, distinct_counts, raw_pairs_many, restate
from test_gpu_verify_many import _bump, mutate

pytestmark = pytest.mark.gpu


def _cfg(nq=20, blowup=4, last=0, pow_bits=4):
    import frieda_amd

    return frieda_amd.PcsConfig(frieda_amd.FriConfig(blowup, last, nq), pow_bits)


@pytest.fixture(scope="module")
def host_ctx():
    """a second context whose verify calls never use the kernel"""
    import frieda_amd

    ctx = frieda_amd.Context(0)
    ctx.set_option("FRIEDA_VERIFY_DEVICE_MIN", 1 << 31)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def dev_ctx():
    """a context whose verify calls always use the kernel for the shapes it takes"""
    import frieda_amd

    ctx = frieda_amd.Context(0)
    ctx.set_option("FRIEDA_VERIFY_DEVICE_MIN", 0)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def kib(gpu_ctx):
    """the 1 KiB blob of the issue (L 7, blowup 2^4: 2^11 positions, 130 points needed) under 12 seeds, 20 queries each"""
    data = splitmix64_bytes(1, 1024).tobytes()
    nf, npad, lg = C.c_size_t(), C.c_size_t(), C.c_uint32()
    assert gpu_ctx._L.frieda_codec_shape(len(data), C.byref(nf), C.byref(npad), C.byref(lg)) == 0 and lg.value == 7
    seeds = list(range(1, 13))
    root, proofs = gpu_ctx.commit_and_generate_proofs_for_seeds(data, seeds, _cfg())
    assert proofs[0].log_size_bound == 7
    return data, root, seeds, proofs


def _encode(ctx, data, B):
    from test_gpu_reconstruct_points import _encode_on_device

    return _encode_on_device(ctx, data, B)


def _check_rows(status, points, proofs, seeds):
    for i, (p, s) in enumerate(zip(proofs, seeds if seeds is not None else [None] * len(proofs))):
        r = restate(p, s)
        if r is None:
            assert status[i] != ACCEPTED and points[i] is None, i
        else:
            assert status[i] == ACCEPTED, (i, int(status[i]))
            assert np.array_equal(points[i][0], r[0]) and np.array_equal(points[i][1], r[1]), i


# ---------------------------------------------------------------- 1 + 2. route parity, the restatement, the codeword
SHAPES = [
    # (bytes, n_queries, blowup, last)
    (1024, 20, 4, 0),
    (1024, 64, 1, 0),   # a 2^8 domain: many pairs with both members queried, many duplicate draws
    (1024, 65, 4, 0),   # the second 64-entry chunk and the carry lane
    (1024, 300, 4, 0),  # q_cap 512
    (16, 20, 4, 0),     # the smallest blob the prover accepts (15 bytes have log_size_bound 0): no inner layer, which the reference's verifier panics on
    (31, 20, 4, 0),     # the smallest blob whose proof verifies: log_size_bound 2, one inner layer
]


@pytest.mark.parametrize("with_seeds", [False, True], ids=["none", "some"])
@pytest.mark.parametrize("nbytes,nq,blowup,last", SHAPES, ids=lambda v: str(v))
def test_route_parity_restatement_and_codeword(gpu_ctx, dev_ctx, host_ctx, nbytes, nq, blowup, last, with_seeds):
    import frieda_amd

    cfg = _cfg(nq, blowup, last)
    if with_seeds:
        data = splitmix64_bytes(40 + nq, nbytes).tobytes()
        seeds = [3, 4, 5]
        _, proofs = gpu_ctx.commit_and_generate_proofs_for_seeds(data, seeds, cfg)
        blobs = [data] * 3
    else:
        blobs = [splitmix64_bytes(50 + i, nbytes).tobytes() for i in range(2)]
        seeds = None
        proofs = [p for _, p in gpu_ctx.commit_and_generate_proof_batch(blobs, None, cfg)]
    expect = ACCEPTED
    if nbytes == 16:
        with pytest.raises(frieda_amd.FriedaError):
            gpu_ctx.commit_and_generate_proof(bytes(15), None, cfg)
        expect = INVARIANT
    res = {}
    for name, ctx in (("device", dev_ctx), ("host", host_ctx)):
        st, pts = ctx.verify_pairs_many(proofs, seeds)
        _check_rows(st, pts, proofs, seeds)
        assert set(st) == {expect}
        res[name] = (st.tobytes(), [None if p is None else (p[0].tobytes(), p[1].tobytes()) for p in pts])
    assert res["device"] == res["host"]
    if expect != ACCEPTED:
        return
    # truth: every returned (position, value) is the codeword's entry
    for b, (pos, val) in zip(blobs, pts):
        ev, L, n = _encode(gpu_ctx, b, blowup)
        assert pos.max() < (1 << n) and np.all(np.diff(pos.astype(np.int64)) > 0)
        assert np.array_equal(ev[:, pos].T, val)


# ---------------------------------------------------------------- 3. nothing tentative leaks
def test_nothing_tentative_leaks(gpu_ctx, dev_ctx, host_ctx, kib):
    import frieda_amd

    data, root, seeds, proofs = kib
    ni = proofs[0].n_inner_layers
    assert ni >= 3
    inner_bad = mutate(proofs[1], lambda d: _bump(d["inner"][ni // 2]["fri"], 1))  # layer 0 passes, a later layer rejects
    last_bad = mutate(proofs[3], lambda d: _bump(d["last"], 0))
    other = gpu_ctx.commit_and_generate_proof(splitmix64_bytes(2, 1024).tobytes(), 5, _cfg())[1]  # another blob: wrong commitment
    short = mutate(proofs[6], lambda d: d.__setitem__("evals", d["evals"][:-4]))
    # the first layer of the two corrupted proofs is intact: their rows ARE written on the device, tentatively
    for m in (inner_bad, last_bad):
        assert m.layer(0)["fri_witness"].tobytes() == proofs[1 if m is inner_bad else 3].layer(0)["fri_witness"].tobytes()
    items = [proofs[0], inner_bad, proofs[2], last_bad, proofs[4], other, short, proofs[7]]
    sds = [seeds[0], seeds[1], seeds[2], seeds[3], seeds[4], 5, seeds[6], seeds[7]]
    expect = [ACCEPTED, REJECTED, ACCEPTED, REJECTED, ACCEPTED, WRONG_COMMITMENT, INVARIANT, ACCEPTED]
    pitch = 47
    out = {}
    for name, ctx in (("device", dev_ctx), ("host", host_ctx)):
        rc, st, pos, val, npts = raw_pairs_many(ctx, items, sds, root, pitch)
        assert rc == 0 and list(st) == expect, (name, list(st))
        for i, e in enumerate(expect):
            if e != ACCEPTED:
                assert npts[i] == 0 and np.all(pos[i] == SENTINEL) and np.all(val[i] == SENTINEL), (name, i)
            else:
                rp, rv = restate(items[i], sds[i])
                k = int(npts[i])
                assert k == len(rp) and np.array_equal(pos[i, :k], rp) and np.array_equal(val[i, :k], rv), (name, i)
                assert np.all(pos[i, k:] == SENTINEL) and np.all(val[i, k:] == SENTINEL), (name, i)
        out[name] = (st.tobytes(), pos.tobytes(), val.tobytes(), npts.tobytes())
    assert out["device"] == out["host"]
    # the mixed list rebuilds exactly what the accepted proofs alone rebuild
    extra, extra_seeds = list(proofs[8:]), list(seeds[8:])
    good = [items[i] for i, e in enumerate(expect) if e == ACCEPTED] + extra
    good_seeds = [sds[i] for i, e in enumerate(expect) if e == ACCEPTED] + extra_seeds
    b1, st1, n1 = dev_ctx.reconstruct_from_proof_pairs(items + extra, sds + extra_seeds, root, len(data))
    b2, st2, n2 = dev_ctx.reconstruct_from_proof_pairs(good, good_seeds, root, len(data))
    assert b1 == b2 == data and n1 == n2 == distinct_counts(good, good_seeds)[1]
    assert list(st1) == expect + [ACCEPTED] * len(extra) and set(st2) == {ACCEPTED}


# ---------------------------------------------------------------- 4. the point of the feature
def test_five_proofs_rebuild_the_blob_only_with_their_siblings(dev_ctx, kib):
    import frieda_amd

    data, root, seeds, proofs = kib
    proofs, seeds = proofs[:5], seeds[:5]  # seeds 1 .. 5: chosen on the CPU from oracle-made proofs of this blob (96 queried, 190 pair points)
    n_queried, n_points = distinct_counts(proofs, seeds)
    print(f"distinct queried positions {n_queried}, distinct pair points {n_points}, needed 130")
    assert n_queried < 130 <= n_points
    with pytest.raises(frieda_amd.FriedaError) as e:
        dev_ctx.reconstruct_from_proofs(proofs, seeds, root, len(data))
    assert e.value.status == ERR_ARG and e.value.n_points == n_queried
    out, st, n = dev_ctx.reconstruct_from_proof_pairs(proofs, seeds, root, len(data))
    assert out == data and set(st) == {ACCEPTED} and n == n_points


# ---------------------------------------------------------------- 5. passes
def test_several_passes_and_a_host_route_proof(gpu_ctx, kib):
    import frieda_amd

    data, root, seeds, proofs = kib
    # more than 1024 queries: a shape the kernel does not take, which the prover produces
    big_cfg = _cfg(1025, 4, 0)
    big = gpu_ctx.commit_and_generate_proof(data, 99, big_cfg)[1]
    items = list(proofs[:5]) + [big] + list(proofs[5:])
    sds = list(seeds[:5]) + [99] + list(seeds[5:])
    one = frieda_amd.Context(0)
    many = frieda_amd.Context(0)
    try:
        for c in (one, many):
            c.set_option("FRIEDA_VERIFY_DEVICE_MIN", 0)
        budget = 3 * len(proofs[0].serialize())  # three small proofs per pass: a dozen proofs take at least four
        assert many._L.frieda_ctx_test_set_verify_pass_bytes(many._h, budget) == 0
        st1, p1 = one.verify_pairs_many(items, sds, root)
        st2, p2 = many.verify_pairs_many(items, sds, root)
        assert set(st1) == {ACCEPTED} and np.array_equal(st1, st2)
        _check_rows(st1, p1, items, sds)
        for a, b in zip(p1, p2):
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        r1 = one.reconstruct_from_proof_pairs(items, sds, root, len(data))
        r2 = many.reconstruct_from_proof_pairs(items, sds, root, len(data))
        assert r1[0] == r2[0] == data and r1[2] == r2[2] == distinct_counts(items, sds)[1]
        # the kernel's proofs alone, in passes: the pool offsets continue across them
        r3 = many.reconstruct_from_proof_pairs(proofs, seeds, root, len(data))
        assert r3[0] == data and r3[2] == distinct_counts(proofs, seeds)[1]
        assert many._L.frieda_ctx_test_set_verify_pass_bytes(many._h, 0) == 0
        assert many.reconstruct_from_proof_pairs(proofs, seeds, root, len(data))[2] == r3[2]
    finally:
        one.close()
        many.close()


# ---------------------------------------------------------------- 6. product-tree route
def test_golden_blob_from_900_proofs(gpu_ctx, dev_ctx, blob):
    """the reference's 128 KiB fixture at the README's sizes: 900 proofs of 20 queries do not hold 2^15 + 2 queried positions; with the
    siblings they do"""
    from util import load_vectors

    golden = load_vectors()["commit"][0]  # the reference's golden root (src/commit.rs:28-38)
    assert golden["input"] == "blob" and golden["log_blowup_factor"] == 4
    cfg = _cfg(20, 4, 0, 0)
    seeds = list(range(1, 901))
    enc = gpu_ctx.encode(blob, 4)
    try:
        root = enc.commitment
        proofs = []
        for at in range(0, 900, 150):
            proofs += gpu_ctx.prove_seeds(enc, seeds[at : at + 150], cfg)
    finally:
        enc.close()
    assert proofs[0].log_size_bound == 15
    assert root.hex() == golden["root"]
    st, pts = dev_ctx.verify_pairs_many(proofs, seeds, root)
    assert set(st) == {ACCEPTED}
    need = (1 << 15) + 2
    n_queried = len(set(np.concatenate([_positions(p, s) for p, s in zip(proofs, seeds)]).tolist()))
    n_points = len(set(np.concatenate([p[0] for p in pts]).tolist()))
    print(f"distinct queried positions {n_queried}, distinct pair points {n_points}, needed {need}")
    assert n_queried < need <= n_points
    # a sample of the rows against the restatement (every row was compared with it at the small shapes)
    for i in range(0, 900, 60):
        rp, rv = restate(proofs[i], seeds[i])
        assert np.array_equal(pts[i][0], rp) and np.array_equal(pts[i][1], rv)
    out, st2, n = dev_ctx.reconstruct_from_proof_pairs(proofs, seeds, root, len(blob))
    assert out == blob and n == n_points and set(st2) == {ACCEPTED}


def _positions(p, s):
    import frieda_amd

    return frieda_amd.verify_samples(p, s)[1]


# ---------------------------------------------------------------- 7. too few points, shapes that disagree
def test_too_few_points_leave_the_buffer_untouched(dev_ctx, kib):
    data, root, seeds, proofs = kib
    L = dev_ctx._L
    out = (C.c_uint8 * len(data))(*([0xAB] * len(data)))
    status = (C.c_uint8 * 3)()
    n = C.c_size_t(0)
    arr = (C.c_void_p * 3)(*[p._h.value for p in proofs[:3]])
    sd = (C.c_uint64 * 3)(*seeds[:3])
    rc = L.frieda_reconstruct_from_proof_pairs(dev_ctx._h, arr, sd, 3, (C.c_uint8 * 32)(*root), len(data), out, status, C.byref(n))
    want = distinct_counts(proofs[:3], seeds[:3])[1]
    assert want < 130
    assert rc == ERR_ARG and n.value == want and bytes(out) == b"\xab" * len(data) and list(status) == [ACCEPTED] * 3
    assert b"130 needed" in L.frieda_last_error(dev_ctx._h)
    # a len that does not match the commitment, with enough points
    import frieda_amd

    with pytest.raises(frieda_amd.FriedaError) as e:
        dev_ctx.reconstruct_from_proof_pairs(proofs, seeds, root, len(data) - 1)
    assert e.value.status == ERR_ARG and e.value.n_points == distinct_counts(proofs, seeds)[1]


def test_shape_disagreement_behaves_as_the_existing_call(dev_ctx, kib):
    """the same codeword read as (L 8, blowup 2^3, last-layer bound 1) verifies — a polynomial below 2^7 coefficients is below 2^8 — but
    disagrees with the proofs before it on the shape: both calls stop there, with the points pooled before it"""
    import frieda_amd

    data, root, seeds, proofs = kib

    def reshape(d):
        d["L"] = 8
        d["cfg"][1] = 3
        d["cfg"][2] = 1

    odd = mutate(proofs[2], reshape)
    assert frieda_amd.verify_samples(odd, seeds[2])[0]
    items, sds = [proofs[0], proofs[1], odd] + list(proofs[3:]), seeds
    nq, npts = distinct_counts(items[:2], sds[:2])
    for call, want in ((dev_ctx.reconstruct_from_proofs, nq), (dev_ctx.reconstruct_from_proof_pairs, npts)):
        with pytest.raises(frieda_amd.FriedaError) as e:
            call(items, sds, root, len(data))
        assert e.value.status == ERR_ARG and "disagree" in str(e.value) and e.value.n_points == want
        assert list(e.value.proof_status) == [ACCEPTED] * len(items)


def test_pitch_below_twice_n_queries_is_refused_and_in_flight(gpu_ctx, kib):
    import frieda_amd

    data, root, seeds, proofs = kib
    rc, st, pos, val, npts = raw_pairs_many(gpu_ctx, proofs[:2], seeds[:2], root, pitch=39)
    assert rc == ERR_ARG and np.all(pos == SENTINEL) and np.all(st == 0xEE)
    gpu_ctx.prove_begin(data, seeds[0], _cfg())
    try:
        for call in (lambda: gpu_ctx.verify_pairs_many(proofs[:2], seeds[:2]), lambda: gpu_ctx.reconstruct_from_proof_pairs(proofs, seeds, root, len(data))):
            with pytest.raises(frieda_amd.FriedaError) as e:
                call()
            assert e.value.status == ERR_ARG
    finally:
        gpu_ctx.prove_finish()
