"""GPU: block proofs (frieda_prove_block_seeds, frieda_verify_block): one FRI proof for all blobs of a block.

For every shape: the client's check accepts every proof under its own seed; the FRI part is byte for byte frieda_prove_seeds of the
aggregate; the opening part is byte for byte frieda_open_stripe_bundles at the indices the proof's queries give; the host and device
stripe-bundle verifiers and the ordinary verifiers accept the parts; the wire image round-trips.  The sum the client checks is
recomputed here from the oracle's multiplication for every opened pair.  Every tampering is rejected with the reason of the first step
that can see it.

The case (len 1, K 2, S 1) of the grid is a blob of one felt: its polynomial has 2^0 coefficients per column, where the reference's
prover panics and frieda_prove_seeds returns FRIEDA_ERR_INVARIANT.  frieda_prove_block_seeds follows the calls it is made of, so the
case asserts exactly that; (32, 2, 1) — two coefficients per column are still too few: the reference's verifier panics on a proof without
inner layers — is the shortest blob whose proof verifies, and runs the full checks next to it."""
import numpy as np
import pytest

from block_util import combine_values, oracle_rho
from conftest import splitmix64_bytes
from workspace_rows import cfg_of

pytestmark = pytest.mark.gpu

P = 2**31 - 1
OK, SHAPE, FRI, INDICES, BUNDLE, COMBINATION = range(6)


def blob(length, seed):
    return splitmix64_bytes(0xB10C2 + 1000 * seed + length % 997, length).tobytes()


def indices_of(fri, seed):
    import frieda_amd

    ok, positions = frieda_amd.verify_samples(fri, seed)
    assert ok
    return np.unique(positions >> 1).astype(np.uint32)


def full_checks(ctx, oracle, encs, agg, seeds, cfg):
    import frieda_amd

    commitments = [e.commitment for e in encs]
    n = encs[0].shape[1]
    k = len(encs)
    rho = oracle_rho(oracle, commitments)
    assert frieda_amd.block_challenge(commitments) == rho
    bps = ctx.prove_block_seeds(agg, encs, seeds, cfg)
    assert len(bps) == len(seeds)
    for seed, bp in zip(seeds, bps):
        assert frieda_amd.verify_block(commitments, bp, seed) == (True, OK)
        # the FRI part: exactly the proof of the aggregate under this seed
        fri = bp.fri
        assert fri.serialize() == ctx.prove_seeds(agg, [seed], cfg)[0].serialize()
        assert fri.commitment == agg.commitment
        assert frieda_amd.verify(fri, seed)
        assert list(ctx.verify_many([fri], [seed])) == [1]
        # the opening part: exactly the stripe bundle at the indices the queries give
        idx = indices_of(fri, seed)
        assert bp.n_blobs == k and bp.n_stripes == len(idx) and np.array_equal(bp.stripe_index, idx)
        values, witness, wfirst = frieda_amd.open_stripe_bundles(ctx, encs, 1, [idx])
        assert bp.witness_hashes == int(wfirst[1])
        assert bp.values.tobytes() == values.tobytes() and bp.witness.tobytes() == witness.tobytes()
        assert np.all(frieda_amd.verify_stripe_bundles(commitments, n, 1, [bp.stripe_index], bp.values, bp.witness, [0, bp.witness_hashes]) == 1)
        assert np.all(ctx.verify_stripe_bundles_many(commitments, n, 1, [bp.stripe_index], bp.values, bp.witness, [0, bp.witness_hashes]) == 1)
        # the combination, from the oracle's arithmetic: both entries of every opened pair
        ok, pos, val = frieda_amd.verify_pairs(fri, seed)
        assert ok and np.array_equal(pos, (2 * idx[:, None] + np.arange(2, dtype=np.uint32)).reshape(-1))
        for t in range(len(idx)):
            for e in range(2):
                assert combine_values(oracle, bp.values[t, :, :, e], rho) == tuple(int(v) for v in val[2 * t + e]), (t, e)
        # the wire image
        image = bp.serialize()
        back = frieda_amd.BlockProof.from_bytes(image)
        assert back.serialize() == image
        assert frieda_amd.verify_block(commitments, back, seed) == (True, OK)
        assert frieda_amd.BlockProof.from_parts(fri, bp.stripe_index, bp.values, bp.witness).serialize() == image
        # another seed's proof is not this seed's
        assert frieda_amd.verify_block(commitments, bp, seed + 1) == (False, FRI)
    return bps


@pytest.mark.parametrize("length,k,s", [(1, 2, 1), (32, 2, 1), (1024, 3, 2), (1024, 17, 3), (131072, 4, 2)])
def test_block_proofs_verify_and_are_made_of_the_two_calls(gpu_ctx, oracle, length, k, s):
    import frieda_amd

    cfg = cfg_of(4, 4, 0, 20)
    seeds = [100 + i for i in range(s)]
    encs = gpu_ctx.encode_batch([blob(length, i) for i in range(k)], 4)
    try:
        with gpu_ctx.aggregate_encoded(encs) as agg:
            if encs[0].shape[0] < 1:
                # one coefficient per column: no proof exists (the reference panics), of the aggregate as of any blob
                with pytest.raises(frieda_amd.FriedaPanic):
                    gpu_ctx.prove_seeds(agg, seeds, cfg)
                with pytest.raises(frieda_amd.FriedaPanic):
                    gpu_ctx.prove_block_seeds(agg, encs, seeds, cfg)
                return
            full_checks(gpu_ctx, oracle, encs, agg, seeds, cfg)
    finally:
        for e in encs:
            e.close()


def test_three_hundred_queries(gpu_ctx, oracle):
    encs = gpu_ctx.encode_batch([blob(1024, i) for i in range(3)], 4)
    try:
        with gpu_ctx.aggregate_encoded(encs) as agg:
            (bp,) = full_checks(gpu_ctx, oracle, encs, agg, [5], cfg_of(4, 4, 0, 300))
            assert 150 < bp.n_stripes <= 300
    finally:
        for e in encs:
            e.close()


@pytest.fixture(scope="module")
def block(gpu_ctx):
    """one small block of three blobs, a fourth blob of the same shape, the aggregate and one proof"""
    cfg = cfg_of(4, 4, 0, 20)
    encs = gpu_ctx.encode_batch([blob(1024, i) for i in range(4)], 4)
    agg = gpu_ctx.aggregate_encoded(encs[:3])
    seed = 11
    (bp,) = gpu_ctx.prove_block_seeds(agg, encs[:3], [seed], cfg)
    yield {"cfg": cfg, "encs": encs[:3], "other": encs[3], "agg": agg, "seed": seed, "bp": bp, "commitments": [e.commitment for e in encs[:3]]}
    agg.close()
    for e in encs:
        e.close()


def test_rejections_name_the_first_failing_step(gpu_ctx, block):
    import frieda_amd

    V, BP = frieda_amd.verify_block, frieda_amd.BlockProof
    com, bp, seed, encs = block["commitments"], block["bp"], block["seed"], block["encs"]
    idx, values, witness = bp.stripe_index, bp.values, bp.witness
    n = encs[0].shape[1]
    assert V(com, bp, seed) == (True, OK)
    # FRI: a wrong seed, no seed, the nonce
    assert V(com, bp, seed + 1) == (False, FRI)
    assert V(com, bp, None) == (False, FRI)
    fri = bp.fri
    fri.proof_of_work = fri.proof_of_work + 1
    assert V(com, BP.from_parts(fri, idx, values, witness), seed) == (False, FRI)
    # BUNDLE: one value word of blob 1 at one stripe
    j, t = 1, len(idx) // 2
    bad = values.copy()
    bad[t, j, 2, 1] = (int(bad[t, j, 2, 1]) + 1) % P
    assert V(com, BP.from_parts(bp.fri, idx, bad, witness), seed) == (False, BUNDLE)
    # COMBINATION: blob 1's piece and commitment replaced by those of another blob of the same shape opened at the same indices
    o_values, o_witness, _ = frieda_amd.open_stripe_bundles(gpu_ctx, [block["other"]], 1, [idx])
    forged_v, forged_w, forged_c = values.copy(), witness.copy(), list(com)
    forged_v[:, j] = o_values[:, 0]
    forged_w[j] = o_witness.reshape(1, -1, 32)[0]
    forged_c[j] = block["other"].commitment
    assert np.all(frieda_amd.verify_stripe_bundles(forged_c, n, 1, [idx], forged_v, forged_w, [0, bp.witness_hashes]) == 1)
    assert V(forged_c, BP.from_parts(bp.fri, idx, forged_v, forged_w), seed) == (False, COMBINATION)
    # ... and with the commitments left alone that piece does not open: BUNDLE
    assert V(com, BP.from_parts(bp.fri, idx, forged_v, forged_w), seed) == (False, BUNDLE)
    # COMBINATION: two commitments swapped together with their pieces (every bundle verifies, rho is another)
    perm = [1, 0, 2]
    sw_v, sw_w, sw_c = np.ascontiguousarray(values[:, perm]), np.ascontiguousarray(witness[perm]), [com[p] for p in perm]
    assert np.all(frieda_amd.verify_stripe_bundles(sw_c, n, 1, [idx], sw_v, sw_w, [0, bp.witness_hashes]) == 1)
    assert frieda_amd.block_challenge(sw_c) != frieda_amd.block_challenge(com)
    assert V(sw_c, BP.from_parts(bp.fri, idx, sw_v, sw_w), seed) == (False, COMBINATION)
    # INDICES: a stripe dropped, an extra stripe appended or inserted, each with the witness that belongs to it
    absent = [i for i in range(1 << (n - 1)) if i not in set(int(x) for x in idx)]
    for other_idx in (idx[:-1], idx[1:], np.append(idx, max(int(idx[-1]) + 1, absent[-1])), np.sort(np.append(idx, absent[0]))):
        other_idx = np.asarray(other_idx, dtype=np.uint32)
        if len(np.unique(other_idx)) != len(other_idx) or other_idx[-1] >= 1 << (n - 1):
            continue
        v2, w2, _ = frieda_amd.open_stripe_bundles(gpu_ctx, encs, 1, [other_idx])
        forged = BP.from_parts(bp.fri, other_idx, v2, w2)
        assert np.all(frieda_amd.verify_stripe_bundles(com, n, 1, [other_idx], forged.values, forged.witness, [0, forged.witness_hashes]) == 1)
        assert V(com, forged, seed) == (False, INDICES)
    # SHAPE: another number of commitments
    assert V(com[:2], bp, seed) == (False, SHAPE)
    assert V(com + [com[0]], bp, seed) == (False, SHAPE)
    # and nothing above changed the proof
    assert V(com, bp, seed) == (True, OK)


def test_wire_images_that_are_refused(block):
    import frieda_amd

    image = block["bp"].serialize()
    for bad in (image[:-1], image + b"\0", image[:31], b"", b"X" + image[1:], image[:4] + b"\2" + image[5:]):
        with pytest.raises(frieda_amd.FriedaError) as e:
            frieda_amd.BlockProof.from_bytes(bad)
        assert e.value.status == 1
    # indices that are not strictly ascending, a witness count the indices do not give, a broken proof image
    bp = block["bp"]
    idx = bp.stripe_index.copy()
    idx[[0, 1]] = idx[[1, 0]]
    for make in (
        lambda: frieda_amd.BlockProof.from_parts(bp.fri, idx, bp.values, bp.witness),
        lambda: frieda_amd.BlockProof.from_parts(bp.fri, bp.stripe_index, bp.values, bp.witness[:, :-1]),
        lambda: frieda_amd.BlockProof.from_bytes(image[:32] + b"\xff" * 8 + image[40:]),
    ):
        with pytest.raises(frieda_amd.FriedaError) as e:
            make()
        assert e.value.status == 1


def test_prover_argument_errors(gpu_ctx, block):
    import frieda_amd

    cfg, encs, agg, other = block["cfg"], block["encs"], block["agg"], block["other"]

    def refused(*args):
        with pytest.raises(frieda_amd.FriedaError) as e:
            gpu_ctx.prove_block_seeds(*args)
        assert e.value.status == 1, e.value
        return str(e.value)

    # an aggregate of other blobs, of the same blobs in another order, of another number of blobs; no aggregate at all; a given rho
    with gpu_ctx.aggregate_encoded([encs[0], encs[1], other]) as wrong:
        assert "not made from these commitments" in refused(wrong, encs, [1], cfg)
    with gpu_ctx.aggregate_encoded([encs[1], encs[0], encs[2]]) as wrong:
        assert "not made from these commitments" in refused(wrong, encs, [1], cfg)
    with gpu_ctx.aggregate_encoded(encs[:2]) as wrong:
        assert "not an aggregate of n_blobs" in refused(wrong, encs, [1], cfg)
    assert "not an aggregate" in refused(encs[0], encs, [1], cfg)
    with gpu_ctx.aggregate_encoded(encs, rho=(1, 0, 0, 0)) as wrong:
        assert "not made from these commitments" in refused(wrong, encs, [1], cfg)
    # more queries than a bundle holds cells; no seeds; another blow-up
    assert "n_queries" in refused(agg, encs, [1], cfg_of(4, 4, 0, 1025))
    refused(agg, encs, [], cfg)
    refused(agg, encs, [1], cfg_of(4, 3, 0, 20))
    # the context stays usable, and 1024 queries are allowed
    (bp,) = gpu_ctx.prove_block_seeds(agg, encs, [2], cfg_of(4, 4, 0, 1024))
    assert frieda_amd.verify_block(block["commitments"], bp, 2) == (True, OK)
    assert bp.n_stripes <= 1024
