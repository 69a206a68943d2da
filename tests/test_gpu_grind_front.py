"""GPU: the batched proof-of-work search under the front rule (frieda_amd/csrc/tree.hip grind_dev_kernel; option FRIEDA_GRIND_FRONT_WGS): with k
blobs still searching only max(k x the launch's workgroups per blob, FRIEDA_GRIND_FRONT_WGS) workgroups go on claiming windows.  Whatever
leaves, every blob's nonce must stay the MINIMUM qualifying nonce — the reference's sequential search — and the proof the oracle's.

Batches of 1, 2, 3, 15, 16, 17 and 40 blobs of a 2^12 domain, pow_bits 0, 1, 8, 16, 20, each with the default front, with a front of 4
workgroups (so that workgroups do leave in launches of 64 .. 2048) and with the rule off; all of it again with a 2^10-nonce first range (test
hook), which sends every blob whose nonce lies beyond it through the next-range retry of prove_finish_batch.  A batch of 40 repeats
twenty (blob, seed) pairs: equal transcripts, equal nonces.  Batches of 65 and 130 blobs (pow_bits 8 and 16) are launched without the
rule — wave 0's one ballot no longer sees the whole batch — whatever the option says: the same nonces and proofs.
"""
import pytest

from conftest import splitmix64_bytes
from util import blob_len_for

pytestmark = pytest.mark.gpu

BATCHES = (1, 2, 3, 15, 16, 17, 40)
POW_BITS = (0, 1, 8, 16, 20)
FRONTS = (None, 4, 0)  # None: the default
N_PAIRS, N_QUERIES = 20, 4
_want = {}


def pairs():
    n = blob_len_for(12) - 7
    return [(splitmix64_bytes(5300 + i, n).tobytes(), 900 + i) for i in range(N_PAIRS)]


def oracle_proofs(oracle, pow_bits):
    """[(root, proof bytes, nonce)] of the twenty pairs"""
    if pow_bits not in _want:
        ocfg = oracle.make_config(pow_bits, 4, 0, N_QUERIES)
        out = []
        for b, s in pairs():
            r, p = oracle.commit_and_generate_proof(b, s, ocfg)
            out.append((bytes(r), p.serialize(), int(p.c.proof_of_work)))
        _want[pow_bits] = out
    return _want[pow_bits]


@pytest.fixture(scope="module")
def ctx():
    import frieda_amd

    c = frieda_amd.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("first_log", [0, 10])
@pytest.mark.parametrize("pow_bits", POW_BITS)
def test_minimum_nonce_in_every_batch(ctx, oracle, pow_bits, first_log):
    import frieda_amd

    cfg = frieda_amd.PcsConfig(frieda_amd.FriConfig(4, 0, N_QUERIES), pow_bits)
    want = oracle_proofs(oracle, pow_bits)
    pr = pairs()
    assert ctx._L.frieda_ctx_test_set_grind_first_log(ctx._h, first_log) == 0
    try:
        for front in FRONTS:
            ctx.set_option("FRIEDA_GRIND_FRONT_WGS", 768 if front is None else front)
            for count in BATCHES:
                idx = [i % N_PAIRS for i in range(count)]
                got = ctx.commit_and_generate_proof_batch([pr[i][0] for i in idx], [pr[i][1] for i in idx], cfg)
                for i, (r, p) in zip(idx, got):
                    assert int(p.proof_of_work) == want[i][2], (front, count, i, int(p.proof_of_work), want[i][2])
                    assert (bytes(r), p.serialize()) == want[i][:2], (front, count, i)
                    assert frieda_amd.verify(p, pr[i][1]), (front, count, i)
    finally:
        ctx.set_option("FRIEDA_GRIND_FRONT_WGS", 768)
        assert ctx._L.frieda_ctx_test_set_grind_first_log(ctx._h, 0) == 0


@pytest.mark.parametrize("pow_bits", [8, 16])
@pytest.mark.parametrize("count", [65, 130])
def test_more_than_64_blobs(ctx, oracle, count, pow_bits):
    import frieda_amd

    cfg = frieda_amd.PcsConfig(frieda_amd.FriConfig(4, 0, N_QUERIES), pow_bits)
    want = oracle_proofs(oracle, pow_bits)
    pr = pairs()
    idx = [i % N_PAIRS for i in range(count)]
    try:
        for front in FRONTS:
            ctx.set_option("FRIEDA_GRIND_FRONT_WGS", 768 if front is None else front)
            got = ctx.commit_and_generate_proof_batch([pr[i][0] for i in idx], [pr[i][1] for i in idx], cfg)
            for i, (r, p) in zip(idx, got):
                assert int(p.proof_of_work) == want[i][2], (front, count, i)
                assert (bytes(r), p.serialize()) == want[i][:2], (front, count, i)
    finally:
        ctx.set_option("FRIEDA_GRIND_FRONT_WGS", 768)


@pytest.mark.parametrize("first_log", [0, 10])
def test_one_blob_far_behind_the_others(ctx, oracle, first_log):
    """pow_bits 16, sixteen seeds of one blob: the seed whose minimum nonce is the largest of sixty candidates among the fifteen whose
    nonces are the smallest (picked on the CPU by the oracle).  The fifteen finish at once; the launch shrinks to the front while the
    sixteenth still searches — its nonce must still be the minimum of the whole range."""
    import frieda_amd

    blob = pairs()[0][0]
    if "far" not in _want:
        ocfg = oracle.make_config(16, 4, 0, N_QUERIES)
        cand = []
        for s in range(7000, 7060):
            r, p = oracle.commit_and_generate_proof(blob, s, ocfg)
            cand.append((int(p.c.proof_of_work), s, bytes(r), p.serialize()))
        cand.sort()
        _want["far"] = cand[:15] + [cand[-1]]
    chosen = _want["far"]
    assert chosen[-1][0] > 8 * chosen[14][0]  # far indeed (the largest of sixty draws of mean 2^16 against the fifteenth smallest)
    order = chosen[:7] + [chosen[-1]] + chosen[7:15]  # the slow one in the middle of the batch
    cfg = frieda_amd.PcsConfig(frieda_amd.FriConfig(4, 0, N_QUERIES), 16)
    assert ctx._L.frieda_ctx_test_set_grind_first_log(ctx._h, first_log) == 0
    try:
        for front in FRONTS:
            ctx.set_option("FRIEDA_GRIND_FRONT_WGS", 768 if front is None else front)
            got = ctx.commit_and_generate_proof_batch([blob] * len(order), [c[1] for c in order], cfg)
            for c, (r, p) in zip(order, got):
                assert int(p.proof_of_work) == c[0], (front, c[1])
                assert (bytes(r), p.serialize()) == c[2:], (front, c[1])
                assert frieda_amd.verify(p, c[1])
    finally:
        ctx.set_option("FRIEDA_GRIND_FRONT_WGS", 768)
        assert ctx._L.frieda_ctx_test_set_grind_first_log(ctx._h, 0) == 0


def test_option_range(ctx):
    import frieda_amd

    with pytest.raises(frieda_amd.FriedaError):
        ctx.set_option("FRIEDA_GRIND_FRONT_WGS", 2049)
    ctx.set_option("FRIEDA_GRIND_FRONT_WGS", 768)
