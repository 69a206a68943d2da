"""frieda_verify_stripe_bundles, the host verifier of stripe bundles, against blocks built by the CPU oracle (no GPU).

Blocks of 1, 3 and 5 blobs at the (log_domain, blowup, log_cell) cases of cells_util.HOST_CASES.  Status byte (b, j) must be
bundles_util.independent_status of blob j's piece of bundle b alone, which is asserted on the untouched block before the library is
called; the mutation matrix of bundles_util.mutations is applied to one blob's piece and must change byte (b, j) only; a malformed
bundle marks its whole row and leaves the other rows alone."""
import numpy as np
import pytest

import bundles_util as B
import stripe_bundles_util as S
import test_cells_blobs_host as H
from bundles_util import ACCEPTED, MALFORMED, REJECTED
from cells_util import ERR_ARG, HOST_CASES, POISON


def small_bundles(n, c):
    """three bundles of 5, 2 and 9 stripes (fewer where the domain is smaller), as bundles_util.small_call"""
    total = 1 << (n - c)
    return [B.pick(n, c, min(k, total), seed=40 + j) for j, k in enumerate((5, 2, 9))]


@pytest.mark.parametrize("k", [1, 3, 5])
@pytest.mark.parametrize("n,b,c", HOST_CASES)
def test_accepts_every_shape(n, b, c, k):
    """the shapes of bundles_util.shape_bundles (sizes 1 .. 300, every stripe of the domain, a pair, the first, the last) over k blobs"""
    blobs = H.block(n, b, k=k)
    shapes = B.shape_bundles(n, c)
    call = S.build(blobs, c, [i for _, i in shapes])
    if k == 3:  # (the independent check of every piece once per shape; the other blob counts compare with the layout alone)
        assert (S.independent(call) == ACCEPTED).all(), "the oracle-built block must pass the independent check"
    rc, st = S.raw_verify(call)
    assert rc == 0 and st.shape == (len(shapes), k)
    assert (st == ACCEPTED).all(), [(l, s.tolist()) for (l, _), s in zip(shapes, st) if (s != ACCEPTED).any()]
    # blob j's piece is that blob's cell-bundle witness: the single-blob verifier accepts it as it lies
    for j in range(k):
        rc, one = B.raw_verify(call.blob_call(j))
        assert rc == 0 and (one == ACCEPTED).all(), j
    # W_b is frieda_cell_bundle_witness_count of the bundle's indices, once per bundle
    for (label, idx), w0, w1 in zip(shapes, call.wfirst[:-1], call.wfirst[1:]):
        assert B.witness_count(n, c, idx) == (0, int(w1 - w0)), label


@pytest.mark.parametrize("k", [1, 3, 5])
@pytest.mark.parametrize("n,b,c", HOST_CASES)
def test_mutation_matrix_on_one_blobs_piece(n, b, c, k):
    blobs = H.block(n, b, k=k)
    calls = S.blob_calls(blobs, c, small_bundles(n, c))
    call = S.assemble(calls)
    rc, st = S.raw_verify(call)
    assert rc == 0 and (st == ACCEPTED).all()
    j = k // 2
    muts = S.mutations(calls, j)
    assert {"word", "out_of_range", "long"} <= {m[0] for m in muts}
    for label, hit, must, shared, mutated in muts:
        want = S.independent(mutated)
        S.check_mutation(label, hit, must, shared, j, want)
        rc, st = S.raw_verify(mutated)
        assert rc == 0, label
        assert st.tolist() == want.tolist(), (label, hit)
        # byte (b, j) is exactly what the single-blob verifier says about blob j's piece alone
        for jj in range(k):
            rc, one = B.raw_verify(mutated.blob_call(jj))
            assert rc == 0 and one.tolist() == st[:, jj].tolist(), (label, jj)


def test_a_malformed_bundle_marks_its_whole_row():
    n, b, c, k = 11, 4, 3, 3
    blobs = H.block(n, b, k=k)
    bundles = small_bundles(n, c)
    call = S.build(blobs, c, bundles)
    for bad in (bundles[1][::-1].copy(), np.array([7, 7], np.uint32), np.array([0, 1 << (n - c)], np.uint32)):
        mutated = call.replace(bundles=[bundles[0], bad, bundles[2]])
        want = S.independent(mutated)
        assert want.tolist() == [[ACCEPTED] * k, [MALFORMED] * k, [ACCEPTED] * k]
        rc, st = S.raw_verify(mutated)
        assert rc == 0 and st.tolist() == want.tolist()
    # one commitment of the block swapped for another blob's: that column is rejected, no other byte moves
    coms = list(call.commitments)
    coms[2] = coms[0]
    rc, st = S.raw_verify(call.replace(commitments=coms))
    assert rc == 0 and (st[:, 2] == REJECTED).all() and (st[:, :2] == ACCEPTED).all()


def test_argument_errors_leave_the_status_untouched():
    n, b, c, k = 5, 1, 1, 3
    call = S.build(H.block(n, b, k=k), c, small_bundles(n, c))
    for bad in (call.replace(n=29), call.replace(c=n + 1), call.replace(wfirst=call.wfirst[::-1].copy())):
        rc, st = S.raw_verify(bad)
        assert rc == ERR_ARG and (st == POISON).all()
    rc, st = S.raw_verify(call, n_blobs=0)
    assert rc == ERR_ARG and (st == POISON).all()
    from frieda_amd import _lib

    assert _lib.lib().frieda_verify_stripe_bundles(None, k, n, c, None, None, 0, None, None, None, None) == 0  # no bundles: a no-op
