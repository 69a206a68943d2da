"""frieda_verify_cell_bundles and frieda_cell_bundle_witness_count, the host side of cell bundles, against bundles built by the CPU oracle
(no GPU).

Domains: the (log_domain, blowup) pairs of cells_util.BLOB_LEN; log_cell in {0, 1, 3, 6, log_domain where that is <= 10}; bundles of 1, 2,
63, 64, 65 and 300 cells, all cells of the domain (an empty witness), one adjacent pair, only the first and only the last cell.  The
witness is read out of oracle.merkle_commit's layers along stwo's merge walk (bundles_util.merge_walk); every expected status comes
from bundles_util.independent_status, which is asserted on the untouched bundles before the library is called."""
import numpy as np
import pytest

import bundles_util as B
import cells_util as U
from bundles_util import ACCEPTED, MALFORMED, REJECTED
from cells_util import ERR_ARG, HOST_CASES, POISON, P31


@pytest.mark.parametrize("depth", [1, 2, 5, 13])
def test_the_merge_walk_and_the_emit_rule_agree(depth):
    """stwo's walk (push the unknown child, per level, per parent) and the E_s tables (every level from the positions alone) are the same
    list: all subsets of the small trees, random subsets of the large one"""
    rng = np.random.default_rng(depth)
    total = 1 << depth
    if total <= 4:
        subsets = [[i for i in range(total) if (m >> i) & 1] for m in range(1, 1 << total)]
    else:
        subsets = [np.sort(rng.choice(total, size=int(k), replace=False)) for k in list(rng.integers(1, min(total, 600) + 1, size=60)) + [1, 2, min(total, 1024)]]
        subsets += [[0], [total - 1], [0, total - 1], list(range(total))[:1024], [6, 7]]
    for idx in subsets:
        assert B.merge_walk(depth, idx) == B.emit_tables(depth, idx), list(idx)[:8]


@pytest.mark.parametrize("n,b,c", HOST_CASES)
def test_accepts_every_shape(n, b, c):
    labels, call = B.shapes_call(n, b, c)
    want = B.independent_status(call)
    assert (want == ACCEPTED).all(), "the oracle-built bundles must pass the independent check"
    rc, st = B.raw_verify(call)
    assert rc == 0
    assert st.tolist() == want.tolist(), [l for l, s in zip(labels, st) if s != ACCEPTED]
    for label, idx, w0, w1 in zip(labels, call.bundles, call.wfirst[:-1], call.wfirst[1:]):
        rc, cnt = B.witness_count(n, c, idx)
        assert rc == 0 and cnt == int(w1 - w0), label
        if label == "all":
            assert cnt == 0


@pytest.mark.parametrize("n,b,c", HOST_CASES)
def test_a_one_cell_bundle_is_that_cells_path(n, b, c):
    _, ev, layers, _, _ = U.case(n, b)
    for cell in (0, (1 << (n - c)) - 1, int(B.pick(n, c, 1, seed=9)[0])):
        _, paths = U.open_oracle(ev, layers, c, [cell])
        assert B.witness_oracle(layers, n, c, [cell]).tobytes() == paths[0].tobytes()


@pytest.mark.parametrize("n,b,c", HOST_CASES)
def test_the_shared_witness_is_smaller(n, b, c):
    depth = n - c
    for _, idx in B.shape_bundles(n, c):
        rc, cnt = B.witness_count(n, c, idx)
        assert rc == 0
        if len(idx) == 1:
            assert cnt == depth
        else:
            assert cnt < len(idx) * depth


def test_the_counts_of_the_record():
    """shared witness against separate paths at the sizes the header quotes (random indices, fixed seed: the order of magnitude)"""
    rng = np.random.default_rng(0)
    for depth, k in ((13, 64), (13, 499), (24, 1024)):
        idx = np.sort(rng.choice(1 << depth, size=k, replace=False)).astype(np.uint32)
        rc, cnt = B.witness_count(depth, 0, idx)
        assert rc == 0 and cnt == len(B.merge_walk(depth, idx)) and cnt < k * depth * 0.6


@pytest.mark.parametrize("n,b,c", HOST_CASES)
def test_mutation_matrix(n, b, c):
    """no mutated bundle is accepted, the other bundles of the call keep their status, a length or order fault is MALFORMED"""
    call = B.small_call(n, b, c)
    assert (B.independent_status(call) == ACCEPTED).all()
    rc, st = B.raw_verify(call)
    assert rc == 0 and (st == ACCEPTED).all()
    muts = B.mutations(call)
    assert {"word", "out_of_range", "long"} <= {m[0] for m in muts}
    for label, hit, must, mutated in muts:
        want = B.independent_status(mutated)
        B.check_mutation(label, hit, must, want, len(call.bundles))
        rc, st = B.raw_verify(mutated)
        assert rc == 0, label
        assert st.tolist() == want.tolist(), (label, hit)


@pytest.mark.parametrize("c", [0, 3])
@pytest.mark.parametrize("word", [P31, 1 << 31, 0xFFFFFFFF])
def test_non_canonical_word_rejects_the_bundle(c, word):
    """a tree built over a codeword that HOLDS the word: the hashes are consistent, only the canonical-word rule can reject"""
    from oracle import oracle as O

    n = 5
    _, ev, _, _, _ = U.case(n, 1)
    ev2 = ev.copy()
    bundles = [B.pick(n, c, 3, seed=1), B.pick(n, c, 2, seed=2)]
    ev2[2, (int(bundles[0][1]) << c) + ((1 << c) - 1)] = word
    call = B.build_call(ev2, O.merkle_commit(ev2), c, bundles)
    want = B.independent_status(call)
    hit = int(bundles[0][1]) in [int(x) for x in bundles[1]]
    assert want.tolist() == [REJECTED, REJECTED if hit else ACCEPTED]
    rc, st = B.raw_verify(call)
    assert rc == 0 and st.tolist() == want.tolist()


def test_wrong_commitment_rejects_all():
    _, call = B.shapes_call(11, 4, 3)
    root = bytearray(call.commitment)
    root[7] ^= 0x10
    wrong = call.replace(commitment=bytes(root))
    assert (B.independent_status(wrong) == REJECTED).all()
    rc, st = B.raw_verify(wrong)
    assert rc == 0 and (st == REJECTED).all()


def test_the_cap():
    """1024 cells are a bundle, 1025 are MALFORMED (and the count call refuses them)"""
    n, c = 12, 0
    _, ev, layers, _, _ = U.case(n, 4)
    at_cap, over = B.pick(n, c, 1024, seed=5), B.pick(n, c, 1025, seed=6)
    call = B.build_call(ev, layers, c, [at_cap, over, B.pick(n, c, 3, seed=7)])
    want = B.independent_status(call)
    assert want.tolist() == [ACCEPTED, MALFORMED, ACCEPTED]
    rc, st = B.raw_verify(call)
    assert rc == 0 and st.tolist() == want.tolist()
    assert B.witness_count(n, c, at_cap)[0] == 0
    assert B.witness_count(n, c, over) == (ERR_ARG, 0xDEAD)


def test_an_empty_bundle_is_malformed_and_costs_only_itself():
    _, ev, layers, n, _ = U.case(5, 1)
    call = B.build_call(ev, layers, 0, [B.pick(n, 0, 3, seed=1), np.zeros(0, np.uint32), B.pick(n, 0, 4, seed=2)])
    rc, st = B.raw_verify(call)
    assert rc == 0 and st.tolist() == [ACCEPTED, MALFORMED, ACCEPTED] == B.independent_status(call).tolist()
    assert B.witness_count(n, 0, np.zeros(0, np.uint32)) == (ERR_ARG, 0xDEAD)
    assert B.witness_count(n, 0, [3, 3])[0] == ERR_ARG and B.witness_count(n, 0, [4, 3])[0] == ERR_ARG and B.witness_count(n, 0, [32])[0] == ERR_ARG


def test_call_structure_errors_leave_the_status_untouched():
    """FRIEDA_ERR_ARG is for the call's own structure: a *_first array that does not start at 0 or that decreases, the shape out of range"""
    from frieda_amd import _lib
    import ctypes as C

    _, ev, layers, n, _ = U.case(5, 1)
    call = B.build_call(ev, layers, 1, [B.pick(n, 1, 3, seed=1), B.pick(n, 1, 4, seed=2)])
    L = _lib.lib()
    idx = np.concatenate(call.bundles)
    com = (C.c_uint8 * 32)(*call.commitment)

    def run(first, wfirst, log_domain=n, log_cell=1):
        first, wfirst = np.asarray(first, np.uint32), np.asarray(wfirst, np.uint64)
        st = np.full(4, POISON, np.uint8)
        rc = L.frieda_verify_cell_bundles(com, log_domain, log_cell, idx.ctypes.data, first.ctypes.data, 2, call.values.ctypes.data, call.witness.ctypes.data,
                                          wfirst.ctypes.data, st.ctypes.data)
        return rc, st

    f, w = call.first, call.wfirst
    assert run(f, w)[0] == 0
    for first, wfirst in (([1, f[1], f[2]], w), ([0, 5, 3], w), (f, [1, w[1], w[2]]), (f, [0, w[2], w[1]])):
        rc, st = run(first, wfirst)
        assert rc == ERR_ARG and (st == POISON).all(), (first, wfirst)
    for log_domain, log_cell in ((29, 1), (n, n + 1), (12, 11), (n, 0xFFFFFFFF)):
        rc, st = run(f, w, log_domain, log_cell)
        assert rc == ERR_ARG and (st == POISON).all(), (log_domain, log_cell)
    st = np.full(4, POISON, np.uint8)
    assert L.frieda_verify_cell_bundles(com, n, 1, None, None, 0, None, None, None, st.ctypes.data) == 0 and (st == POISON).all()  # no bundles: a no-op


def test_python_wrapper_checks_the_sizes():
    import frieda_amd

    _, call = B.shapes_call(5, 1, 1)
    st = frieda_amd.verify_cell_bundles(call.commitment, 5, 1, call.bundles, call.values, call.witness, call.wfirst)
    assert (st == ACCEPTED).all() and len(st) == len(call.bundles)
    with pytest.raises(frieda_amd.FriedaError):
        frieda_amd.verify_cell_bundles(call.commitment, 5, 1, call.bundles, call.values[:-1], call.witness, call.wfirst)  # a short array must not reach the library
    with pytest.raises(frieda_amd.FriedaError):
        frieda_amd.verify_cell_bundles(call.commitment, 5, 1, call.bundles, call.values, call.witness[:-1], call.wfirst)
    with pytest.raises(frieda_amd.FriedaError):
        frieda_amd.verify_cell_bundles(call.commitment, 5, 1, call.bundles, call.values, call.witness, call.wfirst[:-1])
    assert frieda_amd.cell_bundle_witness_count(5, 1, call.bundles[0]) == int(call.wfirst[1])
    with pytest.raises(frieda_amd.FriedaError):
        frieda_amd.cell_bundle_witness_count(5, 1, [3, 2])
