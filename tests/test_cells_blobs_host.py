"""frieda_verify_cells_blobs, the host verifier over (blob, cell) pairs of a block, against openings built by the CPU oracle (no GPU).

K = 3 blobs of one shape at (log_domain, blowup) = (5, 1), (11, 4) and (12, 1), log_cell in {0, 1, 3, 6, log_domain where that is <= 10},
9 pairs in unsorted blob order with a repeated pair.  Every expected status comes from cells_util.independent_status applied per blob,
asserted on the untouched openings before the library is called."""
import numpy as np
import pytest

import cells_util as U
from cells_util import ACCEPTED, ERR_ARG, POISON, REJECTED

K = 3
SHAPES = [(5, 1), (11, 4), (12, 1)]
CASES = [(n, b, c) for (n, b) in SHAPES for c in sorted({0, 1, 3, 6, n if n <= 10 else 0}) if c <= min(n, 10)]


def block(n, b, k=K):
    """k different blobs of the shape (n, b): [(data, ev, layers)], all from the oracle"""
    out = []
    for j in range(k):
        data, ev, layers, n_, _ = U.codeword(U.BLOB_LEN[(n, b)], b, seed=7700 + 13 * j + n)
        assert n_ == n
        out.append((data, ev, layers))
    assert len({bl[2][0][0].tobytes() for bl in out}) == k, "the blobs of the block must differ"
    return out


def commitments_of(blobs):
    return [bl[2][0][0].tobytes() for bl in blobs]


def pair_list(n, c, count, k=K, seed=3):
    """`count` (blob, cell) pairs: unsorted blob order, every blob present, one pair repeated"""
    rng = np.random.default_rng(seed + 31 * n + c)
    bidx = rng.integers(0, k, size=count).astype(np.uint32)
    bidx[:k] = np.arange(k, dtype=np.uint32)[::-1]
    idx = U.cell_list(n, c, count, seed=seed)
    if count > 4:
        bidx[4], idx[4] = bidx[1], idx[1]
    return bidx, idx


def open_pairs(blobs, c, bidx, idx):
    """values [k, 4, 2^c], paths [k, n - c, 32] of the pairs, each read out of its own blob's codeword and tree"""
    n = blobs[0][1].shape[1].bit_length() - 1
    values = np.zeros((len(idx), 4, 1 << c), dtype=np.uint32)
    paths = np.zeros((len(idx), n - c, 32), dtype=np.uint8)
    for b in range(len(blobs)):
        sel = np.flatnonzero(bidx == b)
        if len(sel):
            values[sel], paths[sel] = U.open_oracle(blobs[b][1], blobs[b][2], c, idx[sel])
    return values, paths


def independent_pairs(commitments, n, c, bidx, idx, values, paths):
    """cells_util.independent_status per blob: the pairs of blob b against commitment b"""
    want = np.zeros(len(idx), dtype=np.uint8)
    for b in range(len(commitments)):
        sel = np.flatnonzero(np.asarray(bidx) == b)
        if len(sel):
            want[sel] = U.independent_status(commitments[b], n, c, np.asarray(idx)[sel], values[sel], paths[sel])
    return want


def pair_mutations(n, c, bidx, idx, values, paths, k=K):
    """cells_util.mutations on the pair list, plus a valid cell attributed to another blob: (label, target, bidx', idx', values', paths')"""
    out = [(label, t, bidx, i2, v2, p2) for label, t, i2, v2, p2 in U.mutations(n, c, idx, values, paths)]
    t = len(idx) - 2
    b2 = bidx.copy()
    b2[t] = (int(bidx[t]) + 1) % k
    out.append(("blob", t, b2, idx, values, paths))
    return out


def raw_verify(commitments, n, c, bidx, idx, values, paths, n_blobs=None):
    """frieda_verify_cells_blobs into a poison-filled status array: (rc, status)"""
    from frieda_amd import _lib

    bidx = np.ascontiguousarray(bidx, dtype=np.uint32)
    idx = np.ascontiguousarray(idx, dtype=np.uint32)
    values = np.ascontiguousarray(values, dtype=np.uint32)
    paths = np.ascontiguousarray(paths, dtype=np.uint8)
    status = np.full(max(1, len(idx)), POISON, dtype=np.uint8)
    com = np.frombuffer(b"".join(commitments), dtype=np.uint8).copy()
    rc = _lib.lib().frieda_verify_cells_blobs(com.ctypes.data, len(commitments) if n_blobs is None else n_blobs, n, c, bidx.ctypes.data, idx.ctypes.data,
                                              len(idx), values.ctypes.data, paths.ctypes.data if paths.size else None, status.ctypes.data)
    return rc, status[: len(idx)]


@pytest.mark.parametrize("n,b,c", CASES)
def test_pairs_and_the_mutation_matrix(n, b, c):
    import frieda_amd

    blobs = block(n, b)
    coms = commitments_of(blobs)
    bidx, idx = pair_list(n, c, 9)
    values, paths = open_pairs(blobs, c, bidx, idx)
    assert independent_pairs(coms, n, c, bidx, idx, values, paths).all(), "the oracle-built openings must pass the independent check"
    rc, st = raw_verify(coms, n, c, bidx, idx, values, paths)
    assert rc == 0 and (st == ACCEPTED).all()
    muts = pair_mutations(n, c, bidx, idx, values, paths)
    assert len(muts) == 2 + (n - c) + (1 if n > c else 0)
    for label, t, b2, i2, v2, p2 in muts:
        want = independent_pairs(coms, n, c, b2, i2, v2, p2)
        hit = np.arange(len(idx)) == t  # (a repeated pair shares nothing with its twin: slot t alone)
        assert (want == np.where(hit, REJECTED, ACCEPTED)).all(), (label, want)
        rc, st = raw_verify(coms, n, c, b2, i2, v2, p2)
        assert rc == 0, label
        assert st.tolist() == want.tolist(), (label, t)
        # the single-blob verifier on that one cell gives the same byte
        one = frieda_amd.verify_cells(coms[int(b2[t])], n, c, i2[t : t + 1], v2[t : t + 1], p2[t : t + 1])
        assert one.tolist() == [want[t]]


@pytest.mark.parametrize("n,b,c", CASES)
def test_argument_errors_leave_the_status_untouched(n, b, c):
    blobs = block(n, b)
    coms = commitments_of(blobs)
    bidx, idx = pair_list(n, c, 9)
    values, paths = open_pairs(blobs, c, bidx, idx)
    bad_b = bidx.copy()
    bad_b[3] = K  # the first blob number out of range
    rc, st = raw_verify(coms, n, c, bad_b, idx, values, paths)
    assert rc == ERR_ARG and (st == POISON).all()
    bad_i = idx.copy()
    bad_i[5] = 1 << (n - c)
    rc, st = raw_verify(coms, n, c, bidx, bad_i, values, paths)
    assert rc == ERR_ARG and (st == POISON).all()
    for n_blobs in (0, 65537):
        rc, st = raw_verify(coms, n, c, np.zeros(9, np.uint32), idx, values, paths, n_blobs=n_blobs)
        assert rc == ERR_ARG and (st == POISON).all(), n_blobs
    rc, st = raw_verify(coms, n, 11, bidx, np.zeros(9, np.uint32), values, paths)
    assert rc == ERR_ARG and (st == POISON).all()


def test_no_cells_is_a_no_op():
    rc, st = raw_verify([bytes(32)], 12, 3, np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros(1, np.uint32), np.zeros(1, np.uint8))
    assert rc == 0 and len(st) == 0


def test_python_wrapper_checks_the_shapes():
    import frieda_amd

    n, b, c = 5, 1, 3
    blobs = block(n, b)
    coms = commitments_of(blobs)
    bidx, idx = pair_list(n, c, 4)
    values, paths = open_pairs(blobs, c, bidx, idx)
    assert frieda_amd.verify_cells_blobs(coms, n, c, bidx, idx, values, paths).tolist() == [ACCEPTED] * 4
    for args in ((bidx[:3], idx, values, paths), (bidx, idx, values[:3], paths), (bidx, idx, values, paths[:, :1])):
        with pytest.raises(frieda_amd.FriedaError):
            frieda_amd.verify_cells_blobs(coms, n, c, *args)  # a short array must not reach the library
    with pytest.raises(frieda_amd.FriedaError):
        frieda_amd.verify_cells_blobs([], n, c, bidx, idx, values, paths)
