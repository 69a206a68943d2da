"""frieda_verify_cells, the host verifier of opened cells, against openings built by the CPU oracle (no GPU).

Blobs at log_domain 5, 11 and 12, blowup 1 and 4, log_cell in {0, 1, 3, 6, log_domain where that is <= 10}.  Every expected status comes
from cells_util.independent_status (merkle_commit_layer over the cell's leaves and up its path), which is asserted on the untouched
openings before the library is called."""
import ctypes as C

import numpy as np
import pytest

import cells_util as U
from cells_util import ACCEPTED, ERR_ARG, HOST_CASES, POISON, P31, REJECTED


def raw_verify(commitment, n, c, idx, values, paths, status=None):
    """frieda_verify_cells into a poison-filled status array: (rc, status)"""
    from frieda_amd import _lib

    idx = np.ascontiguousarray(idx, dtype=np.uint32)
    values = np.ascontiguousarray(values, dtype=np.uint32)
    paths = np.ascontiguousarray(paths, dtype=np.uint8)
    if status is None:
        status = np.full(max(1, len(idx)), POISON, dtype=np.uint8)
    com = (C.c_uint8 * 32)(*bytes(commitment))
    rc = _lib.lib().frieda_verify_cells(com, n, c, idx.ctypes.data, len(idx), values.ctypes.data, paths.ctypes.data if paths.size else None,
                                        status.ctypes.data)
    return rc, status[: len(idx)]


def every_cell(n, c):
    """all cells of the codeword, shuffled, three of them twice"""
    rng = np.random.default_rng(77 + n + c)
    idx = rng.permutation(1 << (n - c)).astype(np.uint32)
    return np.concatenate([idx, idx[:3]])


@pytest.mark.parametrize("n,b,c", HOST_CASES)
def test_accepts_every_cell(n, b, c):
    _, ev, layers, _, _ = U.case(n, b)
    root = layers[0][0].tobytes()
    idx = every_cell(n, c)
    values, paths = U.open_oracle(ev, layers, c, idx)
    assert U.independent_status(root, n, c, idx, values, paths).all(), "the oracle-built openings must pass the independent check"
    rc, st = raw_verify(root, n, c, idx, values, paths)
    assert rc == 0
    assert (st == ACCEPTED).all(), np.flatnonzero(st != ACCEPTED)[:8]


@pytest.mark.parametrize("n,b,c", HOST_CASES)
def test_mutation_matrix(n, b, c):
    """one word of the values, one byte of each path entry, the index: the mutated cell is rejected, every other cell keeps its status"""
    _, ev, layers, _, _ = U.case(n, b)
    root = layers[0][0].tobytes()
    idx = U.cell_list(n, c, 9)
    values, paths = U.open_oracle(ev, layers, c, idx)
    assert U.independent_status(root, n, c, idx, values, paths).all()
    muts = U.mutations(n, c, idx, values, paths)
    assert len(muts) == 1 + (n - c) + (1 if n > c else 0)
    for label, t, i2, v2, p2 in muts:
        want = U.independent_status(root, n, c, i2, v2, p2)
        assert want[t] == REJECTED and want.sum() == len(idx) - 1, (label, want)
        rc, st = raw_verify(root, n, c, i2, v2, p2)
        assert rc == 0, label
        assert st.tolist() == want.tolist(), (label, t)


@pytest.mark.parametrize("n,b,c", HOST_CASES)
@pytest.mark.parametrize("word", [P31, 1 << 31, 0xFFFFFFFF])
def test_non_canonical_word_rejects_the_cell(n, b, c, word):
    """A tree built over a codeword that HOLDS the non-canonical word: the hashes of the opening are consistent with its root, so only the
    canonical-word rule can reject the cell."""
    from oracle import oracle as O

    _, ev, _, _, _ = U.case(n, b)
    idx = U.cell_list(n, c, 5)
    t = 1
    ev2 = ev.copy()
    ev2[2, (int(idx[t]) << c) + ((1 << c) - 1)] = word
    layers2 = O.merkle_commit(ev2)
    root2 = layers2[0][0].tobytes()
    values, paths = U.open_oracle(ev2, layers2, c, idx)
    want = U.independent_status(root2, n, c, idx, values, paths)
    hit = idx == idx[t]
    assert (want == np.where(hit, REJECTED, ACCEPTED)).all()
    rc, st = raw_verify(root2, n, c, idx, values, paths)
    assert rc == 0 and st.tolist() == want.tolist()


@pytest.mark.parametrize("n,b,c", HOST_CASES)
def test_wrong_commitment_rejects_all(n, b, c):
    _, ev, layers, _, _ = U.case(n, b)
    root = bytearray(layers[0][0].tobytes())
    idx = U.cell_list(n, c, 6)
    values, paths = U.open_oracle(ev, layers, c, idx)
    root[int(n + c) % 32] ^= 0x10
    assert not U.independent_status(bytes(root), n, c, idx, values, paths).any()
    rc, st = raw_verify(bytes(root), n, c, idx, values, paths)
    assert rc == 0 and (st == REJECTED).all()


@pytest.mark.parametrize("n,b,c", HOST_CASES)
def test_argument_errors_leave_the_status_untouched(n, b, c):
    _, ev, layers, _, _ = U.case(n, b)
    root = layers[0][0].tobytes()
    idx = U.cell_list(n, c, 4)
    values, paths = U.open_oracle(ev, layers, c, idx)
    bad = idx.copy()
    bad[2] = 1 << (n - c)  # the first index out of range
    rc, st = raw_verify(root, n, c, bad, values, paths)
    assert rc == ERR_ARG and (st == POISON).all()
    bad[2] = 0xFFFFFFFF
    rc, st = raw_verify(root, n, c, bad, values, paths)
    assert rc == ERR_ARG and (st == POISON).all()
    for log_cell in (n + 1, 11, 0xFFFFFFFF):  # beyond log_domain, beyond FRIEDA_MAX_LOG_OPEN_CELL
        rc, st = raw_verify(root, n, log_cell, np.zeros(4, np.uint32), values, paths)
        assert rc == ERR_ARG and (st == POISON).all(), log_cell


def test_no_cells_is_a_no_op():
    rc, st = raw_verify(bytes(32), 12, 3, np.zeros(0, np.uint32), np.zeros(1, np.uint32), np.zeros(1, np.uint8))
    assert rc == 0 and len(st) == 0


def test_python_wrapper_checks_the_shapes():
    import frieda_amd

    _, ev, layers, n, _ = U.case(5, 1)
    root = layers[0][0].tobytes()
    idx = U.cell_list(n, 3, 4)
    values, paths = U.open_oracle(ev, layers, 3, idx)
    assert frieda_amd.verify_cells(root, n, 3, idx, values, paths).tolist() == [ACCEPTED] * 4
    with pytest.raises(frieda_amd.FriedaError):
        frieda_amd.verify_cells(root, n, 3, idx, values[:3], paths)  # a short array must not reach the library
    with pytest.raises(frieda_amd.FriedaError):
        frieda_amd.verify_cells(root, n, 3, idx, values, paths[:, :1])
