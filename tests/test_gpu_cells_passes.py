"""The one pass driver of the cells verifier (cells_host.cpp: verify_cells_passes) where its two callers that pool — the rebuild from
opened cells and the rebuild from opened stripes — can still go wrong after sharing it: a pass in the middle of a call that gathers
nothing (the pool numbering carries over it), and the error path of a rebuild that ends up with too few entries (the call's device
buffers are released, the context stays usable).

Shape: the (5, 1) blob of cells_util.BLOB_LEN — a 2^5 domain, 2^4 coefficients per column — at log_cell 1: 16 cells, 9 needed.  The
pass budget is the formula of cells_pass.h for exactly five cells (or five stripes) per pass: passes of 5, 5, 5 and 1."""
import numpy as np
import pytest

import cells_util as U
import test_cells_blobs_host as H
from cells_util import ACCEPTED, ERR_ARG, REJECTED
from test_gpu_cells import raw_reconstruct
from test_gpu_cells_blobs import open_stripes_oracle, raw_stripes

pytestmark = pytest.mark.gpu

N, BLOWUP, C_ = 5, 1, 1
CELLS, NEED, PER_PASS = 1 << (N - C_), (1 << (N - BLOWUP - C_)) + 1, 5
VB, PB = 16 << C_, 32 * (N - C_)  # bytes of a cell's values / path


def budget(ctx, group, with_blob_numbers):
    """cells_pass.h: a pass takes max(1, budget / (group * (unit + vb + pb))) * group cells, unit = 4 (one commitment) or 8 bytes"""
    assert ctx._L.frieda_ctx_test_set_verify_pass_bytes(ctx._h, PER_PASS * group * ((8 if with_blob_numbers else 4) + VB + PB)) == 0


def test_an_empty_pass_in_the_middle_of_the_cells(gpu_ctx):
    import frieda_amd

    data, ev, layers, n, L = U.case(N, BLOWUP)
    root = layers[0][0].tobytes()
    assert (CELLS, NEED) == (16, 9)
    idx = np.random.default_rng(71).permutation(CELLS).astype(np.uint32)
    values, paths = U.open_oracle(ev, layers, C_, idx)
    values = values.copy()
    for j in range(PER_PASS, 2 * PER_PASS):  # the whole second pass
        values[j, j % 4, j % 2] ^= 4
    want = frieda_amd.verify_cells(root, n, C_, idx, values, paths)
    assert np.flatnonzero(want == REJECTED).tolist() == list(range(PER_PASS, 2 * PER_PASS))
    budget(gpu_ctx, 1, False)
    try:
        rc, out, st, used = raw_reconstruct(gpu_ctx, root, BLOWUP, len(data), C_, idx, values, paths)
    finally:
        gpu_ctx._L.frieda_ctx_test_set_verify_pass_bytes(gpu_ctx._h, 0)
    assert rc == 0, gpu_ctx._L.frieda_last_error(gpu_ctx._h)
    assert st.tolist() == want.tolist() and used == CELLS - PER_PASS == 11 and out == data


def test_an_empty_pass_in_the_middle_of_the_stripes(gpu_ctx):
    import frieda_amd

    k = 3
    blobs = H.block(N, BLOWUP, k=k)
    coms = H.commitments_of(blobs)
    length = len(blobs[0][0])
    stripes = np.random.default_rng(72).permutation(CELLS).astype(np.uint32)
    values, paths = open_stripes_oracle(blobs, C_, stripes)  # [S, K, 4, 2], [S, K, 4, 32]
    for t in range(PER_PASS, 2 * PER_PASS):  # one cell of one blob in every stripe of the second pass
        values[t, t % k, t % 4, t % 2] ^= 4
    bidx, idx = np.tile(np.arange(k, dtype=np.uint32), CELLS), np.repeat(stripes, k)
    want = frieda_amd.verify_cells_blobs(coms, N, C_, bidx, idx, values.reshape(-1, 4, 1 << C_), paths.reshape(-1, N - C_, 32)).reshape(CELLS, k)
    assert [np.flatnonzero(want[t] == REJECTED).tolist() for t in range(CELLS)] == [[t % k] if PER_PASS <= t < 2 * PER_PASS else [] for t in range(CELLS)]
    budget(gpu_ctx, k, True)
    try:
        rc, out, st, used = raw_stripes(gpu_ctx, coms, BLOWUP, length, C_, stripes, values, paths)
    finally:
        gpu_ctx._L.frieda_ctx_test_set_verify_pass_bytes(gpu_ctx._h, 0)
    assert rc == 0, gpu_ctx._L.frieda_last_error(gpu_ctx._h)
    assert st[PER_PASS:2 * PER_PASS].tolist() == want[PER_PASS:2 * PER_PASS].tolist(), "the 15 status bytes of the second pass"
    assert st.tolist() == want.tolist() and used == CELLS - PER_PASS == 11
    assert out == [bl[0] for bl in blobs]


def test_too_few_after_a_rejection_leaves_the_context_usable(gpu_ctx):
    import frieda_amd

    data, ev, layers, n, L = U.case(N, BLOWUP)
    root = layers[0][0].tobytes()
    idx = np.random.default_rng(73).permutation(CELLS)[:NEED].astype(np.uint32)
    values, paths = U.open_oracle(ev, layers, C_, idx)
    bad = values.copy()
    bad[2, 1, 0] ^= 4
    bad[7, 3, 1] ^= 4  # (one in each of the two passes)
    budget(gpu_ctx, 1, False)
    try:
        with pytest.raises(frieda_amd.FriedaError) as e:
            gpu_ctx.reconstruct_from_opened_cells(root, BLOWUP, len(data), C_, idx, bad, paths)
        assert e.value.status == ERR_ARG and "7 distinct accepted cells, 9 needed" in str(e.value)
        assert e.value.n_cells_used == 7
        assert e.value.cell_status.tolist() == [REJECTED if j in (2, 7) else ACCEPTED for j in range(NEED)]
        out, st, used = gpu_ctx.reconstruct_from_opened_cells(root, BLOWUP, len(data), C_, idx, values, paths)
    finally:
        gpu_ctx._L.frieda_ctx_test_set_verify_pass_bytes(gpu_ctx._h, 0)
    assert out == data and used == NEED and (st == ACCEPTED).all()
