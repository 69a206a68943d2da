"""GPU: the contiguous last transform pass (ntt_tile12_kernel<3, 0>, frieda_amd/csrc/ntt.hip: the last pass of every polynomial of 2^12
coefficients or more per column) against the oracle, bit for bit: frieda_circle_evaluate at log domains 12, 13, 16 and 20 with 1 and 4
columns (one column per workgroup below 512 tiles, four from there on: the fill of column c + 1 follows stage 2 of column c behind one
barrier; the two small domains also run without blow-up, where the pass is this kernel), and whole proofs of a 2^16 domain, one blob and
a batch of three at a stride larger than the blobs, byte for byte.  (Written for a wave-local fill of the tile that was measured and not
kept, profiles/r17_batched_leftovers.txt: the cases stand for the kernel as it is.)
"""
import numpy as np
import pytest

from conftest import splitmix64_bytes
from util import DevBuf, blob_len_for, poison_bytes

pytestmark = pytest.mark.gpu

P = (1 << 31) - 1
_cache = {}


@pytest.fixture(scope="module")
def ctx():
    import frieda_amd

    c = frieda_amd.Context(0)
    yield c
    c.close()


def evaluation(oracle, n, L, ncols):
    key = (n, L, ncols)
    if key not in _cache:
        rng = np.random.default_rng(6100 + 32 * n + ncols)
        coef = rng.integers(0, P, (ncols, 1 << L), dtype=np.uint32)
        coef[0, :4] = (0, P - 1, 1, P - 1)  # the ends of the field's range too
        _cache[key] = (coef, oracle.circle_evaluate(coef, n))
    return _cache[key]


@pytest.mark.parametrize("ncols", [1, 4])
@pytest.mark.parametrize("n,L", [(12, 8), (12, 12), (13, 9), (13, 12), (13, 13), (16, 12), (20, 16)])
def test_circle_evaluate(ctx, oracle, n, L, ncols):
    coef, exp = evaluation(oracle, n, L, ncols)
    d_c = DevBuf.from_array(ctx, coef)
    d_o = DevBuf(ctx, 4 * ncols << n)
    assert ctx._L.frieda_circle_evaluate(ctx._h, d_c.ptr, ncols, L, n, d_o.ptr) == 0
    assert np.array_equal(d_o.to_array(np.uint32, (ncols, 1 << n)), exp)
    d_c.free()
    d_o.free()


def proofs(oracle, count):
    n = blob_len_for(16) - 3
    blobs = [splitmix64_bytes(6200 + i, n) for i in range(count)]
    seeds = [71 + i for i in range(count)]
    want = []
    for b, s in zip(blobs, seeds):
        if ("proof", s) not in _cache:
            r, p = oracle.commit_and_generate_proof(b.tobytes(), s, oracle.make_config(4, 4, 0, 8))
            _cache[("proof", s)] = (bytes(r), p.serialize())
        want.append(_cache[("proof", s)])
    return blobs, seeds, want


@pytest.mark.parametrize("count", [1, 3])
def test_whole_proofs_at_2_16(ctx, oracle, count):
    import frieda_amd

    blobs, seeds, want = proofs(oracle, count)
    n = len(blobs[0])
    stride = ((n + 3) & ~3) + 516
    img = np.ascontiguousarray(poison_bytes(0, count * stride))
    for i, b in enumerate(blobs):
        img[i * stride : i * stride + n] = b
    cfg = frieda_amd.PcsConfig(frieda_amd.FriConfig(4, 0, 8), 4)
    buf = DevBuf.from_array(ctx, img)
    ctx.set_kernel_timing(True)
    ctx.kernel_timing_report(reset=True)
    try:
        got = ctx.commit_and_generate_proof_batch_device(buf.ptr, stride, n, count, seeds, cfg)
        launches = {k["name"] for k in ctx.kernel_timing_report(reset=True)}
    finally:
        ctx.set_kernel_timing(False)
    assert "ntt_pass_last" in launches, sorted(launches)
    assert [(bytes(r), p.serialize()) for r, p in got] == want
    assert ctx.commit_batch_device(buf.ptr, stride, n, count, 4) == [w[0] for w in want]
    buf.free()
