"""GPU: the first transform pass reading the packed blob itself (ntt_tile12_rep_kernel's packed source form, frieda_amd/csrc/ntt.hip;
option FRIEDA_NTT_PACKED_SRC, default on) instead of coefficients that an unpack30 launch wrote.

Shape: 2^17 coefficients per column on a 2^21 domain — the smallest whose first pass is the rep kernel (a batch of two or more by the
default rule, one blob with FRIEDA_NTT_REP = 1).  Roots and whole proofs are compared with the option on, with it off and against the
oracle, on blob lengths that end at every kind of place in the packed stream, with the blob in front of different poison, in a strided
batch, and at pointers the fused form must refuse (the kernel-timing report then lists the unpack30 launch).

Nothing here reads past an allocation: that no dword starting at or beyond the blob's end is loaded is a property of the kernel's guard
(packed_dword); what a test can see is that the bytes BEHIND the blob never reach the output.
"""
import numpy as np
import pytest

from conftest import splitmix64_bytes
from util import DevBuf, poison_bytes

pytestmark = pytest.mark.gpu

L, B, SEED = 17, 4, 21
EXACT = (4 << L) * 30 // 8  # bytes whose felts exactly fill the four columns
LENGTHS = {
    "exact": EXACT,
    "one_byte_short": EXACT - 1,
    "one_past_felt_boundary": 15 * (EXACT // 15 - 1000) + 1,  # four felts are 15 bytes: a felt boundary on a byte boundary
    "one_short_of_felt_boundary": 15 * (EXACT // 15 - 1000) - 1,
    "last_column_all_padding": 3 * EXACT // 4 - 1493,  # column 3 starts at byte 3/4 EXACT; still more than half: the same L
}
_oracle_proofs = {}


def blob_of(kind):
    return splitmix64_bytes(8000 + sorted(LENGTHS).index(kind), LENGTHS[kind])


def cfg():
    import frieda_amd

    return frieda_amd.PcsConfig(frieda_amd.FriConfig(B, 0, 20), 6)


def oracle_proof(oracle, data, seed=SEED):
    key = (bytes(data[:64]), len(data), seed)
    if key not in _oracle_proofs:
        r, p = oracle.commit_and_generate_proof(bytes(data), seed, oracle.make_config(6, B, 0, 20))
        _oracle_proofs[key] = (r, p.serialize())
    return _oracle_proofs[key]


def make_ctx(packed):
    import frieda_amd

    ctx = frieda_amd.Context(0)
    ctx.set_option("FRIEDA_NTT_REP", 1)
    ctx.set_option("FRIEDA_NTT_PACKED_SRC", packed)
    return ctx


@pytest.fixture(scope="module")
def ctx_on():
    ctx = make_ctx(1)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def ctx_off():
    ctx = make_ctx(0)
    yield ctx
    ctx.close()


def timed(ctx, call):
    """(result, {kernel name: launches}) of one call"""
    ctx.set_kernel_timing(True)
    ctx.kernel_timing_report(reset=True)
    try:
        res = call()
        rep = ctx.kernel_timing_report(reset=True)
    finally:
        ctx.set_kernel_timing(False)
    return res, {k["name"]: k["launches"] for k in rep}


def device_image(ctx, data, front, tail, fill):
    """One device allocation: `front` bytes, the blob, `tail` bytes; everything that is not blob holds `fill` (a byte value) or, with
    fill = None, the position-dependent poison of util.poison_bytes.  Returns (buffer, pointer to the blob)."""
    total = (front + len(data) + tail + 3) & ~3
    img = np.ascontiguousarray(poison_bytes(0, total)) if fill is None else np.full(total, fill, dtype=np.uint8)
    img[front : front + len(data)] = data
    buf = DevBuf.from_array(ctx, img)
    return buf, buf.ptr.value + front


def test_lengths_have_the_shape(gpu_ctx):
    import ctypes as C

    for kind, n in LENGTHS.items():
        lgs, nf, npad = C.c_uint32(), C.c_size_t(), C.c_size_t()
        gpu_ctx._L.frieda_codec_shape(n, C.byref(nf), C.byref(npad), C.byref(lgs))
        assert lgs.value == L, kind
    assert LENGTHS["last_column_all_padding"] * 8 < 3 * (1 << L) * 30  # no bit of column 3


@pytest.mark.parametrize("kind", sorted(LENGTHS))
def test_root_and_proof_on_off_oracle(ctx_on, ctx_off, oracle, kind):
    data = blob_of(kind)
    o_root, o_bytes = oracle_proof(oracle, data)
    for name, ctx in (("on", ctx_on), ("off", ctx_off)):
        buf, ptr = device_image(ctx, data, 0, 256, None)
        (root, proof), launches = timed(ctx, lambda: ctx.commit_and_generate_proof_device(ptr, len(data), SEED, cfg()))
        assert ("unpack30" in launches) == (name == "off"), (name, sorted(launches))
        assert root == o_root and proof.serialize() == o_bytes, (name, kind)
        assert ctx.commit(data.tobytes(), B) == o_root, (name, kind)  # a host blob: copied into the workspace, then the same passes
        buf.free()


def test_encode_handle_commitment(ctx_on, oracle):
    data = blob_of("one_byte_short")
    o_root, _ = oracle_proof(oracle, data)
    with ctx_on.encode(data.tobytes(), B) as enc:
        assert enc.commitment == o_root


@pytest.mark.parametrize("kind", ["one_byte_short", "one_short_of_felt_boundary"])
def test_bytes_behind_the_blob_never_reach_the_output(ctx_on, oracle, kind):
    """the blob ends where the poison begins (its last dword is ragged: the length is no multiple of four), three different poisons"""
    data = blob_of(kind)
    assert len(data) % 4
    o_root, o_bytes = oracle_proof(oracle, data)
    for fill in (0xFF, 0x00, None):
        buf, ptr = device_image(ctx_on, data, 64, 4096, fill)
        (root, proof), launches = timed(ctx_on, lambda: ctx_on.commit_and_generate_proof_device(ptr, len(data), SEED, cfg()))
        assert "unpack30" not in launches
        assert root == o_root and proof.serialize() == o_bytes, (kind, fill)
        buf.free()


def test_batch_of_three_with_a_stride_larger_than_the_length(gpu_ctx, ctx_off, oracle):
    """default options (the rep kernel by the 1024-workgroup rule, packed source on); the gaps between the blobs hold poison"""
    n = LENGTHS["one_past_felt_boundary"]
    stride = ((n + 3) & ~3) + 1028
    blobs = [splitmix64_bytes(8100 + i, n) for i in range(3)]
    seeds = [31, 32, 33]
    want = [oracle_proof(oracle, b, s) for b, s in zip(blobs, seeds)]
    img = np.ascontiguousarray(poison_bytes(0, 3 * stride))
    for i, b in enumerate(blobs):
        img[i * stride : i * stride + n] = b
    for name, ctx in (("on", gpu_ctx), ("off", ctx_off)):
        buf = DevBuf.from_array(ctx, img)
        got, launches = timed(ctx, lambda: ctx.commit_and_generate_proof_batch_device(buf.ptr, stride, n, 3, seeds, cfg()))
        assert ("unpack30" in launches) == (name == "off"), (name, sorted(launches))
        for (r, p), (o_r, o_b) in zip(got, want):
            assert r == o_r and p.serialize() == o_b, name
        assert ctx.commit_batch_device(buf.ptr, stride, n, 3, B) == [w[0] for w in want], name
        buf.free()


@pytest.mark.parametrize("off", [1, 2])
def test_unaligned_pointer_takes_the_unfused_path(ctx_on, oracle, off):
    data = blob_of("exact")
    o_root, o_bytes = oracle_proof(oracle, data)
    buf, ptr = device_image(ctx_on, data, 256 + off, 256, None)
    assert ptr % 4 == off
    (root, proof), launches = timed(ctx_on, lambda: ctx_on.commit_and_generate_proof_device(ptr, len(data), SEED, cfg()))
    assert launches.get("unpack30") == 1, sorted(launches)
    assert root == o_root and proof.serialize() == o_bytes
    buf.free()


def test_unaligned_batch_stride_takes_the_unfused_path(gpu_ctx, oracle):
    data = blob_of("exact")
    o_root, _ = oracle_proof(oracle, data)
    stride = len(data) + 2
    img = np.ascontiguousarray(poison_bytes(0, 2 * stride + 2))
    img[: len(data)] = data
    img[stride : stride + len(data)] = data
    buf = DevBuf.from_array(gpu_ctx, img)
    roots, launches = timed(gpu_ctx, lambda: gpu_ctx.commit_batch_device(buf.ptr, stride, len(data), 2, B))
    assert launches.get("unpack30") == 1, sorted(launches)
    assert roots == [o_root, o_root]
    buf.free()


def test_batched_proof_has_one_launch_fewer(gpu_ctx, ctx_off):
    """a 2^21 batched proof with the option on: no unpack30 entry, one launch fewer than with it off, the same bytes"""
    n = LENGTHS["exact"]
    img = np.concatenate([splitmix64_bytes(8200 + i, n) for i in range(2)])
    res = {}
    for name, ctx in (("on", gpu_ctx), ("off", ctx_off)):
        buf = DevBuf.from_array(ctx, img)
        got, launches = timed(ctx, lambda: ctx.commit_and_generate_proof_batch_device(buf.ptr, n, n, 2, [1, 2], cfg()))
        res[name] = ([(r, p.serialize()) for r, p in got], launches)
        buf.free()
    assert res["on"][0] == res["off"][0]
    assert "unpack30" not in res["on"][1] and res["off"][1].get("unpack30") == 1
    assert sum(res["on"][1].values()) == sum(res["off"][1].values()) - 1
