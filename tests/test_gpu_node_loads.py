"""GPU: the node launches of tree5r_kernel and tree5_kernel (T_NODE: level A is hashed from the hashes of the level below,
frieda_amd/csrc/tree.hip) at the smallest sizes at which the launcher picks each of them, in the throughput and in the plain form.

Which kernel a node launch takes is the launcher's choice (tree_kernel_for): a node launch of 2^16 nodes or more — narrower ones go to
the quad kernel — takes tree5r when level_a + log2(batch) >= FRIEDA_T5_WIDE_LOG (default 18, smallest value 16), else the nine-level
kernel up to FRIEDA_T9_MAX_LOG, else tree5.  The smallest tree with a node launch of 2^16 nodes has 2^21 leaves (the leaf launch yields five
levels), or 2^19 where every level is kept and FRIEDA_T5_REG3_LOG makes the leaf launch stop after three; FRIEDA_TP_MIN_WGS picks the
throughput or the plain form of the compressions.  Every level of every tree is compared with the oracle's.  The timing report names
every node launch of launch_tree_a "tree5_node", whichever kernel runs it; its byte figure (96 bytes per node of every level produced)
tells the five-level kernels from the nine-level one, so a route that slid to tree9 fails here.  tree5r against tree5 and the throughput
against the plain form are the launcher's rules as read (tree_kernel_for, tp_launch): the report cannot tell them apart.
"""
import numpy as np
import pytest

from conftest import splitmix64_bytes
from util import DevBuf, GuardedBuf, blob_len_for, poison_bytes
from workspace_rows import poison

pytestmark = pytest.mark.gpu

# (kernel, form) -> the options that make the 2^16-node launch take it
ROUTES = {
    ("tree5r", "tp"): {"FRIEDA_T5_WIDE_LOG": 16, "FRIEDA_TP_MIN_WGS": 1},
    ("tree5r", "plain"): {"FRIEDA_T5_WIDE_LOG": 16, "FRIEDA_TP_MIN_WGS": 1 << 30},
    ("tree5", "tp"): {"FRIEDA_T5_WIDE_LOG": 24, "FRIEDA_T9_MAX_LOG": 15, "FRIEDA_TP_MIN_WGS": 1},
    ("tree5", "plain"): {"FRIEDA_T5_WIDE_LOG": 24, "FRIEDA_T9_MAX_LOG": 15, "FRIEDA_TP_MIN_WGS": 1 << 30},
}
M_ALL, M_ROOT, N_PROOF = 19, 21, 19
_cache = {}


def make_ctx(route, reg3=None):
    import frieda_amd

    ctx = frieda_amd.Context(0)
    for k, v in ROUTES[route].items():
        ctx.set_option(k, v)
    if reg3 is not None:
        ctx.set_option("FRIEDA_T5_REG3_LOG", reg3)
    return ctx


def launches_of(ctx, call):
    ctx.set_kernel_timing(True)
    ctx.kernel_timing_report(reset=True)
    try:
        res = call()
        rep = ctx.kernel_timing_report(reset=True)
    finally:
        ctx.set_kernel_timing(False)
    _cache["bytes"] = {k["name"]: k["alg_bytes"] for k in rep}
    return res, {k["name"]: k["launches"] for k in rep}


def assert_one_five_level_node_launch(launches, blobs=1):
    """one launch named tree5_node, of 2^16 nodes, that produced five levels (tree9 would report nine)"""
    assert launches.get("tree5_node") == 1, sorted(launches.items())
    assert _cache["bytes"]["tree5_node"] == 96.0 * blobs * sum(1 << (16 - i) for i in range(5)), _cache["bytes"]["tree5_node"]


def tree_of(oracle, m):
    if ("tree", m) not in _cache:
        cols = np.random.default_rng(4100 + m).integers(0, (1 << 31) - 1, (4, 1 << m), dtype=np.uint32)
        _cache[("tree", m)] = (cols, oracle.merkle_commit(cols))
    return _cache[("tree", m)]


def check_layers(ctx, buf, layers, m):
    for l in range(m + 1):
        off = ctx._L.frieda_merkle_layer_offset(m, l)
        assert np.array_equal(buf[off : off + (32 << l)].reshape(-1, 32), layers[l]), f"layer {l}"


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_every_level_kept(oracle, route):
    """frieda_merkle_commit of 2^19 leaves, the leaf launch three levels: node launch of 2^16 nodes, then the narrow kernels"""
    cols, layers = tree_of(oracle, M_ALL)
    ctx = make_ctx(route, reg3=M_ALL)
    try:
        d_c = DevBuf.from_array(ctx, cols)
        total = 32 * ((2 << M_ALL) - 1)
        d_l = DevBuf(ctx, total)
        rc, launches = launches_of(ctx, lambda: ctx._L.frieda_merkle_commit(ctx._h, d_c.ptr, M_ALL, d_l.ptr))
        assert rc == 0
        assert_one_five_level_node_launch(launches)
        check_layers(ctx, d_l.to_array(np.uint8, (total,)), layers, M_ALL)
    finally:
        ctx.close()


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_last_level_only(oracle, route):
    """frieda_merkle_root of 2^21 leaves: nothing kept, the node launch of 2^16 nodes writes its last level into the scratch"""
    cols, layers = tree_of(oracle, M_ROOT)
    ctx = make_ctx(route)
    try:
        d_c = DevBuf.from_array(ctx, cols)
        d_r = DevBuf(ctx, 32)
        rc, launches = launches_of(ctx, lambda: ctx._L.frieda_merkle_root(ctx._h, d_c.ptr, M_ROOT, d_r.ptr))
        assert rc == 0
        assert_one_five_level_node_launch(launches)
        assert bytes(d_r.to_array(np.uint8, (32,))) == bytes(layers[0][0])
    finally:
        ctx.close()


@pytest.mark.parametrize("kernel", ["tree5r", "tree5"])
def test_offset_pointers(oracle, kernel):
    """columns and tree storage 48 bytes into their allocations (16-byte aligned, nothing more), red zones on both sides"""
    cols, layers = tree_of(oracle, M_ALL)
    ctx = make_ctx((kernel, "tp"), reg3=M_ALL)
    try:
        total = 32 * ((2 << M_ALL) - 1)
        g_c = GuardedBuf(ctx, cols.nbytes, offset=48).upload(cols)
        g_l = GuardedBuf(ctx, total, offset=48)
        assert g_l.ptr.value % 64 == 48
        rc, launches = launches_of(ctx, lambda: ctx._L.frieda_merkle_commit(ctx._h, g_c.ptr, M_ALL, g_l.ptr))
        assert rc == 0
        assert_one_five_level_node_launch(launches)
        check_layers(ctx, g_l.payload(np.uint8, (total,)), layers, M_ALL)
        g_l.assert_zones_intact("tree storage")
        g_c.assert_zones_intact("columns")
        g_c.assert_payload_equals(cols, "columns")
        g_c.free()
        g_l.free()
    finally:
        ctx.close()


def proofs_of(oracle, count):
    """(blobs, seeds, [(root, proof bytes)]) of 2^19-domain blobs, 6 queries, no proof of work"""
    n = blob_len_for(N_PROOF) - 5
    blobs = [splitmix64_bytes(4200 + i, n) for i in range(count)]
    seeds = [61 + i for i in range(count)]
    want = []
    for b, s in zip(blobs, seeds):
        if ("proof", s) not in _cache:
            r, p = oracle.commit_and_generate_proof(b.tobytes(), s, oracle.make_config(0, 4, 0, 6))
            _cache[("proof", s)] = (bytes(r), p.serialize())
        want.append(_cache[("proof", s)])
    return blobs, seeds, want


@pytest.mark.parametrize("kernel", ["tree5r", "tree5"])
@pytest.mark.parametrize("count", [1, 3])
def test_proofs_batch_and_stride(oracle, kernel, count):
    """whole proofs of a 2^19 domain, every launch three register levels: the first tree's node launch has 2^16 nodes per blob
    (blockIdx.y = blob, the workspaces a batch stride apart); the blobs sit 1028 bytes further apart than they are long, poison between"""
    import frieda_amd

    blobs, seeds, want = proofs_of(oracle, count)
    n = len(blobs[0])
    stride = ((n + 3) & ~3) + 1028
    img = np.ascontiguousarray(poison_bytes(0, count * stride))
    for i, b in enumerate(blobs):
        img[i * stride : i * stride + n] = b
    cfg = frieda_amd.PcsConfig(frieda_amd.FriConfig(4, 0, 6), 0)
    ctx = make_ctx((kernel, "tp"), reg3=10)
    try:
        buf = DevBuf.from_array(ctx, img)
        got, launches = launches_of(ctx, lambda: ctx.commit_and_generate_proof_batch_device(buf.ptr, stride, n, count, seeds, cfg))
        assert_one_five_level_node_launch(launches, count)
        assert [(bytes(r), p.serialize()) for r, p in got] == want
        buf.free()
    finally:
        ctx.close()


def test_poisoned_workspace(oracle):
    """the same batch on a context whose every allocation is filled with 0xFFFFFFFF, then with 0, before its first use"""
    import frieda_amd

    blobs, seeds, want = proofs_of(oracle, 3)
    cfg = frieda_amd.PcsConfig(frieda_amd.FriConfig(4, 0, 6), 0)
    ctx = make_ctx(("tree5r", "tp"), reg3=10)
    try:
        for word in (0xFFFFFFFF, 0):
            poison(ctx, word)
            got = ctx.commit_and_generate_proof_batch([b.tobytes() for b in blobs], seeds, cfg)
            assert [(bytes(r), p.serialize()) for r, p in got] == want, hex(word)
    finally:
        ctx.close()
