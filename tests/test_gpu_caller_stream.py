"""GPU: a context on the CALLER's stream (frieda_ctx_create(device, stream, ..): "e.g. torch's current stream").

Same bytes: a dozen rows of tests/workspace_rows.py on a context made over a torch stream equal the result of a private-stream context.

Ordering in: the entry points documented "asynchronous on the ctx stream — no host synchronisation" are enqueued behind work of the
caller's own on that stream — a long chain of matmuls, then the copy that writes the real input into a buffer that until then holds other
valid data — and their output is cloned by the caller on the same stream, with no host synchronisation anywhere in between.  A launch
or copy of the library that lands on another stream (the null stream: the library's private streams are non-blocking, so nothing orders
it) reads the other data, and the clone is not the oracle's answer for the real input.  The precondition is measured in the test: the
filler lasts at least ten times as long as the op, else the op could finish in order by luck.

The stream survives the context (own_stream = false), and two contexts share one stream."""
import numpy as np
import pytest

import test_gpu_buffer_contract as BC
import workspace_rows as W
from workspace_rows import ROWS, norm, setup

pytestmark = pytest.mark.gpu

SAME_BYTES = ("commit/general", "commit/small_fused", "prove/general", "prove/small_fused", "prove_seeds/2p16", "evaluate/tile12", "merkle_root",
              "decommit_device/multi_block", "verify_many", "open_cells/small_fused", "reconstruct_from_proof_pairs",
              "reconstruct_blobs_from_opened_stripes", "interpolate_points/tree")


@pytest.fixture(scope="module")
def stream():
    import torch

    assert torch.cuda.is_available()
    return torch.cuda.Stream()


def on_stream(stream, row=None):
    import frieda_amd

    ctx = frieda_amd.Context(0, stream=stream.cuda_stream)
    if row is not None:
        setup(ctx, row)
    return ctx


@pytest.mark.parametrize("name", SAME_BYTES)
def test_same_bytes_as_on_a_private_stream(oracle, stream, name):
    import frieda_amd

    row = ROWS[name]
    private = frieda_amd.Context(0)
    try:
        setup(private, row)
        r0 = norm(row.run(private, oracle))
    finally:
        private.close()
    ctx = on_stream(stream, row)
    try:
        assert norm(row.run(ctx, oracle)) == r0
        W.poison(ctx, 0xFFFFFFFF)
        assert norm(row.run(ctx, oracle)) == r0
    finally:
        ctx.close()


# ---- ordering in ---------------------------------------------------------------------------------------------------------------------
# (entry point of test_gpu_buffer_contract.TABLE, shape of its SHAPES list): the asynchronous entry points
ASYNC_OPS = [("frieda_commit_device", 3001), ("frieda_commit_device", (4 << 17) * 30 // 8 - 4321), ("frieda_unpack30", 262147), ("frieda_circle_evaluate", (12, 16, 4)),
             ("frieda_merkle_root", 12), ("frieda_fold_line", 12), ("frieda_bit_reverse_column", (12, 4, 5000)), ("frieda_dev_gather_device", (4, 4096)),
             ("frieda_merkle_decommit_device", (12, 600))]
KEEP = ("d_idx", "d_positions")  # index lists stay as they are: the "other valid data" must still be a valid call


def _other(arr):
    """other valid data of the same shape: the same words, rotated by one"""
    a = np.ascontiguousarray(arr)
    return np.roll(a.reshape(-1), 1).reshape(a.shape)


class Filler:
    """a chain of matmuls on scratch tensors, enqueued on the current stream"""

    def __init__(self, n=2048):
        import torch

        self.a = torch.rand((n, n), device="cuda") / n
        self.b = torch.rand((n, n), device="cuda") / n
        self.count = 8

    def enqueue(self):
        import torch

        x = self.a
        for _ in range(self.count):
            x = torch.mm(x, self.b)
        return x


def _elapsed_ms(stream, fn):
    import torch

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        e0.record()
        fn()
        e1.record()
    stream.synchronize()
    return e0.elapsed_time(e1)


@pytest.mark.parametrize("entry,shape", ASYNC_OPS, ids=[f"{e}-{s}".replace(" ", "") for e, s in ASYNC_OPS])
def test_an_asynchronous_call_runs_behind_the_callers_work(oracle, stream, entry, shape):
    import torch

    case = W.cached(("case", entry, shape), lambda: BC.BUILDERS[entry](oracle, shape))
    params = BC.TABLE[entry]
    ctx = on_stream(stream)
    try:
        with torch.cuda.stream(stream):
            bufs = {p: torch.full((case.size[p] + 3 & ~3,), 0xEE, dtype=torch.uint8, device="cuda") for p in case.size}
            real = {p: [(at, torch.from_numpy(np.ascontiguousarray(arr).reshape(-1).view(np.uint8).copy()).cuda()) for at, arr in segs]
                    for p, segs in case.inputs.items()}

            def load(other):
                for p, segs in case.inputs.items():
                    for at, arr in segs:
                        a = _other(arr) if other and p not in KEEP else np.ascontiguousarray(arr)
                        bufs[p][at:at + a.nbytes].copy_(torch.from_numpy(a.reshape(-1).view(np.uint8).copy()))

            load(other=False)
        stream.synchronize()
        addr = {p: b.data_ptr() for p, b in bufs.items()}
        assert all(a % 16 == 0 for a in addr.values())

        def call():
            rc = case.call(ctx, addr, {})
            assert rc == 0, (rc, ctx._L.frieda_last_error(ctx._h))

        # the precondition: an idle run of the op (twice: the first pays the twiddles and the workspace) against the filler
        _elapsed_ms(stream, call)
        op_ms = _elapsed_ms(stream, call)
        filler = Filler()
        _elapsed_ms(stream, filler.enqueue)
        fill_ms = _elapsed_ms(stream, filler.enqueue)
        while fill_ms < 10 * op_ms and filler.count < 4096:
            filler.count *= 2
            fill_ms = _elapsed_ms(stream, filler.enqueue)
        times = f"filler of {filler.count} matmuls {fill_ms:.3f} ms, idle {entry} {op_ms:.3f} ms"
        assert fill_ms >= 10 * op_ms, times

        outs = [p for p, (role, _) in params.items() if role != "in" and p in case.expect]
        assert outs, f"{entry}: no device output to clone (the ordering test would pass without reading anything)"
        with torch.cuda.stream(stream):
            load(other=True)
            for p in outs:
                if params[p][0] == "out":
                    bufs[p].fill_(0xEE)
        stream.synchronize()
        with torch.cuda.stream(stream):
            filler.enqueue()                                   # 1. the caller's own work
            for p, segs in real.items():                        # 2. the copy that writes the real input
                for at, t in segs:
                    bufs[p][at:at + t.numel()].copy_(t, non_blocking=True)
            call()                                             # 3. the op: no host synchronisation
            clones = {p: bufs[p].clone() for p in outs}        # 4. the caller reads the output on its stream, then overwrites it
            for p in outs:
                bufs[p].fill_(0x11)
        stream.synchronize()
        for p in outs:
            got = clones[p].cpu().numpy()
            for at, exp in case.expect[p]:
                exp = np.ascontiguousarray(exp).reshape(-1).view(np.uint8)
                assert np.array_equal(got[at:at + exp.size], exp), f"{entry}: {p} is not the oracle's answer for the real input ({times})"
    finally:
        ctx.close()


# ---- the stream is the caller's --------------------------------------------------------------------------------------------------------
def test_the_stream_survives_the_context(oracle):
    import torch

    s = torch.cuda.Stream()
    row = ROWS["prove/general"]
    ctx = on_stream(s, row)
    r0 = norm(row.run(ctx, oracle))
    ctx.close()  # own_stream = false: the stream is not destroyed
    with torch.cuda.stream(s):
        x = torch.arange(1 << 20, device="cuda", dtype=torch.int64)
        total = (x * 2).sum()
    s.synchronize()
    assert int(total) == (1 << 20) * ((1 << 20) - 1)
    again = on_stream(s, row)
    try:
        assert norm(row.run(again, oracle)) == r0
    finally:
        again.close()
    assert s.query()


def test_two_contexts_on_one_stream_interleaved(oracle, stream):
    """frieda_commit_device and frieda_circle_evaluate of two contexts alternate on one stream with no synchronisation in between"""
    import torch

    jobs = [("frieda_commit_device", 3001), ("frieda_circle_evaluate", (12, 16, 4)), ("frieda_commit_device", (4 << 17) * 30 // 8 - 4321),
            ("frieda_merkle_root", 12), ("frieda_circle_evaluate", (5, 9, 4)), ("frieda_fold_line", 12)]
    a, b = on_stream(stream), on_stream(stream)
    try:
        state = []
        with torch.cuda.stream(stream):
            for rounds in range(2):
                for i, (entry, shape) in enumerate(jobs):
                    case = W.cached(("case", entry, shape), lambda: BC.BUILDERS[entry](oracle, shape))
                    bufs = {p: torch.full((case.size[p] + 3 & ~3,), 0xEE, dtype=torch.uint8, device="cuda") for p in case.size}
                    for p, segs in case.inputs.items():
                        for at, arr in segs:
                            h = torch.from_numpy(np.ascontiguousarray(arr).reshape(-1).view(np.uint8).copy())
                            bufs[p][at:at + h.numel()].copy_(h)
                    ctx = (a, b)[(i + rounds) % 2]
                    assert case.call(ctx, {p: t.data_ptr() for p, t in bufs.items()}, {}) == 0
                    state.append((entry, case, bufs))
        stream.synchronize()
        for entry, case, bufs in state:
            for p, segs in case.expect.items():
                got = bufs[p].cpu().numpy()
                for at, exp in segs:
                    exp = np.ascontiguousarray(exp).reshape(-1).view(np.uint8)
                    assert np.array_equal(got[at:at + exp.size], exp), (entry, p)
    finally:
        a.close()
        b.close()
