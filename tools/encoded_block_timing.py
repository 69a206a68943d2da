#!/usr/bin/env python3
"""Encoded handles for a block in one call and straight from a rebuild, each new call against what it replaces, in the same run:

    python tools/encoded_block_timing.py [--reps 21] > profiles/r18_encoded_block.txt

Inputs: the 128 KiB fixture (tests/golden/blob: 2^15 coefficients per column, blowup 2^4, a 2^19 codeword) with the 513 cells of 2^6 entries
the reconstruction needs; a block of 16 such blobs (the fixture and 15 rotations) with 513 stripes; 64 blobs of 1 KiB.

Rows (form "new" against form "old"):
  encode_batch                       frieda_encode_batch over the block           | the loop of K frieda_encode
  rebuild/opened_cells               frieda_rebuild_encoded_from_opened_cells      | frieda_reconstruct_from_opened_cells, then frieda_encode of its bytes
  rebuild/cell_bundles               frieda_rebuild_encoded_from_cell_bundles      | frieda_reconstruct_from_cell_bundles, then frieda_encode
  rebuild/opened_stripes             frieda_rebuild_encoded_blobs_from_opened_stripes | frieda_reconstruct_blobs_from_opened_stripes, then K frieda_encode
  rebuild/stripe_bundles             frieda_rebuild_encoded_blobs_from_stripe_bundles | frieda_reconstruct_blobs_from_stripe_bundles, then K frieda_encode
  rebuild/..., form "new_no_bytes"   the new call with out_bytes = NULL (nothing packed or downloaded)

Every row is warmed twice, then all rows are alternated `reps` times; a row gives the median and the spread (min, max) of the HIP-event
time on the context's stream (every call ends in a synchronise of that stream) and the host clock beside it.  Closing the handles a
row made is part of the row in both forms.  Making the openings is not part of the rebuild rows.  Records, not gates.  One JSON line
per row."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--log-cell", type=int, default=6)
    ap.add_argument("--blobs", type=int, default=16)
    args = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "this tool measures on the GPU: there is no CPU figure"
    import frieda_amd

    with open(os.path.join(ROOT, "tests", "golden", "blob"), "rb") as f:
        base = f.read()
    K, c, B = args.blobs, args.log_cell, 4
    blobs = [base[j:] + base[:j] for j in range(K)]
    small = [bytes((i * 7 + j) % 256 for i in range(1024)) for j in range(64)]
    stream = torch.cuda.Stream()
    ctx = frieda_amd.Context(0, stream.cuda_stream)
    encs = [ctx.encode(d, B) for d in blobs]
    coms = [e.commitment for e in encs]
    L, n = encs[0].shape
    length = len(base)
    need = (1 << (L - c)) + 1 if c else (1 << L) + 2
    pick = np.random.default_rng(11).permutation(1 << (n - c))[:need].astype(np.uint32)
    bundles = [np.sort(p) for p in np.array_split(pick, 8)]
    v1, p1 = encs[0].open_cells(ctx, c, pick)
    bv1, bw1, bf1 = encs[0].open_cell_bundles(ctx, c, bundles)
    sv, sp = frieda_amd.open_stripes(ctx, encs, c, pick)
    bv, bw, bf = frieda_amd.open_stripe_bundles(ctx, encs, c, bundles)
    for e in encs:
        e.close()

    def close(es):
        for e in es:
            e.close()

    def commitments(es):
        r = [e.commitment for e in es]
        close(es)
        return r

    def new(fn, *a, **kw):
        r = fn(*a, **kw)
        return commitments(r[3] if isinstance(r[3], list) else [r[3]])

    def old(fn, *a):
        r = fn(*a)
        return commitments([ctx.encode(d, B) for d in (r[0] if isinstance(r[0], list) else [r[0]])])

    small_roots = ctx.commit_batch(small, B)
    calls = {
        ("encode_batch", "16 x 128 KiB", "new"): (lambda: commitments(ctx.encode_batch(blobs, B)), coms),
        ("encode_batch", "16 x 128 KiB", "old"): (lambda: commitments([ctx.encode(d, B) for d in blobs]), coms),
        ("encode_batch", "64 x 1 KiB", "new"): (lambda: commitments(ctx.encode_batch(small, B)), small_roots),
        ("encode_batch", "64 x 1 KiB", "old"): (lambda: commitments([ctx.encode(d, B) for d in small]), small_roots),
    }
    one = (coms[0], B, length, c)
    blk = (coms, B, length, c)
    for row, shape, new_fn, old_fn, head, tail, want in [
        ("rebuild/opened_cells", "1 x 128 KiB, 513 cells", ctx.rebuild_encoded_from_opened_cells, ctx.reconstruct_from_opened_cells, one, (pick, v1, p1), coms[:1]),
        ("rebuild/cell_bundles", "1 x 128 KiB, 513 cells in 8 bundles", ctx.rebuild_encoded_from_cell_bundles, ctx.reconstruct_from_cell_bundles, one, (bundles, bv1, bw1, bf1), coms[:1]),
        ("rebuild/opened_stripes", "16 x 128 KiB, 513 stripes", ctx.rebuild_encoded_blobs_from_opened_stripes, ctx.reconstruct_blobs_from_opened_stripes, blk, (pick, sv, sp), coms),
        ("rebuild/stripe_bundles", "16 x 128 KiB, 513 stripes in 8 bundles", ctx.rebuild_encoded_blobs_from_stripe_bundles, ctx.reconstruct_blobs_from_stripe_bundles, blk, (bundles, bv, bw, bf), coms),
    ]:
        a = head + tail
        calls[(row, shape, "new")] = (lambda f=new_fn, a=a: new(f, *a), want)
        calls[(row, shape, "new_no_bytes")] = (lambda f=new_fn, a=a: new(f, *a, want_bytes=False), want)
        calls[(row, shape, "old")] = (lambda f=old_fn, a=a: old(f, *a), want)

    for name, (call, want) in calls.items():
        for _ in range(2):
            assert call() == want, name
    ev_ms = {name: [] for name in calls}
    host_ms = {name: [] for name in calls}
    for _ in range(args.reps):
        for name, (call, _) in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            t0 = time.perf_counter()
            call()
            host_ms[name].append((time.perf_counter() - t0) * 1e3)
            e1.record(stream)
            e1.synchronize()
            ev_ms[name].append(e0.elapsed_time(e1))
    for (row, shape, form) in calls:
        t = ev_ms[(row, shape, form)]
        print(json.dumps({"row": row, "shape": shape, "form": form, "log_cell": c, "clock": "events", "ms_median": round(statistics.median(t), 3),
                          "ms_min": round(min(t), 3), "ms_max": round(max(t), 3), "host_ms_median": round(statistics.median(host_ms[(row, shape, form)]), 3),
                          "reps": len(t)}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
