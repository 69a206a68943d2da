#!/usr/bin/env python3
"""The cells of a block in one call against the loop of single-blob calls.  Block: the reference's 128 KiB fixture (tests/golden/blob: 2^15
coefficients per column, blowup 2^4, a 2^19 codeword) plus 15 splitmix blobs of the same length (K = 16), cells of 2^6 entries, the 513
stripes the reconstruction needs:

    python tools/stripes_timing.py [--reps 21] >> profiles/r12_stripes.txt

  open/blobs       frieda_open_cells_blobs: the 513 stripes of all 16 blobs, one call
  open/loop        16 x frieda_open_cells on the same 513 cells
  verify/blobs     frieda_verify_cells_blobs_many of those 8208 cells, one call
  verify/loop      16 x frieda_verify_cells_many
  rebuild/stripes  frieda_reconstruct_blobs_from_opened_stripes: verify, accept and gather by stripe, ONE reconstruction over 64 columns,
                   pack, batched commit check
  rebuild/loop     16 x frieda_reconstruct_from_opened_cells

The loop rows are the single-blob calls, on the same stripes, in the same run.  Every row is warmed twice, then the rows are alternated
`reps` times; a row gives the median and the spread of the HIP-event time on the context's stream (every call ends in a synchronise of
that stream) and the host clock beside it.  Encoding the blobs and slicing the loop's per-blob arrays is not part of any row.  One JSON
line per row, then one line with the three ratios loop / new call."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--log-cell", type=int, default=6)
    ap.add_argument("--blobs", type=int, default=16)
    args = ap.parse_args()
    assert args.reps >= 21, "at least 21 alternated calls per row"
    import torch

    assert torch.cuda.is_available(), "this tool measures on the GPU: there is no CPU figure"
    import frieda_amd
    from conftest import splitmix64_bytes

    with open(os.path.join(ROOT, "tests", "golden", "blob"), "rb") as f:
        first = f.read()
    K, c = args.blobs, args.log_cell
    datas = [first] + [splitmix64_bytes(1200 + j, len(first)).tobytes() for j in range(1, K)]
    stream = torch.cuda.Stream()
    ctx = frieda_amd.Context(0, stream.cuda_stream)
    encs = [ctx.encode(d, 4) for d in datas]
    coms = [e.commitment for e in encs]
    L, n = encs[0].shape
    need = (1 << (L - c)) + 1 if c else (1 << L) + 2
    stripes = np.random.default_rng(11).permutation(1 << (n - c))[:need].astype(np.uint32)
    bidx, idx = np.tile(np.arange(K, dtype=np.uint32), need), np.repeat(stripes, K)
    values, paths = frieda_amd.open_stripes(ctx, encs, c, stripes)  # [S, K, 4, 2^c], [S, K, n - c, 32]
    flat_v, flat_p = values.reshape(need * K, 4, -1), paths.reshape(need * K, n - c, 32)
    per_v = [np.ascontiguousarray(values[:, b]) for b in range(K)]
    per_p = [np.ascontiguousarray(paths[:, b]) for b in range(K)]

    def check_open_loop(r):
        for b in range(K):
            assert r[b][0].tobytes() == per_v[b].tobytes() and r[b][1].tobytes() == per_p[b].tobytes()

    def check_rebuild(blobs):
        assert list(blobs) == datas

    calls = {
        "open/blobs": (lambda: frieda_amd.open_cells_blobs(ctx, encs, c, bidx, idx),
                       lambda r: r[0].tobytes() == flat_v.tobytes() and r[1].tobytes() == flat_p.tobytes() or sys.exit("open/blobs differs")),
        "open/loop": (lambda: [encs[b].open_cells(ctx, c, stripes) for b in range(K)], check_open_loop),
        "verify/blobs": (lambda: ctx.verify_cells_blobs_many(coms, n, c, bidx, idx, flat_v, flat_p), lambda r: r.all() or sys.exit("verify/blobs rejected a cell")),
        "verify/loop": (lambda: [ctx.verify_cells_many(coms[b], n, c, stripes, per_v[b], per_p[b]) for b in range(K)],
                        lambda r: all(x.all() for x in r) or sys.exit("verify/loop rejected a cell")),
        "rebuild/stripes": (lambda: ctx.reconstruct_blobs_from_opened_stripes(coms, 4, len(first), c, stripes, values, paths)[0], check_rebuild),
        "rebuild/loop": (lambda: [ctx.reconstruct_from_opened_cells(coms[b], 4, len(first), c, stripes, per_v[b], per_p[b])[0] for b in range(K)], check_rebuild),
    }
    for name, (call, check) in calls.items():
        for _ in range(2):
            check(call())
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
    med = {}
    for name in calls:
        t = ev_ms[name]
        med[name] = statistics.median(t)
        print(json.dumps({"row": name, "blobs": K, "log_cell": c, "stripes": int(need), "cells": int(need * K), "clock": "events",
                          "ms_median": round(med[name], 3), "ms_min": round(min(t), 3), "ms_max": round(max(t), 3),
                          "host_ms_median": round(statistics.median(host_ms[name]), 3), "reps": len(t)}), flush=True)
    print(json.dumps({"ratio_loop_over_new": {a: round(med[b] / med[a], 2) for a, b in (("open/blobs", "open/loop"), ("verify/blobs", "verify/loop"),
                                                                                      ("rebuild/stripes", "rebuild/loop"))}}), flush=True)
    for e in encs:
        e.close()
    ctx.close()


if __name__ == "__main__":
    main()
