#!/usr/bin/env python3
"""Cell bundles against separate cells on the reference's 128 KiB fixture (tests/golden/blob: 2^15 coefficients per column, blowup 2^4, a
2^19 codeword), cells of 2^6 entries, the 513 cells the reconstruction needs:

    python tools/cell_bundles_timing.py [--reps 21] > profiles/r15_cell_bundles.txt

Shapes: the 513 cells as ONE bundle, and as EIGHT bundles of about 64 cells.  For each shape, the bundle form against the per-cell form
(frieda_open_cells / frieda_verify_cells_many / frieda_verify_cells / frieda_reconstruct_from_opened_cells) on the same cells in the same run:

  bytes          what travels: indices + values + witness (bundle form) or + paths (per-cell form).  Arithmetic; the witness hashes are
                 asserted against frieda_cell_bundle_witness_count
  open           frieda_open_cell_bundles (the wrapper's two calls: the size query, then the opening) / frieda_open_cells
  verify/device  frieda_verify_cell_bundles_many / frieda_verify_cells_many
  verify/host    frieda_verify_cell_bundles / frieda_verify_cells (one core)
  rebuild        frieda_reconstruct_from_cell_bundles / frieda_reconstruct_from_opened_cells: verify, pool, reconstruct, pack, commit check

Every row is warmed twice, then all rows are alternated `reps` times; a row gives the median and the spread (min, max) of the HIP-event
time on the context's stream (every call ends in a synchronise of that stream; the host rows have no device work and give the host
clock) and the host clock beside it.  Making the openings is not part of the verify and rebuild rows.  The times are records, not
gates: one wave verifies one bundle, so a call of few large bundles is latency-bound by design.  One JSON line per row."""
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
    args = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "this tool measures on the GPU: there is no CPU figure"
    import frieda_amd

    with open(os.path.join(ROOT, "tests", "golden", "blob"), "rb") as f:
        data = f.read()
    stream = torch.cuda.Stream()
    ctx = frieda_amd.Context(0, stream.cuda_stream)
    c = args.log_cell
    enc = ctx.encode(data, 4)
    root = enc.commitment
    L, n = enc.shape
    need = (1 << (L - c)) + 1 if c else (1 << L) + 2
    pick = np.random.default_rng(11).permutation(1 << (n - c))[:need].astype(np.uint32)
    shapes = {"1_bundle": [np.sort(pick)], "8_bundles": [np.sort(p) for p in np.array_split(pick, 8)]}

    def check_rebuild(r):
        assert r[0] == data

    def all_ok(r):
        assert (r == 1).all()

    calls, meta = {}, {}
    for shape, bundles in shapes.items():
        idx = np.concatenate(bundles)
        values, witness, wfirst = enc.open_cell_bundles(ctx, c, bundles)
        cvalues, paths = enc.open_cells(ctx, c, idx)
        assert cvalues.tobytes() == values.tobytes()
        hashes = sum(frieda_amd.cell_bundle_witness_count(n, c, b) for b in bundles)
        assert hashes == int(wfirst[-1]) == len(witness)
        payload = 4 * len(idx) + values.nbytes
        meta[shape] = {"bundles": len(bundles), "cells": int(len(idx)), "witness_hashes": hashes, "path_hashes": int(len(idx)) * (n - c),
                       "bytes_bundles": payload + 32 * hashes + 8 * len(bundles), "bytes_cells": payload + paths.nbytes}

        def add(row, bundle_call, cell_call, check):
            calls[(shape, row, "bundles")] = (bundle_call, check)
            calls[(shape, row, "cells")] = (cell_call, check)

        add("open", lambda b=bundles: enc.open_cell_bundles(ctx, c, b), lambda i=idx: enc.open_cells(ctx, c, i), lambda r: None)
        add("verify/device", lambda b=bundles, v=values, w=witness, f=wfirst: ctx.verify_cell_bundles_many(root, n, c, b, v, w, f),
            lambda i=idx, v=values, p=paths: ctx.verify_cells_many(root, n, c, i, v, p), all_ok)
        add("verify/host", lambda b=bundles, v=values, w=witness, f=wfirst: frieda_amd.verify_cell_bundles(root, n, c, b, v, w, f),
            lambda i=idx, v=values, p=paths: frieda_amd.verify_cells(root, n, c, i, v, p), all_ok)
        add("rebuild", lambda b=bundles, v=values, w=witness, f=wfirst: ctx.reconstruct_from_cell_bundles(root, 4, len(data), c, b, v, w, f),
            lambda i=idx, v=values, p=paths: ctx.reconstruct_from_opened_cells(root, 4, len(data), c, i, v, p), check_rebuild)

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
    for shape in shapes:
        print(json.dumps(dict({"row": "bytes", "shape": shape, "log_cell": c}, **meta[shape])), flush=True)
    for (shape, row, form) in calls:
        name = (shape, row, form)
        host = row == "verify/host"
        t = host_ms[name] if host else ev_ms[name]
        print(json.dumps({"row": row, "shape": shape, "form": form, "log_cell": c, "cells": meta[shape]["cells"], "bundles": meta[shape]["bundles"],
                          "clock": "host" if host else "events", "ms_median": round(statistics.median(t), 3), "ms_min": round(min(t), 3),
                          "ms_max": round(max(t), 3), "host_ms_median": round(statistics.median(host_ms[name]), 3), "reps": len(t)}), flush=True)
    enc.close()
    ctx.close()


if __name__ == "__main__":
    main()
