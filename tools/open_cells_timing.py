#!/usr/bin/env python3
"""Authenticated cells on the reference's 128 KiB fixture (tests/golden/blob: 2^15 coefficients per column, blowup 2^4, a 2^19 codeword),
cells of 2^6 entries, the 513 cells the reconstruction needs:

    python tools/open_cells_timing.py [--reps 21] >> profiles/r11_open_cells.txt

  open          frieda_open_cells of the 513 cells (upload of the indices, two launches, one download)
  verify/device frieda_verify_cells_many of those cells
  verify/host   frieda_verify_cells of the same cells (one core)
  rebuild/cells frieda_reconstruct_from_opened_cells: verify, pool, reconstruct, pack, commit check
  rebuild/pairs frieda_reconstruct_from_proof_pairs from the smallest list of 20-query proofs that holds 2^15 + 2 pair points

Every row is warmed twice, then the rows are alternated `reps` times; a row gives the median and the spread of the HIP-event time on the
context's stream (every call ends in a synchronise of that stream; the host row has no device work and gives the host clock) and the
host clock beside it.  Making the proofs and the openings is not part of any row.  One JSON line per row."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--log-cell", type=int, default=6)
    ap.add_argument("--chunk", type=int, default=128, help="seeds per prove_seeds call")
    args = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "this tool measures on the GPU: there is no CPU figure"
    import frieda_amd
    from pooled_pairs_timing import prefix_needed

    with open(os.path.join(ROOT, "tests", "golden", "blob"), "rb") as f:
        data = f.read()
    stream = torch.cuda.Stream()
    ctx = frieda_amd.Context(0, stream.cuda_stream)
    c = args.log_cell
    enc = ctx.encode(data, 4)
    root = enc.commitment
    L, n = enc.shape
    need = (1 << (L - c)) + 1 if c else (1 << L) + 2
    idx = np.random.default_rng(11).permutation(1 << (n - c))[:need].astype(np.uint32)
    values, paths = enc.open_cells(ctx, c, idx)

    # the proofs of the pair row
    cfg = frieda_amd.PcsConfig(frieda_amd.FriConfig(4, 0, 20), 0)
    proofs, seeds, points = [], [], []
    n_p = None
    while n_p is None:
        new = list(range(len(seeds) + 1, len(seeds) + 1 + args.chunk))
        ps = ctx.prove_seeds(enc, new, cfg)
        st, pts = ctx.verify_pairs_many(ps, new, root)
        assert set(st) == {1}
        proofs += ps
        seeds += new
        points += [p[0] for p in pts]
        if len(seeds) * 40 >= (1 << L) + 2:
            n_p = prefix_needed(points, (1 << L) + 2)

    def check_rebuild(r):
        assert r[0] == data

    calls = {
        "open": (lambda: enc.open_cells(ctx, c, idx), lambda r: None),
        "verify/device": (lambda: ctx.verify_cells_many(root, n, c, idx, values, paths), lambda r: r.all() or sys.exit("device verifier rejected a cell")),
        "verify/host": (lambda: frieda_amd.verify_cells(root, n, c, idx, values, paths), lambda r: r.all() or sys.exit("host verifier rejected a cell")),
        "rebuild/cells": (lambda: ctx.reconstruct_from_opened_cells(root, 4, len(data), c, idx, values, paths), check_rebuild),
        "rebuild/pairs": (lambda: ctx.reconstruct_from_proof_pairs(proofs[:n_p], seeds[:n_p], root, len(data)), check_rebuild),
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
    for name in calls:
        t = host_ms[name] if name == "verify/host" else ev_ms[name]
        row = {"row": name, "log_cell": c, "cells": int(need), "clock": "host" if name == "verify/host" else "events",
               "ms_median": round(statistics.median(t), 3), "ms_min": round(min(t), 3), "ms_max": round(max(t), 3),
               "host_ms_median": round(statistics.median(host_ms[name]), 3), "reps": len(t)}
        if name == "rebuild/pairs":
            row["proofs"] = n_p
        print(json.dumps(row), flush=True)
    enc.close()
    ctx.close()


if __name__ == "__main__":
    main()
