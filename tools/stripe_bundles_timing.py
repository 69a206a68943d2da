#!/usr/bin/env python3
"""Stripe bundles against the loop of single-blob bundle calls and against the per-cell stripe calls, on a block of 16 blobs of 128 KiB
(the reference's fixture tests/golden/blob and 15 rotations of it: 2^15 coefficients per column, blowup 2^4, 2^19 codewords), stripes
of 2^6 entries, the 513 stripes the reconstruction needs:

    python tools/stripe_bundles_timing.py [--reps 21] > profiles/r16_stripe_bundles.txt

Shapes: the 513 stripes as ONE bundle, and as EIGHT bundles of about 64 stripes.  For each shape three forms on the same stripes in the
same run:

  stripe_bundles   frieda_open_stripe_bundles / frieda_verify_stripe_bundles_many / frieda_verify_stripe_bundles /
                   frieda_reconstruct_blobs_from_stripe_bundles: one call over the block, one erasure locator
  bundle_loop      16 calls of frieda_open_cell_bundles / frieda_verify_cell_bundles_many / frieda_verify_cell_bundles /
                   frieda_reconstruct_from_cell_bundles, one per blob: sixteen locators
  stripes          the per-cell block calls: frieda_open_cells_blobs over (stripe, blob) pairs / frieda_verify_cells_blobs_many /
                   frieda_verify_cells_blobs / frieda_reconstruct_blobs_from_opened_stripes: a full path per (stripe, blob) cell

Rows: bytes (what travels: indices + values + witness or paths; arithmetic, the witness hashes asserted against
frieda_cell_bundle_witness_count), open, verify/device, verify/host (one core), rebuild (verify, pool, reconstruct, pack, commit check).

Every row is warmed twice, then all rows are alternated `reps` times; a row gives the median and the spread (min, max) of the HIP-event
time on the context's stream (every call ends in a synchronise of that stream; the host rows have no device work and give the host
clock) and the host clock beside it.  Making the openings is not part of the verify and rebuild rows.  The times are records, not
gates: the bundle form buys bytes.  One JSON line per row."""
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
    K, c = args.blobs, args.log_cell
    blobs = [base[j:] + base[:j] for j in range(K)]
    stream = torch.cuda.Stream()
    ctx = frieda_amd.Context(0, stream.cuda_stream)
    encs = [ctx.encode(d, 4) for d in blobs]
    coms = [e.commitment for e in encs]
    assert len(set(coms)) == K
    L, n = encs[0].shape
    length = len(base)
    need = (1 << (L - c)) + 1 if c else (1 << L) + 2
    pick = np.random.default_rng(11).permutation(1 << (n - c))[:need].astype(np.uint32)
    shapes = {"1_bundle": [np.sort(pick)], "8_bundles": [np.sort(p) for p in np.array_split(pick, 8)]}

    def check_rebuild(r):
        assert r == blobs

    def all_ok(r):
        assert all((x == 1).all() for x in (r if isinstance(r, list) else [r]))

    calls, meta = {}, {}
    for shape, bundles in shapes.items():
        idx = np.concatenate(bundles)
        S = len(idx)
        values, witness, wfirst = frieda_amd.open_stripe_bundles(ctx, encs, c, bundles)
        per_blob = [e.open_cell_bundles(ctx, c, bundles) for e in encs]
        svalues, spaths = frieda_amd.open_stripes(ctx, encs, c, idx)
        assert svalues.tobytes() == values.tobytes()
        for j, (v1, w1, wf1) in enumerate(per_blob):
            assert v1.tobytes() == np.ascontiguousarray(values[:, j]).tobytes() and wf1.tolist() == wfirst.tolist()
        hashes = sum(frieda_amd.cell_bundle_witness_count(n, c, b) for b in bundles)
        assert hashes == int(wfirst[-1]) and len(witness) == K * hashes
        payload = 4 * S + values.nbytes
        meta[shape] = {"blobs": K, "bundles": len(bundles), "stripes": int(S), "witness_hashes": K * hashes, "witness_hashes_per_blob": hashes,
                       "path_hashes": K * int(S) * (n - c), "bytes_stripe_bundles": payload + 32 * K * hashes + 8 * len(bundles),
                       "bytes_bundle_loop": K * (4 * S + 8 * len(bundles)) + values.nbytes + 32 * K * hashes, "bytes_stripes": payload + spaths.nbytes}
        bidx, pidx = np.tile(np.arange(K, dtype=np.uint32), S), np.repeat(idx, K)
        pv, pp = svalues.reshape(S * K, 4, -1), spaths.reshape(S * K, -1, 32)

        def add(row, stripe_call, loop_call, cells_call, check):
            calls[(shape, row, "stripe_bundles")] = (stripe_call, check)
            calls[(shape, row, "bundle_loop")] = (loop_call, check)
            calls[(shape, row, "stripes")] = (cells_call, check)

        add("open", lambda b=bundles: frieda_amd.open_stripe_bundles(ctx, encs, c, b), lambda b=bundles: [e.open_cell_bundles(ctx, c, b) for e in encs],
            lambda i=idx: frieda_amd.open_stripes(ctx, encs, c, i), lambda r: None)
        add("verify/device", lambda b=bundles, v=values, w=witness, f=wfirst: ctx.verify_stripe_bundles_many(coms, n, c, b, v, w, f),
            lambda b=bundles, pb=per_blob: [ctx.verify_cell_bundles_many(coms[j], n, c, b, *pb[j]) for j in range(K)],
            lambda v=pv, p=pp, bi=bidx, pi=pidx: ctx.verify_cells_blobs_many(coms, n, c, bi, pi, v, p), all_ok)
        add("verify/host", lambda b=bundles, v=values, w=witness, f=wfirst: frieda_amd.verify_stripe_bundles(coms, n, c, b, v, w, f),
            lambda b=bundles, pb=per_blob: [frieda_amd.verify_cell_bundles(coms[j], n, c, b, *pb[j]) for j in range(K)],
            lambda v=pv, p=pp, bi=bidx, pi=pidx: frieda_amd.verify_cells_blobs(coms, n, c, bi, pi, v, p), all_ok)
        add("rebuild", lambda b=bundles, v=values, w=witness, f=wfirst: ctx.reconstruct_blobs_from_stripe_bundles(coms, 4, length, c, b, v, w, f)[0],
            lambda b=bundles, pb=per_blob: [ctx.reconstruct_from_cell_bundles(coms[j], 4, length, c, b, *pb[j])[0] for j in range(K)],
            lambda i=idx, v=svalues, p=spaths: ctx.reconstruct_blobs_from_opened_stripes(coms, 4, length, c, i, v, p)[0], check_rebuild)

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
        print(json.dumps({"row": row, "shape": shape, "form": form, "log_cell": c, "blobs": K, "stripes": meta[shape]["stripes"],
                          "bundles": meta[shape]["bundles"], "clock": "host" if host else "events", "ms_median": round(statistics.median(t), 3),
                          "ms_min": round(min(t), 3), "ms_max": round(max(t), 3), "host_ms_median": round(statistics.median(host_ms[name]), 3), "reps": len(t)}),
              flush=True)
    for e in encs:
        e.close()
    ctx.close()


if __name__ == "__main__":
    main()
