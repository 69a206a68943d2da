#!/usr/bin/env python3
"""A block of encoded blobs proved under one seed list: ONE frieda_prove_seeds_blobs call against the loop of K frieda_prove_seeds calls
over the same handles, in the same run:

    python tools/prove_seeds_blobs_timing.py [--reps 21] > profiles/r19_prove_seeds_blobs.txt

Configuration: blowup 2^4, 20 queries, 20-bit proof of work; route A (FRIEDA_SEEDS_FOLD_GROUP 0) and the seed-looped kernel with groups of 4.
Shapes (blobs x seeds): 64 blobs of 1 KiB x 4 seeds, 16 blobs of 128 KiB x 8 seeds, 4 blobs of a 2^22 domain x 4 seeds.

Rows: form "new" = one prove_seeds_blobs call, form "old" = the loop of K prove_seeds calls (S seeds each); both give the K * S proofs as
objects, and dropping them is part of the row in both forms.  The handles are encoded once, outside every row.

Every row is warmed twice (the first warm-up also checks that both forms serialise to the same bytes), then all rows are alternated
`reps` times; a row gives the median and the spread (min, max) of the HIP-event time on the context's stream (every call ends in a
synchronise of that stream) and the host clock beside it.  The garbage collector is off while a clock runs.  Then, in a pass of its
own with the library's kernel timer on, every row runs `--timer-reps` times and the per-kernel sums of one call are printed: where the
time went.  Records, not gates.  One JSON line per row."""
import argparse
import gc
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def blob_len_for(log_domain, log_blowup=4):
    return (4 << (log_domain - log_blowup)) * 30 // 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--timer-reps", type=int, default=3)
    ap.add_argument("--large-log-domain", type=int, default=22)
    args = ap.parse_args()
    import numpy as np
    import torch

    assert torch.cuda.is_available(), "this tool measures on the GPU: there is no CPU figure"
    import frieda_amd

    B = 4
    pcs = frieda_amd.PcsConfig(frieda_amd.FriConfig(B, 0, 20), 20)
    with open(os.path.join(ROOT, "tests", "golden", "blob"), "rb") as f:
        base = f.read()
    rng = np.random.default_rng(19)
    shapes = [
        ("64 x 1 KiB x 4 seeds", [bytes((i * 7 + j) % 256 for i in range(1024)) for j in range(64)], 4),
        ("16 x 128 KiB x 8 seeds", [base[j:] + base[:j] for j in range(16)], 8),
        (f"4 x 2^{args.large_log_domain} domain x 4 seeds", [rng.integers(0, 256, blob_len_for(args.large_log_domain), dtype=np.uint8).tobytes() for _ in range(4)], 4),
    ]
    stream = torch.cuda.Stream()
    ctx = frieda_amd.Context(0, stream.cuda_stream)
    calls = {}
    handles = []
    for shape, blobs, n_seeds in shapes:
        encs = ctx.encode_batch(blobs, B)
        handles.extend(encs)
        seeds = [1000 + 17 * s for s in range(n_seeds)]
        for group in (0, 4):
            def new(encs=encs, seeds=seeds, group=group):
                ctx.set_option("FRIEDA_SEEDS_FOLD_GROUP", group)
                return [p for row in ctx.prove_seeds_blobs(encs, seeds, pcs) for p in row]

            def old(encs=encs, seeds=seeds, group=group):
                ctx.set_option("FRIEDA_SEEDS_FOLD_GROUP", group)
                return [p for e in encs for p in ctx.prove_seeds(e, seeds, pcs)]

            calls[(shape, group, "new")] = (new, len(encs), n_seeds, len(blobs[0]))
            calls[(shape, group, "old")] = (old, len(encs), n_seeds, len(blobs[0]))

    for (shape, group, form), (call, *_rest) in calls.items():
        if form == "new":
            a = [p.serialize() for p in call()]
            b = [p.serialize() for p in calls[(shape, group, "old")][0]()]
            assert a == b, (shape, group)
        call()
    ev_ms = {name: [] for name in calls}
    host_ms = {name: [] for name in calls}
    gc.collect()
    gc.disable()
    try:
        for _ in range(args.reps):
            for name, (call, *_rest) in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                t0 = time.perf_counter()
                proofs = call()
                del proofs
                host_ms[name].append((time.perf_counter() - t0) * 1e3)
                e1.record(stream)
                e1.synchronize()
                ev_ms[name].append(e0.elapsed_time(e1))
    finally:
        gc.enable()
    for (shape, group, form), (_, k, s, length) in calls.items():
        t = ev_ms[(shape, group, form)]
        med = statistics.median(t)
        print(json.dumps({"row": "prove_seeds_blobs", "shape": shape, "seeds_fold_group": group, "form": form, "calls": 1 if form == "new" else k,
                          "proofs": k * s, "clock": "events", "ms_median": round(med, 3), "ms_min": round(min(t), 3), "ms_max": round(max(t), 3),
                          "host_ms_median": round(statistics.median(host_ms[(shape, group, form)]), 3), "proofs_per_s": round(k * s / med * 1e3),
                          "workspace_bytes": frieda_amd.seeds_blobs_workspace_bytes(length, pcs, k, s) if form == "new" else frieda_amd.seeds_workspace_bytes(length, pcs, s),
                          "reps": len(t)}), flush=True)
    # where the time went: the library's per-kernel event timer, in a pass of its own (the timer's events lengthen a call)
    ctx.set_kernel_timing(True)
    for (shape, group, form), (call, *_rest) in calls.items():
        ctx.kernel_timing_report(reset=True)
        for _ in range(args.timer_reps):
            call()
        rows = ctx.kernel_timing_report(reset=True)
        print(json.dumps({"row": "kernel_timer", "shape": shape, "seeds_fold_group": group, "form": form, "reps": args.timer_reps, "kernels": rows}), flush=True)
    ctx.set_kernel_timing(False)
    for e in handles:
        e.close()
    ctx.close()


if __name__ == "__main__":
    main()
