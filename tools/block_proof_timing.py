#!/usr/bin/env python3
"""Block proofs against one proof per commitment, and the aggregate handle they rest on, in one run on one MI355X:

    python tools/block_proof_timing.py [--reps 21] > profiles/r24_block_proof.txt

Configuration: blowup 2^4, 20 queries, 20-bit proof of work.  Blocks: 64 blobs of 1 KiB under 4 seeds, 16 blobs of 128 KiB under 8
seeds, 4 blobs of a 2^22 domain under 4 seeds (the rectangles of profiles/r19_prove_seeds_blobs.txt).  The handles are encoded once,
outside every row.

Rows of a block ("form"):
    aggregate, aggregate_plain, aggregate_split   frieda_aggregate_encoded (and the handle freed): the route the library picks, and
                    FRIEDA_AGG_SPLIT 1 / 2, the one-thread chain and the chain split over a workgroup's waves.  Once per block, whatever the seeds.
    block           frieda_prove_block_seeds: S block proofs from the aggregate and the K handles
    blobs           frieda_prove_seeds_blobs on the same handles and seeds: K * S proofs   (what the parent commit offers)
Every row is warmed twice (the first warm-up also checks that every block proof verifies and that the three aggregate routes give one
commitment), then all rows are alternated `reps` times; a row gives the median and the spread (min, max) of the HIP-event time on the
context's stream (every call ends in a synchronise of that stream) and the host clock beside it.  The garbage collector is off while a
clock runs.

Beside them, per block:
    bytes           one serialised block proof against the K serialised proofs it replaces (the same seed)
    client          frieda_verify_block on one core against K times frieda_verify (host clock, median of `reps`)
Records, not gates.  One JSON line per row.

The combination kernel alone has no timer name of its own (aggregate.hip); its time comes from a kernel trace in a run of its own,

    rocprofv3 --kernel-trace --stats -d OUT -- python tools/block_proof_timing.py --aggregate-only 20

which does nothing but 20 frieda_aggregate_encoded calls per block and route (aggregate_kernel: FRIEDA_AGG_SPLIT 1, aggregate_split_kernel: 2)
after printing, per block, the bytes the kernel moves, 16 * (K + 1) * 2^n, and the time they take at 8.0 TB/s (the HBM specification) and
at 6.3 TB/s (what a streaming copy achieves on this chip)."""
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
    ap.add_argument("--large-log-domain", type=int, default=22)
    ap.add_argument("--aggregate-only", type=int, default=0, metavar="N", help="N aggregate calls per block and route, nothing else (for a kernel trace)")
    args = ap.parse_args()
    import numpy as np
    import torch

    assert torch.cuda.is_available(), "this tool measures on the GPU: there is no CPU figure"
    import frieda_amd

    B = 4
    pcs = frieda_amd.PcsConfig(frieda_amd.FriConfig(B, 0, 20), 20)
    with open(os.path.join(ROOT, "tests", "golden", "blob"), "rb") as f:
        base = f.read()
    rng = np.random.default_rng(24)
    shapes = [
        ("64 x 1 KiB", [bytes((i * 7 + j) % 256 for i in range(1024)) for j in range(64)], 4),
        ("16 x 128 KiB", [base[j:] + base[:j] for j in range(16)], 8),
        (f"4 x 2^{args.large_log_domain} domain", [rng.integers(0, 256, blob_len_for(args.large_log_domain), dtype=np.uint8).tobytes() for _ in range(4)], 4),
    ]
    stream = torch.cuda.Stream()
    ctx = frieda_amd.Context(0, stream.cuda_stream)
    calls, keep = {}, []
    for shape, blobs, n_seeds in shapes:
        encs = ctx.encode_batch(blobs, B)
        keep.extend(encs)
        k, log_domain = len(encs), encs[0].shape[1]
        seeds = [1000 + 17 * s for s in range(n_seeds)]
        commitments = [e.commitment for e in encs]
        agg = ctx.aggregate_encoded(encs)
        keep.append(agg)

        def run_aggregate(mode, encs=encs):
            ctx.set_option("FRIEDA_AGG_SPLIT", mode)
            try:
                return ctx.aggregate_encoded(encs)
            finally:
                ctx.set_option("FRIEDA_AGG_SPLIT", 0)

        def run_block(encs=encs, agg=agg, seeds=seeds):
            return ctx.prove_block_seeds(agg, encs, seeds, pcs)

        def run_blobs(encs=encs, seeds=seeds):
            return ctx.prove_seeds_blobs(encs, seeds, pcs)

        if args.aggregate_only:
            nbytes = 16 * (k + 1) * (1 << log_domain)
            print(json.dumps({"row": "kernel_bytes", "shape": shape, "blobs": k, "log_domain": log_domain, "alg_bytes": nbytes,
                              "us_at_8.0_TB_s": round(nbytes / 8.0e12 * 1e6, 2), "us_at_6.3_TB_s": round(nbytes / 6.3e12 * 1e6, 2)}), flush=True)
            for mode in (1, 2):
                for _ in range(args.aggregate_only):
                    run_aggregate(mode).close()
            continue
        calls[(shape, "aggregate")] = (lambda f=run_aggregate: f(0).close(), 0)
        calls[(shape, "aggregate_plain")] = (lambda f=run_aggregate: f(1).close(), 0)
        calls[(shape, "aggregate_split")] = (lambda f=run_aggregate: f(2).close(), 0)
        calls[(shape, "block")] = (run_block, n_seeds)
        calls[(shape, "blobs")] = (run_blobs, k * n_seeds)
        # the first warm-up: every block proof verifies, and the routes agree
        bps = run_block()
        for s, bp in zip(seeds, bps):
            assert frieda_amd.verify_block(commitments, bp, s) == (True, 0), (shape, s)
        roots = set()
        for mode in (0, 1, 2):
            with run_aggregate(mode) as g:
                roots.add(g.commitment)
        assert roots == {agg.commitment}, shape
        proofs = run_blobs()
        # bytes: one block proof against the K proofs of the same seed
        block_bytes = len(bps[0].serialize())
        proof_bytes = sum(len(proofs[b][0].serialize()) for b in range(k))
        print(json.dumps({"row": "bytes", "shape": shape, "blobs": k, "log_domain": log_domain, "block_proof_bytes": block_bytes,
                          "fri_part_bytes": len(bps[0].fri.serialize()), "stripes": bps[0].n_stripes, "witness_hashes_per_blob": bps[0].witness_hashes,
                          "k_proofs_bytes": proof_bytes, "ratio": round(block_bytes / proof_bytes, 3)}), flush=True)
        # the client: one core, host clock
        t_block, t_loop = [], []
        firsts = [proofs[b][0] for b in range(k)]
        gc.collect()
        gc.disable()
        try:
            for _ in range(args.reps):
                t0 = time.perf_counter()
                ok = frieda_amd.verify_block(commitments, bps[0], seeds[0])
                t_block.append((time.perf_counter() - t0) * 1e3)
                assert ok == (True, 0)
                t0 = time.perf_counter()
                oks = [frieda_amd.verify(p, seeds[0]) for p in firsts]
                t_loop.append((time.perf_counter() - t0) * 1e3)
                assert all(oks)
        finally:
            gc.enable()
        print(json.dumps({"row": "client", "shape": shape, "blobs": k, "verify_block_ms_median": round(statistics.median(t_block), 3),
                          "verify_block_ms_min": round(min(t_block), 3), "verify_block_ms_max": round(max(t_block), 3),
                          "k_times_verify_ms_median": round(statistics.median(t_loop), 3), "k_times_verify_ms_min": round(min(t_loop), 3),
                          "k_times_verify_ms_max": round(max(t_loop), 3), "reps": len(t_block)}), flush=True)
        del bps, proofs, firsts
    for call, _ in calls.values():
        call()
    ev_ms = {name: [] for name in calls}
    host_ms = {name: [] for name in calls}
    gc.collect()
    gc.disable()
    try:
        for _ in range(args.reps):
            for name, (call, _) in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                t0 = time.perf_counter()
                out = call()
                del out
                host_ms[name].append((time.perf_counter() - t0) * 1e3)
                e1.record(stream)
                e1.synchronize()
                ev_ms[name].append(e0.elapsed_time(e1))
    finally:
        gc.enable()
    for (shape, form), (_, proofs) in calls.items():
        t = ev_ms[(shape, form)]
        print(json.dumps({"row": "block_proof", "shape": shape, "form": form, "proofs_made": proofs, "clock": "events", "ms_median": round(statistics.median(t), 3),
                          "ms_min": round(min(t), 3), "ms_max": round(max(t), 3), "host_ms_median": round(statistics.median(host_ms[(shape, form)]), 3),
                          "reps": len(t)}), flush=True)
    for e in keep:
        e.close()
    ctx.close()


if __name__ == "__main__":
    main()
