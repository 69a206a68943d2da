#!/usr/bin/env python3
"""A sparse request queue over a block of encoded blobs: ONE frieda_prove_jobs call against what a provider had for that queue before,
in the same run:

    python tools/prove_jobs_timing.py [--reps 21] > profiles/r22_prove_jobs.txt

Configuration: blowup 2^4, 20 queries, 20-bit proof of work; route A (FRIEDA_SEEDS_FOLD_GROUP 0) and the seed-looped kernel with groups of 4.
Blocks: 64 handles of 1 KiB, 16 handles of 128 KiB, 4 handles of a 2^22 domain.
The sparse queue of a block: every client has a seed of its own and names a quarter of the blobs (drawn once, seeded); the number of
clients makes the job count that of the block's row in profiles/r19_prove_seeds_blobs.txt (256, 128, 16 jobs).  The jobs are listed
client by client, i.e. unsorted by blob.

Rows of a block ("form"):
    jobs        one prove_jobs call over the sparse queue
    loop        the loop of prove_seeds, one call per distinct blob with that blob's seeds           (what the parent commit offers, a)
    rectangle   prove_seeds_blobs on the bounding rectangle, every named blob under every client's seed: most proofs are thrown away  (b)
    rect_jobs / rect_blobs   the r19 rectangle itself (K blobs x S seeds) through prove_jobs and through prove_seeds_blobs: the same launches
    jobs_3pass  the sparse queue again under an arena limit that forces three passes (frieda_prove_jobs_plan is printed): the price of a pass
All forms return their proofs as objects, and dropping them is part of the row.  The handles are encoded once, outside every row.

Every row is warmed twice (the first warm-up also checks the bytes of `jobs` against `loop`, `rectangle` and `jobs_3pass`, and of
rect_jobs against rect_blobs), then all rows are alternated `reps` times; a row gives the median and the spread (min, max) of the HIP-event time on the
context's stream (every call ends in a synchronise of that stream) and the host clock beside it.  The garbage collector is off while a
clock runs.  Records, not gates.  One JSON line per row."""
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
    args = ap.parse_args()
    import numpy as np
    import torch

    assert torch.cuda.is_available(), "this tool measures on the GPU: there is no CPU figure"
    import frieda_amd

    B = 4
    pcs = frieda_amd.PcsConfig(frieda_amd.FriConfig(B, 0, 20), 20)
    with open(os.path.join(ROOT, "tests", "golden", "blob"), "rb") as f:
        base = f.read()
    rng = np.random.default_rng(22)
    # (name, blobs, seeds of the r19 rectangle)
    shapes = [
        ("64 x 1 KiB", [bytes((i * 7 + j) % 256 for i in range(1024)) for j in range(64)], 4),
        ("16 x 128 KiB", [base[j:] + base[:j] for j in range(16)], 8),
        (f"4 x 2^{args.large_log_domain} domain", [rng.integers(0, 256, blob_len_for(args.large_log_domain), dtype=np.uint8).tobytes() for _ in range(4)], 4),
    ]
    stream = torch.cuda.Stream()
    ctx = frieda_amd.Context(0, stream.cuda_stream)
    calls, info, handles = {}, {}, []
    for shape, blobs, r19_seeds in shapes:
        encs = ctx.encode_batch(blobs, B)
        handles.extend(encs)
        k, length = len(encs), len(blobs[0])
        quarter = max(1, k // 4)
        n_clients = k * r19_seeds // quarter
        jobs = []
        for c in range(n_clients):
            jobs.extend((int(b), 5000 + 31 * c) for b in rng.choice(k, size=quarter, replace=False))
        named = sorted({b for b, _ in jobs})
        seeds_of = {b: [s for bb, s in jobs if bb == b] for b in named}
        client_seeds = [5000 + 31 * c for c in range(n_clients)]
        rect = [(b, 1000 + 17 * s) for b in range(k) for s in range(r19_seeds)]
        per3 = -(-len(jobs) // 3)
        limit3 = frieda_amd.prove_jobs_workspace_bytes(length, pcs, min(k, per3), per3)
        info[shape] = {"handles": k, "jobs": len(jobs), "clients": n_clients, "blobs_per_client": quarter, "named_blobs": len(named),
                       "most_jobs_on_a_blob": max(len(v) for v in seeds_of.values()), "fewest": min(len(v) for v in seeds_of.values()),
                       "rectangle_proofs": len(named) * n_clients, "length": length}
        for group in (0, 4):
            def run_jobs(encs=encs, jobs=jobs, group=group):
                ctx.set_option("FRIEDA_SEEDS_FOLD_GROUP", group)
                return ctx.prove_jobs(encs, jobs, pcs)

            def run_loop(encs=encs, named=named, seeds_of=seeds_of, group=group):
                ctx.set_option("FRIEDA_SEEDS_FOLD_GROUP", group)
                return {b: ctx.prove_seeds(encs[b], seeds_of[b], pcs) for b in named}

            def run_rectangle(encs=encs, named=named, client_seeds=client_seeds, group=group):
                ctx.set_option("FRIEDA_SEEDS_FOLD_GROUP", group)
                return ctx.prove_seeds_blobs([encs[b] for b in named], client_seeds, pcs)

            def run_rect_jobs(encs=encs, rect=rect, group=group):
                ctx.set_option("FRIEDA_SEEDS_FOLD_GROUP", group)
                return ctx.prove_jobs(encs, rect, pcs)

            def run_rect_blobs(encs=encs, r19_seeds=r19_seeds, group=group):
                ctx.set_option("FRIEDA_SEEDS_FOLD_GROUP", group)
                return [p for row in ctx.prove_seeds_blobs(encs, [1000 + 17 * s for s in range(r19_seeds)], pcs) for p in row]

            def run_3pass(encs=encs, jobs=jobs, group=group, limit3=limit3):
                ctx.set_option("FRIEDA_SEEDS_FOLD_GROUP", group)
                ctx._L.frieda_ctx_test_set_arena_limit(ctx._h, limit3)
                try:
                    return ctx.prove_jobs(encs, jobs, pcs)
                finally:
                    ctx._L.frieda_ctx_test_set_arena_limit(ctx._h, 0)

            for form, call, proofs in (("jobs", run_jobs, len(jobs)), ("loop", run_loop, len(jobs)), ("rectangle", run_rectangle, len(named) * n_clients),
                                       ("rect_jobs", run_rect_jobs, len(rect)), ("rect_blobs", run_rect_blobs, len(rect)), ("jobs_3pass", run_3pass, len(jobs))):
                calls[(shape, group, form)] = (call, proofs)
            # the first warm-up: one set of bytes, whatever the form
            got = [p.serialize() for p in run_jobs()]
            loop = {b: [p.serialize() for p in ps] for b, ps in run_loop().items()}
            taken = {b: 0 for b in named}
            for j, (b, _) in enumerate(jobs):
                assert got[j] == loop[b][taken[b]], (shape, group, j)
                taken[b] += 1
            block = run_rectangle()
            for j, (b, s) in enumerate(jobs):
                assert got[j] == block[named.index(b)][client_seeds.index(s)].serialize(), (shape, group, j)
            del block
            assert [p.serialize() for p in run_3pass()] == got, (shape, group)
            assert [p.serialize() for p in run_rect_jobs()] == [p.serialize() for p in run_rect_blobs()], (shape, group)
        ctx._L.frieda_ctx_test_set_arena_limit(ctx._h, limit3)
        info[shape]["plan_3pass"] = frieda_amd.prove_jobs_plan(length, pcs, k, len(jobs), ctx=ctx)
        ctx._L.frieda_ctx_test_set_arena_limit(ctx._h, 0)
        info[shape]["plan"] = frieda_amd.prove_jobs_plan(length, pcs, k, len(jobs), ctx=ctx)
        print(json.dumps({"row": "queue", "shape": shape, **info[shape]}), flush=True)
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
                proofs = call()
                del proofs
                host_ms[name].append((time.perf_counter() - t0) * 1e3)
                e1.record(stream)
                e1.synchronize()
                ev_ms[name].append(e0.elapsed_time(e1))
    finally:
        gc.enable()
    for (shape, group, form), (_, proofs) in calls.items():
        t = ev_ms[(shape, group, form)]
        med = statistics.median(t)
        wanted = info[shape]["jobs"] if form in ("jobs", "loop", "rectangle", "jobs_3pass") else proofs
        print(json.dumps({"row": "prove_jobs", "shape": shape, "seeds_fold_group": group, "form": form, "proofs_made": proofs, "proofs_wanted": wanted,
                          "clock": "events", "ms_median": round(med, 3), "ms_min": round(min(t), 3), "ms_max": round(max(t), 3),
                          "host_ms_median": round(statistics.median(host_ms[(shape, group, form)]), 3), "wanted_per_s": round(wanted / med * 1e3),
                          "reps": len(t)}), flush=True)
    for e in handles:
        e.close()
    ctx.close()


if __name__ == "__main__":
    main()
