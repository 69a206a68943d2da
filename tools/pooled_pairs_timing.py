#!/usr/bin/env python3
"""From proofs to the blob: frieda_reconstruct_from_proofs (queried positions, pooled through a host map) against
frieda_reconstruct_from_proof_pairs (queried positions and their first-layer siblings, pooled on the device).

    python tools/pooled_pairs_timing.py --log 15 [--log 20] [--reps 5] >> profiles/r10_verify_pairs.txt

Per size three rows, wall time of the whole call (verify, pool, reconstruct, commit check; the call ends in a stream synchronise):
  queried   reconstruct_from_proofs on the smallest prefix of the proof list that holds 2^L + 2 distinct queried positions
  pairs     reconstruct_from_proof_pairs on the smallest prefix that holds 2^L + 2 distinct pair points (about half as many proofs)
  same      both calls on the longer of the two lists: device pooling against the host map, at an equal number of proofs
Both calls are warmed up first (the first call at a size builds the twiddles of the product tree), then alternated `reps` times; the
row gives the median and the spread.  The proofs are made by prove_seeds (20 queries, blowup 2^4) and are not part of the timing.
L 15 is the reference's 128 KiB fixture (tests/golden/blob), L 20 a 15 MiB blob of the bench generator.  One JSON line per row."""
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


def blob_for(log_coef):
    if log_coef == 15:
        with open(os.path.join(ROOT, "tests", "golden", "blob"), "rb") as f:
            return f.read()
    from conftest import splitmix64_bytes

    return splitmix64_bytes(7, (4 << log_coef) * 30 // 8).tobytes()


def prefix_needed(rows, need):
    """smallest number of leading rows whose union holds `need` distinct values (None: the list is too short)"""
    owner = np.concatenate([np.full(len(r), i, dtype=np.int64) for i, r in enumerate(rows)])
    _, first = np.unique(np.concatenate(rows), return_index=True)
    if len(first) < need:
        return None
    return int(np.sort(owner[first])[need - 1]) + 1


def timed(call, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", type=int, action="append", help="log2 of the coefficients per column (15 and 20 are the sizes of the record)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=128, help="seeds per prove_seeds call")
    args = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "this tool measures on the GPU: there is no CPU figure"
    import frieda_amd

    ctx = frieda_amd.Context(0)
    cfg = frieda_amd.PcsConfig(frieda_amd.FriConfig(4, 0, 20), 0)
    for L in args.log or [15]:
        data = blob_for(L)
        need = (1 << L) + 2
        enc = ctx.encode(data, 4)
        root = enc.commitment
        proofs, seeds, queried, points = [], [], [], []
        n_q = n_p = None
        while n_q is None:
            new = list(range(len(seeds) + 1, len(seeds) + 1 + args.chunk))
            ps = ctx.prove_seeds(enc, new, cfg)
            st, pts = ctx.verify_pairs_many(ps, new, root)
            _, pos = ctx.verify_samples_many(ps, new, root)
            assert set(st) == {1}
            proofs += ps
            seeds += new
            queried += pos
            points += [p[0] for p in pts]
            if len(seeds) * 20 >= need:
                n_q = prefix_needed(queried, need)
        n_p = prefix_needed(points, need)
        enc.close()
        n_same = max(n_q, n_p)
        calls = {
            "queried": (lambda: ctx.reconstruct_from_proofs(proofs[:n_q], seeds[:n_q], root, len(data)), n_q),
            "pairs": (lambda: ctx.reconstruct_from_proof_pairs(proofs[:n_p], seeds[:n_p], root, len(data)), n_p),
            "same/queried": (lambda: ctx.reconstruct_from_proofs(proofs[:n_same], seeds[:n_same], root, len(data)), n_same),
            "same/pairs": (lambda: ctx.reconstruct_from_proof_pairs(proofs[:n_same], seeds[:n_same], root, len(data)), n_same),
        }
        for name, (call, _) in calls.items():  # warm-up, and the result itself
            for _ in range(2):
                out, _, n = call()
                assert out == data and n >= need, name
        times = {name: [] for name in calls}
        for _ in range(args.reps):  # alternated: other work shares the host
            for name, (call, _) in calls.items():
                times[name] += timed(call, 1)
        for name, (_, n_proofs) in calls.items():
            t = times[name]
            print(json.dumps({"log_coef": L, "row": name, "proofs": n_proofs, "points_needed": need, "ms_median": round(statistics.median(t), 2),
                              "ms_min": round(min(t), 2), "ms_max": round(max(t), 2), "reps": len(t)}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
