#!/usr/bin/env python3
"""The two launch shapes of the proof verifier against each other and against the host verifier:

    python tools/verify_split_timing.py [--reps 21] > profiles/r23_verify_split.txt

Per row, in the same run and alternated:
  one-kernel   frieda_verify_many with FRIEDA_VERIFY_SPLIT_MAX = 0: one wave per proof (verify.hip)
  split        the same call with FRIEDA_VERIFY_SPLIT_MAX = 2^31: a wave per proof for the value chain, then a wave per (proof, layer)
               for the Merkle walks (verify_split.hip)
  host         the loop of frieda_verify over the same proofs on one host core
Blobs: a 1 KiB blob (a 2^11 codeword, 7 layers) and the reference's 128 KiB fixture (tests/golden/blob: a 2^19 codeword, 15 layers), both at
blowup 2^4, 20 queries, 20 bits of proof of work.  Proof counts 1, 16, 64, 256, 1024, 4096: 1024 distinct proofs per blob (prove_seeds,
seeds 1 .. 1024), the list of 4096 is those four times over (a proof's slot of the staged image is its own either way).
One further row: frieda_reconstruct_from_proof_pairs on the first 846 proofs of the fixture (profiles/r10_verify_pairs.txt), both shapes.

Every device row is warmed twice, then the rows of a count are alternated `reps` times; a device row gives the median and the spread
(min, max) of the HIP-event time on the context's stream around the C call (handle and seed arrays built beforehand; the call packs, uploads,
launches, downloads and synchronises), the host clock beside it.  The host row is the host clock, `reps` times up to 256 proofs and 5 times
above.  The times are records, not gates.  One JSON line per row."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COUNTS = (1, 16, 64, 256, 1024, 4096)
DISTINCT = 1024


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--counts", type=int, nargs="*", default=list(COUNTS))
    args = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "this tool measures on the GPU: there is no CPU figure"
    import frieda_amd

    with open(os.path.join(ROOT, "tests", "golden", "blob"), "rb") as f:
        fixture = f.read()
    blobs = {"1KiB": bytes(i % 256 for i in range(1024)), "128KiB": fixture}
    cfg = frieda_amd.PcsConfig(frieda_amd.FriConfig(4, 0, 20), 20)
    L = frieda_amd._lib.lib()

    ctxs, streams = {}, {}
    for route, split_max in (("one-kernel", 0), ("split", 1 << 31)):
        streams[route] = torch.cuda.Stream()
        ctxs[route] = frieda_amd.Context(0, streams[route].cuda_stream)
        ctxs[route].set_option("FRIEDA_VERIFY_DEVICE_MIN", 0)
        ctxs[route].set_option("FRIEDA_VERIFY_SPLIT_MAX", split_max)
    maker = frieda_amd.Context(0)

    def timed(route, call):
        s = streams[route]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        t0 = time.perf_counter()
        call()
        host = (time.perf_counter() - t0) * 1e3
        e1.record(s)
        e1.synchronize()
        return e0.elapsed_time(e1), host

    def emit(row, ev, host, **kw):
        t = ev if ev else host
        print(json.dumps(dict(kw, row=row, clock="events" if ev else "host", ms_median=round(statistics.median(t), 4), ms_min=round(min(t), 4),
                              ms_max=round(max(t), 4), host_ms_median=round(statistics.median(host), 4), reps=len(t))), flush=True)

    for blob_name, data in blobs.items():
        seeds, proofs, root = list(range(1, DISTINCT + 1)), [], None
        for at in range(0, DISTINCT, 256):
            root, ps = maker.commit_and_generate_proofs_for_seeds(data, seeds[at:at + 256], cfg)
            proofs += ps
        for count in args.counts:
            idx = [i % DISTINCT for i in range(count)]
            arr = (C.c_void_p * count)(*[proofs[i]._h.value if isinstance(proofs[i]._h, C.c_void_p) else proofs[i]._h for i in idx])
            sd = (C.c_uint64 * count)(*[seeds[i] for i in idx])
            com = (C.c_uint8 * 32)(*root)
            status = {r: np.zeros(count, dtype=np.uint8) for r in ctxs}

            def device(route):
                rc = L.frieda_verify_many(ctxs[route]._h, arr, sd, count, com, status[route].ctypes.data)
                assert rc == 0 and (status[route] == 1).all(), (route, rc)

            def host():
                for i in idx:
                    assert frieda_amd.verify(proofs[i], seeds[i])

            for route in ctxs:
                for _ in range(2):
                    device(route)
            ev = {r: [] for r in ctxs}
            hm = {r: [] for r in list(ctxs) + ["host"]}
            host_reps = args.reps if count <= 256 else min(args.reps, 5)
            for rep in range(args.reps):
                for route in ctxs:
                    e, h = timed(route, lambda: device(route))
                    ev[route].append(e)
                    hm[route].append(h)
                if rep < host_reps:
                    t0 = time.perf_counter()
                    host()
                    hm["host"].append((time.perf_counter() - t0) * 1e3)
            for route in ctxs:
                emit("verify_many", ev[route], hm[route], blob=blob_name, proofs=count, route=route)
            emit("verify_many", None, hm["host"], blob=blob_name, proofs=count, route="host")
        if blob_name == "128KiB":
            n = 846
            out = {}

            def rebuild(route):
                out[route] = ctxs[route].reconstruct_from_proof_pairs(proofs[:n], seeds[:n], root, len(data))

            for route in ctxs:
                for _ in range(2):
                    rebuild(route)
                assert out[route][0] == data
            ev = {r: [] for r in ctxs}
            hm = {r: [] for r in ctxs}
            for _ in range(args.reps):
                for route in ctxs:
                    e, h = timed(route, lambda: rebuild(route))
                    ev[route].append(e)
                    hm[route].append(h)
            for route in ctxs:
                emit("reconstruct_from_proof_pairs", ev[route], hm[route], blob=blob_name, proofs=n, route=route, points=int(out[route][2]))
    for c in list(ctxs.values()) + [maker]:
        c.close()


if __name__ == "__main__":
    main()
