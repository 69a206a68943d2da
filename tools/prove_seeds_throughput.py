#!/usr/bin/env python3
"""Throughput of a provider that proves ONE blob under S client seeds: the batch path over S device copies of the blob (what the
library offered before frieda_prove_seeds) against encode-once + prove_seeds, route A (FRIEDA_SEEDS_FOLD_GROUP=0) and route B (the
seed-looped first fold).  One process, arms alternated round by round, every shape warmed, two calls in flight in every arm, the clock
stopped after the last finish (which synchronises); one encode per S is inside the seeds arms' time.

    python tools/prove_seeds_throughput.py [--logs 24,22,20] [--seeds 2,15,60] [--rounds 5] [--group 5] [--window-ms 300]
    python tools/prove_seeds_throughput.py --single 24 15 0      # warm + one prove_seeds call (for a kernel trace): log, S, group

Prints ms per proof as min / median / max per arm and the baseline's round-to-round spread (max - min)."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import frieda_amd  # noqa: E402
from frieda_amd.api import _check  # noqa: E402

CFG = frieda_amd.PcsConfig(frieda_amd.FriConfig(4, 0, 20), 20)


def blob_len_for(log_domain, log_blowup=4):
    """bytes whose 30-bit felts exactly fill 4 columns of a 2^log_domain domain at this blow-up"""
    return (4 << (log_domain - log_blowup)) * 30 // 8


class DevBuf:
    def __init__(self, ctx, arr):
        import ctypes as C

        self.ctx, self.ptr = ctx, C.c_void_p()
        _check(ctx._L.frieda_dev_alloc(ctx._h, max(arr.nbytes, 1), C.byref(self.ptr)), ctx._h)
        _check(ctx._L.frieda_dev_upload(ctx._h, self.ptr, arr.ctypes.data, arr.nbytes), ctx._h)

    def free(self):
        if self.ptr:
            self.ctx._L.frieda_dev_free(self.ctx._h, self.ptr)
            self.ptr = None


def seeds_of(rep, s):
    return [1 + 1000003 * rep + i for i in range(s)]


class Arms:
    def __init__(self, log_domain, s):
        self.s = s
        self.length = blob_len_for(log_domain)
        self.ctxs = [frieda_amd.Context(0), frieda_amd.Context(0)]
        self.enc_ctx = frieda_amd.Context(0)  # encodes while the other two have jobs in flight
        rng = np.random.default_rng(log_domain)
        blob = rng.integers(0, 256, self.length, dtype=np.uint8)
        self.d_one = DevBuf(self.enc_ctx, blob)
        self.stride = (self.length + 255) & ~255
        copies = np.zeros(self.stride * s, dtype=np.uint8)
        for i in range(s):
            copies[i * self.stride : i * self.stride + self.length] = blob
        self.d_copies = DevBuf(self.enc_ctx, copies)
        self.plan = frieda_amd.batch_plan(self.length, s, CFG, in_flight=2, ctx=self.ctxs[0])

    def close(self):
        self.d_one.free()
        self.d_copies.free()
        for c in self.ctxs + [self.enc_ctx]:
            c.close()

    def baseline(self, reps):
        """S proofs of the same blob through the batch path over S device copies, cut by frieda_batch_plan, two calls in flight"""
        pending = [None, None]
        turn = 0
        n = 0
        for rep in range(reps):
            seeds = seeds_of(rep, self.s)
            first = 0
            for cnt in self.plan:
                c = self.ctxs[turn]
                if pending[turn] is not None:
                    n += len(c.prove_batch_finish(pending[turn]))
                c.prove_batch_begin_device(self.d_copies.ptr.value + first * self.stride, self.stride, self.length, cnt, seeds[first : first + cnt], CFG)
                pending[turn] = cnt
                first += cnt
                turn ^= 1
        for t in (turn, turn ^ 1):
            if pending[t] is not None:
                n += len(self.ctxs[t].prove_batch_finish(pending[t]))
        return n

    def seeds_route(self, reps, group):
        """encode once per S, then the S seeds as two prove_seeds calls (one per context), two calls in flight"""
        for c in self.ctxs:
            c.set_option("FRIEDA_SEEDS_FOLD_GROUP", group)
        busy = [False, False]
        stale = []  # handles whose calls may still be in flight: closed once both contexts have moved on
        n = 0
        half = (self.s + 1) // 2
        for rep in range(reps):
            seeds = seeds_of(rep, self.s)
            enc = self.enc_ctx.encode_device(self.d_one.ptr, self.length, 4)
            parts = [seeds[:half], seeds[half:]] if self.s > 1 else [seeds]
            for t, part in enumerate(parts):
                c = self.ctxs[t]
                if busy[t]:
                    n += len(c.prove_seeds_finish())
                c.prove_seeds_begin(enc, part, CFG)
                busy[t] = True
            for old in stale[:-1]:  # every call on a handle two repetitions back has been finished above
                old.close()
            stale = stale[-1:] + [enc]
        for t in (0, 1):
            if busy[t]:
                n += len(self.ctxs[t].prove_seeds_finish())
        for old in stale:
            old.close()
        return n


def timed(fn, reps):
    t0 = time.perf_counter()
    n = fn(reps)
    return (time.perf_counter() - t0) * 1e3 / n


def measure(log_domain, s, group, rounds, window_ms):
    a = Arms(log_domain, s)
    try:
        arms = [("baseline", lambda r: a.baseline(r)), ("route A", lambda r: a.seeds_route(r, 0)), (f"route B g={group}", lambda r: a.seeds_route(r, group))]
        reps = {}
        for name, fn in arms:  # warm every shape, then size the window from a second pass
            fn(1)
            per = timed(fn, 2)
            reps[name] = max(2, int(window_ms / (per * s)) + 1)
        res = {name: [] for name, _ in arms}
        for _ in range(rounds):
            for name, fn in arms:
                res[name].append(timed(fn, reps[name]))
        print(f"2^{log_domain} domain, S = {s}, baseline plan {a.plan}")
        for name, _ in arms:
            v = res[name]
            print(f"  {name:<14} ms/proof  min {min(v):.4f}  median {statistics.median(v):.4f}  max {max(v):.4f}   ({reps[name]} x {s} proofs per window)")
        b = res["baseline"]
        print(f"  baseline spread (max - min over {rounds} rounds): {max(b) - min(b):.4f} ms")
        sys.stdout.flush()
        return res
    finally:
        a.close()


def single(log_domain, s, group):
    a = Arms(log_domain, s)
    try:
        a.seeds_route(2, group)
        a.enc_ctx.synchronize()
        a.seeds_route(1, group)
    finally:
        a.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", default="24,22,20")
    ap.add_argument("--seeds", default="2,15,60")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--group", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--single", nargs=3, type=int, metavar=("LOG", "S", "GROUP"))
    args = ap.parse_args()
    if args.single:
        single(*args.single)
        return
    for lg in [int(x) for x in args.logs.split(",")]:
        for s in [int(x) for x in args.seeds.split(",")]:
            measure(lg, s, min(args.group, s), args.rounds, args.window_ms)


if __name__ == "__main__":
    main()
