"""Proofs per second of frieda_verify_many (device, upload included) against a plain loop of frieda_verify on one core of the same
machine, over proofs made by frieda_prove_seeds: 2^24 and 2^20 domains and a 1 KiB blob, 20 queries, blowup 2^4, 20-bit proof of work,
256 and 4096 proofs per call; and frieda_reconstruct_from_proofs end to end for the 128 KiB tests/golden/blob.

    python tools/verify_throughput.py            # every step, each a child process under its own time limit; stops at the first failure
    python tools/verify_throughput.py --step d24  # one step in this process: d24, d20, kib, reconstruct

One JSON line per measurement.  The output of a run on an MI355X belongs in profiles/r09_verify_many.txt (its section 3).
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

STEPS = {"d24": 300, "d20": 240, "kib": 240, "reconstruct": 240}  # step -> time limit, seconds
DISTINCT = 256  # distinct proofs per shape; a 4096-proof call repeats them (the verifier keeps nothing between proofs)


def _cfg(frieda_amd, nq=20, pow_bits=20):
    return frieda_amd.PcsConfig(frieda_amd.FriConfig(4, 0, nq), pow_bits)


def measure(name, nbytes):
    import numpy as np
    import torch  # noqa: F401  (loads the HIP runtime first, see frieda_amd/_lib.py)

    import frieda_amd
    from conftest import splitmix64_bytes

    ctx = frieda_amd.Context(0)
    data = splitmix64_bytes(24, nbytes).tobytes()
    seeds = list(range(1, DISTINCT + 1))
    enc = ctx.encode(data, 4)
    proofs = []
    for i in range(0, DISTINCT, 32):
        proofs += ctx.prove_seeds(enc, seeds[i : i + 32], _cfg(frieda_amd))
    enc.close()
    ctx.release_workspace()
    proof_bytes = len(proofs[0].serialize())
    # the host loop: one core, frieda_verify per proof
    t0 = time.perf_counter()
    ok = [frieda_amd.verify(p, s) for p, s in zip(proofs, seeds)]
    host_s = (time.perf_counter() - t0) / DISTINCT
    assert all(ok)
    for count in (256, 4096):
        reps = count // DISTINCT
        ps, sd = proofs * reps, seeds * reps
        st = ctx.verify_many(ps, sd)  # first call: staging block and workspace are allocated
        assert set(st.tolist()) == {1}
        best = 1e9
        for _ in range(5):
            t0 = time.perf_counter()
            ctx.verify_many(ps, sd)
            best = min(best, time.perf_counter() - t0)
        print(json.dumps({
            "shape": name, "log_domain": proofs[0].log_size_bound + 4, "proof_bytes": proof_bytes, "proofs_per_call": count,
            "host_loop_ms_per_proof": round(host_s * 1e3, 4), "host_proofs_per_s": round(1 / host_s, 1),
            "device_call_ms": round(best * 1e3, 3), "device_us_per_proof": round(best / count * 1e6, 3),
            "device_proofs_per_s": round(count / best, 1), "ratio_device_over_host": round(host_s * count / best, 1),
        }), flush=True)
    # the smallest count at which the device route is not slower than the host loop
    for count in (1, 2, 4, 8, 16):
        ctx.verify_many(proofs[:count], seeds[:count])
        best = 1e9
        for _ in range(10):
            t0 = time.perf_counter()
            ctx.verify_many(proofs[:count], seeds[:count])
            best = min(best, time.perf_counter() - t0)
        print(json.dumps({"shape": name, "proofs_per_call": count, "device_call_ms": round(best * 1e3, 4), "host_loop_ms": round(host_s * count * 1e3, 4)}), flush=True)
    ctx.close()


def reconstruct():
    import torch  # noqa: F401

    import frieda_amd

    with open(os.path.join(ROOT, "tests", "golden", "blob"), "rb") as f:
        blob = f.read()
    ctx = frieda_amd.Context(0)
    cfg = _cfg(frieda_amd, 20, 0)
    # 2^15 coefficients per column on a 2^19 codeword: 2^15 + 2 distinct points, 20 per proof
    n_proofs = 1760
    seeds = list(range(1, n_proofs + 1))
    enc = ctx.encode(blob, 4)
    root = enc.commitment
    proofs = []
    for i in range(0, n_proofs, 32):
        proofs += ctx.prove_seeds(enc, seeds[i : i + 32], cfg)
    enc.close()
    out, st, n = ctx.reconstruct_from_proofs(proofs, seeds, root, len(blob))
    assert out == blob
    best = 1e9
    for _ in range(3):
        t0 = time.perf_counter()
        ctx.reconstruct_from_proofs(proofs, seeds, root, len(blob))
        best = min(best, time.perf_counter() - t0)
    t0 = time.perf_counter()
    for p, s in zip(proofs[:128], seeds[:128]):
        frieda_amd.verify_samples(p, s)
    host_s = (time.perf_counter() - t0) / 128 * n_proofs
    print(json.dumps({"step": "reconstruct_from_proofs", "blob_bytes": len(blob), "proofs": n_proofs, "distinct_points": n, "needed": (1 << 15) + 2,
                      "end_to_end_ms": round(best * 1e3, 2), "host_verify_loop_alone_ms": round(host_s * 1e3, 1)}), flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEPS))
    args = ap.parse_args()
    if args.step is None:
        for step, limit in STEPS.items():
            r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step])
            if r.returncode != 0:
                print(f"step {step} ended with status {r.returncode}: stopping", file=sys.stderr)
                sys.exit(r.returncode)
        return
    if args.step == "d24":
        measure("2^24 domain", (4 << 20) * 30 // 8)
    elif args.step == "d20":
        measure("2^20 domain", (4 << 16) * 30 // 8)
    elif args.step == "kib":
        measure("1 KiB blob", 1024)
    else:
        reconstruct()


if __name__ == "__main__":
    main()
