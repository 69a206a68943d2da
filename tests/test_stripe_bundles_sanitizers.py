"""CPU: the host side of stripe bundles under sanitizers, as stand-alone programs (each has its own main, built with g++; nothing is
loaded into the interpreter).  Stripe bundles come from untrusted peers, so the argument rule, the once-per-bundle malformed rule and the
host verifier run per blob piece (bundles_host.h) run under AddressSanitizer + UBSan over 4000 mutated images of one valid 3-blob call;
the pass planner with its blob count (bundles_pass.h) runs under UBSan against its formulas written out again."""
import os
import struct
import subprocess

import numpy as np

import bundles_util as B
import stripe_bundles_util as S
import test_cells_blobs_host as H
from test_bundles_sanitizers import _build


def _image(call):
    idx = np.concatenate(call.bundles).astype("<u4")
    head = struct.pack("<5IQ", call.n, call.c, len(call.bundles), len(idx), call.k, int(call.wfirst[-1]))
    return b"".join([head, b"".join(call.commitments), call.first.astype("<u4").tobytes(), call.wfirst.astype("<u8").tobytes(), idx.tobytes(),
                     np.ascontiguousarray(call.values, dtype="<u4").tobytes(), np.ascontiguousarray(call.witness, dtype=np.uint8).tobytes()])


def test_host_verifier_under_asan_accepts_no_mutant(tmp_path):
    exe = _build(tmp_path, "fuzz_stripe_bundles", "address,undefined")
    n, b, c, k = 11, 4, 3, 3
    total = 1 << (n - c)
    call = S.build(H.block(n, b, k=k), c, [B.pick(n, c, min(s, total), seed=60 + j) for j, s in enumerate((5, 1, 17, 2))])
    img = tmp_path / "call.bin"
    img.write_bytes(_image(call))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe, str(img), "4000"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    assert "mutants 4000" in r.stdout and "accepted_mutants 0" in r.stdout


def test_pass_planner_with_blob_counts_matches_the_written_out_formulas(tmp_path):
    """bundles_pass.h under UBSan with blob counts 1, 3, 16 and 256: what a bundle stages (indices once, values and witness per blob), the
    greedy cut, 256-byte rounding, the order of the staged image, whole calls walked pass by pass, and the factor 1 reproducing the plan
    without a factor field by field."""
    exe = _build(tmp_path, "test_stripe_bundles_pass", "undefined")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr
