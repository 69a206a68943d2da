"""CPU: the host side of cell bundles under sanitizers, as stand-alone programs (each has its own main; nothing is loaded into the
interpreter).  Bundles come from untrusted peers, so the malformed rule, the witness count and the host verifier (bundles_host.h) run
under AddressSanitizer + UBSan over thousands of mutated images of one valid call; the pass planner (bundles_pass.h) runs under UBSan
against its formulas written out again."""
import os
import struct
import subprocess

import numpy as np
import pytest

import bundles_util as B
import cells_util as U
from conftest import ROOT

CSRC = os.path.join(ROOT, "frieda_amd", "csrc")


def _build(tmp_path, name, sanitize):
    exe = tmp_path / name
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=" + sanitize, "-fno-sanitize-recover=undefined", "-I" + CSRC,
           os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        # only a missing sanitizer runtime is a reason to skip; a header that no longer compiles with a plain C++ compiler is a failure
        if "asan" in r.stderr.lower() and ("cannot find" in r.stderr or "No such file" in r.stderr):
            pytest.skip("host sanitizer runtime unavailable: " + r.stderr[-400:])
        pytest.fail("host sanitizer build failed: " + r.stderr[-1500:])
    return str(exe)


def _image(call):
    idx = np.concatenate(call.bundles).astype("<u4")
    head = struct.pack("<4IQ", call.n, call.c, len(call.bundles), len(idx), int(call.wfirst[-1]))
    return b"".join([head, call.commitment, call.first.astype("<u4").tobytes(), call.wfirst.astype("<u8").tobytes(), idx.tobytes(),
                     np.ascontiguousarray(call.values, dtype="<u4").tobytes(), np.ascontiguousarray(call.witness, dtype=np.uint8).tobytes()])


@pytest.mark.parametrize("n,b,c", [(5, 1, 0), (11, 4, 3), (12, 4, 0)])
def test_host_verifier_under_asan_accepts_no_mutant(tmp_path, n, b, c):
    exe = _build(tmp_path, "fuzz_bundles", "address,undefined")
    _, ev, layers, _, _ = U.case(n, b)
    total = 1 << (n - c)
    call = B.build_call(ev, layers, c, [B.pick(n, c, min(k, total), seed=60 + j) for j, k in enumerate((5, 1, 17, 2))])
    img = tmp_path / "call.bin"
    img.write_bytes(_image(call))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe, str(img), "4000"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    assert "mutants 4000" in r.stdout and "accepted_mutants 0" in r.stdout


def test_bundles_pass_planner_matches_the_written_out_formulas(tmp_path):
    """bundles_pass.h under UBSan: what a bundle stages, the greedy cut (log_cell 0 .. 10, witness lengths of depth 0 .. 24, bundles of
    1 .. 1024 cells, budgets of one byte, exactly one bundle, one byte less, the whole call and one byte less, the default), 256-byte
    rounding, the order of the staged image, and whole calls walked pass by pass: the passes partition the bundles, no bundle straddles a
    pass, every pass fits the one plan of the call."""
    exe = _build(tmp_path, "test_bundles_pass", "undefined")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr
