"""CPU: the HIP-free halves of the encoded-block handles as stand-alone host programs under AddressSanitizer + UBSan (each has its own
main; nothing is loaded into the interpreter).
  tests/cpp/test_blob_image.cpp     the blob-image rule of blob_image.h — the bounds the kernel blob_image_check shares — for every blob
                                    length 0 .. 600 and {1023, 1024, 1025, 3839, 3840, 3841, 65536}: the unpack of random bytes passes,
                                    every single mutation of one word into a forbidden region fails, pack(unpack(bytes)) == bytes.
  tests/cpp/test_encoded_slab.cpp   the reference-counted owner of encoded_slab.h with a counting free injected: K handles freed in every
                                    order for K <= 4 and in a random order for K = 64, the free exactly once and after the last handle,
                                    two threads freeing disjoint halves."""
import os
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "frieda_amd", "csrc")


def _build(tmp_path, name, sanitize):
    exe = tmp_path / (name + "_" + sanitize.replace(",", "_"))
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=" + sanitize, "-fno-sanitize-recover=undefined", "-I" + CSRC,
           os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        # only a missing sanitizer runtime is a reason to skip; a header that no longer compiles with a plain C++ compiler is a failure
        if ("libasan" in r.stderr or "libubsan" in r.stderr) and ("cannot find" in r.stderr or "No such file" in r.stderr):
            pytest.skip("host sanitizer runtime unavailable: " + r.stderr[-400:])
        pytest.fail("host sanitizer build failed: " + r.stderr[-1500:])
    return str(exe)


def _run(exe):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), (r.stdout + r.stderr)[-2000:]


def test_blob_image_rule_under_asan(tmp_path):
    _run(_build(tmp_path, "test_blob_image", "address,undefined"))


def test_encoded_slab_owner_under_asan(tmp_path):
    _run(_build(tmp_path, "test_encoded_slab", "address,undefined"))
