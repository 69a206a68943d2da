"""GPU: the C++ wrappers of include/frieda.hpp for encoded handles of a block and from a rebuild (Context::encode_batch and the four
Context::rebuild_encoded_*), run as the stand-alone program tests/cpp/test_api_encoded.cpp that build() compiles."""
import os
import subprocess

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_cpp_wrappers_of_the_encoded_block_calls(gpu_ctx):
    exe = os.path.join(ROOT, "tests", "cpp", "test_api_encoded.bin")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
