"""CPU: the HIP-free arithmetic of a verify pass (frieda_amd/csrc/verify_pass.h) as a stand-alone host program under AddressSanitizer +
UBSan (its own main; nothing is loaded into the interpreter), built as tests/test_encoded_host.py builds its programs.
  tests/cpp/test_verify_pass.cpp   the cut of a call into passes and of a split pass by its scratch against the formulas written out again
                                   (a lone oversized proof, 1024 queries x 40 layers, mixed layer counts, a cap hit exactly, random lists);
                                   the status rule of the split route over every (first chain event, set of failing walk layers) of a
                                   4-layer proof and of a proof without inner layers, against the sequential order as a plain loop."""
from test_encoded_host import _build, _run


def test_verify_pass_under_asan(tmp_path):
    _run(_build(tmp_path, "test_verify_pass", "address,undefined"))
