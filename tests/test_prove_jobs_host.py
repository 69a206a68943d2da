"""CPU: the HIP-free arithmetic of a frieda_prove_jobs call (frieda_amd/csrc/prove_jobs_plan.h) as a stand-alone host program under
AddressSanitizer + UBSan (its own main; nothing is loaded into the interpreter), built as tests/test_encoded_host.py builds its programs.
  tests/cpp/test_prove_jobs_plan.cpp   the stable sort by blob and the permutation back, the rows of the distinct blobs, the groups of the
                                       seed-looped fold (sizes 0, 1, 2, 4, 8, 65535), the rectangle's table as frieda_prove_seeds_blobs
                                       staged it, the cut into passes — for hand-made lists (one job, one blob, one job per blob in
                                       descending order, a blob with no job, repeated pairs, 65535 jobs) and random ones."""
from test_encoded_host import _build, _run


def test_prove_jobs_plan_under_asan(tmp_path):
    _run(_build(tmp_path, "test_prove_jobs_plan", "address,undefined"))
