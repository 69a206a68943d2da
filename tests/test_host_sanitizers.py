"""CPU: the proof parser + verifier (host-only product code) under AddressSanitizer / UBSan, fed with thousands of mutated
wire images.  GPU sanitizers are unavailable on the pool, so the memory-safety check of the untrusted-input surface
(frieda_proof_deserialize, frieda_verify) runs here on the CPU build of the same sources."""
import os
import subprocess

import pytest

from conftest import ROOT, pattern_bytes

CSRC = os.path.join(ROOT, "frieda_amd", "csrc")
HOST_SOURCES = ["proof.cpp", "verifier.cpp", "transcript.cpp", "context.cpp", "capi_host_stub.cpp"]


@pytest.fixture(scope="module")
def fuzz_binary(tmp_path_factory):
    out = tmp_path_factory.mktemp("asan")
    stub = out / "capi_host_stub.cpp"
    # the slice of the C ABI the fuzzer needs, without the device-side entry points (which need hipcc)
    stub.write_text(
        '#include <string.h>\n#include <new>\n#include "host.h"\nusing namespace frieda;\n'
        'namespace frieda { namespace k { void gen_twiddles(const Launch&, uint32_t, const TwiddleSeeds&, uint32_t*, uint32_t*, void*) {} } '
        "void ProveJobDeleter::operator()(ProveJob*) const {} }\n"
        'extern "C" {\n'
        "int frieda_proof_deserialize(const uint8_t* buf, size_t len, frieda_proof** out) { if (!buf || !out) return 1; *out = nullptr; "
        "frieda_proof* p = new frieda_proof(); if (!deserialize_proof(buf, len, p->p)) { delete p; return 5; } *out = p; return 0; }\n"
        "int frieda_verify(const frieda_proof* p, const uint64_t* seed, int* ok) { try { return verify(p->p, seed, ok); } catch (...) { return 3; } }\n"
        "void frieda_proof_free(frieda_proof* p) { delete p; }\n}\n"
    )
    exe = out / "fuzz_verify"
    srcs = [os.path.join(CSRC, s) for s in HOST_SOURCES[:-1]] + [str(stub), os.path.join(ROOT, "tests", "cpp", "fuzz_verify.cpp")]
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__",
           "-I/opt/rocm/include", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), "-Wno-unused-parameter", *srcs, "-o", str(exe),
           "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        # only a missing sanitizer runtime is a reason to skip; a source that no longer builds or links on the host is a failure
        # (round 5: a new cross-file reference in context.cpp silently turned this test into a skip)
        if "asan" in r.stderr.lower() and ("cannot find" in r.stderr or "No such file" in r.stderr):
            pytest.skip("host sanitizer runtime unavailable: " + r.stderr[-400:])
        pytest.fail("host sanitizer build failed: " + r.stderr[-1500:])
    return str(exe)


@pytest.mark.parametrize("case", ["pattern", "blob"])
def test_parser_and_verifier_under_asan(fuzz_binary, oracle, blob, tmp_path, case):
    if case == "pattern":
        data, seed, cfg = pattern_bytes(1024).tobytes(), 1024, oracle.make_config(12, 4, 0, 20)
    else:
        data, seed, cfg = blob, None, oracle.make_config(12, 4, 1, 20)
    _, proof = oracle.commit_and_generate_proof(data, seed, cfg)
    img = tmp_path / "proof.bin"
    img.write_bytes(proof.serialize())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([fuzz_binary, str(img), "-" if seed is None else str(seed), "3000"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    assert "accepted_mutants 0" in r.stdout


def _run_host_program(tmp_path, name):
    """tests/cpp/<name>.cpp: a stand-alone host program over the product's headers, built with UBSan; it prints OK"""
    exe = tmp_path / name
    cmd = ["g++", "-std=c++17", "-O2", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-I" + CSRC,
           os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-800:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr


def test_lazy_field_arithmetic_matches_textbook(tmp_path):
    """field.h's lazily reduced fold (one 64-bit accumulator per coordinate) equals the textbook QM31 sequence, under UBSan,
    including the operands that attain the accumulator bound."""
    _run_host_program(tmp_path, "test_field")


def test_channel_streamed_mix_and_draws(tmp_path):
    """channel.h under UBSan: the streamed Channel::mix_felts equals blake2s256 over the zero-padded buffer digest || words for
    0 .. 9, 14 .. 17 and 2048 felts (2 and 6 felts end exactly on a block boundary), draw_block(k) is the draw of a channel whose
    n_sent is k, and mix_u64 / draw_felt on a fixed digest give the recorded words."""
    _run_host_program(tmp_path, "test_channel")


def test_unit_pipeline_order_and_retry(tmp_path):
    """unit_pipeline.h under UBSan, with recording fakes: the whole trace of uploads, begins, finishes and abandons of a pass (one
    to four units, with and without the upload ring, each call failing in turn, abort set: the first error is the status, a begun
    unit is abandoned, `done` ends behind the last finished unit), and the retry of a pass that ran out of device memory (17 cuts
    at most, each from the first blob not done; none for single blobs, another error or an aborted call)."""
    _run_host_program(tmp_path, "test_unit_pipeline")


def test_cells_pass_planner_matches_the_written_out_formulas(tmp_path):
    """cells_pass.h under UBSan against the verifier's formulas restated in the test: cells per pass for one commitment, many blobs and
    stripes (log_cell 0 .. 10, depth 0 .. 12, 1 / 63 / 64 / 65 / 300 cells, groups of 1, 3 and 256, budgets of one byte, exactly k cells,
    one byte less and the default), 256-byte rounding, the order of the staged image, and whole calls walked pass by pass: the passes
    partition the cells, no stripe straddles a pass, every later pass fits the plan of the first."""
    _run_host_program(tmp_path, "test_cells_pass")
