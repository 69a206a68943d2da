"""A block under many seeds (frieda_prove_seeds_blobs*): the parts that need no GPU — the four entry points are declared with one
argument count in every binding and exported, the ABI version stands, the wrappers exist, no parameter claims device memory by its name,
and the workspace function states what the call asks for."""
import os
import re
import subprocess

import pytest

import frieda_amd
from frieda_amd import _lib

from util import blob_len_for

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> number of arguments
NEW_FUNCTIONS = {
    "frieda_prove_seeds_blobs_begin": 6,
    "frieda_prove_seeds_blobs_finish": 2,
    "frieda_prove_seeds_blobs": 7,
    "frieda_seeds_blobs_workspace_bytes": 4,
}


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def _args(text, pattern):
    m = re.search(pattern + r"\s*\(([^;{]*?)\)\s*(?:->[^;]*)?;", text, re.S)
    assert m, pattern
    return [a.strip() for a in m.group(1).split(",") if a.strip()]


@pytest.mark.parametrize("name", sorted(NEW_FUNCTIONS))
def test_declared_with_one_argument_count_in_every_binding(name):
    n = NEW_FUNCTIONS[name]
    header = re.sub(r"/\*.*?\*/", "", _read("include", "frieda_hip.h"), flags=re.S)
    c_args = _args(header, r"\b(?:int|size_t)\s+" + name)
    assert len(c_args) == n, c_args
    assert name in _lib.declared_symbols(), "not in the ctypes table"
    assert len(getattr(_lib.lib(), name).argtypes) == n
    rs_args = _args(_read("bindings", "rust", "frieda-hip-sys", "src", "lib.rs"), r"pub fn " + name)
    assert len(rs_args) == n, rs_args
    hpp = _read("include", "frieda.hpp")
    assert re.search(r"\b" + name + r"\b", hpp), "not used or named by frieda.hpp"
    # no parameter is named as device memory is (the buffer-contract table classifies d / d_*): handles and host arrays only
    for a in c_args:
        assert not re.search(r"\bd(?:_\w+)?$", a), a


def test_the_cpp_wrapper_passes_every_argument():
    hpp = _read("include", "frieda.hpp")
    m = re.search(r"frieda_prove_seeds_blobs\(([^;]*?)\), h_\);", hpp, re.S)
    assert m, "frieda.hpp does not call frieda_prove_seeds_blobs"
    depth, count = 0, 1
    for ch in m.group(1):
        depth += ch in "(<"
        depth -= ch in ")>"
        count += ch == "," and depth == 0
    assert count == NEW_FUNCTIONS["frieda_prove_seeds_blobs"]


def test_header_places_the_section_and_keeps_the_abi_version():
    h = _read("include", "frieda_hip.h")
    first = min(h.index("int " + n + "(") if n != "frieda_seeds_blobs_workspace_bytes" else h.index("size_t " + n + "(") for n in NEW_FUNCTIONS)
    assert h.rindex("frieda_rebuild_encoded_blobs_from_stripe_bundles(") < first < h.index("size_t frieda_workspace_bytes(")
    assert re.search(r"#define\s+FRIEDA_ABI_VERSION\s+1\b", h)


def test_exported_by_the_built_library():
    so = os.path.join(ROOT, "frieda_amd", "lib", "libfrieda_hip.so")
    out = subprocess.check_output(["nm", "-D", "--defined-only", so], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert not [n for n in NEW_FUNCTIONS if n not in exported]
    L = _lib.lib()
    assert not [n for n in NEW_FUNCTIONS if not hasattr(L, n)]
    assert L.frieda_abi_version() == 1  # additions only


def test_wrappers_exist():
    for name in ("prove_seeds_blobs", "prove_seeds_blobs_begin", "prove_seeds_blobs_finish"):
        assert callable(getattr(frieda_amd.Context, name))
    assert callable(frieda_amd.prove_seeds_blobs) and callable(frieda_amd.seeds_blobs_workspace_bytes)
    assert "prove_seeds_blobs" in frieda_amd.__all__ and "seeds_blobs_workspace_bytes" in frieda_amd.__all__


def test_documents_name_the_call():
    for doc in ("DESIGN.md", "README.md", "INTEGRATION.md"):
        assert "frieda_prove_seeds_blobs" in _read(doc), doc


def _cfg(log_blowup=4, last=0, queries=20, pow_bits=20):
    return frieda_amd.PcsConfig(frieda_amd.FriConfig(log_blowup, last, queries), pow_bits)


@pytest.mark.parametrize("log_domain", [5, 12, 18, 22])
def test_workspace_equals_prove_seeds_for_one_blob_and_grows_with_both_counts(log_domain):
    cfg = _cfg()
    length = blob_len_for(log_domain)
    for s in (1, 2, 5, 64, 65535):
        assert frieda_amd.seeds_blobs_workspace_bytes(length, cfg, 1, s) == frieda_amd.seeds_workspace_bytes(length, cfg, s) > 0
    for s in (1, 3, 8):
        prev = 0
        for k in (1, 2, 3, 4, 16, 64, 1000, 65535 // s):
            ws = frieda_amd.seeds_blobs_workspace_bytes(length, cfg, k, s)
            assert ws > prev, (k, s, ws, prev)
            prev = ws
    for k in (1, 2, 3, 8):
        prev = 0
        for s in (1, 2, 3, 4, 5, 16, 64, 1000, 65535 // k):
            ws = frieda_amd.seeds_blobs_workspace_bytes(length, cfg, k, s)
            assert ws > prev, (k, s, ws, prev)
            prev = ws
            # the jobs' share is the one-blob plan at k * s jobs; what the block adds is its table alone (rows, a row per job, a first job per group)
            assert 0 <= ws - frieda_amd.seeds_workspace_bytes(length, cfg, k * s) <= 32 * k + 8 * k * s + 3 * 256


def test_workspace_refuses_what_the_prover_refuses():
    cfg = _cfg()
    for k, s in ((0, 4), (4, 0), (0, 0), (256, 256), (65535, 2), (2, 65535), (65536, 1), (1, 65536)):
        assert frieda_amd.seeds_blobs_workspace_bytes(4096, cfg, k, s) == 0, (k, s)
    assert frieda_amd.seeds_blobs_workspace_bytes(4096, cfg, 255, 257) > 0  # 65535 jobs
    # every shape seeds_workspace_bytes refuses, at one blob and at several
    for length, bad in ((4096, _cfg(last=11)), (4096, _cfg(queries=0)), (4096, _cfg(queries=4097)), (3, _cfg(last=3)), (4096, _cfg(log_blowup=31)),
                        ((1 << 40) + 1, cfg)):
        assert frieda_amd.seeds_workspace_bytes(length, bad, 4) == 0
        for k in (1, 2, 16):
            assert frieda_amd.seeds_blobs_workspace_bytes(length, bad, k, 4) == 0, (length, k)
