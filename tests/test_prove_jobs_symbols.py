"""Any list of (handle, seed) jobs in one call (frieda_prove_jobs*): the parts that need no GPU — the five entry points are declared with
one argument count in every binding and exported, the ABI version stands, the wrappers exist, no parameter claims device memory by its
name, the workspace function is the rectangle's and prove_seeds' where the list is one, and the pass rule is the written one."""
import ctypes as C
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
    "frieda_prove_jobs_begin": 7,
    "frieda_prove_jobs_finish": 2,
    "frieda_prove_jobs": 8,
    "frieda_prove_jobs_workspace_bytes": 4,
    "frieda_prove_jobs_plan": 7,
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
    m = re.search(r"frieda_prove_jobs\(([^;]*?)\), h_\);", hpp, re.S)
    assert m, "frieda.hpp does not call frieda_prove_jobs"
    depth, count = 0, 1
    for ch in m.group(1):
        depth += ch in "(<"
        depth -= ch in ")>"
        count += ch == "," and depth == 0
    assert count == NEW_FUNCTIONS["frieda_prove_jobs"]


def test_header_places_the_section_and_keeps_the_abi_version():
    h = _read("include", "frieda_hip.h")
    first = min(h.index(("size_t " if n == "frieda_prove_jobs_workspace_bytes" else "int ") + n + "(") for n in NEW_FUNCTIONS)
    # directly behind the frieda_prove_seeds_blobs section
    assert h.index("size_t frieda_seeds_blobs_workspace_bytes(") < first < h.index("size_t frieda_workspace_bytes(")
    between = h[h.index("size_t frieda_seeds_blobs_workspace_bytes("):first]
    assert not re.search(r"^(?:int|size_t|void)\s+frieda_(?!prove_jobs)", between.split("\n", 1)[1], re.M)
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
    for name in ("prove_jobs", "prove_jobs_begin", "prove_jobs_finish"):
        assert callable(getattr(frieda_amd.Context, name))
    for name in ("prove_jobs", "prove_jobs_workspace_bytes", "prove_jobs_plan"):
        assert callable(getattr(frieda_amd, name)) and name in frieda_amd.__all__


def test_documents_name_the_call():
    for doc in ("DESIGN.md", "README.md", "INTEGRATION.md"):
        assert "frieda_prove_jobs" in _read(doc), doc
    design = _read("DESIGN.md")
    for m in re.finditer(r"Not built:[^.]*\.", design):
        assert "pair list" not in m.group(0) and "passes" not in m.group(0), m.group(0)


def _cfg(log_blowup=4, last=0, queries=20, pow_bits=20):
    return frieda_amd.PcsConfig(frieda_amd.FriConfig(log_blowup, last, queries), pow_bits)


@pytest.mark.parametrize("log_domain", [5, 12, 18, 22])
def test_workspace_is_the_rectangles_and_prove_seeds_and_grows_with_both_counts(log_domain):
    cfg = _cfg()
    length = blob_len_for(log_domain)
    ws = frieda_amd.prove_jobs_workspace_bytes
    for n in (1, 2, 5, 64, 65535):
        assert ws(length, cfg, 1, n) == frieda_amd.seeds_workspace_bytes(length, cfg, n) > 0
    for k, s in ((1, 1), (2, 1), (2, 2), (3, 5), (4, 9), (16, 64), (255, 257), (65535, 1), (1000, 65)):
        assert ws(length, cfg, k, k * s) == frieda_amd.seeds_blobs_workspace_bytes(length, cfg, k, s) > 0, (k, s)
    # (more handles than jobs is legal: a handle no job names.)  A row of the table is 32 bytes and every piece of the workspace starts on
    # a 256-byte boundary — the rectangle's layout, which must not move: at a fixed job count the bytes never fall with the handles, and
    # grow strictly from one blob to two (the table appears) and whenever eight more rows are asked for
    for n in (1, 9, 300, 65535):
        prev = 0
        for k in (1, 2, 10, 18, 64, 1000, 65535):
            w = ws(length, cfg, k, n)
            assert w > prev, (k, n, w, prev)
            prev = w
        for k in range(2, 40):
            assert ws(length, cfg, k, n) <= ws(length, cfg, k + 1, n), (k, n)
    for s in (1, 3, 8):  # along the rectangle, as its own test walks it
        prev = 0
        for k in (1, 2, 3, 4, 16, 64, 1000, 65535 // s):
            w = ws(length, cfg, k, k * s)
            assert w > prev, (k, s, w, prev)
            prev = w
    for k in (1, 2, 3, 8, 1000):
        prev = 0
        for n in (1, 2, 3, 4, 5, 16, 64, 1000, 65535):
            w = ws(length, cfg, k, n)
            assert w > prev, (k, n, w, prev)
            prev = w
            # the jobs' share is the one-blob plan; what the block adds is its table alone (rows, a row and at most a group entry per job)
            assert 0 <= w - frieda_amd.seeds_workspace_bytes(length, cfg, n) <= 32 * k + 8 * n + 3 * 256


def test_workspace_refuses_what_the_rectangle_refuses():
    cfg = _cfg()
    ws = frieda_amd.prove_jobs_workspace_bytes
    for k, n in ((0, 4), (4, 0), (0, 0), (1, 65536), (4, 65536), (65536, 65536), (0, 65535), (1, 1 << 31)):
        assert ws(4096, cfg, k, n) == 0, (k, n)
    assert ws(4096, cfg, 255, 65535) > 0 and ws(4096, cfg, 65535, 65535) > 0
    for length, bad in ((4096, _cfg(last=11)), (4096, _cfg(queries=0)), (4096, _cfg(queries=4097)), (3, _cfg(last=3)), (4096, _cfg(log_blowup=31)),
                        ((1 << 40) + 1, cfg)):
        assert frieda_amd.seeds_blobs_workspace_bytes(length, bad, 2, 2) == 0
        for k in (1, 2, 16):
            assert ws(length, bad, k, 16) == 0, (length, k)


def _default_budget():
    # batch_budget_bytes of the default options: sixteen proofs of a 2^24 domain (15 MiB blobs, blow-up 16) in workspace bytes
    return 16 * frieda_amd.workspace_bytes(15 << 20, 4, 0, True)


@pytest.mark.parametrize("log_domain,n_blobs,n_jobs", [(12, 4, 9), (12, 64, 256), (18, 16, 64), (18, 1, 70000), (22, 4, 16), (22, 4, 1000), (24, 8, 100),
                                                      (24, 1, 1), (10, 300, 200000)])
def test_plan_without_a_context_follows_the_written_rule(log_domain, n_blobs, n_jobs):
    cfg = _cfg()
    length = blob_len_for(log_domain)
    limit = _default_budget()
    ws = lambda p: frieda_amd.prove_jobs_workspace_bytes(length, cfg, min(n_blobs, p), p)
    per, passes = frieda_amd.prove_jobs_plan(length, cfg, n_blobs, n_jobs)
    cap = min(n_jobs, 65535)
    assert 1 <= per <= cap
    # the largest p within the limit (the workspace grows with p: p fits, p + 1 does not), or 1
    if ws(1) > limit:
        assert per == 1
    else:
        assert ws(per) <= limit and (per == cap or ws(per + 1) > limit)
        for p in (1, max(1, per // 2), max(1, per - 1)):
            assert ws(p) <= limit
    assert passes == -(-n_jobs // per)


def test_plan_refuses_bad_arguments():
    L = _lib.lib()
    per, n = C.c_uint32(7), C.c_uint32(7)
    cfg = _cfg()._c()
    assert L.frieda_prove_jobs_plan(None, 4096, cfg, 0, 4, C.byref(per), C.byref(n)) == _lib.ERR_ARG
    assert L.frieda_prove_jobs_plan(None, 4096, cfg, 4, 0, C.byref(per), C.byref(n)) == _lib.ERR_ARG
    assert L.frieda_prove_jobs_plan(None, 4096, _cfg(queries=0)._c(), 4, 4, C.byref(per), C.byref(n)) == _lib.ERR_ARG
    assert (per.value, n.value) == (0, 0)
    assert L.frieda_prove_jobs_plan(None, 4096, cfg, 4, 4, None, C.byref(n)) == _lib.ERR_ARG
    assert L.frieda_prove_jobs_plan(None, 4096, cfg, 4, 4, C.byref(per), None) == _lib.ERR_ARG
