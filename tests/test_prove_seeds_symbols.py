"""One blob under many seeds (frieda_encode / frieda_prove_seeds*): the parts that need no GPU — every new entry point is declared
and exported in every binding, the workspace function states the memory claim, the route option exists and is documented."""
import os
import re
import subprocess

import pytest

import frieda_amd
from frieda_amd import _lib

from util import blob_len_for

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_FUNCTIONS = [
    "frieda_encode",
    "frieda_encode_device",
    "frieda_encoded_commitment",
    "frieda_encoded_bytes",
    "frieda_encoded_free",
    "frieda_prove_seeds_begin",
    "frieda_prove_seeds_finish",
    "frieda_prove_seeds",
    "frieda_commit_and_generate_proofs_for_seeds",
    "frieda_seeds_workspace_bytes",
]


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


@pytest.mark.parametrize("name", NEW_FUNCTIONS)
def test_declared_in_every_binding(name):
    assert re.search(r"\b" + name + r"\s*\(", _read("include", "frieda_hip.h")), "not declared in the header"
    assert name in _lib.declared_symbols(), "not in the ctypes table"
    assert re.search(r"pub fn " + name + r"\s*\(", _read("bindings", "rust", "frieda-hip-sys", "src", "lib.rs")), "not in the Rust extern block"
    assert re.search(r"\b" + name + r"\b", _read("include", "frieda.hpp")), "not used or named by frieda.hpp"


def test_exported_by_the_built_library():
    so = os.path.join(ROOT, "frieda_amd", "lib", "libfrieda_hip.so")
    out = subprocess.check_output(["nm", "-D", "--defined-only", so], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert not [n for n in NEW_FUNCTIONS if n not in exported]
    L = _lib.lib()
    assert not [n for n in NEW_FUNCTIONS if not hasattr(L, n)]
    assert L.frieda_abi_version() == 1  # additions only


def test_wrappers_exist():
    for name in ("encode", "encode_device", "prove_seeds", "prove_seeds_begin", "prove_seeds_finish", "commit_and_generate_proofs_for_seeds"):
        assert callable(getattr(frieda_amd.Context, name))
    assert callable(frieda_amd.commit_and_generate_proofs_for_seeds) and callable(frieda_amd.seeds_workspace_bytes)
    for name in ("commitment", "nbytes", "close"):
        assert hasattr(frieda_amd.Encoded, name)
    rs = _read("bindings", "rust", "frieda-hip-sys", "src", "lib.rs")
    assert "pub struct Encoded" in rs and "impl Drop for Encoded" in rs
    assert re.search(r"class Encoded\b", _read("include", "frieda.hpp"))


def _cfg(log_blowup=4, last=0, queries=20, pow_bits=20):
    return frieda_amd.PcsConfig(frieda_amd.FriConfig(log_blowup, last, queries), pow_bits)


def _encoded_bytes(log_domain):
    """evaluations + first tree + root, each from a 256-byte boundary (the layout of a frieda_encoded)"""
    up = lambda b: (b + 255) & ~255
    return up(16 << log_domain) + up((64 << log_domain) - 64 + 32) + up(32)


@pytest.mark.parametrize("log_domain", [12, 14, 16, 18, 20, 22, 24])
def test_workspace_is_increasing_and_states_the_memory_claim(log_domain):
    cfg = _cfg()
    length = blob_len_for(log_domain)
    per_blob = frieda_amd.workspace_bytes(length, 4, 0, True)
    assert per_blob > 0
    prev = 0
    for s in [1, 2, 3, 5, 8, 15, 16, 60, 64, 255, 4096, 65535]:
        ws = frieda_amd.seeds_workspace_bytes(length, cfg, s)
        assert ws > prev, (s, ws, prev)
        prev = ws
        if s >= 2:
            # the S proofs share ONE evaluation and first tree: less memory than S proofs' workspaces, the shared part included
            assert ws + _encoded_bytes(log_domain) < s * per_blob, (log_domain, s, ws, per_blob)


def test_workspace_refuses_what_the_prover_refuses():
    cfg = _cfg()
    assert frieda_amd.seeds_workspace_bytes(4096, cfg, 0) == 0
    assert frieda_amd.seeds_workspace_bytes(4096, cfg, 65536) == 0
    assert frieda_amd.seeds_workspace_bytes(4096, _cfg(last=11), 4) == 0
    assert frieda_amd.seeds_workspace_bytes(4096, _cfg(queries=0), 4) == 0
    assert frieda_amd.seeds_workspace_bytes(3, _cfg(last=3), 4) == 0  # polynomial too small for the configuration


def test_route_option_is_registered_and_documented():
    import ctypes as C

    from frieda_amd.api import _check  # noqa: F401

    h = _read("frieda_amd", "csrc", "context.cpp")
    assert '"FRIEDA_SEEDS_FOLD_GROUP"' in h
    assert "FRIEDA_SEEDS_FOLD_GROUP" in _read("DESIGN.md")
    assert "FRIEDA_SEEDS_FOLD_GROUP" in _read("include", "frieda_hip.h")
    # tuning_set through the C ABI needs a context (a device); the table itself is what accepts the name: the same check the
    # library makes, on the table's text — name present with a range that holds 0 (route A) and a group size
    m = re.search(r'\{"FRIEDA_SEEDS_FOLD_GROUP",\s*(\d+),\s*(\d+),', h)
    assert m and int(m.group(1)) == 0 and int(m.group(2)) >= 8
    assert C.sizeof(C.c_void_p) == 8
