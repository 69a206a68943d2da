"""frieda_verify_pairs / frieda_verify_pairs_many / frieda_reconstruct_from_proof_pairs: declared in the header, the ctypes table,
frieda.hpp and the Rust extern block with matching argument counts; host pointers and handles only (no parameter named d / d_*); the
Python surface; the in-flight list; the test hook of the pass budget."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = {"frieda_verify_pairs": 7, "frieda_verify_pairs_many": 10, "frieda_reconstruct_from_proof_pairs": 9}


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def _header_decls(name="frieda_hip.h"):
    text = re.sub(r"/\*.*?\*/", "", _read("include", name), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(frieda_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", text)}


@pytest.mark.parametrize("name", sorted(FUNCS))
def test_declared_everywhere_with_matching_argument_counts(name):
    from frieda_amd import _lib

    decls = _header_decls()
    assert name in decls, "not declared in include/frieda_hip.h"
    assert decls[name].count(",") + 1 == FUNCS[name]
    L = _lib.lib()
    assert hasattr(L, name), "not exported by the library"
    assert len(L._signatures[name][1]) == FUNCS[name], "ctypes argument count"
    rs = re.search(r"pub fn " + name + r"\s*\(([^)]*)\)", _read("bindings", "rust", "frieda-hip-sys", "src", "lib.rs"))
    assert rs, "not in the Rust extern block"
    assert rs.group(1).count(":") == FUNCS[name]
    assert re.search(r"\b" + name + r"\s*\(", _read("include", "frieda.hpp")), "not called by frieda.hpp"


@pytest.mark.parametrize("name", sorted(FUNCS))
def test_parameters_are_host_pointers_and_handles(name):
    for a in _header_decls()[name].split(","):
        pname = re.match(r"^.*?(\w+)(?:\[\d*\])?\s*$", a.strip()).group(1)
        assert not re.fullmatch(r"d|d_\w+", pname), f"{name}: parameter {pname} is named like a device pointer"


def test_python_surface():
    import frieda_amd

    for f in ("verify_pairs", "verify_pairs_many", "reconstruct_from_proof_pairs"):
        assert callable(getattr(frieda_amd, f, None)), f
        assert f in frieda_amd.__all__, f
    for f in ("verify_pairs_many", "reconstruct_from_proof_pairs"):
        assert callable(getattr(frieda_amd.Context, f, None)), f


def test_in_flight_list_names_the_calls():
    hdr = _read("include", "frieda_hip.h")
    in_flight = hdr[hdr.index("While one is in flight"):hdr.index("int frieda_prove_begin(")]
    for name in FUNCS:
        assert name in in_flight, name


def test_pass_budget_hook():
    from frieda_amd import _lib

    name = "frieda_ctx_test_set_verify_pass_bytes"
    assert name in _header_decls("frieda_hip_testing.h") and name not in _header_decls()
    L = _lib.lib()
    assert len(L._signatures[name][1]) == 2
    assert L.frieda_ctx_test_set_verify_pass_bytes(None, 0) == 1  # a null context is refused


def test_docs_no_longer_leave_the_siblings_out():
    design = _read("DESIGN.md")
    assert "not pooled: the verified sibling values" not in design
    for doc in (design, _read("README.md"), _read("INTEGRATION.md")):
        assert "frieda_reconstruct_from_proof_pairs" in doc
