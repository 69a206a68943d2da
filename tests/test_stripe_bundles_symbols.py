"""frieda_open_stripe_bundles / frieda_verify_stripe_bundles / frieda_verify_stripe_bundles_many /
frieda_reconstruct_blobs_from_stripe_bundles: declared in the header, the ctypes table and the Rust extern block with matching argument
counts; host pointers and handles only (no parameter named d / d_*); ABI version 1; the Python surface; the in-flight list; null
arguments refused without a device; the Makefile wiring; the docs and the profile record."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = {"frieda_open_stripe_bundles": 11, "frieda_verify_stripe_bundles": 11, "frieda_verify_stripe_bundles_many": 12,
         "frieda_reconstruct_blobs_from_stripe_bundles": 15}
CTX_CALLS = ("frieda_open_stripe_bundles", "frieda_verify_stripe_bundles_many", "frieda_reconstruct_blobs_from_stripe_bundles")


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


@pytest.mark.parametrize("name", sorted(FUNCS))
def test_parameters_are_host_pointers_and_handles(name):
    for a in _header_decls()[name].split(","):
        pname = re.match(r"^.*?(\w+)(?:\[\d*\])?\s*$", a.strip()).group(1)
        assert not re.fullmatch(r"d|d_\w+", pname), f"{name}: parameter {pname} is named like a device pointer"


def test_abi_version_stays_1():
    m = re.search(r"#define\s+FRIEDA_ABI_VERSION\s+(\d+)", _read("include", "frieda_hip.h"))
    assert m and int(m.group(1)) == 1
    from frieda_amd import _lib

    assert _lib.lib().frieda_abi_version() == 1  # the stripe bundles only add to the interface


def test_python_surface():
    import frieda_amd

    for f in ("open_stripe_bundles", "verify_stripe_bundles", "verify_stripe_bundles_many", "reconstruct_blobs_from_stripe_bundles"):
        assert callable(getattr(frieda_amd, f, None)), f
        assert f in frieda_amd.__all__, f
    for f in ("verify_stripe_bundles_many", "reconstruct_blobs_from_stripe_bundles"):
        assert callable(getattr(frieda_amd.Context, f, None)), f


def test_in_flight_list_names_the_calls():
    hdr = _read("include", "frieda_hip.h")
    in_flight = hdr[hdr.index("While one is in flight"):hdr.index("int frieda_prove_begin(")]
    for name in CTX_CALLS:
        assert name in in_flight, name


def test_null_arguments_are_refused_without_a_device():
    from frieda_amd import _lib

    L = _lib.lib()
    assert L.frieda_open_stripe_bundles(None, None, 1, 0, None, None, 1, None, None, 0, None) == _lib.ERR_ARG
    assert L.frieda_verify_stripe_bundles_many(None, None, 1, 4, 0, None, None, 1, None, None, None, None) == _lib.ERR_ARG
    assert L.frieda_verify_stripe_bundles(None, 1, 4, 0, None, None, 1, None, None, None, None) == _lib.ERR_ARG
    assert L.frieda_verify_stripe_bundles(None, 1, 4, 0, None, None, 0, None, None, None, None) == _lib.OK  # no bundles: a no-op
    assert L.frieda_reconstruct_blobs_from_stripe_bundles(None, None, 1, 4, 100, 0, None, None, 0, None, None, None, None, None, None) == _lib.ERR_ARG
    # the host verifier's own argument rule: no blobs, too many blobs, a shape out of range, *_first that does not start at 0
    com = (C.c_uint8 * 64)()
    first, wfirst = (C.c_uint32 * 2)(0, 1), (C.c_uint64 * 2)(0, 4)
    idx, values, witness, status = (C.c_uint32 * 1)(3), (C.c_uint32 * 8)(), (C.c_uint8 * 256)(), (C.c_uint8 * 2)(0xEE, 0xEE)
    args = (idx, first, 1, values, witness, wfirst, status)
    assert L.frieda_verify_stripe_bundles(com, 0, 4, 0, *args) == _lib.ERR_ARG
    assert L.frieda_verify_stripe_bundles(com, 65537, 4, 0, *args) == _lib.ERR_ARG
    assert L.frieda_verify_stripe_bundles(com, 2, 29, 0, *args) == _lib.ERR_ARG
    assert L.frieda_verify_stripe_bundles(com, 2, 4, 0, idx, (C.c_uint32 * 2)(1, 1), 1, values, witness, wfirst, status) == _lib.ERR_ARG
    assert bytes(status) == b"\xee\xee"
    assert L.frieda_verify_stripe_bundles(com, 2, 4, 0, *args) == _lib.OK and bytes(status) == b"\x00\x00"  # well formed, the zeros do not verify


def test_the_sources_are_wired_in():
    mk = _read("frieda_amd", "csrc", "Makefile")
    assert " stripe_bundles.hip " in mk and " stripe_bundles_host.cpp " in mk
    kernels = _read("frieda_amd", "csrc", "stripe_bundles.hip")
    for h in ("cells_dev.h", "queries_dev.h", "walk_dev.h", "tree_dev.h"):
        assert '#include "' + h + '"' in kernels, h
    code = re.sub(r"//.*", "", kernels)
    for shared in ("cellsdev::open_node", "qdev::emit_of", "walkdev::walk_level"):
        assert shared in code, shared
    assert "Scope" not in code, "no kernel-timer scopes: the timer's names are tied to tests/workspace_rows.py"
    for f in ("bundles.hip", "cells.hip"):
        assert "stripe_bundle_" not in re.sub(r"//.*", "", _read("frieda_amd", "csrc", f)), f


def test_docs_describe_the_stripe_bundles():
    design = _read("DESIGN.md")
    for doc in (design, _read("README.md"), _read("INTEGRATION.md")):
        assert "frieda_open_stripe_bundles" in doc and "frieda_reconstruct_blobs_from_stripe_bundles" in doc
    assert "stripe_bundles.hip" in design and "stripe_bundle_walk" in design
    assert "stripe_bundles_timing.py" in _read("tools", "README.md")
    out_of_scope = design[design.index("## 9"):design.index("## 10")]
    assert "over the blobs of a block" not in out_of_scope and "wire format" in out_of_scope
    assert "profiles/r16_stripe_bundles.txt" in design and "r16_stripe_bundles.txt" in _read("profiles", "README.md")
    profile = _read("profiles", "r16_stripe_bundles.txt")
    for shape in ("1_bundle", "8_bundles"):
        assert re.search(r'^\{"row": "bytes", "shape": "' + shape + r'".*"witness_hashes": \d+', profile, flags=re.M), shape
        for row in ("open", "verify/device", "verify/host", "rebuild"):
            for form in ("stripe_bundles", "bundle_loop", "stripes"):
                assert re.search(r'^\{"row": "' + row + r'", "shape": "' + shape + r'", "form": "' + form + r'".*"ms_median": [0-9.]+.*"ms_min".*"ms_max"', profile,
                                 flags=re.M), (shape, row, form)
    for text in (design, profile, _read("include", "frieda_hip.h"), _read("profiles", "README.md")):
        assert "@@" not in text, "a template marker was left in"
