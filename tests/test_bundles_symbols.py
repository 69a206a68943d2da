"""frieda_cell_bundle_witness_count / frieda_open_cell_bundles / frieda_verify_cell_bundles / frieda_verify_cell_bundles_many /
frieda_reconstruct_from_cell_bundles: declared in the header, the ctypes table and the Rust extern block with matching argument counts;
host pointers and handles only (no parameter named d / d_*); the constants; the Python surface; the in-flight list; null arguments
refused without a device; the docs."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = {"frieda_cell_bundle_witness_count": 5, "frieda_open_cell_bundles": 10, "frieda_verify_cell_bundles": 10, "frieda_verify_cell_bundles_many": 11,
         "frieda_reconstruct_from_cell_bundles": 14}
CTX_CALLS = ("frieda_open_cell_bundles", "frieda_verify_cell_bundles_many", "frieda_reconstruct_from_cell_bundles")


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


def test_constants_and_abi_version():
    hdr = _read("include", "frieda_hip.h")
    rs = _read("bindings", "rust", "frieda-hip-sys", "src", "lib.rs")
    for name, value in (("FRIEDA_MAX_BUNDLE_CELLS", 1024), ("FRIEDA_BUNDLE_REJECTED", 0), ("FRIEDA_BUNDLE_ACCEPTED", 1), ("FRIEDA_BUNDLE_MALFORMED", 2),
                        ("FRIEDA_ABI_VERSION", 1)):
        m = re.search(r"#define\s+" + name + r"\s+(\d+)", hdr)
        assert m and int(m.group(1)) == value, name
        if name != "FRIEDA_ABI_VERSION":
            assert re.search(r"pub const " + name + r": \w+ = " + str(value) + ";", rs), name
    from frieda_amd import _lib

    assert (_lib.BUNDLE_REJECTED, _lib.BUNDLE_ACCEPTED, _lib.BUNDLE_MALFORMED, _lib.MAX_BUNDLE_CELLS) == (0, 1, 2, 1024)
    assert _lib.lib().frieda_abi_version() == 1  # the bundles only add to the interface


def test_python_surface():
    import frieda_amd

    for f in ("open_cell_bundles", "verify_cell_bundles", "verify_cell_bundles_many", "reconstruct_from_cell_bundles", "cell_bundle_witness_count"):
        assert callable(getattr(frieda_amd, f, None)), f
        assert f in frieda_amd.__all__, f
    for f in ("verify_cell_bundles_many", "reconstruct_from_cell_bundles"):
        assert callable(getattr(frieda_amd.Context, f, None)), f
    assert callable(getattr(frieda_amd.Encoded, "open_cell_bundles", None))


def test_in_flight_list_names_the_calls():
    hdr = _read("include", "frieda_hip.h")
    in_flight = hdr[hdr.index("While one is in flight"):hdr.index("int frieda_prove_begin(")]
    for name in CTX_CALLS:
        assert name in in_flight, name


def test_null_arguments_are_refused_without_a_device():
    from frieda_amd import _lib

    L = _lib.lib()
    n = C.c_size_t(0)
    assert L.frieda_cell_bundle_witness_count(4, 0, None, 1, C.byref(n)) == _lib.ERR_ARG
    assert L.frieda_cell_bundle_witness_count(4, 0, None, 0, None) == _lib.ERR_ARG
    assert L.frieda_open_cell_bundles(None, None, 0, None, None, 1, None, None, 0, None) == _lib.ERR_ARG
    assert L.frieda_verify_cell_bundles_many(None, None, 4, 0, None, None, 1, None, None, None, None) == _lib.ERR_ARG
    assert L.frieda_verify_cell_bundles(None, 4, 0, None, None, 1, None, None, None, None) == _lib.ERR_ARG
    assert L.frieda_verify_cell_bundles(None, 4, 0, None, None, 0, None, None, None, None) == _lib.OK  # no bundles: a no-op
    assert L.frieda_reconstruct_from_cell_bundles(None, None, 4, 100, 0, None, None, 0, None, None, None, None, None, None) == _lib.ERR_ARG


def test_the_sources_are_wired_in():
    mk = _read("frieda_amd", "csrc", "Makefile")
    assert " bundles.hip " in mk and " bundles_host.cpp " in mk
    cells = _read("frieda_amd", "csrc", "cells.hip")
    assert "bundle_" not in re.sub(r"//.*", "", cells), "the bundle kernels live in bundles.hip"
    for f in ("bundles.hip", "cells.hip"):
        assert '#include "cells_dev.h"' in _read("frieda_amd", "csrc", f), f
    for f in ("bundles.hip", "verify.hip"):
        assert '#include "walk_dev.h"' in _read("frieda_amd", "csrc", f), f


def test_docs_describe_the_bundles():
    design = _read("DESIGN.md")
    for doc in (design, _read("README.md"), _read("INTEGRATION.md")):
        assert "frieda_open_cell_bundles" in doc and "frieda_reconstruct_from_cell_bundles" in doc
    assert "bundles.hip" in design and "bundle_walk" in design
    assert "cell_bundles_timing.py" in _read("tools", "README.md")
    out_of_scope = design[design.index("## 9"):design.index("## 10")]
    assert "compacted multi-cell witnesses" not in out_of_scope and "wire format" in out_of_scope
    assert "profiles/r15_cell_bundles.txt" in design and "r15_cell_bundles.txt" in _read("profiles", "README.md")
    profile = _read("profiles", "r15_cell_bundles.txt")
    for shape in ("1_bundle", "8_bundles"):
        assert re.search(r'^\{"row": "bytes", "shape": "' + shape + r'".*"witness_hashes": \d+', profile, flags=re.M), shape
        for row in ("open", "verify/device", "verify/host", "rebuild"):
            for form in ("bundles", "cells"):
                assert re.search(r'^\{"row": "' + row + r'", "shape": "' + shape + r'", "form": "' + form + r'".*"ms_median": [0-9.]+.*"ms_min".*"ms_max"', profile,
                                 flags=re.M), (shape, row, form)
    for text in (design, profile, _read("include", "frieda_hip.h"), _read("profiles", "README.md")):
        assert "@@" not in text, "a template marker was left in"
