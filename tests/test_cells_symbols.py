"""frieda_encoded_shape / frieda_open_cells / frieda_verify_cells / frieda_verify_cells_many / frieda_reconstruct_from_opened_cells: declared in
the header, the ctypes table, frieda.hpp and the Rust extern block with matching argument counts; host pointers and handles only (no
parameter named d / d_*); the Python surface; the in-flight list; the docs."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = {"frieda_encoded_shape": 3, "frieda_open_cells": 7, "frieda_verify_cells": 8, "frieda_verify_cells_many": 9,
         "frieda_reconstruct_from_opened_cells": 12}
CTX_CALLS = ("frieda_open_cells", "frieda_verify_cells_many", "frieda_reconstruct_from_opened_cells")


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


def test_header_constants():
    hdr = _read("include", "frieda_hip.h")
    for name, value in (("FRIEDA_MAX_LOG_OPEN_CELL", 10), ("FRIEDA_CELL_REJECTED", 0), ("FRIEDA_CELL_ACCEPTED", 1)):
        m = re.search(r"#define\s+" + name + r"\s+(\d+)", hdr)
        assert m and int(m.group(1)) == value, name
    from frieda_amd import _lib

    assert (_lib.CELL_REJECTED, _lib.CELL_ACCEPTED, _lib.MAX_LOG_OPEN_CELL) == (0, 1, 10)


def test_python_surface():
    import frieda_amd

    for f in ("open_cells", "verify_cells", "verify_cells_many", "reconstruct_from_opened_cells"):
        assert callable(getattr(frieda_amd, f, None)), f
        assert f in frieda_amd.__all__, f
    for f in ("verify_cells_many", "reconstruct_from_opened_cells"):
        assert callable(getattr(frieda_amd.Context, f, None)), f
    assert callable(getattr(frieda_amd.Encoded, "open_cells", None))
    assert isinstance(frieda_amd.Encoded.shape, property)


def test_in_flight_list_names_the_calls():
    hdr = _read("include", "frieda_hip.h")
    in_flight = hdr[hdr.index("While one is in flight"):hdr.index("int frieda_prove_begin(")]
    for name in CTX_CALLS:
        assert name in in_flight, name


def test_null_arguments_are_refused_without_a_device():
    from frieda_amd import _lib

    L = _lib.lib()
    assert L.frieda_encoded_shape(None, None, None) == _lib.ERR_ARG
    assert L.frieda_open_cells(None, None, 0, None, 1, None, None) == _lib.ERR_ARG
    assert L.frieda_verify_cells_many(None, None, 4, 0, None, 1, None, None, None) == _lib.ERR_ARG
    assert L.frieda_verify_cells(None, 4, 0, None, 1, None, None, None) == _lib.ERR_ARG
    assert L.frieda_verify_cells(None, 4, 0, None, 0, None, None, None) == _lib.OK  # no cells: a no-op


def test_docs_describe_the_flow():
    design = _read("DESIGN.md")
    for doc in (design, _read("README.md"), _read("INTEGRATION.md")):
        assert "frieda_open_cells" in doc and "frieda_reconstruct_from_opened_cells" in doc
    assert "cells.hip" in design
    assert "profiles/r11_open_cells.txt" in design
    profile = _read("profiles", "r11_open_cells.txt")
    for row in ("open", "verify/device", "verify/host", "rebuild/cells", "rebuild/pairs"):
        assert re.search(r'^\{"row": "' + row + r'".*"ms_median": [0-9.]+', profile, flags=re.M), f"no measured row {row}"
    for text in (design, profile, _read("include", "frieda_hip.h"), _read("profiles", "README.md")):
        assert "@@" not in text, "a template marker was left in"
