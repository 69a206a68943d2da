"""frieda_open_cells_blobs / frieda_verify_cells_blobs / frieda_verify_cells_blobs_many / frieda_reconstruct_blobs_from_opened_stripes: declared in
the header, the ctypes table, frieda.hpp and the Rust extern block with matching argument counts; host pointers and handles only (no
parameter named d / d_*); the ABI version unchanged; the Python surface; the in-flight list; the docs and the measured record."""
import json
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = {"frieda_open_cells_blobs": 9, "frieda_verify_cells_blobs": 10, "frieda_verify_cells_blobs_many": 11,
         "frieda_reconstruct_blobs_from_opened_stripes": 13}
CTX_CALLS = ("frieda_open_cells_blobs", "frieda_verify_cells_blobs_many", "frieda_reconstruct_blobs_from_opened_stripes")
ROWS = ("open/blobs", "open/loop", "verify/blobs", "verify/loop", "rebuild/stripes", "rebuild/loop")


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


def test_additions_only():
    """the ABI version stays 1, and the single-blob declarations are still there"""
    hdr = _read("include", "frieda_hip.h")
    assert re.search(r"#define\s+FRIEDA_ABI_VERSION\s+1\b", hdr)
    decls = _header_decls()
    for name, count in (("frieda_open_cells", 7), ("frieda_verify_cells", 8), ("frieda_verify_cells_many", 9), ("frieda_reconstruct_from_opened_cells", 12)):
        assert decls[name].count(",") + 1 == count, name


def test_python_surface():
    import frieda_amd

    for f in ("open_cells_blobs", "open_stripes", "verify_cells_blobs", "verify_cells_blobs_many", "reconstruct_blobs_from_opened_stripes"):
        assert callable(getattr(frieda_amd, f, None)), f
        assert f in frieda_amd.__all__, f
    for f in ("verify_cells_blobs_many", "reconstruct_blobs_from_opened_stripes"):
        assert callable(getattr(frieda_amd.Context, f, None)), f


def test_in_flight_list_names_the_calls():
    hdr = _read("include", "frieda_hip.h")
    in_flight = hdr[hdr.index("While one is in flight"):hdr.index("int frieda_prove_begin(")]
    for name in CTX_CALLS:
        assert name in in_flight, name


def test_header_states_the_contract():
    hdr = _read("include", "frieda_hip.h")
    text = " ".join(re.sub(r"\n \* ?", "\n", hdr[hdr.index("the cells of a block"):hdr.index("---- batch policy")]).split())
    for phrase in ("STRIPE", "blob_index[i] < n_blobs", "never depends on the other cells", "NO per-blob fallback", "frieda_reconstruct_from_opened_cells per blob",
                   "cut at stripe boundaries", "names the blob", "profiles/r12_stripes.txt"):
        assert phrase in text, phrase


def test_null_arguments_are_refused_without_a_device():
    from frieda_amd import _lib

    L = _lib.lib()
    assert L.frieda_open_cells_blobs(None, None, 1, 0, None, None, 1, None, None) == _lib.ERR_ARG
    assert L.frieda_verify_cells_blobs_many(None, None, 1, 4, 0, None, None, 1, None, None, None) == _lib.ERR_ARG
    assert L.frieda_reconstruct_blobs_from_opened_stripes(None, None, 1, 4, 100, 0, None, 1, None, None, None, None, None) == _lib.ERR_ARG
    assert L.frieda_verify_cells_blobs(None, 1, 4, 0, None, None, 1, None, None, None) == _lib.ERR_ARG
    assert L.frieda_verify_cells_blobs(None, 1, 4, 0, None, None, 0, None, None, None) == _lib.OK  # no cells: a no-op


def test_docs_and_record():
    design = _read("DESIGN.md")
    for doc in (design, _read("README.md"), _read("INTEGRATION.md")):
        assert "frieda_open_cells_blobs" in doc and "frieda_reconstruct_blobs_from_opened_stripes" in doc
    assert "profiles/r12_stripes.txt" in design
    assert "r12_stripes.txt" in _read("profiles", "README.md")
    assert "stripes_timing.py" in _read("tools", "README.md")
    assert os.path.exists(os.path.join(ROOT, "tools", "stripes_timing.py"))
    profile = _read("profiles", "r12_stripes.txt")
    med = {}
    for row in ROWS:
        m = re.search(r'^\{"row": "' + row + r'".*"ms_median": ([0-9.]+), "ms_min": [0-9.]+, "ms_max": [0-9.]+.*"reps": (\d+)', profile, flags=re.M)
        assert m, f"no measured row {row} with its spread"
        assert int(m.group(2)) >= 21, row
        med[row] = float(m.group(1))
    for kernel in ("cells_open_blobs_paths_kernel", "cells_walk_blobs_kernel", "cells_stripe_accept_kernel", "cells_stripe_gather_kernel"):
        assert kernel in profile, kernel
    # the header and DESIGN quote the record's ratios (its last line: loop median / new-call median) and its medians
    ratios = json.loads(re.search(r'^\{"ratio_loop_over_new".*$', profile, flags=re.M).group(0))["ratio_loop_over_new"]
    for new, loop in (("open/blobs", "open/loop"), ("verify/blobs", "verify/loop"), ("rebuild/stripes", "rebuild/loop")):
        assert abs(ratios[new] - med[loop] / med[new]) < 0.02, new
        quoted = f"{ratios[new]:.2f} times"
        for text, where in ((design, "DESIGN.md"), (_read("include", "frieda_hip.h"), "frieda_hip.h")):
            assert quoted in text, (where, new, quoted)
    for text in (design, profile, _read("include", "frieda_hip.h"), _read("profiles", "README.md")):
        assert "@@" not in text, "a template marker was left in"
