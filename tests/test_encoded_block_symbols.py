"""CPU: the five entry points that make encoded handles for a block or from a rebuild (frieda_encode_batch, frieda_rebuild_encoded_*)
are declared with one argument count in every layer: include/frieda_hip.h, the ctypes table of frieda_amd/_lib.py, the Rust FFI
declarations, and wrapped by include/frieda.hpp and by the Python Context; each rebuild call takes its reconstruct twin's arguments plus
the handle pointer."""
import os
import re

import pytest

from conftest import ROOT

NAMES = {
    "frieda_encode_batch": None,
    "frieda_rebuild_encoded_from_opened_cells": "frieda_reconstruct_from_opened_cells",
    "frieda_rebuild_encoded_from_cell_bundles": "frieda_reconstruct_from_cell_bundles",
    "frieda_rebuild_encoded_blobs_from_opened_stripes": "frieda_reconstruct_blobs_from_opened_stripes",
    "frieda_rebuild_encoded_blobs_from_stripe_bundles": "frieda_reconstruct_blobs_from_stripe_bundles",
}
EXPECTED_ARGS = {
    "frieda_encode_batch": 7,
    "frieda_rebuild_encoded_from_opened_cells": 13,
    "frieda_rebuild_encoded_from_cell_bundles": 15,
    "frieda_rebuild_encoded_blobs_from_opened_stripes": 14,
    "frieda_rebuild_encoded_blobs_from_stripe_bundles": 16,
}


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def _top_level_args(text):
    """number of comma-separated arguments of a parenthesised list, commas inside nested brackets not counted"""
    depth, count = 0, 1
    if not text.strip():
        return 0
    for ch in text:
        if ch in "([":
            depth += 1
        elif ch in ")]":
            depth -= 1
        elif ch == "," and depth == 0:
            count += 1
    return count


def _c_args(header, name):
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    return _top_level_args(m.group(1)) if m else None


def _rust_args(src, name):
    m = re.search(r"pub fn " + name + r"\s*\(([^;]*?)\)\s*->\s*c_int\s*;", src, flags=re.S)
    return _top_level_args(m.group(1)) if m else None


def _ctypes_args(src, name):
    m = re.search(r'"' + name + r'":\s*\(C\.c_int,\s*\[(.*?)\]\),', src)
    return _top_level_args(m.group(1)) if m else None


@pytest.mark.parametrize("name", sorted(NAMES))
def test_declared_in_every_layer_with_one_argument_count(name):
    header = _read("include", "frieda_hip.h")
    want = EXPECTED_ARGS[name]
    assert _c_args(header, name) == want, "include/frieda_hip.h"
    assert _ctypes_args(_read("frieda_amd", "_lib.py"), name) == want, "frieda_amd/_lib.py"
    assert _rust_args(_read("bindings", "rust", "frieda-hip-sys", "src", "lib.rs"), name) == want, "bindings/rust/frieda-hip-sys/src/lib.rs"
    twin = NAMES[name]
    if twin:
        assert _c_args(header, twin) == want - 1, "the rebuild call takes its twin's arguments plus the handle pointer"
    # the C++ wrapper calls the entry point with every argument
    hpp = _read("include", "frieda.hpp")
    at = hpp.find(name + "(h_,")
    assert at >= 0, "include/frieda.hpp does not call " + name
    start = at + len(name) + 1
    depth, end = 1, start
    while depth:
        depth += {"(": 1, ")": -1}.get(hpp[end], 0)
        end += 1
    assert _top_level_args(hpp[start : end - 1]) == want, "include/frieda.hpp"


def test_the_section_follows_the_stripe_bundles():
    header = _read("include", "frieda_hip.h")
    assert header.index("frieda_reconstruct_blobs_from_stripe_bundles(") < header.index("frieda_encode_batch(") < header.index("frieda_batch_plan")


def test_python_methods_exist():
    import frieda_amd
    from frieda_amd import api

    for short in ["encode_batch"] + [n[len("frieda_"):] for n in NAMES if NAMES[n]]:
        assert callable(getattr(api.Context, short)), short
        assert callable(getattr(api, short)), short
        assert callable(getattr(frieda_amd, short)), short
