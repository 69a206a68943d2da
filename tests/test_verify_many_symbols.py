"""frieda_verify_many / frieda_verify_samples_many / frieda_reconstruct_from_proofs: declared in the header, the ctypes table, frieda.hpp
and the Rust extern block with matching argument counts; host pointers and handles only (no parameter named d / d_*); the four status
constants everywhere; the route option documented."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = {"frieda_verify_many": 6, "frieda_verify_samples_many": 9, "frieda_reconstruct_from_proofs": 9}
STATUS = {"FRIEDA_VERIFY_REJECTED": 0, "FRIEDA_VERIFY_ACCEPTED": 1, "FRIEDA_VERIFY_INVARIANT": 2, "FRIEDA_VERIFY_WRONG_COMMITMENT": 3}


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def _header_decls():
    text = re.sub(r"/\*.*?\*/", "", _read("include", "frieda_hip.h"), flags=re.S)
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


def test_status_constants():
    from frieda_amd import _lib

    hdr = _read("include", "frieda_hip.h")
    rs = _read("bindings", "rust", "frieda-hip-sys", "src", "lib.rs")
    hpp = _read("include", "frieda.hpp")
    for name, value in STATUS.items():
        assert re.search(rf"#define {name} {value}\b", hdr), name
        assert re.search(rf"pub const {name}: u8 = {value};", rs), name
        assert name in hpp, name
        assert getattr(_lib, name[len("FRIEDA_"):]) == value


def test_python_surface():
    import frieda_amd

    for f in ("verify_many", "verify_samples_many", "reconstruct_from_proofs"):
        assert callable(getattr(frieda_amd, f, None)), f
        assert callable(getattr(frieda_amd.Context, f, None)), f


def test_option_is_documented_and_in_flight_list_names_the_calls():
    hdr = _read("include", "frieda_hip.h")
    assert "FRIEDA_VERIFY_DEVICE_MIN" in hdr
    design = _read("DESIGN.md")
    sec10 = design[design.index("## 10"):]
    assert "FRIEDA_VERIFY_DEVICE_MIN" in sec10
    in_flight = hdr[hdr.index("While one is in flight"):hdr.index("int frieda_prove_begin(")]
    for name in FUNCS:
        assert name in in_flight, name


def test_option_is_registered():
    """a row of the option table: frieda_ctx_set_option accepts it and the unknown-variable note does not name it"""
    assert re.search(r'\{"FRIEDA_VERIFY_DEVICE_MIN",\s*0,', _read("frieda_amd", "csrc", "context.cpp"))
