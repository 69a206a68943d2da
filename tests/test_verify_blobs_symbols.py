"""frieda_verify_blobs_many and the split route's option: the parts that need no GPU — the entry point is declared with one argument
list in the header, the ctypes table, the Rust extern block and frieda.hpp, and exported; the wrappers exist; no parameter claims device
memory by its name; the option is a row of the table, a Tuning field and a line of DESIGN.md section 10; the new source is built."""
import re
import subprocess
import os

import frieda_amd
from frieda_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "frieda_verify_blobs_many"
# the argument list, in order: (name, C type without spaces, Rust type)
ARGS = [
    ("ctx", "frieda_ctx*", "*mut frieda_ctx"),
    ("proofs", "constfrieda_proof*const*", "*const *const frieda_proof"),
    ("seeds", "constuint64_t*", "*const u64"),
    ("count", "uint32_t", "u32"),
    ("commitments", "constuint8_t*", "*const u8"),
    ("n_blobs", "uint32_t", "u32"),
    ("blob_index", "constuint32_t*", "*const u32"),
    ("out_status", "uint8_t*", "*mut u8"),
    ("out_accepted_per_blob", "uint32_t*", "*mut u32"),
]


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def _c_args():
    header = re.sub(r"/\*.*?\*/", "", _read("include", "frieda_hip.h"), flags=re.S)
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^;{]*?)\)\s*;", header, re.S)
    assert m, "not declared in include/frieda_hip.h"
    return [a.strip() for a in m.group(1).split(",")]


def test_header_argument_list():
    got = []
    for a in _c_args():
        m = re.match(r"^(.*?)(\w+)$", a)
        got.append((m.group(2), m.group(1).replace(" ", "")))
    assert got == [(n, c) for n, c, _ in ARGS]
    for n, _ in got:
        assert not re.fullmatch(r"d|d_\w+", n), n  # host arrays and handles only


def test_rust_argument_list():
    rs = _read("bindings", "rust", "frieda-hip-sys", "src", "lib.rs")
    m = re.search(r"pub fn " + NAME + r"\s*\(([^)]*)\)\s*->\s*c_int;", rs)
    assert m, "not in the Rust extern block"
    got = [tuple(x.strip() for x in a.split(":", 1)) for a in m.group(1).split(",")]
    assert got == [(n, r) for n, _, r in ARGS]


def test_ctypes_table_and_export():
    assert NAME in _lib.declared_symbols()
    L = _lib.lib()
    assert len(getattr(L, NAME).argtypes) == len(ARGS)
    so = os.path.join(ROOT, "frieda_amd", "lib", "libfrieda_hip.so")
    out = subprocess.check_output(["nm", "-D", "--defined-only", so], text=True)
    assert NAME in {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert L.frieda_abi_version() == 1  # additions only


def test_cpp_wrapper_passes_every_argument():
    hpp = _read("include", "frieda.hpp")
    m = re.search(NAME + r"\(([^;]*?)\),\s*h_\);", hpp, re.S)
    assert m, "frieda.hpp does not call " + NAME
    depth, count = 0, 1
    for ch in m.group(1):
        depth += ch in "(<"
        depth -= ch in ")>"
        count += ch == "," and depth == 0
    assert count == len(ARGS)


def test_python_surface():
    assert callable(frieda_amd.Context.verify_blobs_many)
    assert callable(frieda_amd.verify_blobs_many) and "verify_blobs_many" in frieda_amd.__all__
    import inspect

    assert list(inspect.signature(frieda_amd.Context.verify_blobs_many).parameters) == ["self", "proofs", "commitments", "blob_index", "seeds"]


def test_null_context_is_refused():
    assert _lib.lib().frieda_verify_blobs_many(None, None, None, 0, None, 0, None, None, None) == _lib.ERR_ARG


def test_header_sits_next_to_verify_many_and_states_the_contract():
    h = _read("include", "frieda_hip.h")
    at = h.index("int " + NAME + "(")
    assert h.index("int frieda_verify_many(") < at < h.index("int frieda_verify_samples_many(")
    comment = h[h.rindex("/*", 0, at):at]
    for word in ("blob_index", "FRIEDA_VERIFY_WRONG_COMMITMENT", "out_accepted_per_blob", "FRIEDA_ERR_ARG", "FRIEDA_VERIFY_SPLIT_MAX"):
        assert word in comment, word


def test_option_is_registered_and_documented():
    assert re.search(r'\{"FRIEDA_VERIFY_SPLIT_MAX",\s*0,\s*2147483648L', _read("frieda_amd", "csrc", "context.cpp"))
    assert "verify_split_max" in _read("frieda_amd", "csrc", "kernels.h")
    design = _read("DESIGN.md")
    assert "FRIEDA_VERIFY_SPLIT_MAX" in design[design.index("## 10"):]
    assert "verify_chain_kernel" in design and "verify_walk_kernel" in design and NAME in design
    assert NAME in _read("README.md")


def test_makefile_builds_the_new_source():
    mk = _read("frieda_amd", "csrc", "Makefile")
    src = re.search(r"^SRC :=(.*)$", mk, re.M).group(1).split()
    assert "verify_split.hip" in src and "verify.hip" in src
