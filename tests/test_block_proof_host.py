"""CPU: the host-only pieces of block proofs (one FRI proof for all blobs of a block).
  frieda_block_challenge against the oracle's channel for K = 1, 2, 3, 17, and its sensitivity to the order of the roots;
  the new symbols in the header, the ctypes table, include/frieda.hpp and the Rust extern block, with matching argument counts;
  tests/cpp/test_block_proof_plan.cpp (block_proof.h: queries -> stripe indices, the wire image) as a stand-alone program under
  AddressSanitizer + UBSan, built as tests/test_encoded_host.py builds its programs."""
import ctypes as C
import hashlib
import os
import re

import pytest

from block_util import oracle_rho
from conftest import ROOT
from test_encoded_host import _build, _run

P = 2**31 - 1

BOUNDARY = (
    "frieda_block_challenge",
    "frieda_aggregate_encoded",
    "frieda_encoded_aggregate_of",
    "frieda_prove_block_seeds",
    "frieda_verify_block",
    "frieda_block_proof_free",
    "frieda_block_proof_fri",
    "frieda_block_proof_n_blobs",
    "frieda_block_proof_n_stripes",
    "frieda_block_proof_stripe_index",
    "frieda_block_proof_values",
    "frieda_block_proof_witness",
    "frieda_block_proof_witness_hashes",
    "frieda_block_proof_serialize",
    "frieda_block_proof_deserialize",
)
HOOK = "frieda_test_aggregate_with_rho"


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def _decls(header):
    text = re.sub(r"/\*.*?\*/", "", _read("include", header), flags=re.S)
    out = {}
    for m in re.finditer(r"\b(frieda_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", text):
        args = m.group(2).strip()
        out[m.group(1)] = 0 if args in ("", "void") else args.count(",") + 1
    return out


def _roots(k):
    return [hashlib.sha256(b"root %d" % i).digest() for i in range(k)]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build()
    from frieda_amd import _lib

    return _lib.lib()


@pytest.mark.parametrize("k", [1, 2, 3, 17])
def test_block_challenge_is_the_oracle_channels_draw(lib, oracle, k):
    import frieda_amd

    roots = _roots(k)
    rho = frieda_amd.block_challenge(roots)
    assert rho == oracle_rho(oracle, roots)
    assert all(0 <= v < P for v in rho)
    # n_blobs is part of the transcript: the first k - 1 roots alone give another challenge
    if k > 1:
        assert frieda_amd.block_challenge(roots[:-1]) != rho


def test_block_challenge_depends_on_the_order_of_the_roots(lib, oracle):
    import frieda_amd

    roots = _roots(3)
    swapped = [roots[1], roots[0], roots[2]]
    assert frieda_amd.block_challenge(swapped) != frieda_amd.block_challenge(roots)
    assert frieda_amd.block_challenge(swapped) == oracle_rho(oracle, swapped)


def test_block_challenge_argument_rules(lib):
    out = (C.c_uint32 * 4)(7, 7, 7, 7)
    tab = (C.c_uint8 * 32)()
    assert lib.frieda_block_challenge(None, 1, out) == 1
    assert lib.frieda_block_challenge(tab, 0, out) == 1
    assert lib.frieda_block_challenge(tab, 65536, out) == 1
    assert lib.frieda_block_challenge(tab, 1, None) == 1
    assert list(out) == [7, 7, 7, 7]


def test_host_entry_points_refuse_null_arguments(lib):
    ok, reason = C.c_int(5), C.c_uint32(9)
    tab = (C.c_uint8 * 32)()
    assert lib.frieda_verify_block(tab, 1, None, None, C.byref(ok), C.byref(reason)) == 1
    out = C.c_void_p()
    assert lib.frieda_block_proof_deserialize(None, 0, C.byref(out)) == 1
    assert lib.frieda_block_proof_deserialize(tab, 32, C.byref(out)) == 1 and not out.value  # 32 zero bytes: no magic
    assert lib.frieda_aggregate_encoded(None, None, 1, C.byref(out)) == 1
    assert lib.frieda_encoded_aggregate_of(None) == 0
    assert lib.frieda_block_proof_n_blobs(None) == 0 and lib.frieda_block_proof_serialize(None, None, 0) == 0
    lib.frieda_block_proof_free(None)


@pytest.mark.parametrize("name", BOUNDARY + (HOOK,))
def test_symbol_is_declared_everywhere(lib, name):
    from frieda_amd import _lib

    boundary, testing = _decls("frieda_hip.h"), _decls("frieda_hip_testing.h")
    if name == HOOK:
        assert name in testing and name not in boundary, "the hook belongs to frieda_hip_testing.h alone"
        want = testing[name]
        assert name not in _read("include", "frieda.hpp")
    else:
        assert name in boundary and name not in testing
        want = boundary[name]
        assert re.search(r"\b" + name + r"\s*\(", _read("include", "frieda.hpp")), "not called by frieda.hpp"
    assert name in _lib.declared_symbols() and hasattr(lib, name)
    assert len(lib._signatures[name][1]) == want, "the ctypes table has another argument count"
    rs = re.search(r"pub fn " + name + r"\s*\(([^)]*)\)", _read("bindings", "rust", "frieda-hip-sys", "src", "lib.rs"))
    assert rs, "not in the Rust extern block"
    assert (0 if not rs.group(1).strip() else rs.group(1).count(":")) == want


def test_python_layer_and_documents_name_the_feature():
    import frieda_amd

    for name in ("aggregate_encoded", "prove_block_seeds", "verify_block", "block_challenge", "BlockProof"):
        assert hasattr(frieda_amd, name), name
    assert hasattr(frieda_amd.BlockProof, "serialize") and hasattr(frieda_amd.BlockProof, "from_bytes")
    assert hasattr(frieda_amd.Context, "aggregate_encoded") and hasattr(frieda_amd.Context, "prove_block_seeds")
    for doc in ("DESIGN.md", "README.md", "INTEGRATION.md"):
        assert "frieda_prove_block_seeds" in _read(doc), doc
    design = _read("DESIGN.md")
    assert "FRIEDA_AGG_SPLIT" in design and "unreviewed" in design.lower()
    assert "aggregate.hip" in _read("frieda_amd", "csrc", "Makefile") and "block_host.cpp" in _read("frieda_amd", "csrc", "Makefile")


def test_block_proof_plan_under_asan(tmp_path):
    _run(_build(tmp_path, "test_block_proof_plan", "address,undefined"))
