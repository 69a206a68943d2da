"""frieda_ctx_test_poison (the test hook behind tests/test_gpu_workspace_history.py): declared in the testing header, the ctypes table
and the Rust extern block with matching argument counts, outside the drop-in boundary, refused without a context, named by DESIGN.md —
and the closure of the poisoned case table: every kernel the library can launch (every Scope name of frieda_amd/csrc/*.hip) is claimed
by a row of tests/workspace_rows.py or listed in its EXEMPT dict with a reason, so a new kernel fails here until it has a poisoned row."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOOK, N_ARGS = "frieda_ctx_test_poison", 4

# Scope names that reach the timer through an argument, with the call sites that pass them (checked below against the source)
PASSED_IN = {
    "ntt.hip": ("launch_pass", {"ntt_pass_mid", "ntt_pass_last"}),
    "tree.hip": ("launch_tree_a", {"tree5_node", "tree5_leaf", "tree5_fold_circle", "tree5_fold_line"}),
}


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def _decls(name):
    text = re.sub(r"/\*.*?\*/", "", _read("include", name), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(frieda_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", text)}


def test_declared_everywhere_with_matching_argument_counts():
    from frieda_amd import _lib

    decls = _decls("frieda_hip_testing.h")
    assert HOOK in decls and decls[HOOK].count(",") + 1 == N_ARGS
    assert HOOK not in _decls("frieda_hip.h"), "a test hook is not part of the boundary"
    assert HOOK not in _read("include", "frieda.hpp")
    L = _lib.lib()
    assert hasattr(L, HOOK), "not exported by the library"
    assert len(L._signatures[HOOK][1]) == N_ARGS, "ctypes argument count"
    rs = re.search(r"pub fn " + HOOK + r"\s*\(([^)]*)\)", _read("bindings", "rust", "frieda-hip-sys", "src", "lib.rs"))
    assert rs, "not in the Rust extern block"
    assert rs.group(1).count(":") == N_ARGS


def test_a_null_context_is_refused_without_a_device():
    import ctypes as C

    from frieda_amd import _lib

    out = (C.c_uint64 * 4)(9, 9, 9, 9)
    assert _lib.lib().frieda_ctx_test_poison(None, 0, 1, out) == _lib.ERR_ARG
    assert list(out) == [9, 9, 9, 9]


def test_docs_name_the_hook():
    design = _read("DESIGN.md")
    assert HOOK in design and "tests/test_gpu_workspace_history.py" in design
    hdr = _read("include", "frieda_hip_testing.h")
    text = " ".join(re.sub(r"\n \* ?", "\n", hdr[hdr.index("The state a call starts from"):hdr.index("int " + HOOK)]).split())
    for phrase in ("whole workspace arena", "pinned staging block", "pinned input block", "generator scratch", "sticky", "frieda_dev_alloc", "in flight"):
        assert phrase in text, phrase


def scope_names():
    """every name a Scope can carry: the literals of its constructor calls (both arms of a ?:) and the names passed in through PASSED_IN"""
    names = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "frieda_amd", "csrc", "*.hip"))):
        src = open(path).read()
        base = os.path.basename(path)
        for m in re.finditer(r"\bScope\s+\w+\s*\(\s*\w+\s*,\s*([^,]*(?:\?[^,]*)?),", src):
            lits = re.findall(r'"([a-z0-9_]+)"', m.group(1))
            if lits:
                for lit in lits:
                    names.setdefault(lit, base)
            else:
                assert base in PASSED_IN, f"{base}: a Scope takes its name from `{m.group(1).strip()}`: list the call sites in PASSED_IN"
        if base in PASSED_IN:
            fn, listed = PASSED_IN[base]
            found = set()
            for call in re.finditer(r"\b" + fn + r"\s*\(([^;]*)\)\s*;", src):
                found |= set(re.findall(r'"([a-z0-9_]+)"', call.group(1)))
            # (tree.hip picks the name of build_tree's launch in a conditional expression right above the call)
            for m in re.finditer(r"const char\*\s*nm\s*=([^;]*);", src):
                found |= set(re.findall(r'"([a-z0-9_]+)"', m.group(1)))
            assert found == listed, f"{base}: {fn} is called with {sorted(found)}, PASSED_IN lists {sorted(listed)}"
            for lit in listed:
                names.setdefault(lit, base)
    return names


def test_every_kernel_is_claimed_by_a_poisoned_row_or_exempt():
    import workspace_rows as W

    names = scope_names()
    assert len(names) >= 60 and {"small_first", "fri_tail", "erasure_sample_lists", "cells_inverse", "ntt_pass_mid", "tree5_fold_line"} <= set(names)
    claimed = set()
    for row in W.ROWS.values():
        assert row.kernels, "a row names the kernels it must launch"
        claimed |= set(row.kernels)
    assert claimed <= set(names), f"rows claim names no Scope carries: {sorted(claimed - set(names))}"
    assert not (claimed & set(W.EXEMPT)), "exempt and claimed"
    for name, reason in W.EXEMPT.items():
        assert name in names and len(reason) > 20, name
    missing = {n: f for n, f in names.items() if n not in claimed and n not in W.EXEMPT}
    assert not missing, f"kernels without a poisoned row (tests/workspace_rows.py) or an EXEMPT reason: {missing}"


def test_the_table_covers_the_listed_entry_points():
    """the rows the test plan lists, by the prefix of their names"""
    import workspace_rows as W

    for prefix in ("commit/", "commit_device", "commit_batch/", "prove/small_fused", "prove/small_general", "prove/general/host_channel", "prove/general/host_decommit",
                   "prove/grind_retry", "prove_batch/2p11", "prove_batch/2p12", "prove_begin_finish", "prove_seeds/2p16/fold_group", "prove_seeds/2p16/tree_levels_skipped",
                   "unpack30", "pack30", "precompute_twiddles/cache", "precompute_twiddles/no_cache", "evaluate/broadcast", "evaluate/tile", "evaluate/tile12",
                   "fold2/accumulate", "fold2/overwrite", "fold2/accumulate/no_cp", "interpolate", "interpolate/generic", "interpolate_cells/", "interpolate_cells_any",
                   "interpolate_cells/device_solve", "interpolate_points/lines", "interpolate_points/tree", "merkle_commit", "merkle_commit_layer", "merkle_root",
                   "fold_circle_into_line", "fold_line", "bit_reverse_column", "circle_extend", "eval_at_point", "fri_decompose", "grind", "dev_gather_device",
                   "gather_hashes", "decommit_device/small", "decommit_device/multi_block", "verify_many", "verify_many/passes", "verify_pairs_many/passes",
                   "reconstruct_from_proofs", "reconstruct_from_proof_pairs", "open_cells/", "verify_cells_many/passes", "reconstruct_from_opened_cells/",
                   "open_cells_blobs", "verify_cells_blobs_many/passes", "reconstruct_blobs_from_opened_stripes", "reconstruct_blobs_from_opened_stripes/passes"):
        assert any(name.startswith(prefix) for name in W.ROWS), prefix
    assert W.WORDS == (0x00000000, 0xFFFFFFFF, 0x7FFFFFFF)
