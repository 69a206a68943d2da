"""The buffer-contract table of tests/test_gpu_buffer_contract.py against include/frieda_hip.h (no GPU): every device-pointer parameter of
the C ABI is either a row of the table, with a role and an alignment class, or listed in EXEMPT with the reason it needs no
red-zone run.  A new entry point with a device pointer fails here until someone classifies it."""
import os
import re

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "frieda_hip.h")

CONTRACT = ("A device pointer to words needs 4-byte alignment, a pointer to bytes none, and a pointer to hashes 16 bytes, unless the function "
            "says otherwise. No call writes outside the extents it documents. No call modifies a `const` argument.")

# (function, parameter) -> why it has no row
EXEMPT = {
    ("frieda_dev_alloc", "d_out"): "host pointer that receives the allocation's address",
    ("frieda_dev_free", "d"): "handed back to the allocator, never dereferenced by a kernel",
    ("frieda_dev_upload", "d_dst"): "a hipMemcpy destination: the harness itself is built on it (and its self-test plants bytes with it)",
    ("frieda_dev_download", "d_src"): "a hipMemcpy source: every zone check goes through it",
    ("frieda_dev_at", "d_col"): "one 4-byte hipMemcpy to the host, no kernel",
    ("frieda_dev_at_secure", "d_cols"): "one strided hipMemcpy2D to the host, no kernel",
    ("frieda_dev_gather", "d_cols"): "host form of frieda_dev_gather_device (same kernel, results staged through the workspace): the device form has the row",
    ("frieda_merkle_decommit", "d_layers"): "host form of frieda_merkle_decommit_device: same kernels, outputs in host memory",
    ("frieda_merkle_decommit", "d_cols"): "host form of frieda_merkle_decommit_device: same kernels, outputs in host memory",
    ("frieda_precompute_twiddles", "d_twiddles"): "host pointer that receives the address of a table the context owns",
    ("frieda_precompute_twiddles", "d_inv_twiddles"): "host pointer that receives the address of a table the context owns",
    ("frieda_prove_begin_device", "d_data"): "the first half of frieda_commit_and_generate_proof_device, which has the row",
    ("frieda_commit_and_generate_proof_batch_device", "d_data"): "frieda_prove_batch_begin_device + _finish, which has the row",
    ("frieda_encode_device", "d_data"): "the unpack and encode launches of frieda_commit_device on the same pointer, which has the row",
}

DECL = re.compile(r"^(?:int|size_t|uint32_t|uint64_t|void|const char\*|frieda_ctx\*|frieda_pcs_config|uint32_t\*|const uint8_t\*|const uint32_t\*)\s+(frieda_\w+)\(([^;{]*?)\);", re.M | re.S)


def device_pointer_params():
    """{(function, parameter)} of the header: parameters that are pointers and are named d or d_*"""
    with open(HEADER) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    found, functions = set(), set()
    for m in DECL.finditer(text):
        fn, args = m.group(1), m.group(2)
        functions.add(fn)
        for a in args.split(","):
            a = a.strip()
            pm = re.match(r"^(.*?\*+)\s*(?:const\s+)?(\w+)(?:\[\d*\])?$", a)
            if pm and re.fullmatch(r"d|d_\w+", pm.group(2)):
                found.add((fn, pm.group(2)))
    return found, functions


def table_pairs(variants=True):
    from test_gpu_buffer_contract import OFFSETS, TABLE

    pairs = {}
    for key, params in TABLE.items():
        fn = key.split("[")[0]
        if fn != key and not variants:
            continue  # an aliasing variant of a function that has its plain row (d_g = d_eval: the const pointer is also the output)
        for p, (role, cls) in params.items():
            assert role in ("in", "out", "inout") and cls in OFFSETS, (key, p, role, cls)
            pairs[(fn, p)] = (role, cls)
    return pairs


def test_the_parser_sees_the_abi():
    found, functions = device_pointer_params()
    assert len(functions) > 90, len(functions)  # the header declares ~100 functions: the pattern must not silently stop matching
    for known in (("frieda_fold_line", "d_src"), ("frieda_merkle_decommit_device", "d_n_hashes"), ("frieda_dev_free", "d"),
                  ("frieda_commit_device", "d_out_root"), ("frieda_circle_evaluate_fold2", "d_line2")):
        assert known in found, known


def test_every_device_pointer_is_classified_or_exempt():
    found, _ = device_pointer_params()
    pairs = table_pairs()
    missing = sorted(p for p in found if p not in pairs and p not in EXEMPT)
    assert not missing, f"device-pointer parameters with neither a row in test_gpu_buffer_contract.TABLE nor an exemption: {missing}"
    both = sorted(p for p in pairs if p in EXEMPT)
    assert not both, f"classified and exempt at once: {both}"
    for p, reason in EXEMPT.items():
        assert isinstance(reason, str) and reason.strip() and "\n" not in reason, p


def test_table_and_exemptions_name_only_what_the_header_declares():
    found, _ = device_pointer_params()
    stale = sorted(p for p in list(table_pairs()) + list(EXEMPT) if p not in found)
    assert not stale, f"not device-pointer parameters of the header (renamed or removed?): {stale}"


def test_const_parameters_are_inputs():
    """a parameter the header declares `const` cannot have the role out / inout, and the other way round"""
    with open(HEADER) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    for (fn, p), (role, _) in table_pairs(variants=False).items():
        m = re.search(rf"\b{fn}\((?:[^;]*?,)?\s*((?:const\s+)?\w+\s*\*(?:\s*const\s*\*)?)\s*{p}\s*[,)]", text, flags=re.S)
        assert m, (fn, p)
        assert m.group(1).startswith("const") == (role == "in"), (fn, p, role, m.group(1))


def test_header_states_the_contract():
    with open(HEADER) as f:
        text = f.read()
    assert CONTRACT in text
    assert text.index(CONTRACT) > text.index("---- Level B: backend-trait granular operations")
    assert text.index(CONTRACT) < text.index("int frieda_dev_alloc(")


# pointer parameters NOT named d / d_* whose preceding comment puts their name and the word "device" into one sentence: host memory
# all the same, each with the reason
HOST_DESPITE_THE_COMMENT = {}


def test_no_device_pointer_hides_under_another_name():
    """The classification above goes by the naming rule (device pointers are called d or d_*).  A `void*` / `uint32_t*` / `uint8_t*` /
    `uint64_t*` parameter under another name whose comment speaks of device memory in the same sentence as its name would slip past
    it: none may exist outside HOST_DESPITE_THE_COMMENT."""
    with open(HEADER) as f:
        suspects = _device_by_comment(f.read())
    suspects = [x for x in suspects if (x[0], x[1]) not in HOST_DESPITE_THE_COMMENT]
    assert not suspects, f"pointer parameters documented as device memory but not named d_*: {suspects}"
    # the guard itself: a declaration of that kind is found, the same comment about a host array is not
    fake = "/* cols: the columns in device memory, n words each. */\nint frieda_fake(frieda_ctx* ctx, const uint32_t* cols, size_t n);\n"
    assert [x[:2] for x in _device_by_comment(fake)] == [("frieda_fake", "cols")]
    assert not _device_by_comment(fake.replace("in device memory", "(host)"))


def _device_by_comment(raw):
    suspects = []
    for m in re.finditer(r"((?:/\*(?:(?!\*/).)*\*/\s*)+)(?:int|size_t|uint32_t|uint64_t|void)\s+(frieda_\w+)\(([^;{]*?)\);", raw, flags=re.S):
        comment, fn, args = m.group(1), m.group(2), m.group(3)
        sentences = re.split(r"(?<=[.;])\s+|\n\s*\*\s*\n", comment)
        for a in args.split(","):
            pm = re.match(r"^\s*(?:const\s+)?(void|uint32_t|uint8_t|uint64_t)\s*\*+\s*(?:const\s+)?(\w+)(?:\[\d*\])?\s*$", a)
            if not pm or re.fullmatch(r"d|d_\w+", pm.group(2)):
                continue
            name = pm.group(2)
            for sen in sentences:
                if re.search(rf"\b{name}\b", sen) and re.search(r"\bdevice (?:memory|buffer|pointer|array)|\bon the device\b|\bin device\b", sen) \
                        and not re.search(rf"\b{name}\b[^,()]*\(host", sen) and "host" not in sen.split(name, 1)[1][:40]:
                    suspects.append((fn, name, " ".join(sen.split())[:120]))
                    break
    return suspects
