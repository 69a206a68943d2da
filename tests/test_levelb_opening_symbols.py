"""Level B openings (frieda_dev_gather*, frieda_merkle_decommit*): the library exports them, the binding declares them, and the
decommitment order the kernels implement (opening.hip: E_s tables, one emit per parent group) is stwo's MerkleProver::decommit walk.

stwo_decommit_walk below is the reference the GPU tests (test_gpu_levelb_opening.py) check the device against: a restatement of the
merge loop of stwo core/vcs/prover.rs for a tree whose only columns sit on the leaf layer (the oracle's merkle_decommit)."""
import random

NEW_SYMBOLS = [
    "frieda_dev_gather",
    "frieda_dev_gather_hashes",
    "frieda_dev_gather_device",
    "frieda_merkle_decommit",
    "frieda_merkle_decommit_device",
]


def stwo_decommit_walk(positions, log_size):
    """MerkleProver::decommit's hash witness as [(layer_log, node)], in output order.  Layers from the leaves up; at each layer the
    nodes are the merge of the parents of the layer below and the column queries of this layer (only the leaf layer has any); for
    each node the left then the right child's hash is pushed unless that child is a node of the layer below."""
    out = []
    last = []
    for layer_log in range(log_size, -1, -1):
        colq = list(positions) if layer_log == log_size else []
        total = []
        pi = ci = 0
        while pi < len(last) or ci < len(colq):
            if pi < len(last) and ci < len(colq):
                node = min(last[pi] // 2, colq[ci])
            elif pi < len(last):
                node = last[pi] // 2
            else:
                node = colq[ci]
            if layer_log < log_size:
                for child in (2 * node, 2 * node + 1):
                    if pi < len(last) and last[pi] == child:
                        pi += 1
                    else:
                        out.append((layer_log + 1, child))
            if ci < len(colq) and colq[ci] == node:
                ci += 1
            total.append(node)
        last = total
    return out


def e_tables_walk(positions, log_size):
    """E_1, ..., E_L with E_s = the children of unique(p >> s) missing from unique(p >> (s - 1)), read at layer L - s + 1."""
    out = []
    for s in range(1, log_size + 1):
        below = set(p >> (s - 1) for p in positions)
        for v in sorted(set(p >> s for p in positions)):
            for child in (2 * v, 2 * v + 1):
                if child not in below:
                    out.append((log_size - s + 1, child))
    return out


def emit_rule_walk(positions, log_size):
    """What each kernel thread decides (opening.hip emit_at): position i emits at level s iff it is the first of its parent group and
    lies in the right child, or the last and lies in the left child; emits are compacted in position order, levels one after another."""
    out = []
    p = list(positions)
    for s in range(1, log_size + 1):
        for i, x in enumerate(p):
            v, bit = x >> s, (x >> (s - 1)) & 1
            first = i == 0 or (p[i - 1] >> s) != v
            last = i + 1 == len(p) or (p[i + 1] >> s) != v
            if first and bit:
                out.append((log_size - s + 1, 2 * v))
            elif last and not bit:
                out.append((log_size - s + 1, 2 * v + 1))
    return out


def hash_bound(n_pos, log_size):
    return sum(min(n_pos, 1 << (log_size - s)) for s in range(1, log_size + 1))


def test_library_exports_the_opening_entry_points():
    from frieda_amd import _lib

    declared = _lib.declared_symbols()
    L = _lib.lib()
    for s in NEW_SYMBOLS:
        assert s in declared, s
        assert hasattr(L, s), s
        assert s in L._signatures, s


def test_context_has_the_opening_methods():
    import frieda_amd

    for m in ("dev_gather", "dev_gather_hashes", "merkle_decommit"):
        assert callable(getattr(frieda_amd.Context, m, None)), m


def test_header_documents_the_route_option():
    """the context option that moves short position lists to the multi-block route is named where the device form is declared"""
    from frieda_amd import _lib

    src = open(_lib.HEADER_PATH).read()
    assert "FRIEDA_OPEN_SMALL_MAX" in src


def _position_sets(rng):
    for _ in range(300):
        L = rng.randint(0, 14)
        kind = rng.choice(["one", "all", "pairs", "random", "ends", "dense"])
        N = 1 << L
        if kind == "one":
            pos = [rng.randrange(N)]
        elif kind == "all":
            pos = list(range(N))
        elif kind == "pairs":
            pos = sorted(set(x for p in rng.sample(range(max(N // 2, 1)), min(5, max(N // 2, 1))) for x in (2 * p, 2 * p + 1) if x < N))
        elif kind == "random":
            pos = sorted(rng.sample(range(N), min(N, rng.choice([1, 2, 3, 20, 64, 300]))))
        elif kind == "ends":
            pos = sorted({0, N - 1})
        else:
            pos = sorted(rng.sample(range(N), rng.randint(1, N)))
        yield L, pos


def test_e_tables_and_the_emit_rule_equal_the_stwo_walk():
    rng = random.Random(11)
    for L, pos in _position_sets(rng):
        ref = stwo_decommit_walk(pos, L)
        assert e_tables_walk(pos, L) == ref, (L, pos)
        assert emit_rule_walk(pos, L) == ref, (L, pos)
        assert len(ref) <= hash_bound(len(pos), L) <= len(pos) * L


def test_walk_edge_cases():
    assert stwo_decommit_walk([0], 0) == []
    assert stwo_decommit_walk(list(range(8)), 3) == []  # every leaf opened: nothing to witness
    # one leaf of four: its sibling, then the other subtree's root
    assert stwo_decommit_walk([2], 2) == [(2, 3), (1, 0)]
    assert stwo_decommit_walk([0, 3], 2) == [(2, 1), (2, 2)]
