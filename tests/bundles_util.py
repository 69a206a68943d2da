"""Shared by the cell-bundle tests: bundles built by the CPU oracle alone (cells_util.codeword, oracle.merkle_commit), stwo's merge walk
restated (per level, per parent in ascending order, push the child that is not known), the emit rule restated apart from it, an
independent acceptance check over merkle_commit_layer, the shapes and the mutation matrix both verifiers are run over.  Nothing here
calls the library under test except the two raw_* wrappers at the end."""
import ctypes as C
import functools

import numpy as np

import cells_util as U
from cells_util import P31, POISON

REJECTED, ACCEPTED, MALFORMED = 0, 1, 2
MAX_BUNDLE_CELLS = 1024
SIZES = (1, 2, 63, 64, 65, 300)


# ---- the witness, stated twice ----------------------------------------------------------------------------------------------------------
def merge_walk(depth, idx):
    """stwo's MerkleProver::decommit on the tree cut at level `depth`: [(tree level, node)] in witness order.  Bottom-up; per level the
    parents of the known nodes in ascending order; of each parent's two children the one that is not known is pushed."""
    known = [int(i) for i in idx]
    out = []
    for level in range(depth, 0, -1):
        have = set(known)
        parents = sorted(set(x >> 1 for x in known))
        for v in parents:
            for child in (2 * v, 2 * v + 1):
                if child not in have:
                    out.append((level, child))
        known = parents
    return out


def emit_tables(depth, idx):
    """The same list from the emit rule of the E_s tables, every level on its own from the positions alone: position i contributes to E_s
    iff it is the first of its group (p >> s) and lies in the right child, or the last and lies in the left child."""
    p = [int(i) for i in idx]
    out = []
    for s in range(1, depth + 1):
        for i, x in enumerate(p):
            v, bit = x >> s, (x >> (s - 1)) & 1
            first = i == 0 or (p[i - 1] >> s) != v
            last = i + 1 == len(p) or (p[i + 1] >> s) != v
            if first and bit:
                out.append((depth - s + 1, 2 * v))
            elif last and not bit:
                out.append((depth - s + 1, 2 * v + 1))
    return out


def witness_oracle(layers, n, c, idx):
    """uint8 [H, 32]: the merge walk's nodes read out of the oracle's tree"""
    nodes = merge_walk(n - c, idx)
    if not nodes:
        return np.zeros((0, 32), dtype=np.uint8)
    return np.stack([layers[level][node] for level, node in nodes])


# ---- shapes -----------------------------------------------------------------------------------------------------------------------------
def pick(n, c, k, seed):
    """k distinct cell indices, ascending"""
    rng = np.random.default_rng(seed + 1009 * n + 31 * c + k)
    return np.sort(rng.choice(1 << (n - c), size=k, replace=False)).astype(np.uint32)


def shape_bundles(n, c):
    """[(label, ascending indices)]: sizes 1, 2, 63, 64, 65, 300 where the domain has that many cells, every cell of the domain (an empty
    witness) where the cap allows it, one adjacent pair, only the first cell, only the last"""
    total = 1 << (n - c)
    out = [(f"k{k}", pick(n, c, k, seed=3)) for k in SIZES if k <= total]
    if total <= MAX_BUNDLE_CELLS:
        out.append(("all", np.arange(total, dtype=np.uint32)))
    if total >= 2:
        a = 2 * int(np.random.default_rng(n + c).integers(0, total // 2))
        out.append(("pair", np.array([a, a + 1], dtype=np.uint32)))
    out.append(("first", np.array([0], dtype=np.uint32)))
    out.append(("last", np.array([total - 1], dtype=np.uint32)))
    return out


class Call:
    """one call: bundles (index lists), values [cells, 4, 2^c], witness [H, 32], witness_first [n_bundles + 1]"""

    def __init__(self, n, c, commitment, bundles, values, witness, wfirst):
        self.n, self.c, self.commitment = n, c, bytes(commitment)
        self.bundles = [np.asarray(b, dtype=np.uint32) for b in bundles]
        self.values, self.witness, self.wfirst = values, witness, np.asarray(wfirst, dtype=np.uint64)

    def replace(self, **kw):
        d = dict(n=self.n, c=self.c, commitment=self.commitment, bundles=self.bundles, values=self.values, witness=self.witness, wfirst=self.wfirst)
        d.update(kw)
        return Call(**d)

    @property
    def first(self):
        return np.concatenate([[0], np.cumsum([len(b) for b in self.bundles])]).astype(np.uint32)


def build_call(ev, layers, c, bundles):
    n = ev.shape[1].bit_length() - 1
    idx = np.concatenate(bundles) if bundles else np.zeros(0, np.uint32)
    values, _ = U.open_oracle(ev, layers, c, idx)
    wits = [witness_oracle(layers, n, c, b) for b in bundles]
    wfirst = np.concatenate([[0], np.cumsum([len(w) for w in wits])]).astype(np.uint64)
    witness = np.concatenate(wits) if wits else np.zeros((0, 32), np.uint8)
    return Call(n, c, layers[0][0].tobytes(), bundles, values, np.ascontiguousarray(witness), wfirst)


@functools.lru_cache(maxsize=None)
def shapes_call(n, b, c):
    """every shape of shape_bundles(n, c) as one call (computed once; callers copy before they mutate)"""
    _, ev, layers, _, _ = U.case(n, b)
    shapes = shape_bundles(n, c)
    return [label for label, _ in shapes], build_call(ev, layers, c, [i for _, i in shapes])


# ---- the independent check ----------------------------------------------------------------------------------------------------------------
def _hash_pairs(pairs):
    """uint8 [m, 2, 32] -> the m parents, by merkle_commit_layer over a power-of-two layer"""
    from oracle import oracle as O

    m = len(pairs)
    mp = 1 << max(0, (m - 1).bit_length())
    prev = np.zeros((2 * mp, 32), dtype=np.uint8)
    prev[: 2 * m] = pairs.reshape(2 * m, 32)
    return O.merkle_commit_layer(mp.bit_length() - 1, prev, None)[:m]


def _cell_roots(c, values):
    from oracle import oracle as O

    k = len(values)
    kp = 1 << max(0, (k - 1).bit_length())
    cols = np.zeros((4, kp << c), dtype=np.uint32)
    cols[:, : k << c] = values.transpose(1, 0, 2).reshape(4, -1)
    lg = (kp << c).bit_length() - 1
    h = O.merkle_commit_layer(lg, None, cols)
    for _ in range(c):
        lg -= 1
        h = O.merkle_commit_layer(lg, h, None)
    return h[:k]


def malformed(n, c, idx, n_witness):
    k = len(idx)
    if k == 0 or k > MAX_BUNDLE_CELLS:
        return True
    p = [int(i) for i in idx]
    if any(x >> (n - c) for x in p) or any(a >= b for a, b in zip(p, p[1:])):
        return True
    return len(merge_walk(n - c, p)) != n_witness


def independent_status(call):
    """The acceptance rule restated: malformed by the rule of the header; else every word canonical and stwo's MerkleVerifier::verify
    (the merge walk from the verifier's side, one merkle_commit_layer per level) gives the commitment with the witness used up."""
    out = []
    first = call.first
    values = np.asarray(call.values, dtype=np.uint32).reshape(-1, 4, 1 << call.c)
    want = np.frombuffer(call.commitment, dtype=np.uint8)
    for b, idx in enumerate(call.bundles):
        w0, w1 = int(call.wfirst[b]), int(call.wfirst[b + 1])
        if w1 < w0 or malformed(call.n, call.c, idx, w1 - w0):
            out.append(MALFORMED)
            continue
        v = values[first[b]:first[b + 1]]
        wit = call.witness[w0:w1]
        ok = bool((v < P31).all())
        known = [int(i) for i in idx]
        h = {x: r for x, r in zip(known, _cell_roots(call.c, v))}
        used = 0
        for _ in range(call.n - call.c):
            parents = sorted(set(x >> 1 for x in known))
            pairs = np.zeros((len(parents), 2, 32), dtype=np.uint8)
            for j, p in enumerate(parents):
                for side, child in enumerate((2 * p, 2 * p + 1)):
                    if child in h:
                        pairs[j, side] = h[child]
                    else:
                        pairs[j, side] = wit[used]
                        used += 1
            h = dict(zip(parents, _hash_pairs(pairs)))
            known = parents
        ok = ok and used == len(wit) and known == [known[0]] and (h[known[0]] == want).all()
        out.append(ACCEPTED if ok else REJECTED)
    return np.array(out, dtype=np.uint8)


# ---- the mutation matrix ------------------------------------------------------------------------------------------------------------------
def small_call(n, b, c):
    """three bundles of 5, 2 and 9 cells (fewer where the domain is smaller); the first is the one the matrix mutates"""
    _, ev, layers, _, _ = U.case(n, b)
    total = 1 << (n - c)
    sizes = [min(k, total) for k in (5, 2, 9)]
    return build_call(ev, layers, c, [pick(n, c, k, seed=40 + j) for j, k in enumerate(sizes)])


def _with_witness(call, b, new_rows):
    """bundle b's witness replaced by new_rows; the later bundles keep theirs"""
    w0, w1 = int(call.wfirst[b]), int(call.wfirst[b + 1])
    witness = np.concatenate([call.witness[:w0], new_rows, call.witness[w1:]])
    wfirst = call.wfirst.astype(np.int64).copy()
    wfirst[b + 1:] += len(new_rows) - (w1 - w0)
    return call.replace(witness=np.ascontiguousarray(witness), wfirst=wfirst.astype(np.uint64))


def mutations(call, seed=7):
    """[(label, mutated bundles, must_be_malformed, call')]: one word of the values; one byte of every witness hash of bundle 0; one index
    moved keeping the order; one index repeated; one index out of range; the witness one hash short and one long; the witnesses of
    bundles 0 and 1 swapped."""
    n, c = call.n, call.c
    rng = np.random.default_rng(seed + 17 * n + c)
    out = []
    idx0 = call.bundles[0]
    k0 = len(idx0)
    v = call.values.copy()
    t, col, j = int(rng.integers(0, k0)), int(rng.integers(0, 4)), int(rng.integers(0, 1 << c))
    v[t, col, j] = (int(v[t, col, j]) + 1) % P31
    out.append(("word", [0], False, call.replace(values=v)))
    for hsh in range(int(call.wfirst[1])):
        w = call.witness.copy()
        w[hsh, int(rng.integers(0, 32))] ^= 1 << int(rng.integers(0, 8))
        out.append((f"hash{hsh}", [0], False, call.replace(witness=w)))
    # an index moved to a free neighbour value, keeping the order
    p = [int(x) for x in idx0]
    for i in range(k0):
        lo = p[i - 1] + 1 if i else 0
        hi = p[i + 1] - 1 if i + 1 < k0 else (1 << (n - c)) - 1
        free = [x for x in (p[i] - 1, p[i] + 1) if lo <= x <= hi]
        if free:
            moved = idx0.copy()
            moved[i] = free[0]
            out.append(("moved", [0], False, call.replace(bundles=[moved] + call.bundles[1:])))
            break
    if k0 >= 2:
        rep = idx0.copy()
        rep[1] = rep[0]
        out.append(("repeated", [0], True, call.replace(bundles=[rep] + call.bundles[1:])))
    oor = idx0.copy()
    oor[-1] = 1 << (n - c)
    out.append(("out_of_range", [0], True, call.replace(bundles=[oor] + call.bundles[1:])))
    w0 = call.witness[: int(call.wfirst[1])]
    if len(w0):
        out.append(("short", [0], True, _with_witness(call, 0, w0[:-1])))
    out.append(("long", [0], True, _with_witness(call, 0, np.concatenate([w0, np.full((1, 32), 0x5A, np.uint8)]))))
    if len(call.bundles) >= 2 and int(call.wfirst[2]) > 0:
        w1 = call.witness[int(call.wfirst[1]):int(call.wfirst[2])]
        if not (len(w0) == len(w1) and (w0 == w1).all()):
            swapped = _with_witness(_with_witness(call, 1, w0), 0, w1)
            out.append(("swapped", [0, 1], len(w0) != len(w1), swapped))
    return out


def check_mutation(label, hit, must_be_malformed, want, n_bundles):
    """what the independent check must say about a mutated call before a verifier is asked"""
    for b in range(n_bundles):
        if b in hit:
            assert want[b] != ACCEPTED, (label, b)
            if must_be_malformed:
                assert want[b] == MALFORMED, (label, b)
        else:
            assert want[b] == ACCEPTED, (label, b)


# ---- the library under test ---------------------------------------------------------------------------------------------------------------
def raw_verify(call, ctx=None):
    """frieda_verify_cell_bundles (ctx None) or frieda_verify_cell_bundles_many into a poison-filled status array: (rc, status)"""
    from frieda_amd import _lib

    L = _lib.lib()
    idx = np.ascontiguousarray(np.concatenate(call.bundles) if call.bundles else np.zeros(1, np.uint32), dtype=np.uint32)
    first = np.ascontiguousarray(call.first, dtype=np.uint32)
    values = np.ascontiguousarray(call.values, dtype=np.uint32)
    witness = np.ascontiguousarray(call.witness, dtype=np.uint8)
    wfirst = np.ascontiguousarray(call.wfirst, dtype=np.uint64)
    nb = len(call.bundles)
    status = np.full(nb + 8, POISON, dtype=np.uint8)
    com = (C.c_uint8 * 32)(*call.commitment)
    args = (com, call.n, call.c, idx.ctypes.data, first.ctypes.data, nb, values.ctypes.data if values.size else None,
            witness.ctypes.data if witness.size else None, wfirst.ctypes.data, status.ctypes.data)
    rc = L.frieda_verify_cell_bundles(*args) if ctx is None else L.frieda_verify_cell_bundles_many(ctx._h, *args)
    assert (status[nb:] == POISON).all(), "red zone behind out_status"
    return rc, status[:nb]


def witness_count(n, c, idx):
    from frieda_amd import _lib

    idx = np.ascontiguousarray(idx, dtype=np.uint32)
    out = C.c_size_t(0xDEAD)
    rc = _lib.lib().frieda_cell_bundle_witness_count(n, c, idx.ctypes.data if idx.size else None, len(idx), C.byref(out))
    return rc, out.value
