"""Shared by the authenticated-cells tests: openings built by the CPU oracle alone (codeword from polynomial_from_bytes + circle_evaluate,
tree from merkle_commit, a cell's path read out of those layers), an independent acceptance check that recomputes every subtree and
path with merkle_commit_layer, and the mutation matrix both verifiers are run over.  Nothing here calls the library under test."""
import functools

import numpy as np

from conftest import splitmix64_bytes

P31 = (1 << 31) - 1
ERR_ARG = 1
REJECTED, ACCEPTED = 0, 1
POISON = 0xEE

# (log_domain, log_blowup_factor) -> blob length whose polynomial has 2^(log_domain - log_blowup_factor) coefficients per column
BLOB_LEN = {(5, 1): 200, (5, 4): 20, (11, 1): 12000, (11, 4): 1024, (12, 1): 24000, (12, 4): 3000}
HOST_CASES = [(n, b, c) for (n, b) in sorted(BLOB_LEN) for c in sorted({0, 1, 3, 6, n if n <= 10 else 0}) if c <= min(n, 10)]


@functools.lru_cache(maxsize=None)
def _codeword_cached(length, blowup, seed):
    from oracle import oracle as O

    O.build()
    data = splitmix64_bytes(seed, length).tobytes()
    coef, L = O.polynomial_from_bytes(data)
    n = L + blowup
    ev = O.circle_evaluate(coef, n)
    layers = O.merkle_commit(ev)
    ev.setflags(write=False)
    return data, ev, layers, n, L


def codeword(length, blowup, seed=None):
    """(data, evaluation [4, 2^n] in bit-reversed order, tree layers (layers[0] = root), n, L) of a splitmix blob — computed once"""
    return _codeword_cached(length, blowup, 9100 + length if seed is None else seed)


def case(log_domain, blowup):
    data, ev, layers, n, L = codeword(BLOB_LEN[(log_domain, blowup)], blowup)
    assert n == log_domain, (n, log_domain)
    return data, ev, layers, n, L


def open_oracle(ev, layers, c, idx):
    """values [k, 4, 2^c] and paths [k, n - c, 32] (bottom-up) of the cells `idx`, read out of the oracle's codeword and tree"""
    n = ev.shape[1].bit_length() - 1
    idx = np.asarray(idx, dtype=np.int64)
    values = np.stack([ev[:, (i << c):((i + 1) << c)] for i in idx]).astype(np.uint32) if len(idx) else np.zeros((0, 4, 1 << c), np.uint32)
    paths = np.zeros((len(idx), n - c, 32), dtype=np.uint8)
    for s in range(n - c):
        paths[:, s, :] = layers[n - c - s][(idx >> s) ^ 1]
    return np.ascontiguousarray(values), paths


def independent_status(commitment, n, c, idx, values, paths):
    """The acceptance rule restated over merkle_commit_layer: every word canonical, the subtree over the cell's leaves hashed level by
    level, carried up the path (left child when bit s of the index is 0), compared with the commitment.  All cells of the call are
    batched into power-of-two layers; a cell's result depends on its own row only."""
    from oracle import oracle as O

    idx = np.asarray(idx, dtype=np.int64)
    k = len(idx)
    if k == 0:
        return np.zeros(0, dtype=np.uint8)
    values = np.asarray(values, dtype=np.uint32).reshape(k, 4, 1 << c)
    paths = np.asarray(paths, dtype=np.uint8).reshape(k, n - c, 32)
    kp = 1 << max(0, (k - 1).bit_length())
    cols = np.zeros((4, kp << c), dtype=np.uint32)
    cols[:, : k << c] = values.transpose(1, 0, 2).reshape(4, -1)
    lg = (kp << c).bit_length() - 1
    h = O.merkle_commit_layer(lg, None, cols)
    for _ in range(c):
        lg -= 1
        h = O.merkle_commit_layer(lg, h, None)
    assert h.shape[0] == kp
    for s in range(n - c):
        prev = np.zeros((2 * kp, 32), dtype=np.uint8)
        right = ((idx >> s) & 1).astype(bool)  # this node is the right child
        sib = paths[:, s, :]
        prev[0 : 2 * k : 2] = np.where(right[:, None], sib, h[:k])
        prev[1 : 2 * k : 2] = np.where(right[:, None], h[:k], sib)
        h = O.merkle_commit_layer(kp.bit_length() - 1, prev, None)
    canonical = (values.reshape(k, -1) < P31).all(axis=1)
    same = (h[:k] == np.frombuffer(bytes(commitment), dtype=np.uint8)[None, :]).all(axis=1)
    return (canonical & same).astype(np.uint8)


def cell_list(n, c, count, seed=1):
    """`count` cell indices: the first and the last cell, unsorted, with a repeat when there is room"""
    total = 1 << (n - c)
    rng = np.random.default_rng(seed + 131 * n + c)
    idx = rng.integers(0, total, size=count, dtype=np.int64)
    idx[0] = total - 1
    if count > 1:
        idx[-1] = 0
    if count > 3:
        idx[2] = idx[1]
    return idx.astype(np.uint32)


def mutations(n, c, idx, values, paths, seed=5):
    """The mutation matrix: (label, target cell, idx', values', paths') — one word of the values, one byte of each path entry, and the
    index moved to another in-range cell (where the domain has more than one cell)."""
    rng = np.random.default_rng(seed + 17 * n + c)
    k = len(idx)
    out = []
    t = int(rng.integers(0, k))
    v = values.copy()
    col, j = int(rng.integers(0, 4)), int(rng.integers(0, 1 << c))
    v[t, col, j] = (int(v[t, col, j]) + 1) % P31
    out.append(("word", t, idx, v, paths))
    for s in range(n - c):
        t = int(rng.integers(0, k))
        p = paths.copy()
        p[t, s, int(rng.integers(0, 32))] ^= 1 << int(rng.integers(0, 8))
        out.append((f"path{s}", t, idx, values, p))
    if n > c:
        t = int(rng.integers(0, k))
        i2 = idx.copy()
        i2[t] = (int(idx[t]) + 1 + int(rng.integers(0, (1 << (n - c)) - 1))) % (1 << (n - c))
        assert i2[t] != idx[t]
        out.append(("index", t, i2, values, paths))
    return out
