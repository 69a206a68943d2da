"""Shared by the encoded-block GPU tests: what "handle X is indistinguishable from frieda_encode of the same bytes" means, measured
through the calls that take a handle.  The reference of every comparison is the lone frieda_encode handle of the bytes (facts_of_bytes,
computed once per (bytes, blowup) and kept)."""
import numpy as np

import frieda_amd

_facts = {}


def pcs(blowup):
    return frieda_amd.PcsConfig(frieda_amd.FriConfig(log_blowup_factor=blowup, log_last_layer_degree_bound=0, n_queries=20), 8)


SEEDS = [0, 7, 0xFFFFFFFFFFFFFFFF]


def facts(ctx, enc, prove=True):
    """everything a caller can learn from a handle: commitment, shape, open_cells at log_cell 0 and 3 (every cell of the domain up to 2^13
    points, 300 seeded cells above), one seeded cell bundle, and three proofs as serialised bytes"""
    L, n = enc.shape
    out = {"commitment": enc.commitment, "shape": (L, n), "nbytes": enc.nbytes}
    rng = np.random.default_rng(1000 + n)
    for c in (0, 3):
        if c > n:
            continue
        total = 1 << (n - c)
        idx = np.arange(total, dtype=np.uint32) if n <= 13 else rng.choice(total, size=300, replace=False).astype(np.uint32)
        v, p = enc.open_cells(ctx, c, idx)
        out["cells%d" % c] = (v.tobytes(), p.tobytes())
    total = 1 << n
    bundle = np.sort(rng.choice(total, size=min(64, total), replace=False)).astype(np.uint32)
    v, w, wf = enc.open_cell_bundles(ctx, 0, [bundle])
    out["bundle"] = (v.tobytes(), w.tobytes(), wf.tolist())
    if prove:
        out["proofs"] = [p.serialize() for p in ctx.prove_seeds(enc, SEEDS, pcs(enc.log_blowup_factor))]
    return out


def facts_of_bytes(ctx, data, blowup, prove=True):
    """the facts of H0 = frieda_encode(data) on a context with default options; computed once"""
    key = (bytes(data), blowup, prove)
    if key not in _facts:
        enc = ctx.encode(data, blowup)
        try:
            _facts[key] = facts(ctx, enc, prove)
        finally:
            enc.close()
    return _facts[key]


def assert_same(got, want, what=""):
    assert set(got) == set(want), what
    for k in want:
        assert got[k] == want[k], (what, k)


def call(fn, *args, **kw):
    """a reconstruct_* / rebuild_encoded_* method -> (status code, bytes, status array, n_used, handles): the exception of a failed call
    unfolded, so that a twin and its new call compare field by field"""
    try:
        r = fn(*args, **kw)
    except frieda_amd.FriedaError as e:
        st = getattr(e, "cell_status", None)
        if st is None:
            st = e.bundle_status
        used = getattr(e, "n_cells_used", None)
        if used is None:
            used = e.n_stripes_used
        return e.status, None, np.asarray(st).copy(), used, None
    if len(r) == 3:
        return 0, r[0], np.asarray(r[1]).copy(), r[2], None
    encs = r[3] if isinstance(r[3], list) else [r[3]]
    return 0, r[0], np.asarray(r[1]).copy(), r[2], encs


def close_all(encs):
    for e in encs or []:
        e.close()
