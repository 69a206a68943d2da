"""Shared by the frieda_verify_pairs* tests: the restatement of what an accepted proof authenticates, written from the proof's accessors
alone, and a raw call of frieda_verify_pairs_many into sentinel-filled buffers."""
import ctypes as C

import numpy as np

ERR_ARG, ERR_INVARIANT = 1, 3
REJECTED, ACCEPTED, INVARIANT, WRONG_COMMITMENT = 0, 1, 2, 3
SENTINEL = 0xA5A5A5A5


def restate(proof, seed):
    """(positions, values) of both members of every first-layer pair the proof opened, or None unless verify_samples accepts it: a queried
    position takes its value from `evaluations`; a sibling q ^ 1 that was not queried takes the next entry of layer(0)'s fri_witness."""
    import frieda_amd

    try:
        ok, q = frieda_amd.verify_samples(proof, seed)
    except frieda_amd.FriedaPanic:
        return None
    if not ok:
        return None
    ev = proof.evaluations
    fw = proof.layer(0)["fri_witness"]
    assert len(q) == len(ev)
    queried = {int(x): ev[i] for i, x in enumerate(q)}
    pts, wi = {}, 0
    for v in sorted({x >> 1 for x in queried}):
        for pos in (2 * v, 2 * v + 1):
            if pos in queried:
                pts[pos] = queried[pos]
            else:
                pts[pos] = fw[wi]
                wi += 1
    assert wi == len(fw), "the restatement does not use the first layer's witness exactly"
    pos = np.array(sorted(pts), dtype=np.uint32)
    return pos, np.stack([pts[int(p)] for p in pos]).astype(np.uint32)


def distinct_counts(proofs, seeds):
    """(distinct queried positions, distinct pair points) over the accepted proofs, from the restatement"""
    import frieda_amd

    queried, points = set(), set()
    for p, s in zip(proofs, seeds):
        r = restate(p, s)
        if r is None:
            continue
        queried.update(frieda_amd.verify_samples(p, s)[1].tolist())
        points.update(r[0].tolist())
    return len(queried), len(points)


def raw_pairs_many(ctx, proofs, seeds, commitment=None, pitch=None):
    """frieda_verify_pairs_many into buffers filled with SENTINEL: (rc, status, positions [count, pitch], values [count, pitch, 4], counts)"""
    count = len(proofs)
    if pitch is None:
        pitch = 2 * max(int(p.pcs_config.fri_config.n_queries) for p in proofs)
    status = np.full(count, 0xEE, dtype=np.uint8)
    pos = np.full((count, pitch), SENTINEL, dtype=np.uint32)
    val = np.full((count, pitch, 4), SENTINEL, dtype=np.uint32)
    npts = np.full(count, SENTINEL, dtype=np.uint32)
    arr = (C.c_void_p * count)(*[p._h.value if isinstance(p._h, C.c_void_p) else p._h for p in proofs])
    sd = (C.c_uint64 * count)(*seeds) if seeds is not None else None
    com = (C.c_uint8 * 32)(*commitment) if commitment is not None else None
    rc = ctx._L.frieda_verify_pairs_many(ctx._h, arr, sd, count, com, status.ctypes.data, pos.ctypes.data, val.ctypes.data, pitch, npts.ctypes.data)
    return rc, status, pos, val, npts
