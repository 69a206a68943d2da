"""CPU: frieda_verify_pairs (the host verifier's pair points) on oracle-made proofs, against a restatement written from the proof's
accessors (pairs_util.restate) and against the oracle's own encode of the blob."""
import ctypes as C

import numpy as np
import pytest

from conftest import pattern_bytes
from pairs_util import ERR_ARG, ERR_INVARIANT, restate

INPUTS = {"blob": (None, None, 4), "p1024": (pattern_bytes(1024).tobytes(), 1024, 4), "small": (pattern_bytes(300).tobytes(), 9, 2)}


@pytest.fixture(scope="module")
def proofs(oracle, blob):
    import __graft_entry__ as g

    g.build()
    import frieda_amd

    cfgs = {"blob": oracle.make_config(20, 4, 1, 20), "p1024": oracle.make_config(20, 4, 0, 20), "small": oracle.make_config(8, 2, 1, 12)}
    out = {}
    for name, (data, seed, B) in INPUTS.items():
        data = blob if data is None else data
        _, op = oracle.commit_and_generate_proof(data, seed, cfgs[name])
        out[name] = (data, seed, B, frieda_amd.Proof.deserialize(op.serialize()))
    return out


@pytest.mark.parametrize("name", sorted(INPUTS))
def test_pair_points_equal_the_restatement_and_the_codeword(oracle, proofs, name):
    import frieda_amd

    data, seed, B, p = proofs[name]
    ok, pos, val = frieda_amd.verify_pairs(p, seed)
    assert ok
    rpos, rval = restate(p, seed)
    assert np.array_equal(pos, rpos) and np.array_equal(val, rval)
    assert np.all(np.diff(pos.astype(np.int64)) > 0), "ascending and distinct"
    _, q = frieda_amd.verify_samples(p, seed)
    assert len(q) < len(pos) <= 2 * len(q) and set(pos.tolist()) == set(q.tolist()) | set((q ^ 1).tolist())
    assert np.array_equal(val[np.searchsorted(pos, q)], p.evaluations), "a queried position holds the proof's evaluation"
    coef, lg = oracle.polynomial_from_bytes(data)
    ev = oracle.circle_evaluate(coef, lg + B)
    assert np.array_equal(ev[:, pos].T, val), "a sibling value is not the codeword's"


def test_rejected_proof_gives_no_points(proofs):
    import frieda_amd

    _, seed, _, p = proofs["p1024"]
    assert frieda_amd.verify_pairs(p, 777) == (False, None, None)
    L = frieda_amd._lib.lib()
    ok, n = C.c_int(1), C.c_size_t(99)
    pos, val = np.full(40, 7, np.uint32), np.full(160, 7, np.uint32)
    assert L.frieda_verify_pairs(p._h, C.byref(C.c_uint64(777)), C.byref(ok), pos.ctypes.data, val.ctypes.data, 40, C.byref(n)) == 0
    assert ok.value == 0 and n.value == 0 and np.all(pos == 7) and np.all(val == 7)


def test_cap_one_short_and_null_arguments(proofs):
    import frieda_amd

    _, seed, _, p = proofs["p1024"]
    _, rpos, _ = frieda_amd.verify_pairs(p, seed)
    L = frieda_amd._lib.lib()
    ok, n = C.c_int(0), C.c_size_t(0)
    cap = len(rpos) - 1
    pos, val = np.full(cap, 7, np.uint32), np.full(4 * cap, 7, np.uint32)
    sp = C.byref(C.c_uint64(seed))
    assert L.frieda_verify_pairs(p._h, sp, C.byref(ok), pos.ctypes.data, val.ctypes.data, cap, C.byref(n)) == ERR_ARG
    assert ok.value == 1 and n.value == len(rpos) and np.all(pos == 7) and np.all(val == 7)
    assert L.frieda_verify_pairs(p._h, sp, C.byref(ok), pos.ctypes.data, val.ctypes.data, cap + 1, None) == ERR_ARG
    assert L.frieda_verify_pairs(None, sp, C.byref(ok), pos.ctypes.data, val.ctypes.data, cap, C.byref(n)) == ERR_ARG
    assert L.frieda_verify_pairs(p._h, sp, C.byref(ok), pos.ctypes.data, None, cap, C.byref(n)) == ERR_ARG


def test_truncated_evaluations_are_an_invariant_failure(proofs):
    import frieda_amd

    _, seed, _, base = proofs["p1024"]
    p = base.clone()
    p.evaluations = p.evaluations[:-1]
    with pytest.raises(frieda_amd.FriedaPanic):
        frieda_amd.verify_pairs(p, seed)
    # one evaluation too many: frieda_verify accepts it, the sample forms do not (the rule of frieda_verify_samples)
    p = base.clone()
    p.evaluations = np.concatenate([p.evaluations, p.evaluations[:1]])
    assert frieda_amd.verify(p, seed)
    L = frieda_amd._lib.lib()
    ok, n = C.c_int(0), C.c_size_t(5)
    pos, val = np.zeros(64, np.uint32), np.zeros(256, np.uint32)
    assert L.frieda_verify_pairs(p._h, C.byref(C.c_uint64(seed)), C.byref(ok), pos.ctypes.data, val.ctypes.data, 64, C.byref(n)) == ERR_INVARIANT
    assert n.value == 0
