"""CPU: the size of the last FRI layer through the product's host verifier, against the oracle.

`last` = log_last_layer_degree_bound runs over 0 .. 13 (np = 2^last = 1 .. 8192 coefficients of last_layer_poly), at blow-ups 2^0, 2^1 and
2^4 and L = last + 1 (no inner layer: the reference's verifier panics), last + 2 and last + 4, every domain <= 2^17.  The oracle makes the
proofs; the product reads their wire image (Proof.deserialize) and must give the oracle's verdict or panic under the right seed and under
a wrong one, and sample the oracle's positions.  Then last_layer_poly is edited — coefficient bumps at both ends and around the middle, a
swap, truncation to np / 2, extension to 2 np — and the product's status must again be the oracle's, and never "accepted".

tests/test_gpu_last_layer.py feeds the same edits (EDITS, edited_proof) to the device verifier.
"""
import ctypes as C

import numpy as np
import pytest

from conftest import splitmix64_bytes

P = 2**31 - 1
REJECTED, ACCEPTED, INVARIANT = 0, 1, 2
NQ, POW = 24, 3
SEED, WRONG_SEED = 77, 78


def exact_len(L):
    """Bytes whose 30-bit felts exactly fill 4 columns of 2^L coefficients (tests/test_gpu_shapes.py has the same helper; that module
    is marked gpu as a whole, this one is not)."""
    return (4 << L) * 30 // 8


CASES = [(last, B, L) for last in range(14) for B in (0, 1, 4) for L in (last + 1, last + 2, last + 4) if 2 <= L + B <= 17]


def test_the_grid_is_what_the_module_claims():
    assert {c[0] for c in CASES} == set(range(14))
    assert {c[2] - c[0] - 1 for c in CASES} == {0, 1, 3}  # inner layers
    assert max(L + B for _, B, L in CASES) == 17 and min(L + B for _, B, L in CASES) == 2
    assert {last + B for last, B, _ in CASES} >= set(range(0, 16))  # log size of the last layer's domain: both sides of 11 / 12


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build()
    from frieda_amd import _lib

    return _lib.lib()


def blob_of(last, B, L):
    return splitmix64_bytes(9000 + 64 * last + 8 * B + (L - last), exact_len(L) - 3).tobytes()


@pytest.fixture(scope="module")
def proofs(oracle, lib):
    """(last, B, L) -> (oracle proof, the product's Proof from its wire image), made on first use and then left alone"""
    import frieda_amd

    made = {}

    def get(last, B, L):
        key = (last, B, L)
        if key not in made:
            root, op = oracle.commit_and_generate_proof(blob_of(last, B, L), SEED, oracle.make_config(POW, B, last, NQ))
            img = op.serialize()
            p = frieda_amd.Proof.deserialize(img)
            assert p.serialize() == img and p.commitment == root and p.log_size_bound == L
            assert p.n_inner_layers == L - 1 - last and len(p.last_layer_poly) == 1 << last
            made[key] = (op, p)
        return made[key]

    return get


def oracle_status(oracle, op, seed):
    try:
        return ACCEPTED if oracle.verify(op, seed) else REJECTED
    except RuntimeError:  # the reference panics here
        return INVARIANT


def product_status(p, seed):
    import frieda_amd

    try:
        return ACCEPTED if frieda_amd.verify(p, seed) else REJECTED
    except frieda_amd.FriedaPanic:
        return INVARIANT


def product_samples(p, seed):
    import frieda_amd

    try:
        ok, pos = frieda_amd.verify_samples(p, seed)
        return (ACCEPTED, pos) if ok else (REJECTED, None)
    except frieda_amd.FriedaPanic:
        return INVARIANT, None


def oracle_positions(oracle, op, seed):
    """sample_query_positions restated from the oracle's channel primitives: the transcript of the proof as the verifier replays it
    (seed, every layer's root and alpha, last_layer_poly, the nonce), then Queries::generate on the whole domain"""
    O, c = oracle.lib(), op.c
    ch = oracle.Channel()
    O.fo_channel_init(C.byref(ch))
    if seed is not None:
        O.fo_channel_mix_u64(C.byref(ch), seed)
    alpha = (C.c_uint32 * 4)()
    for lay in [c.first_layer] + [c.inner_layers[i] for i in range(c.n_inner_layers)]:
        O.fo_channel_mix_root(C.byref(ch), bytes(lay.commitment))
        O.fo_channel_draw_felt(C.byref(ch), alpha)
    O.fo_channel_mix_felts(C.byref(ch), c.last_layer_poly, c.n_last_layer_poly)
    O.fo_channel_mix_u64(C.byref(ch), c.proof_of_work)
    assert O.fo_channel_trailing_zeros(C.byref(ch)) >= c.pcs_config.pow_bits
    out = np.zeros(c.pcs_config.n_queries, dtype=np.uint32)
    u = O.fo_queries_generate(C.byref(ch), c.log_size_bound + c.pcs_config.log_blowup_factor, c.pcs_config.n_queries, out.ctypes.data)
    return out[:u].copy()


@pytest.mark.parametrize("last,B,L", CASES, ids=[f"last{c[0]}-B{c[1]}-L{c[2]}" for c in CASES])
def test_verdict_and_positions_equal_the_oracle(oracle, proofs, last, B, L):
    op, p = proofs(last, B, L)
    want = oracle_status(oracle, op, SEED)
    assert want == (INVARIANT if L == last + 1 else ACCEPTED)  # no inner layer: the reference's verifier panics
    assert product_status(p, SEED) == want
    st, pos = product_samples(p, SEED)
    assert st == want
    if want == ACCEPTED:
        assert np.array_equal(pos, oracle_positions(oracle, op, SEED))
        assert len(pos) == len(p.evaluations)
    # a wrong seed: another transcript; the proof of work or the first opening fails (or the same panic)
    wrong = oracle_status(oracle, op, WRONG_SEED)
    assert wrong != ACCEPTED
    assert product_status(p, WRONG_SEED) == wrong
    assert product_samples(p, WRONG_SEED) == (wrong, None)


# ---- edits of last_layer_poly: name -> function of the coefficient words (uint32 [np, 4]) -> edited words, or None where np is too small
def _bump(j):
    def f(w):
        if not 0 <= j(len(w)) < len(w):
            return None
        w = w.copy()
        w[j(len(w)), 0] = (int(w[j(len(w)), 0]) + 1) % P
        return w

    return f


def _swap(w):
    if len(w) < 2:
        return None
    assert not np.array_equal(w[0], w[-1])
    w = w.copy()
    w[[0, -1]] = w[[-1, 0]]
    return w


EDITS = {
    "bump 0": _bump(lambda n: 0),
    "bump 1": _bump(lambda n: 1),
    "bump np/2-1": _bump(lambda n: n // 2 - 1),
    "bump np/2": _bump(lambda n: n // 2),
    "bump np-1": _bump(lambda n: n - 1),
    "swap first and last": _swap,
    "truncated to np/2": lambda w: w[: len(w) // 2].copy(),
    "extended to 2 np": lambda w: np.concatenate([w, np.zeros_like(w)]),
}


def edited_proof(p, words):
    """the product's Proof with last_layer_poly replaced (through the wire image)"""
    from test_gpu_verify_many import mutate

    return mutate(p, lambda d: d.__setitem__("last", [int(x) for x in words.reshape(-1)]))


def oracle_status_with_last(oracle, op, words, seed):
    """the oracle's verdict on a clone of `op` whose last_layer_poly points at `words` for the length of the call (the clone gets its own
    buffer back before it is freed; the address is kept as an integer: a pointer field read from a ctypes structure is a view of the field)"""
    o2 = op.clone()
    c = o2.c
    keep_ptr, keep_n = C.cast(c.last_layer_poly, C.c_void_p).value, c.n_last_layer_poly
    arr = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1)
    buf = np.concatenate([arr, np.zeros(4, dtype=np.uint32)])  # never a zero-length buffer
    try:
        c.last_layer_poly = C.cast(buf.ctypes.data, oracle.u32p)
        c.n_last_layer_poly = arr.size // 4
        return oracle_status(oracle, o2, seed)
    finally:
        c.last_layer_poly = C.cast(keep_ptr, oracle.u32p)
        c.n_last_layer_poly = keep_n


@pytest.mark.parametrize("last,B,L", CASES, ids=[f"last{c[0]}-B{c[1]}-L{c[2]}" for c in CASES])
def test_edited_last_layer_poly_is_never_accepted(oracle, proofs, last, B, L):
    op, p = proofs(last, B, L)
    base = p.last_layer_poly
    assert np.array_equal(base.reshape(-1), np.ctypeslib.as_array(op.c.last_layer_poly, shape=(4 << last,)))
    ran = 0
    for name, fn in EDITS.items():
        words = fn(base)
        if words is None:
            continue
        assert words.shape != base.shape or not np.array_equal(words, base), name
        ran += 1
        want = oracle_status_with_last(oracle, op, words, SEED)
        assert want != ACCEPTED, f"the oracle accepts '{name}': it tests nothing"
        m = edited_proof(p, words)
        assert product_status(m, SEED) == want, name
        assert product_samples(m, SEED) == (want, None), name
    assert ran == (5 if last == 0 else 8)  # np = 1: no coefficient 1 or np/2 - 1 and nothing to swap (several names are then the same edit)
    # the oracle's proof is as it was
    assert oracle_status(oracle, op, SEED) == (INVARIANT if L == last + 1 else ACCEPTED)
