"""GPU: the split route of the proof verifier (FRIEDA_VERIFY_SPLIT_MAX, verify_split.hip: a wave per proof for the value chain, a wave per
(proof, layer) for the Merkle walks) against the host verifier proof by proof, and against the one-kernel route.

Two contexts of the module's own: `split` takes the split route for every pass (2^31), `one` never (0); both use the device for every
eligible proof.  The reference of every status is frieda_verify / frieda_verify_samples / frieda_verify_pairs on the same proof object.

Resources of the new kernels (tests/test_verify_split_registers.py holds the limits): verify_walk_kernel 48 VGPRs (8 waves per SIMD), no
scratch, no static LDS, 36 bytes of dynamic LDS per entry of q_cap; verify_chain_kernel<false> / <true> 143 / 143 VGPRs (3 waves per
SIMD), no scratch, no spill of either kind, 644 bytes of static and 24 bytes per entry of dynamic LDS; verify_many_kernel<false> / <true> 144 / 145 VGPRs, as at
the parent commit.
"""
import copy
import ctypes as C

import numpy as np
import pytest

from conftest import pattern_bytes, splitmix64_bytes
from pairs_util import restate
from test_gpu_verify_many import ACCEPTED, INVARIANT, REJECTED, _bump, _layer_of, _mutations, build, host_samples, host_status, mutate, parse

pytestmark = pytest.mark.gpu


def _cfg(nq=20, blowup=4, last=0, pow_bits=20):
    import frieda_amd

    return frieda_amd.PcsConfig(frieda_amd.FriConfig(blowup, last, nq), pow_bits)


def _ctx(split_max):
    import frieda_amd

    ctx = frieda_amd.Context(0)
    ctx.set_option("FRIEDA_VERIFY_DEVICE_MIN", 0)
    ctx.set_option("FRIEDA_VERIFY_SPLIT_MAX", split_max)
    return ctx


@pytest.fixture(scope="module")
def split():
    ctx = _ctx(1 << 31)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def one():
    ctx = _ctx(0)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def kib(gpu_ctx):
    """1 KiB blob under 33 seeds (prove_seeds): (data, commitment, seeds, proofs)"""
    data = pattern_bytes(1024).tobytes()
    seeds = [1000 + 7 * i for i in range(33)]
    root, proofs = gpu_ctx.commit_and_generate_proofs_for_seeds(data, seeds, _cfg())
    return data, root, seeds, proofs


@pytest.fixture(scope="module")
def deep(gpu_ctx):
    """30 KiB blob, blowup 2^2, last-layer bound 2: (seed, proof) with 8 inner layers (the `deep` proof of tests/test_gpu_verify_many.py)"""
    data = splitmix64_bytes(3, 30 * 1024).tobytes()
    _, p = gpu_ctx.commit_and_generate_proof(data, 77, _cfg(20, 2, 2, 8))
    assert p.n_inner_layers == 8
    return 77, p


def check(split, one, proofs, seeds, expect=None):
    """the split route against the host calls proof by proof and against the one-kernel route; returns the statuses"""
    st = split.verify_many(proofs, seeds)
    st2, pos = split.verify_samples_many(proofs, seeds)
    o_st = one.verify_many(proofs, seeds)
    o_st2, o_pos = one.verify_samples_many(proofs, seeds)
    for i, p in enumerate(proofs):
        s = None if seeds is None else seeds[i]
        assert st[i] == host_status(p, s), (i, int(st[i]), host_status(p, s))
        hs, hp = host_samples(p, s)
        assert st2[i] == hs, (i, int(st2[i]), hs)
        if hs == ACCEPTED:
            assert np.array_equal(pos[i], hp), i
        else:
            assert pos[i] is None, i
    assert st.tobytes() == o_st.tobytes() and st2.tobytes() == o_st2.tobytes()
    assert [None if p is None else p.tobytes() for p in pos] == [None if p is None else p.tobytes() for p in o_pos]
    if expect is not None:
        assert [int(x) for x in st] == list(expect)
    return st


def check_pairs(split, one, proofs, seeds):
    """verify_pairs_many: rows, counts and values equal between the routes and to frieda_verify_pairs"""
    import frieda_amd

    st, pts = split.verify_pairs_many(proofs, seeds)
    o_st, o_pts = one.verify_pairs_many(proofs, seeds)
    assert st.tobytes() == o_st.tobytes()
    for i, p in enumerate(proofs):
        s = None if seeds is None else seeds[i]
        try:
            ok, hpos, hval = frieda_amd.verify_pairs(p, s)
            hs = ACCEPTED if ok else REJECTED
        except frieda_amd.FriedaPanic:
            hs = INVARIANT
        assert st[i] == hs, (i, int(st[i]), hs)
        if hs != ACCEPTED:
            assert pts[i] is None and o_pts[i] is None, i
            continue
        assert np.array_equal(pts[i][0], hpos) and np.array_equal(pts[i][1], hval), i
        assert np.array_equal(o_pts[i][0], hpos) and np.array_equal(o_pts[i][1], hval), i
        r = restate(p, s)
        assert np.array_equal(pts[i][0], r[0]) and np.array_equal(pts[i][1], r[1]), i
    return st


def test_the_option_selects_the_launches(split, one, kib):
    """reach: "verify_many" is the timer name of a verify pass's launches on either shape — two per pass on the split context (the chain,
    then the walks), one on the other"""
    _, _, seeds, proofs = kib
    for ctx, per_pass in ((split, 2), (one, 1)):
        ctx.set_kernel_timing(True)
        try:
            ctx.kernel_timing_report()
            ctx.verify_many(proofs[:3], seeds[:3])
            launches = {r["name"]: r["launches"] for r in ctx.kernel_timing_report()}
        finally:
            ctx.set_kernel_timing(False)
        assert launches.get("verify_many") == per_pass, launches


def test_prove_seeds_proofs(split, one, kib):
    _, _, seeds, proofs = kib
    check(split, one, proofs, seeds, expect=[ACCEPTED] * 33)
    # under the wrong seed: the PoW or a later event, whatever the host says
    check(split, one, proofs[:4], [s + 1 for s in seeds[:4]])


def test_deep_proof(split, one, deep):
    seed, p = deep
    check(split, one, [p, p], [seed, seed + 1], expect=[ACCEPTED, REJECTED])
    check_pairs(split, one, [p, p], [seed, seed + 1])


def test_mutation_matrix_on_deep(split, one, deep):
    seed, p = deep
    muts = {name: mutate(p, fn) for name, fn in _mutations(p.n_inner_layers).items()}
    muts["evaluations one long"] = mutate(p, lambda d: d["evals"].extend(d["evals"][:4]))
    names = sorted(muts)
    st = check(split, one, [muts[k] for k in names] + [p], [seed] * (len(names) + 1))
    for k, s in zip(names, st):
        assert (s == ACCEPTED) == (k == "evaluations one long"), k
    assert st[names.index("evaluations one short")] == INVARIANT and st[-1] == ACCEPTED
    check_pairs(split, one, [muts[k] for k in names] + [p], [seed] * (len(names) + 1))


def test_single_bit_flips(split, one, kib):
    import frieda_amd

    _, _, seeds, proofs = kib
    d = parse(proofs[2].serialize())
    lists = lambda x: [x["evals"], x["nonce"], x["last"]] + [y for l in [x["first"]] + x["inner"] for y in (l["com"], l["fri"], l["hash"])]
    total = sum(len(x) for x in lists(d))
    rng = np.random.default_rng(23)
    flipped = []
    for _ in range(64):
        dd = copy.deepcopy(d)
        k = int(rng.integers(total))
        for x in lists(dd):
            if k < len(x):
                x[k] ^= 1 << int(rng.integers(32))
                break
            k -= len(x)
        flipped.append(frieda_amd.Proof.deserialize(build(dd)))
    st = check(split, one, flipped, [seeds[2]] * 64)
    assert ACCEPTED not in set(st)


# ---------------------------------------------------------------- the event order
def _flip_first_layer_hash(d):
    # the first layer's Merkle path: a hash of its witness, or — a tree the queries cover without one — a sibling value, which only the leaf hash reads
    if d["first"]["hash"]:
        d["first"]["hash"][0] ^= 1
    else:
        _bump(d["first"]["fri"], 0)


def test_event_order_too_few_evaluations(split, one, deep):
    seed, p = deep
    short = mutate(p, lambda d: d.__setitem__("evals", d["evals"][:-4]))
    both = mutate(p, lambda d: (d.__setitem__("evals", d["evals"][:-4]), _flip_first_layer_hash(d)))
    hashed = mutate(p, _flip_first_layer_hash)
    check(split, one, [short, both, hashed], [seed] * 3, expect=[INVARIANT, INVARIANT, REJECTED])


def test_event_order_no_inner_layers(gpu_ctx, split, one):
    _, p = gpu_ctx.commit_and_generate_proof(splitmix64_bytes(11, 20).tobytes(), None, _cfg(3, 2, 0, 4))
    assert p.n_inner_layers == 0
    bad = mutate(p, _flip_first_layer_hash)
    # the reference asserts on the missing inner layers only after the first layer's tree has been checked
    check(split, one, [p, bad, p], None, expect=[INVARIANT, REJECTED, INVARIANT])


def test_event_order_walk_before_a_later_value_stage(split, one, deep):
    seed, p = deep

    def walk1_values3(d):
        _layer_of(d, 1)["hash"][0] ^= 1
        _layer_of(d, 3)["fri"] = _layer_of(d, 3)["fri"][:-4]

    def values3_only(d):
        _layer_of(d, 3)["fri"] = _layer_of(d, 3)["fri"][:-4]

    def last_poly_and_last_walk(d):
        _bump(d["last"], 1)
        _layer_of(d, len(d["inner"]))["hash"][-1] ^= 1

    ms = [mutate(p, f) for f in (walk1_values3, values3_only, last_poly_and_last_walk)]
    check(split, one, ms + [p], [seed] * 4, expect=[REJECTED, REJECTED, REJECTED, ACCEPTED])


# ---------------------------------------------------------------- shapes
def _flip_deepest_hash(d):
    # the last hash of the deepest layer that has a hash witness (a small layer under many queries has none); else a sibling value
    for l in reversed([d["first"]] + d["inner"]):
        if l["hash"]:
            l["hash"][-1] ^= 2
            return
    _bump(d["first"]["fri"], 0)


@pytest.mark.parametrize("nq,blowup", [(1, 4), (20, 4), (64, 1), (65, 4), (300, 4), (300, 1)])
def test_query_counts(gpu_ctx, split, one, nq, blowup):
    """1 and 20 queries; 64 on a 2^8 domain (pairs with both members queried); 65: the chunk carry of group_of; 300: q_cap 512, and on
    the 2^8 domain layers with fewer positions than queries"""
    data = splitmix64_bytes(40 + nq, 1024).tobytes()
    seeds = [3, 4, 5]
    _, proofs = gpu_ctx.commit_and_generate_proofs_for_seeds(data, seeds, _cfg(nq, blowup, 0, 4))
    bad = mutate(proofs[1], _flip_deepest_hash)
    check(split, one, proofs + [bad], seeds + [4], expect=[ACCEPTED] * 3 + [REJECTED])
    check_pairs(split, one, proofs + [bad], seeds + [4])


def test_mixed_layer_counts_and_a_host_route_proof(gpu_ctx, split, one, kib, deep):
    """1 KiB and 30 KiB proofs in one grid: the walk waves beyond a proof's last layer leave; a proof beyond the kernel goes to the host"""
    seed, good = deep
    _, _, kseeds, kproofs = kib
    big = gpu_ctx.commit_and_generate_proof(splitmix64_bytes(8, 5000).tobytes(), 4, _cfg(1025, 4, 1, 0))[1]
    small = gpu_ctx.commit_and_generate_proof(pattern_bytes(300).tobytes(), 4, _cfg(12, 2, 1, 8))[1]
    assert len({good.n_inner_layers, kproofs[0].n_inner_layers, small.n_inner_layers}) == 3
    proofs = [kproofs[0], big, good, small, kproofs[1], big, good]
    seeds = [kseeds[0], 4, seed, 4, kseeds[1], 5, seed]
    check(split, one, proofs, seeds, expect=[ACCEPTED, ACCEPTED, ACCEPTED, ACCEPTED, ACCEPTED, REJECTED, ACCEPTED])
    check_pairs(split, one, proofs, seeds)


def _launches(ctx, call):
    """the launches of the verify passes of `call` on ctx (the timer name of both shapes: two per split pass)"""
    ctx.set_kernel_timing(True)
    try:
        ctx.kernel_timing_report()
        call()
        return {r["name"]: r["launches"] for r in ctx.kernel_timing_report()}.get("verify_many", 0)
    finally:
        ctx.set_kernel_timing(False)


def test_three_passes(split, one, kib, deep):
    seed, good = deep
    _, _, kseeds, kproofs = kib
    proofs = kproofs[:6] + [good]
    seeds = kseeds[:6] + [seed]
    proofs[4] = mutate(kproofs[4], lambda d: _bump(d["first"]["hash"], 3))
    # three small proofs per pass (a proof stages its image and a 64-byte header; the image is the wire image give or take its count
    # words), not four; the deep one does not fit behind three small ones: a pass of its own
    small = len(kproofs[0].serialize())
    budget = 3 * (small + 128)
    assert 4 * (small - 128) > budget and 3 * (small - 128) + len(good.serialize()) - 128 > budget
    assert split._L.frieda_ctx_test_set_verify_pass_bytes(split._h, budget) == 0
    try:
        st = check(split, one, proofs, seeds)
        check_pairs(split, one, proofs, seeds)
        assert _launches(split, lambda: split.verify_many(proofs, seeds)) == 2 * 3
    finally:
        assert split._L.frieda_ctx_test_set_verify_pass_bytes(split._h, 0) == 0
    assert [int(x) for x in st] == [ACCEPTED] * 4 + [REJECTED] + [ACCEPTED] * 2
    assert _launches(split, lambda: split.verify_many(proofs, seeds)) == 2


def test_passes_cut_for_their_scratch_alone(split, one, kib, deep):
    """a scratch cap of exactly two of the small proofs (7 layers x 64 entries x 36 bytes each): five of them and the deep one (9 layers:
    every slot of its pass would be 9 layers deep) go as 2 + 2 + 1 + 1, and give what the uncut pass gives"""
    seed, good = deep
    _, _, kseeds, kproofs = kib
    assert kproofs[0].n_inner_layers == 6 and good.n_inner_layers == 8
    proofs = kproofs[:5] + [good]
    seeds = kseeds[:5] + [seed]
    proofs[3] = mutate(kproofs[3], lambda d: _bump(_layer_of(d, 2)["hash"], 0))
    uncut = (split.verify_many(proofs, seeds).tobytes(), [None if p is None else p.tobytes() for p in split.verify_samples_many(proofs, seeds)[1]])
    assert _launches(split, lambda: split.verify_many(proofs, seeds)) == 2
    assert split._L.frieda_ctx_test_set_verify_scratch_bytes(split._h, 2 * 7 * 64 * 36) == 0
    try:
        st = check(split, one, proofs, seeds, expect=[ACCEPTED] * 3 + [REJECTED] + [ACCEPTED] * 2)
        check_pairs(split, one, proofs, seeds)
        cut = (st.tobytes(), [None if p is None else p.tobytes() for p in split.verify_samples_many(proofs, seeds)[1]])
        assert _launches(split, lambda: split.verify_many(proofs, seeds)) == 2 * 4
    finally:
        assert split._L.frieda_ctx_test_set_verify_scratch_bytes(split._h, 0) == 0
    assert cut == uncut


@pytest.mark.parametrize("word", [0x00000000, 0xFFFFFFFF, 0x00000003])
def test_poisoned_workspace(one, kib, deep, word):
    """sticky poison before the first call of a fresh context: every allocation starts as `word`, so a count or a row of a layer the
    chain did not reach (3 as a count: a walk over three pairs nobody wrote) would change a status"""
    seed, good = deep
    _, _, kseeds, kproofs = kib
    proofs = [kproofs[0], good, mutate(good, lambda d: _bump(_layer_of(d, 4)["fri"], 1)), kproofs[1], mutate(kproofs[2], lambda d: d["nonce"].__setitem__(0, d["nonce"][0] ^ 1))]
    seeds = [kseeds[0], seed, seed, kseeds[1], kseeds[2]]
    ctx = _ctx(1 << 31)
    try:
        assert ctx._L.frieda_ctx_test_poison(ctx._h, word, 1, None) == 0
        check(ctx, one, proofs, seeds, expect=[ACCEPTED, ACCEPTED, REJECTED, ACCEPTED, REJECTED])
        check_pairs(ctx, one, proofs, seeds)
    finally:
        ctx.close()


def test_reconstruct_from_proof_pairs_through_the_split_route(gpu_ctx, split):
    data = splitmix64_bytes(1, 1024).tobytes()
    seeds = list(range(1, 13))
    root, proofs = gpu_ctx.commit_and_generate_proofs_for_seeds(data, seeds, _cfg(20, 4, 0, 4))
    out, st, n = split.reconstruct_from_proof_pairs(proofs, seeds, root, len(data))
    assert out == data and set(st) == {ACCEPTED} and n >= 130
