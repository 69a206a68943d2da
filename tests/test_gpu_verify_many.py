"""GPU: frieda_verify_many / frieda_verify_samples_many / frieda_reconstruct_from_proofs against the host verifier, proof by proof.

The reference of every check is frieda_verify / frieda_verify_samples on the same proof object: the status byte of the batched call
must be what the host call says (0 rejected, 1 accepted, 2 where it raises FriedaPanic) and the positions must be the host's.

Two cases of the issue's list cannot be stated as it words them, and are stated as what the host verifier does instead:
  * an 8-byte blob has log_size_bound 0, which the prover refuses (the reference panics) — there is no such proof; the test asserts the
    refusal and checks a proof whose log_size_bound word is rewritten to 0 (status 2 on both sides);
  * "evaluations one long": frieda_verify ACCEPTS it (the reference never looks at the surplus value) while frieda_verify_samples reports
    the panic; verify_many must say 1 and verify_samples_many 2, as the two host calls do.  Every other mutation is asserted not to
    be accepted by the host.
"""
import struct

import numpy as np
import pytest

from conftest import pattern_bytes, splitmix64_bytes

pytestmark = pytest.mark.gpu

ERR_ARG = 1
REJECTED, ACCEPTED, INVARIANT, WRONG_COMMITMENT = 0, 1, 2, 3


def _cfg(nq=20, blowup=4, last=0, pow_bits=20):
    import frieda_amd

    return frieda_amd.PcsConfig(frieda_amd.FriConfig(blowup, last, nq), pow_bits)


# ---- the wire image as a dict of word lists: mutations edit data words and explicit counts only ----
def parse(image):
    w = list(struct.unpack(f"<{len(image) // 4}I", image))
    pos = [0]

    def take(n):
        r = w[pos[0] : pos[0] + n]
        pos[0] += n
        return r

    def layer():
        com = take(8)
        nf = take(1)[0]
        fw = take(4 * nf)
        nh = take(1)[0]
        hw = take(8 * nh)
        nc = take(1)[0]
        cw = take(nc)
        return {"com": com, "fri": fw, "hash": hw, "col": cw}

    d = {"head": take(2), "cfg": take(4), "L": take(1)[0], "nonce": take(2)}
    ne = take(1)[0]
    d["evals"] = take(4 * ne)
    d["first"] = layer()
    ni = take(1)[0]
    d["inner"] = [layer() for _ in range(ni)]
    nl = take(1)[0]
    d["last"] = take(4 * nl)
    assert pos[0] == len(w)
    return d


def build(d):
    def layer(l):
        return l["com"] + [len(l["fri"]) // 4] + l["fri"] + [len(l["hash"]) // 8] + l["hash"] + [len(l["col"])] + l["col"]

    w = d["head"] + d["cfg"] + [d["L"]] + d["nonce"] + [len(d["evals"]) // 4] + d["evals"] + layer(d["first"]) + [len(d["inner"])]
    for l in d["inner"]:
        w += layer(l)
    w += [len(d["last"]) // 4] + d["last"]
    return struct.pack(f"<{len(w)}I", *w)


def mutate(proof, fn):
    """serialize -> edit -> deserialize; an image that does not parse raises (the test fails, it is not skipped)"""
    import copy

    import frieda_amd

    d = copy.deepcopy(parse(proof.serialize()))
    fn(d)
    return frieda_amd.Proof.deserialize(build(d))


def host_status(p, seed):
    import frieda_amd

    try:
        return ACCEPTED if frieda_amd.verify(p, seed) else REJECTED
    except frieda_amd.FriedaPanic:
        return INVARIANT


def host_samples(p, seed):
    import frieda_amd

    try:
        ok, pos = frieda_amd.verify_samples(p, seed)
        return (ACCEPTED, pos) if ok else (REJECTED, None)
    except frieda_amd.FriedaPanic:
        return INVARIANT, None


def check_against_host(ctx, proofs, seeds, expect=None):
    """both batched calls against the two host calls, proof by proof; returns the statuses of verify_many"""
    st = ctx.verify_many(proofs, seeds)
    st2, pos = ctx.verify_samples_many(proofs, seeds)
    for i, p in enumerate(proofs):
        s = None if seeds is None else seeds[i]
        assert st[i] == host_status(p, s), (i, int(st[i]))
        hs, hp = host_samples(p, s)
        assert st2[i] == hs, (i, int(st2[i]), hs)
        if hs == ACCEPTED:
            assert np.array_equal(pos[i], hp), i
        else:
            assert pos[i] is None, i
    if expect is not None:
        assert list(st) == list(expect)
    return st


@pytest.fixture(scope="module")
def kib(gpu_ctx):
    """1 KiB blob under 33 seeds (prove_seeds): (data, commitment, seeds, proofs)"""
    data = pattern_bytes(1024).tobytes()
    seeds = [1000 + 7 * i for i in range(33)]
    root, proofs = gpu_ctx.commit_and_generate_proofs_for_seeds(data, seeds, _cfg())
    return data, root, seeds, proofs


@pytest.fixture(scope="module")
def deep(gpu_ctx):
    """30 KiB blob, blowup 2^2, last-layer bound 2: (seed, proof) with 9 inner layers — first, middle and last differ"""
    data = splitmix64_bytes(3, 30 * 1024).tobytes()
    _, p = gpu_ctx.commit_and_generate_proof(data, 77, _cfg(20, 2, 2, 8))
    assert p.n_inner_layers >= 3
    return 77, p


# ---------------------------------------------------------------- agreement on good proofs
def test_prove_seeds_proofs_are_accepted(gpu_ctx, kib):
    _, _, seeds, proofs = kib
    st = check_against_host(gpu_ctx, proofs, seeds, expect=[ACCEPTED] * 33)
    assert len(st) == 33


GOOD_CASES = [
    # (bytes, seeds or None, n_queries, blowup, last, pow_bits)
    (1024, None, 1, 1, 0, 0),
    (1024, [5, 6, 7], 20, 2, 1, 20),
    (30 * 1024, [1, 2], 64, 3, 2, 0),
    (30 * 1024, None, 65, 4, 3, 0),
    (64 * 1024, [9], 300, 4, 0, 20),
    (30 * 1024, [1, 2], 20, 2, 6, 0),  # 64 last-layer coefficients: every level of the kernel's one-pass fold up to bit 5
    (100, [3, 4], 300, 1, 0, 0),  # a 2^4 domain under 300 queries: most draws are duplicates
    (20, None, 3, 2, 0, 4),  # no inner layer at all: the reference panics
]


@pytest.mark.parametrize("nbytes,seeds,nq,blowup,last,pow_bits", GOOD_CASES, ids=lambda v: str(v)[:12])
def test_batch_path_proofs_agree(gpu_ctx, nbytes, seeds, nq, blowup, last, pow_bits):
    count = len(seeds) if seeds else 2
    blobs = [splitmix64_bytes(11 + i, nbytes).tobytes() for i in range(count)]
    cfg = _cfg(nq, blowup, last, pow_bits)
    if count > 1 and last + blowup <= 11:
        proofs = [p for _, p in gpu_ctx.commit_and_generate_proof_batch(blobs, seeds, cfg)]
    else:
        proofs = [gpu_ctx.commit_and_generate_proof(b, seeds[i] if seeds else None, cfg)[1] for i, b in enumerate(blobs)]
    st = check_against_host(gpu_ctx, proofs, seeds)
    assert set(st) == ({INVARIANT} if nbytes == 20 else {ACCEPTED})


def test_domain_2_pow_20(gpu_ctx):
    data = splitmix64_bytes(5, (4 << 16) * 30 // 8).tobytes()  # 2^16 coefficients per column, blowup 2^4
    seeds = [21, 22]
    _, proofs = gpu_ctx.commit_and_generate_proofs_for_seeds(data, seeds, _cfg())
    assert proofs[0].log_size_bound + 4 == 20
    check_against_host(gpu_ctx, proofs, seeds, expect=[ACCEPTED, ACCEPTED])


def test_eight_byte_blob_has_no_proof(gpu_ctx, kib):
    import frieda_amd

    with pytest.raises(frieda_amd.FriedaError):
        gpu_ctx.commit_and_generate_proof(bytes(8), None, _cfg(1, 1, 0, 0))
    _, _, seeds, proofs = kib
    m = mutate(proofs[0], lambda d: d.__setitem__("L", 0))
    check_against_host(gpu_ctx, [m], seeds[:1], expect=[INVARIANT])


# ---------------------------------------------------------------- mutation matrix
def _bump(words, i):
    words[i] = (words[i] + 1) % 0x7FFFFFFF


def _layer_of(d, which):
    return d["first"] if which == 0 else d["inner"][which - 1]


def _mutations(n_inner):
    mid, lastl = (n_inner + 1) // 2, n_inner
    muts = {
        "nonce": lambda d: d["nonce"].__setitem__(0, d["nonce"][0] ^ 1),
        "evaluation word": lambda d: _bump(d["evals"], 5),
        "evaluations one short": lambda d: d.__setitem__("evals", d["evals"][:-4]),
        "last-layer coefficient": lambda d: _bump(d["last"], 0),
        "last-layer length 3": lambda d: d.__setitem__("last", (d["last"] * 3)[:12]),
        "last-layer length 2x bound": lambda d: d.__setitem__("last", d["last"] * 2),
        "inner layer dropped": lambda d: d["inner"].pop(mid - 1),
        "inner layer duplicated": lambda d: d["inner"].insert(mid, dict(d["inner"][mid - 1])),
    }
    for name, li in (("first", 0), ("middle", mid), ("last", lastl)):
        muts[f"fri_witness word, {name} layer"] = lambda d, li=li: _bump(_layer_of(d, li)["fri"], 1)
        muts[f"first hash, {name} layer"] = lambda d, li=li: _layer_of(d, li)["hash"].__setitem__(0, _layer_of(d, li)["hash"][0] ^ 1)
        muts[f"last hash, {name} layer"] = lambda d, li=li: _layer_of(d, li)["hash"].__setitem__(-1, _layer_of(d, li)["hash"][-1] ^ 1)
        muts[f"fri_witness one short, {name} layer"] = lambda d, li=li: _layer_of(d, li).__setitem__("fri", _layer_of(d, li)["fri"][:-4])
        muts[f"fri_witness one long, {name} layer"] = lambda d, li=li: _layer_of(d, li)["fri"].extend([1, 2, 3, 4])
        muts[f"hash_witness one short, {name} layer"] = lambda d, li=li: _layer_of(d, li).__setitem__("hash", _layer_of(d, li)["hash"][:-8])
        muts[f"hash_witness one long, {name} layer"] = lambda d, li=li: _layer_of(d, li)["hash"].extend([7] * 8)
        muts[f"commitment, {name} layer"] = lambda d, li=li: _layer_of(d, li)["com"].__setitem__(3, _layer_of(d, li)["com"][3] ^ 4)
        muts[f"column witness, {name} layer"] = lambda d, li=li: _layer_of(d, li)["col"].append(9)
    return muts


@pytest.fixture(scope="module")
def mutants(deep):
    seed, p = deep
    out = {name: mutate(p, fn) for name, fn in _mutations(p.n_inner_layers).items()}
    out["evaluations one long"] = mutate(p, lambda d: d["evals"].extend(d["evals"][:4]))
    return out


def test_mutation_matrix(gpu_ctx, deep, mutants):
    seed, p = deep
    names = sorted(mutants)
    proofs = [mutants[k] for k in names] + [p, p]
    seeds = [seed] * len(names) + [seed, seed + 1]  # the last one: a good proof under the wrong seed
    st = check_against_host(gpu_ctx, proofs, seeds)
    for k, s in zip(names, st):
        print(f"{k}: {int(s)}")
        if k == "evaluations one long":
            assert s == ACCEPTED  # frieda_verify accepts it (module docstring); verify_samples_many said 2 above, as frieda_verify_samples
        else:
            assert s != ACCEPTED, f"the host verifier accepts mutation '{k}': it tests nothing"
    assert st[names.index("evaluations one short")] == INVARIANT
    assert st[-2] == ACCEPTED and st[-1] == REJECTED


# ---------------------------------------------------------------- isolation
@pytest.mark.parametrize("count", [1, 63, 64, 65, 257])
def test_mutated_and_good_proofs_interleaved(gpu_ctx, deep, mutants, kib, count):
    seed, good = deep
    _, _, kseeds, kproofs = kib
    pool = [(good, seed, ACCEPTED), (kproofs[0], kseeds[0], ACCEPTED), (kproofs[1], kseeds[0], REJECTED)]
    for k in sorted(mutants):
        if k != "evaluations one long":
            pool.append((mutants[k], seed, host_status(mutants[k], seed)))
    items = [pool[(5 * i + i // 7) % len(pool)] for i in range(count)]
    # the same proof first, in the middle and last
    probe = pool[3]
    for at in {0, count // 2, count - 1}:
        items[at] = probe
    st = gpu_ctx.verify_many([x[0] for x in items], [x[1] for x in items])
    assert [int(s) for s in st] == [x[2] for x in items]


# ---------------------------------------------------------------- seeded flips
def test_single_bit_flips(gpu_ctx, kib):
    import frieda_amd

    _, _, seeds, proofs = kib
    image = proofs[2].serialize()
    d = parse(image)
    # data words only: evaluations, witnesses, hashes, commitments, last layer, nonce — by their offsets in the image
    lists = [d["evals"], d["nonce"], d["last"]] + [x for l in [d["first"]] + d["inner"] for x in (l["com"], l["fri"], l["hash"])]
    total = sum(len(x) for x in lists)
    rng = np.random.default_rng(20)
    flipped = []
    for _ in range(200):
        import copy

        dd = copy.deepcopy(d)
        ll = [dd["evals"], dd["nonce"], dd["last"]] + [x for l in [dd["first"]] + dd["inner"] for x in (l["com"], l["fri"], l["hash"])]
        k = int(rng.integers(total))
        for x in ll:
            if k < len(x):
                x[k] ^= 1 << int(rng.integers(32))
                break
            k -= len(x)
        flipped.append(frieda_amd.Proof.deserialize(build(dd)))
    st = check_against_host(gpu_ctx, flipped, [seeds[2]] * 200)
    assert ACCEPTED not in set(st)


# ---------------------------------------------------------------- routes
def test_device_and_host_routes_give_identical_bytes(gpu_ctx, deep, mutants, kib):
    seed, good = deep
    _, _, kseeds, kproofs = kib
    proofs = [good] + [mutants[k] for k in sorted(mutants)] + kproofs[:5]
    seeds = [seed] * (1 + len(mutants)) + kseeds[:5]
    res = {}
    try:
        for v in (0, 1 << 31):
            gpu_ctx.set_option("FRIEDA_VERIFY_DEVICE_MIN", v)
            st = gpu_ctx.verify_many(proofs, seeds)
            st2, pos = gpu_ctx.verify_samples_many(proofs, seeds)
            res[v] = (st.tobytes(), st2.tobytes(), [None if p is None else p.tobytes() for p in pos])
    finally:
        gpu_ctx.set_option("FRIEDA_VERIFY_DEVICE_MIN", 1)
    assert res[0] == res[1 << 31]


def test_mixed_sizes_configs_and_a_proof_beyond_the_kernel(gpu_ctx, deep, kib):
    seed, good = deep
    _, _, kseeds, kproofs = kib
    big = gpu_ctx.commit_and_generate_proof(splitmix64_bytes(8, 5000).tobytes(), 4, _cfg(1025, 4, 1, 0))[1]
    small = gpu_ctx.commit_and_generate_proof(pattern_bytes(300).tobytes(), 4, _cfg(12, 2, 1, 8))[1]
    proofs = [kproofs[0], big, good, small, kproofs[1], big]
    seeds = [kseeds[0], 4, seed, 4, kseeds[1], 5]
    check_against_host(gpu_ctx, proofs, seeds, expect=[ACCEPTED, ACCEPTED, ACCEPTED, ACCEPTED, ACCEPTED, REJECTED])


# ---------------------------------------------------------------- commitment
def test_expected_commitment(gpu_ctx, kib):
    _, root, seeds, proofs = kib
    plain = gpu_ctx.verify_many(proofs, seeds)
    assert np.array_equal(gpu_ctx.verify_many(proofs, seeds, expected_commitment=root), plain)
    wrong = bytes([root[0] ^ 1]) + root[1:]
    assert list(gpu_ctx.verify_many(proofs, seeds, expected_commitment=wrong)) == [WRONG_COMMITMENT] * len(proofs)
    st, pos = gpu_ctx.verify_samples_many(proofs, seeds, expected_commitment=wrong)
    assert list(st) == [WRONG_COMMITMENT] * len(proofs) and all(p is None for p in pos)


def test_pitch_below_n_queries_is_refused(gpu_ctx, kib):
    import frieda_amd

    _, _, seeds, proofs = kib
    with pytest.raises(frieda_amd.FriedaError) as e:
        gpu_ctx.verify_samples_many(proofs[:2], seeds[:2], pitch=19)
    assert e.value.status == ERR_ARG


# ---------------------------------------------------------------- in flight
def test_refused_while_a_proof_is_in_flight(gpu_ctx, kib):
    import frieda_amd

    data, root, seeds, proofs = kib
    gpu_ctx.prove_begin(data, seeds[0], _cfg())
    try:
        for call in (
            lambda: gpu_ctx.verify_many(proofs[:2], seeds[:2]),
            lambda: gpu_ctx.verify_samples_many(proofs[:2], seeds[:2]),
            lambda: gpu_ctx.reconstruct_from_proofs(proofs, seeds, root, len(data)),
        ):
            with pytest.raises(frieda_amd.FriedaError) as e:
                call()
            assert e.value.status == ERR_ARG
    finally:
        r, p = gpu_ctx.prove_finish()
    assert r == root and p.serialize() == proofs[0].serialize()


# ---------------------------------------------------------------- reconstruction
def _proofs_for(ctx, data, cfg, n_seeds, first_seed=1):
    seeds = list(range(first_seed, first_seed + n_seeds))
    root, proofs = ctx.commit_and_generate_proofs_for_seeds(data, seeds, cfg)
    return root, seeds, proofs


def test_reconstruct_1kib(gpu_ctx):
    import frieda_amd

    data = splitmix64_bytes(1, 1024).tobytes()
    # 2^7 coefficients per column, 2^11 positions: 130 distinct points needed, 20 per proof
    root, seeds, proofs = _proofs_for(gpu_ctx, data, _cfg(20, 4, 0, 4), 12)
    out, st, n = gpu_ctx.reconstruct_from_proofs(proofs, seeds, root, len(data))
    assert out == data and set(st) == {ACCEPTED} and n >= 130
    # one tampered proof in the pool: rejected, the result unchanged
    bad = mutate(proofs[3], lambda d: _bump(d["evals"], 2))
    out2, st2, n2 = gpu_ctx.reconstruct_from_proofs(proofs[:3] + [bad] + proofs[4:], seeds, root, len(data))
    assert out2 == data and st2[3] == REJECTED and list(st2[:3]) == [ACCEPTED] * 3 and n2 <= n
    # too few proofs: the count is reported, the output untouched
    with pytest.raises(frieda_amd.FriedaError) as e:
        gpu_ctx.reconstruct_from_proofs(proofs[:3], seeds[:3], root, len(data))
    assert e.value.status == ERR_ARG
    pos = [frieda_amd.verify_samples(p, s)[1] for p, s in zip(proofs[:3], seeds[:3])]
    assert e.value.n_points == len(set(np.concatenate(pos).tolist())) < 130
    # a len that does not match the commitment
    with pytest.raises(frieda_amd.FriedaError) as e:
        gpu_ctx.reconstruct_from_proofs(proofs, seeds, root, len(data) - 1)
    assert e.value.status == ERR_ARG


def test_reconstruct_too_few_leaves_the_buffer_untouched(gpu_ctx, kib):
    import ctypes as C

    import frieda_amd

    data, root, seeds, proofs = kib
    L = gpu_ctx._L
    out = (C.c_uint8 * len(data))(*([0xAB] * len(data)))
    status = (C.c_uint8 * 2)()
    n = C.c_size_t(0)
    arr = (C.c_void_p * 2)(proofs[0]._h.value, proofs[1]._h.value)
    sd = (C.c_uint64 * 2)(*seeds[:2])
    rc = L.frieda_reconstruct_from_proofs(gpu_ctx._h, arr, sd, 2, (C.c_uint8 * 32)(*root), len(data), out, status, C.byref(n))
    pos = [frieda_amd.verify_samples(p, s)[1] for p, s in zip(proofs[:2], seeds[:2])]
    assert rc == ERR_ARG and n.value == len(set(np.concatenate(pos).tolist())) and bytes(out) == b"\xab" * len(data)
    assert list(status) == [ACCEPTED, ACCEPTED]


def test_reconstruct_golden_blob(gpu_ctx, blob):
    # 2^15 coefficients per column: 2^15 + 2 distinct points of 2^16 positions (blowup 2), 1024 queries per proof
    cfg = _cfg(1024, 1, 0, 0)
    root, seeds, proofs = _proofs_for(gpu_ctx, blob, cfg, 48)
    out, st, n = gpu_ctx.reconstruct_from_proofs(proofs, seeds, root, len(blob))
    assert out == blob and set(st) == {ACCEPTED} and n >= (1 << 15) + 2
    # one tampered proof in the pool: rejected, the result unchanged (47 proofs still cover more than 2^15 + 2 positions)
    bad = mutate(proofs[5], lambda d: _bump(d["evals"], 2))
    out2, st2, n2 = gpu_ctx.reconstruct_from_proofs(proofs[:5] + [bad] + proofs[6:], seeds, root, len(blob))
    assert out2 == blob and st2[5] == REJECTED and set(st2[:5]) | set(st2[6:]) == {ACCEPTED} and (1 << 15) + 2 <= n2 <= n
