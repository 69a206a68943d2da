"""GPU: every size of the last FRI layer through the prover's one-workgroup tail (tree.hip tail_kernel), the host-channel route behind it and
the device verifier (verify.hip verify_many_kernel) — whole proofs byte-identical to the oracle's, verdicts equal to the host verifier's.

Notation: B = log_blowup_factor, last = log_last_layer_degree_bound, last_log = last + B (log size of the last layer's domain), L = log2 of the
coefficients per column, n = L + B, n_inner = L - 1 - last.  The tail takes a proof whenever last_log <= 11; its LDS regions are sized for
exactly 2^11 points, its interpolation loops more than once per thread only from 2^11 points on, and the verifier's one-pass fold of
last_layer_poly uses bit b of its stack only when the polynomial has more than 2^b coefficients — so every last_log in 0 .. 12 and every
last in 0 .. 10 is visited here, on domains of 2^2 .. 2^17 points.  `route` mirrors the prover's decisions for the test ids and for the
coverage assertion; the product is never told which way to go.

Every blob has exact_len(L) - 3 bytes, every proof 24 queries and 3 .. 5 proof-of-work bits.
"""
import numpy as np
import pytest

from conftest import splitmix64_bytes
from pairs_util import restate
from test_gpu_shapes import exact_len
from test_gpu_verify_many import ACCEPTED, INVARIANT, REJECTED, check_against_host, host_status
from test_last_layer_host import EDITS, edited_proof, oracle_status

pytestmark = pytest.mark.gpu

ERR_ARG = 1
NQ = 24
TAIL_LOG = 11  # kernels.h: the largest last layer the one-workgroup tail (and with it the device channel) takes


def route(L, B, last):
    """what the prover does with this shape (mirror of prover.cpp prove_begin_impl and tree.hip small_domain_shape; ids and coverage only)"""
    n, last_log = L + B, last + B
    tail = last_log <= TAIL_LOG
    return {"n": n, "last_log": last_log, "n_inner": L - 1 - last, "tail": tail, "small": tail and 8 <= n <= 15 and L <= 11}


def folds_outside_the_tail(L, B, last, tail_run_log=9):
    """(tree5_fold_circle launches, tree5_fold_line launches) of a device-channel proof: inner layer kx has 2^(n - 1 - kx) points and goes
    through the multi-workgroup fold + tree launch while it has more than 2^tail_run_log points; the first of them folds the circle layer"""
    r = route(L, B, last)
    m = sum(1 for kx in range(r["n_inner"]) if r["n"] - 1 - kx > tail_run_log)
    return (1 if m else 0), max(m - 1, 0)


def pcs(B, last, pow_bits):
    import frieda_amd

    return frieda_amd.PcsConfig(frieda_amd.FriConfig(B, last, NQ), pow_bits)


def inputs(L, B, last, salt=0):
    """(blob, seed, pow_bits) of a shape; `salt` gives further blobs of the same shape"""
    data = splitmix64_bytes(7000 + 64 * last + 8 * B + L + 1000 * salt, exact_len(L) - 3).tobytes()
    return data, 100 + last + salt, 3 + (L + B + last) % 3


@pytest.fixture(scope="module")
def expected(oracle):
    """(L, B, last, salt, [seed, [length]]) -> (root, wire image, oracle proof), computed once and left alone"""
    made = {}

    def get(L, B, last, salt=0, seed=None, length=None):
        key = (L, B, last, salt, seed, length)
        if key not in made:
            data, s, pw = inputs(L, B, last, salt)
            if length is not None:
                data = data[:length]
            root, op = oracle.commit_and_generate_proof(data, s if seed is None else seed, oracle.make_config(pw, B, last, NQ))
            made[key] = (root, op.serialize(), op)
        return made[key]

    return get


def prove(ctx, L, B, last, salt=0):
    data, seed, pw = inputs(L, B, last, salt)
    return ctx.commit_and_generate_proof(data, seed, pcs(B, last, pw))


def assert_proof(got, want, what=None):
    assert got[0] == want[0], ("root", what)
    assert got[1].serialize() == want[1], ("proof", what)


def launches(ctx, fn):
    """fn()'s result and {kernel name: launches} of the launches it made (the context's per-kernel timing report)"""
    ctx.set_kernel_timing(True)
    try:
        out = fn()
        rep = {k["name"]: k["launches"] for k in ctx.kernel_timing_report()}
    finally:
        ctx.set_kernel_timing(False)
    return out, rep


# ---------------------------------------------------------------- a. the lone-proof matrix
def _matrix():
    shapes = [(L, B, last) for last in range(11) for B in (0, 1, 2, 4) for L in (last + 1, last + 2, last + 3, last + 5)]
    # last_log 10, 11 and 12 reached from the blow-up side (and last = 10 at blow-ups 2^2 and 2^4, which the grid holds already)
    for B, last in ((6, 4), (6, 5), (8, 3), (10, 1), (11, 0), (12, 0), (2, 10), (4, 10)):
        shapes += [(last + 1, B, last), (last + 3, B, last)]
    out = []
    for s in shapes:
        if 2 <= s[0] + s[1] <= 17 and s not in out:
            out.append(s)
    return out


MATRIX = _matrix()


def _id(L, B, last):
    r = route(L, B, last)
    return f"last{last}-B{B}-L{L}-n{r['n']}-ll{r['last_log']}-ni{r['n_inner']}-{'small' if r['small'] else 'general'}-{'tail' if r['tail'] else 'hostchannel'}"


MATRIX_IDS = [_id(*s) for s in MATRIX]


def test_matrix_reaches_every_last_layer_size_and_route():
    import re

    seen = []
    for i in MATRIX_IDS:
        m = re.fullmatch(r"last(\d+)-B(\d+)-L(\d+)-n(\d+)-ll(\d+)-ni(\d+)-(small|general)-(tail|hostchannel)", i)
        d = dict(zip(("last", "B", "L", "n", "ll", "ni"), map(int, m.groups()[:6])))
        d.update(path=m.group(7), chan=m.group(8))
        seen.append(d)
    assert len(MATRIX) == len(set(MATRIX_IDS)) >= 170
    assert {d["ll"] for d in seen} >= set(range(13))  # (13 and 14 as well: last = 9 and 10 at blow-up 2^4)
    assert {d["last"] for d in seen} == set(range(11))
    assert {d["n"] for d in seen} == set(range(2, 18))
    for n in (11, 12):  # the circle layer folded straight into a full-size tail
        assert any(d["ni"] == 0 and d["n"] == n for d in seen), n
    for ll in (10, 11):
        assert {d["path"] for d in seen if d["ll"] == ll} == {"small", "general"}, ll
        assert {d["chan"] for d in seen if d["ll"] == ll} == {"tail"}
        assert {d["ni"] for d in seen if d["ll"] == ll} >= {0, 1, 2, 4}
    assert {d["chan"] for d in seen if d["ll"] == 12} == {"hostchannel"}
    # every prescribed (B, last) pair from the blow-up side
    for B, last in ((6, 4), (6, 5), (8, 3), (10, 1), (11, 0), (12, 0), (2, 10), (4, 10)):
        assert any(d["B"] == B and d["last"] == last for d in seen), (B, last)


@pytest.mark.parametrize("L,B,last", MATRIX, ids=MATRIX_IDS)
def test_lone_proof_matrix(gpu_ctx, oracle, expected, L, B, last):
    """root, wire image and verdict (or panic: no inner layer) against the oracle"""
    want = expected(L, B, last)
    got = prove(gpu_ctx, L, B, last)
    assert_proof(got, want)
    assert got[1].n_inner_layers == L - 1 - last and len(got[1].last_layer_poly) == 1 << last
    seed = inputs(L, B, last)[1]
    verdict = oracle_status(oracle, want[2], seed)
    assert verdict == (INVARIANT if L == last + 1 else ACCEPTED)
    assert host_status(got[1], seed) == verdict
    assert host_status(got[1], seed + 1) == oracle_status(oracle, want[2], seed + 1) != ACCEPTED


@pytest.mark.parametrize("L,B,last", MATRIX, ids=MATRIX_IDS)
def test_lone_proof_matrix_takes_the_kernels_the_mirror_names(gpu_ctx, expected, L, B, last):
    """the tail kernel runs for every last_log <= 11 and never above; the fused small-domain kernel exactly where the mirror says; the
    layers above 2^9 points, and only they, go through the multi-workgroup fold launches (the proof is still the oracle's while timed)"""
    r = route(L, B, last)
    got, rep = launches(gpu_ctx, lambda: prove(gpu_ctx, L, B, last))
    assert_proof(got, expected(L, B, last))
    assert ("fri_tail" in rep) == r["tail"], rep
    assert ("small_first" in rep) == r["small"], rep
    if r["tail"]:
        assert rep["fri_tail"] == 1
        assert (rep.get("tree5_fold_circle", 0), rep.get("tree5_fold_line", 0)) == folds_outside_the_tail(L, B, last), rep


def test_last_11_is_refused_and_the_context_stays_usable(gpu_ctx, expected):
    import frieda_amd

    for L, B in ((12, 0), (13, 1), (16, 1)):
        data, seed, pw = inputs(L, B, 11)
        with pytest.raises(frieda_amd.FriedaError) as e:
            gpu_ctx.commit_and_generate_proof(data, seed, pcs(B, 11, pw))
        assert e.value.status == ERR_ARG and not isinstance(e.value, frieda_amd.FriedaPanic)
        assert "log_last_layer_degree_bound > 10" in str(e.value)
        assert_proof(prove(gpu_ctx, L, B, 10), expected(L, B, 10), (L, B))


# ---------------------------------------------------------------- b. the same shapes off the default route
# one (B, last) per last_log in {0, 5, 9, 10, 11} with 0, 1 and 4 inner layers (last_log 0 without an inner layer would be a 2-point domain
# of one coefficient per column: n = 1, which no configuration has)
OFF_ROUTE = [(last + 1 + ni, B, last) for B, last in ((0, 0), (2, 3), (1, 8), (0, 10), (1, 10)) for ni in (0, 1, 4) if last + 1 + ni + B >= 2]


def test_off_route_shapes_are_what_the_comment_says():
    assert len(OFF_ROUTE) == 14
    assert {(route(*s)["last_log"], route(*s)["n_inner"]) for s in OFF_ROUTE} == {(ll, ni) for ll in (0, 5, 9, 10, 11) for ni in (0, 1, 4)} - {(0, 0)}


def test_host_channel_policy(gpu_ctx, expected):
    """set_host_channel(True): the Fiat-Shamir channel on the host between layers, the last layer interpolated on the host"""
    try:
        gpu_ctx.set_host_channel(True)
        for s in OFF_ROUTE:
            got, rep = launches(gpu_ctx, lambda: prove(gpu_ctx, *s))
            assert_proof(got, expected(*s), s)
            assert "fri_tail" not in rep and "small_first" not in rep, (s, rep)
    finally:
        gpu_ctx.set_host_channel(False)
    got, rep = launches(gpu_ctx, lambda: prove(gpu_ctx, *OFF_ROUTE[-1]))
    assert_proof(got, expected(*OFF_ROUTE[-1]))
    assert "fri_tail" in rep  # restored


@pytest.mark.parametrize("knob", ["FRIEDA_NO_SMALL_FUSED", "FRIEDA_HOST_DECOMMIT"])
def test_off_route_knobs_on_their_own_context(expected, knob):
    import frieda_amd

    ctx = frieda_amd.Context(0)
    try:
        ctx.set_option(knob, 1)
        for s in OFF_ROUTE:
            got, rep = launches(ctx, lambda: prove(ctx, *s))
            assert_proof(got, expected(*s), (knob, s))
            assert "fri_tail" in rep, (knob, s)
            assert ("small_first" in rep) == (route(*s)["small"] and knob != "FRIEDA_NO_SMALL_FUSED"), (knob, s, rep)
    finally:
        ctx.close()


# ---------------------------------------------------------------- c. the tail's run length and the top kernel's hand-over
RUN_SHAPES = [(13, 2, 0), (13, 2, 3), (13, 2, 8), (13, 2, 9), (9, 2, 0), (9, 2, 8), (12, 0, 0), (12, 0, 10)]


@pytest.mark.parametrize("top_max_log", [9, 10, 11])
@pytest.mark.parametrize("tail_run_log", [4, 9, 10, 11])
def test_tail_run_length_and_top_hand_over(expected, tail_run_log, top_max_log):
    """FRIEDA_TAIL_RUN_LOG moves layers between the multi-workgroup fold launches and the tail: at 10 and 11 the tail's own trees have 1024
    and 2048 leaves (the full S0 / S1 regions of its level loop), at 4 every layer down to 32 points is a launch of its own.  (L 9, B 2)
    is an 2^11 domain: at 11 the whole commit phase behind the first tree is one tail launch.  FRIEDA_TOP_MAX_LOG moves the hand-over of
    every multi-workgroup tree to the one-workgroup top kernel.  The launch counts show that the layers went where the option sends them."""
    import frieda_amd

    ctx = frieda_amd.Context(0)
    try:
        ctx.set_option("FRIEDA_TAIL_RUN_LOG", tail_run_log)
        ctx.set_option("FRIEDA_TOP_MAX_LOG", top_max_log)
        for s in RUN_SHAPES:
            got, rep = launches(ctx, lambda: prove(ctx, *s))
            assert_proof(got, expected(*s), s)
            assert rep.get("fri_tail") == 1, (s, rep)
            assert (rep.get("tree5_fold_circle", 0), rep.get("tree5_fold_line", 0)) == folds_outside_the_tail(*s, tail_run_log=tail_run_log), (s, rep)
        if tail_run_log == 11:
            # no layer of <= 2^11 points was folded outside the tail: (L 9, B 2) and (L 12, B 0) have none larger
            for s in RUN_SHAPES[4:]:
                assert folds_outside_the_tail(*s, tail_run_log=11) == (0, 0)
            assert folds_outside_the_tail(13, 2, 0, tail_run_log=11) == (1, 2)  # the layers of 2^14, 2^13 and 2^12 points
        data, seed, pw = inputs(12, 0, 11)
        with pytest.raises(frieda_amd.FriedaError) as e:
            ctx.commit_and_generate_proof(data, seed, pcs(0, 11, pw))
        assert e.value.status == ERR_ARG
        assert_proof(prove(ctx, 12, 0, 10), expected(12, 0, 10))
    finally:
        ctx.close()


# ---------------------------------------------------------------- d. batched entry points at the boundary
def _ragged_len(L):
    return exact_len(L) - 47  # another length with the same L


@pytest.mark.parametrize("last", [8, 9, 10])
def test_batched_entry_points_up_to_the_boundary(gpu_ctx, expected, last):
    """(L 13, B 1): last_log 9, 10 and 11 — the largest last layers the batched calls take; every proof equals the oracle's lone proof"""
    import frieda_amd

    L, B = 13, 1
    pw = inputs(L, B, last)[2]
    cfg = pcs(B, last, pw)
    blobs = [inputs(L, B, last, salt)[0] for salt in range(3)]
    seeds = [inputs(L, B, last, salt)[1] for salt in range(3)]
    for got, salt in zip(gpu_ctx.commit_and_generate_proof_batch(blobs, seeds, cfg), range(3)):
        assert_proof(got, expected(L, B, last, salt), ("batch", salt))
    root, proofs = gpu_ctx.commit_and_generate_proofs_for_seeds(blobs[0], [5, 6, 7], cfg)
    for p, s in zip(proofs, [5, 6, 7]):
        assert_proof((root, p), expected(L, B, last, 0, seed=s), ("seeds", s))
    # prove_many: two blobs of one length (a batch of two on one device) and a shorter one of the same L
    many = [blobs[0], blobs[2][: _ragged_len(L)], blobs[1]]
    mc = frieda_amd.MultiContext([0])
    try:
        got = mc.prove_many(many, seeds, cfg)
    finally:
        mc.close()
    assert_proof(got[0], expected(L, B, last, 0, seed=seeds[0]), "many 0")
    assert_proof(got[1], expected(L, B, last, 2, seed=seeds[1], length=_ragged_len(L)), "many 1")
    assert_proof(got[2], expected(L, B, last, 1, seed=seeds[2]), "many 2")


def test_batched_entry_points_beyond_the_boundary(gpu_ctx, expected):
    """(L 14, B 2, last 10): last_log 12, the host channel.  A batch and a call of several seeds are refused (prover.cpp refuses every
    count > 1 without the device channel — one seed is a lone proof and goes through); prove_many proves such blobs one by one."""
    import frieda_amd

    L, B, last = 14, 2, 10
    pw = inputs(L, B, last)[2]
    cfg = pcs(B, last, pw)
    blobs = [inputs(L, B, last, salt)[0] for salt in range(3)]
    seeds = [inputs(L, B, last, salt)[1] for salt in range(3)]
    for call in (lambda: gpu_ctx.commit_and_generate_proof_batch(blobs, seeds, cfg), lambda: gpu_ctx.commit_and_generate_proofs_for_seeds(blobs[0], [5, 6, 7], cfg)):
        with pytest.raises(frieda_amd.FriedaError) as e:
            call()
        assert e.value.status == ERR_ARG and "batches need the device channel" in str(e.value)
        assert_proof(prove(gpu_ctx, L, B, last), expected(L, B, last))  # the context is usable afterwards
    root, proofs = gpu_ctx.commit_and_generate_proofs_for_seeds(blobs[0], [5], cfg)
    assert len(proofs) == 1
    assert_proof((root, proofs[0]), expected(L, B, last, 0, seed=5))
    many = [blobs[0], blobs[2][: _ragged_len(L)], blobs[1]]
    mc = frieda_amd.MultiContext([0])
    try:
        got = mc.prove_many(many, seeds, cfg)
        assert_proof(got[0], expected(L, B, last, 0, seed=seeds[0]), "many 0")
        assert_proof(got[1], expected(L, B, last, 2, seed=seeds[1], length=_ragged_len(L)), "many 1")
        assert_proof(got[2], expected(L, B, last, 1, seed=seeds[2]), "many 2")
        # the handle is usable afterwards, batches included
        again = mc.prove_many([inputs(L, B, 9, salt)[0] for salt in range(2)], [inputs(L, B, 9, salt)[1] for salt in range(2)], pcs(B, 9, inputs(L, B, 9)[2]))
        for g, salt in zip(again, range(2)):
            assert_proof(g, expected(L, B, 9, salt), ("again", salt))
    finally:
        mc.close()
    assert_proof(prove(gpu_ctx, L, B, last), expected(L, B, last))


# ---------------------------------------------------------------- e. device verifiers
def _proof_of(expected, L, B, last):
    import frieda_amd

    return frieda_amd.Proof.deserialize(expected(L, B, last)[1])


# two accepted shapes per last (the matrix above showed the product's proofs of these shapes to be these very bytes), and two that panic
VERIFY_SHAPES = [s for last in range(11) for s in ((last + 3, 1, last), (last + 2, 4, last))] + [(6, 2, 5), (11, 0, 10)]


def test_device_verifiers_on_every_last(gpu_ctx, expected):
    """verify_many / verify_samples_many / verify_pairs_many in calls of 8 proofs of mixed configurations: np = 1 .. 1024 coefficients run
    every bit of the kernel's one-pass fold of last_layer_poly but the top one"""
    assert {s[2] for s in VERIFY_SHAPES} == set(range(11)) and all(s in MATRIX for s in VERIFY_SHAPES)
    order = [VERIFY_SHAPES[(7 * i) % len(VERIFY_SHAPES)] for i in range(len(VERIFY_SHAPES))]  # (7 and 24 are coprime: a permutation)
    assert sorted(order) == sorted(VERIFY_SHAPES)
    for g in range(0, len(order), 8):
        group = order[g : g + 8]
        assert len({(B, last) for _, B, last in group}) >= 4
        proofs = [_proof_of(expected, *s) for s in group]
        seeds = [inputs(*s)[1] for s in group]
        want = [INVARIANT if s[0] == s[2] + 1 else ACCEPTED for s in group]
        check_against_host(gpu_ctx, proofs, seeds, expect=want)
        st, pts = gpu_ctx.verify_pairs_many(proofs, seeds)
        assert list(st) == want
        for i, (p, s) in enumerate(zip(proofs, seeds)):
            r = restate(p, s)
            if want[i] == ACCEPTED:
                assert np.array_equal(pts[i][0], r[0]) and np.array_equal(pts[i][1], r[1]), group[i]
            else:
                assert r is None and pts[i] is None
        # under the neighbour's seed nothing is accepted
        wrong = [x + 1 for x in seeds]
        st = check_against_host(gpu_ctx, proofs, wrong)
        assert ACCEPTED not in set(st)


# oracle-made proofs the product's own prover refuses to make: np = 2048 is the kernel's limit, 4096 and 8192 are beyond it (host route)
FOREIGN = [(13, 1, 11), (14, 0, 11), (15, 2, 11), (14, 1, 12), (15, 1, 13)]


def test_foreign_proofs_with_last_11_to_13_on_both_routes(gpu_ctx, expected):
    proofs = [_proof_of(expected, *s) for s in FOREIGN] + [_proof_of(expected, 13, 1, 10)]
    seeds = [inputs(*s)[1] for s in FOREIGN] + [inputs(13, 1, 10)[1]]
    assert [len(p.last_layer_poly) for p in proofs] == [2048, 2048, 2048, 4096, 8192, 1024]
    res = {}
    try:
        for v in (0, 1 << 31):
            gpu_ctx.set_option("FRIEDA_VERIFY_DEVICE_MIN", v)
            st = check_against_host(gpu_ctx, proofs, seeds, expect=[ACCEPTED] * len(proofs))
            st2, pos = gpu_ctx.verify_samples_many(proofs, seeds)
            stp, pts = gpu_ctx.verify_pairs_many(proofs, seeds)
            assert list(stp) == [ACCEPTED] * len(proofs)
            res[v] = (st.tobytes(), st2.tobytes(), [p.tobytes() for p in pos], [a.tobytes() + b.tobytes() for a, b in pts])
            bad = check_against_host(gpu_ctx, proofs, [x + 1 for x in seeds])
            assert ACCEPTED not in set(bad)
    finally:
        gpu_ctx.set_option("FRIEDA_VERIFY_DEVICE_MIN", 1)
    assert res[0] == res[1 << 31]
    for p, s, (a, b) in zip(proofs, seeds, pts):
        r = restate(p, s)
        assert np.array_equal(a, r[0]) and np.array_equal(b, r[1])


@pytest.mark.parametrize("L,B,last", [(9, 2, 7), (10, 4, 7), (13, 1, 10), (12, 4, 10), (13, 1, 11), (15, 2, 11)], ids=lambda v: str(v))
def test_edited_last_layer_poly_on_the_device(gpu_ctx, expected, L, B, last):
    """the edits of tests/test_last_layer_host.py (where the oracle refuses each of them) in ONE call, between two copies of the good proof:
    every status is the host verifier's, none is accepted, and the rows before and after an edited proof are what they are without it"""
    good = _proof_of(expected, L, B, last)
    seed = inputs(L, B, last)[1]
    names = sorted(EDITS)
    edited = [edited_proof(good, EDITS[k](good.last_layer_poly)) for k in names]
    proofs = [good]
    for m in edited:
        proofs += [m, good]
    seeds = [seed] * len(proofs)
    alone_st, alone_pos = gpu_ctx.verify_samples_many([good], [seed])
    assert list(alone_st) == [ACCEPTED]
    res = {}
    try:
        for v in (0, 1 << 31):
            gpu_ctx.set_option("FRIEDA_VERIFY_DEVICE_MIN", v)
            st = check_against_host(gpu_ctx, proofs, seeds)
            st2, pos = gpu_ctx.verify_samples_many(proofs, seeds)
            for i, k in enumerate(names):
                assert st[2 * i + 1] in (REJECTED, INVARIANT), f"'{k}' is accepted"
            for i in range(0, len(proofs), 2):
                assert st[i] == ACCEPTED and st2[i] == ACCEPTED and np.array_equal(pos[i], alone_pos[0]), i
            res[v] = (st.tobytes(), st2.tobytes())
    finally:
        gpu_ctx.set_option("FRIEDA_VERIFY_DEVICE_MIN", 1)
    assert res[0] == res[1 << 31]
