"""The case table of tests/test_gpu_workspace_history.py and tests/test_gpu_caller_stream.py: one row per ROUTE of the library, at the
smallest shape of the suite's existing tables that reaches it (test_gpu_value_edges.PROOF_SHAPES / FWD_SMALL and its "Reach" list,
test_gpu_buffer_contract's shape lists, cells_util.BLOB_LEN, test_gpu_cells.OPEN_SHAPES, test_gpu_cells_blobs.STRIPE_CASES).

A row is (how to set a context up, one call, the kernels that call must launch).  `run(ctx, oracle)` makes the call and returns
everything the caller can see of it — output bytes, statuses, counts — as a value that compares with ==; it checks that value against
the CPU oracle itself, with the helper the op's own parity test uses (imported, not copied), so a result that equals an earlier one also
equals the oracle.  Level B rows go through test_gpu_buffer_contract.run_case: every device argument sits in a red-zoned allocation
filled with util.poison_bytes, so the caller-owned outputs are position-dependent poison before every call.  Level A outputs are host
arrays; the rows that call the C ABI directly fill them with a sentinel, the Python binding hands the library zeroed ones.

`kernels` are the Scope names of the context's timing report (kernels.h), asserted on the first run.  The module imports without a GPU:
tests/test_workspace_poison_symbols.py checks that every Scope name of frieda_amd/csrc is claimed by a row or listed in EXEMPT."""
import ctypes as C
from dataclasses import dataclass, field

import numpy as np

import cells_util as U
import test_cells_blobs_host as H
from conftest import splitmix64_bytes
from edge_values import BLOBS
from util import blob_len_for

WORDS = (0x00000000, 0xFFFFFFFF, 0x7FFFFFFF)  # the last is P: not canonical, and zero to lazily reducing code
SEED = 5


@dataclass
class Row:
    run: object
    kernels: tuple
    options: dict = field(default_factory=dict)
    host_channel: bool = False
    twiddle_cache: bool = True
    grind_first_log: int = 0
    pass_bytes: int = 0
    ws: tuple = None      # (len, log_blowup, log_last, prove): frieda_workspace_bytes of the row's shape, where that function applies
    arena: bool = True    # False: the entry point plans no workspace (asserted: nothing of the context is there to poison)


ROWS = {}

# kernels no row claims, each with its reason (tests/test_workspace_poison_symbols.py)
EXEMPT = {
    "tree5_node": "finish_tree takes it only above 2^16 nodes, i.e. for trees of 2^21 leaves (32 MB of columns): no small shape; same arguments and "
                  "scratch halves as tree7q_node, which merkle_root/2p18 poisons; test_gpu_shapes' 2^21 .. 2^24 proofs run it against the oracle",
    "ntt_last_tree5": "FRIEDA_NTT_TREE_REG_ONLY form of ntt_last_tree7 (same launch site and workspace; test_gpu_shapes runs the knob)",
}


def setup(ctx, row):
    """a fresh context -> the row's route"""
    for name, value in row.options.items():
        ctx.set_option(name, value)
    ctx.set_host_channel(row.host_channel)
    ctx.set_twiddle_cache(row.twiddle_cache)
    assert ctx._L.frieda_ctx_test_set_grind_first_log(ctx._h, row.grind_first_log) == 0
    assert ctx._L.frieda_ctx_test_set_verify_pass_bytes(ctx._h, row.pass_bytes) == 0


def poison(ctx, word, sticky=1):
    """frieda_ctx_test_poison -> the bytes filled per region (arena, pinned, pinned input, twiddle sets)"""
    out = (C.c_uint64 * 4)()
    rc = ctx._L.frieda_ctx_test_poison(ctx._h, word, sticky, out)
    assert rc == 0, (rc, ctx._L.frieda_last_error(ctx._h))
    return [int(x) for x in out]


def norm(x):
    """anything a row returns -> something that compares with =="""
    if isinstance(x, np.ndarray):
        return (x.dtype.str, x.shape, x.tobytes())
    if isinstance(x, (list, tuple)):
        return tuple(norm(y) for y in x)
    if hasattr(x, "serialize"):
        return x.serialize()
    return x


_CACHE = {}


def cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def cfg_of(pow_bits, blowup, last, nq):
    import frieda_amd

    return frieda_amd.PcsConfig(frieda_amd.FriConfig(blowup, last, nq), pow_bits)


# ---- Level B: the buffer-contract table's builders, one shape each -------------------------------------------------------------------
def levelb(rowname, entry, shape, kernels, **kw):
    import test_gpu_buffer_contract as BC

    def run(ctx, oracle):
        case = cached(("case", entry, shape), lambda: BC.BUILDERS[entry](oracle, shape))
        BC.run_case(ctx, entry, case, {}, rowname)  # outputs against the oracle, zones intact, inputs unchanged
        return None

    ROWS[rowname] = Row(run, kernels, **kw)


levelb("unpack30", "frieda_unpack30", 4097, ("unpack30",), arena=False)
levelb("pack30", "frieda_pack30", 4097, ("pack30",), arena=False)
levelb("evaluate/broadcast", "frieda_circle_evaluate", (0, 4, 4), ("ntt_broadcast",), arena=False)
levelb("evaluate/tile", "frieda_circle_evaluate", (5, 9, 4), ("ntt_pass_last",), arena=False)
levelb("evaluate/tile12", "frieda_circle_evaluate", (12, 16, 4), ("ntt_pass_last",), arena=False)
levelb("evaluate/tile12_strided", "frieda_circle_evaluate", (16, 18, 4), ("ntt_pass_mid", "ntt_pass_last"), arena=False)
levelb("fold2/accumulate", "frieda_circle_evaluate_fold2", (12, 14), ("ntt_last_fold2",), arena=False)
levelb("fold2/accumulate/no_cp", "frieda_circle_evaluate_fold2", (12, 14), ("ntt_last_fold2",), options={"FRIEDA_NTT_NO_CP": 1}, arena=False)
levelb("fold2/three_calls_below_2p12", "frieda_circle_evaluate_fold2", (5, 9), ("ntt_pass_last", "fold_circle", "fold_line"), arena=False)
levelb("interpolate", "frieda_circle_interpolate", (12, 16, 4), ("intt_block",), arena=False)
levelb("interpolate/strided", "frieda_circle_interpolate", (16, 18, 4), ("intt_block",), arena=False)
levelb("interpolate/generic", "frieda_circle_interpolate", (12, 16, 4), ("intt_block",), options={"FRIEDA_INTT_GENERIC": 1}, arena=False)
levelb("interpolate_cells/host_inverse", "frieda_circle_interpolate_cells", (3, 5, 1), ("cells_combine",))
levelb("interpolate_cells/device_solve", "frieda_circle_interpolate_cells", (10, 14, 1), ("cells_inverse", "cells_combine"))
levelb("interpolate_cells_any", "frieda_circle_interpolate_cells_any", (8, 12, 3), ("cells_combine",))
levelb("interpolate_points/lines", "frieda_circle_interpolate_points", (8, 11, 0), ("erasure_sample_lists", "erasure_points", "erasure_lines", "erasure_zeval", "erasure_scatter", "erasure_fold_prefix", "erasure_divide", "erasure_check"),
       options={"FRIEDA_ERASURE_TREE_MIN_LOG": 32})
levelb("interpolate_points/tree", "frieda_circle_interpolate_points", (8, 11, 0), ("erasure_sample_lists", "erasure_lines", "erasure_lines32", "erasure_ze", "erasure_scatter", "erasure_divide", "erasure_check"),
       options={"FRIEDA_ERASURE_TREE_MIN_LOG": 6})
levelb("reconstruct_device", "frieda_reconstruct_device", 1001, ("intt_block", "pack30"))
levelb("reconstruct_cells_device", "frieda_reconstruct_cells_device", 1001, ("cells_combine", "pack30"))
levelb("reconstruct_points_device", "frieda_reconstruct_points_device", 3001, ("erasure_sample_lists", "pack30"))
levelb("merkle_commit", "frieda_merkle_commit", 12, ("tree5_leaf", "tree_top"), arena=False)
levelb("merkle_commit_layer/leaves", "frieda_merkle_commit_layer", (7, False), ("merkle_leaf4",), arena=False)
levelb("merkle_commit_layer/generic", "frieda_merkle_commit_layer", (7, True), ("merkle_generic",))  # (the column pointer table goes through the arena)
levelb("merkle_root", "frieda_merkle_root", 12, ("tree5_leaf", "tree_top"))
levelb("merkle_root/2p18", "frieda_merkle_root", 18, ("tree5_leaf", "tree7q_node", "tree_top"))  # a register-subtree launch, then node launches
levelb("fold_circle_into_line", "frieda_fold_circle_into_line", 12, ("fold_circle",), arena=False)
levelb("fold_line", "frieda_fold_line", 12, ("fold_line",), arena=False)
levelb("bit_reverse_column", "frieda_bit_reverse_column", (12, 4, 5000), ("bit_reverse_column",), arena=False)
levelb("circle_extend", "frieda_circle_extend", (3, 10, 14), ("circle_extend",), arena=False)
levelb("eval_at_point", "frieda_circle_eval_at_point", (4, 12), ("circle_eval_at_point",))
levelb("fri_decompose", "frieda_fri_decompose", 12, ("fri_decompose",))
levelb("dev_gather_device", "frieda_dev_gather_device", (4, 4096), ("gather_rows",), arena=False)
levelb("gather_hashes", "frieda_dev_gather_hashes", (12, 300), ("gather_hashes",))
levelb("decommit_device/small", "frieda_merkle_decommit_device", (10, 20), ("decommit_small",), arena=False)
levelb("decommit_device/multi_block", "frieda_merkle_decommit_device", (12, 600), ("decommit_count", "decommit_scan", "decommit_emit"))
levelb("decommit_device/multi_block_forced", "frieda_merkle_decommit_device", (10, 20), ("decommit_count", "decommit_scan", "decommit_emit"),
       options={"FRIEDA_OPEN_SMALL_MAX": 0})
levelb("commit_device", "frieda_commit_device", 3001, ("small_first",))
levelb("prove_device", "frieda_commit_and_generate_proof_device", 3001, ("small_first", "fri_tail"))
levelb("commit_batch_device", "frieda_commit_batch_device", (70001, 70003, 3), ("unpack30",))
levelb("prove_batch_begin_device", "frieda_prove_batch_begin_device", (70001, 70003, 3), ("unpack30", "fri_tail"))


def _fold2_overwrite(ctx, oracle):
    """frieda_circle_evaluate_fold2 with accumulate = 0: line 1 is an output, and what it held before (poison) must not enter it"""
    import test_gpu_buffer_contract as BC

    L, n = 12, 14

    def build():
        rng = np.random.default_rng(1300 + 32 * L + n)
        coef, a0, a1 = BC.rand_m31(rng, (4, 1 << L)), BC.rand_m31(rng, (4,)), BC.rand_m31(rng, (4,))
        ev = oracle.circle_evaluate(coef, n)
        l1 = oracle.fold_circle_into_line(ev, a0, None)
        l2 = oracle.fold_line(l1, n, a1)
        return BC.Case(size={"d_coeffs": coef.nbytes, "d_evals": ev.nbytes, "d_line1": l1.nbytes, "d_line2": l2.nbytes}, inputs={"d_coeffs": [(0, coef)]},
                       expect={"d_evals": [(0, ev)], "d_line1": [(0, l1)], "d_line2": [(0, l2)]},
                       call=lambda c, a, h: c._L.frieda_circle_evaluate_fold2(c._h, a["d_coeffs"], L, n, a["d_evals"], a0.ctypes.data, 0, a["d_line1"],
                                                                              a1.ctypes.data, a["d_line2"]))

    BC.run_case(ctx, "frieda_circle_evaluate_fold2", cached("fold2 overwrite", build), {}, "fold2/overwrite")


def _merkle_node_layer(ctx, oracle):
    """frieda_merkle_commit_layer over a previous layer alone (no columns): 2^7 nodes from 2^8 hashes"""
    import test_gpu_buffer_contract as BC

    m = 7

    def build():
        prev = np.random.default_rng(1000 + 2 * m).integers(0, 256, (2 << m, 32), dtype=np.uint8)
        exp = oracle.merkle_commit_layer(m, prev, None)
        return BC.Case(size={"d_prev": prev.nbytes, "d_out": exp.nbytes}, inputs={"d_prev": [(0, prev)]}, expect={"d_out": [(0, exp)]},
                       call=lambda c, a, h: c._L.frieda_merkle_commit_layer(c._h, m, a["d_prev"], None, 0, a["d_out"]))

    BC.run_case(ctx, "frieda_merkle_commit_layer", cached("merkle node layer", build), {}, "merkle_commit_layer/nodes")


ROWS["merkle_commit_layer/nodes"] = Row(_merkle_node_layer, ("merkle_node",), arena=False)
ROWS["fold2/overwrite"] = Row(_fold2_overwrite, ("ntt_last_fold2",), arena=False)
ROWS["fold2/overwrite/no_cp"] = Row(_fold2_overwrite, ("ntt_last_fold2",), options={"FRIEDA_NTT_NO_CP": 1}, arena=False)


def _twiddles(ctx, oracle):
    """frieda_precompute_twiddles at 2^16: both tables of the context against the oracle's"""
    n = 16
    tw, itw = cached(("tw", n), lambda: oracle.precompute_twiddles(n))
    p_tw, p_itw = C.c_void_p(), C.c_void_p()
    assert ctx._L.frieda_precompute_twiddles(ctx._h, n, C.byref(p_tw), C.byref(p_itw)) == 0
    got, goti = np.full(tw.size, 0xA5A5A5A5, np.uint32), np.full(tw.size, 0xA5A5A5A5, np.uint32)
    assert ctx._L.frieda_dev_download(ctx._h, got.ctypes.data, p_tw, got.nbytes) == 0
    assert ctx._L.frieda_dev_download(ctx._h, goti.ctypes.data, p_itw, goti.nbytes) == 0
    assert np.array_equal(got, tw.ravel()) and np.array_equal(goti, itw.ravel())
    return norm((got, goti))


ROWS["precompute_twiddles/cache"] = Row(_twiddles, ("gen_twiddles",), arena=False)
ROWS["precompute_twiddles/no_cache"] = Row(_twiddles, ("gen_twiddles",), twiddle_cache=False, arena=False)


def _grind(ctx, oracle):
    """frieda_grind at 12 bits of work (test_gpu_parity.test_grind_returns_minimum_nonce's case): the minimum nonce"""
    def want():
        ch = oracle.Channel()
        oracle.lib().fo_channel_init(C.byref(ch))
        oracle.lib().fo_channel_mix_u64(C.byref(ch), 3)
        return bytes(ch.digest), int(oracle.lib().fo_grind(C.byref(ch), 12))

    digest, exp = cached("grind", want)
    got = C.c_uint64(0xA5A5A5A5A5A5A5A5)
    assert ctx._L.frieda_grind(ctx._h, digest, 12, C.byref(got)) == 0
    assert got.value == exp
    return got.value


ROWS["grind"] = Row(_grind, ("grind",))


# ---- Level A --------------------------------------------------------------------------------------------------------------------------
def _proof_row(shape, blob="ff_then_00", seed=SEED):
    """commit_and_generate_proof of a test_gpu_value_edges.PROOF_SHAPES shape against that file's cached oracle proof"""
    import test_gpu_value_edges as VE

    n_bytes, (pow_bits, blowup, last, nq) = VE.PROOF_SHAPES[shape]

    def run(ctx, oracle):
        root, proof = ctx.commit_and_generate_proof(BLOBS[blob](n_bytes), seed, cfg_of(pow_bits, blowup, last, nq))
        got = (root, proof.serialize())
        assert got == VE.oracle_proof(oracle, blob, shape, seed)
        return got

    return run, (n_bytes, blowup, last, 1)


def _commit_row(shape, blob="ff_then_00"):
    import test_gpu_value_edges as VE

    n_bytes, (_, blowup, last, _) = VE.PROOF_SHAPES[shape]

    def run(ctx, oracle):
        root = ctx.commit(BLOBS[blob](n_bytes), blowup)
        assert root == VE.oracle_proof(oracle, blob, shape)[0]
        return root

    return run, (n_bytes, blowup, last, 0)


_r, _ws = _commit_row("1KiB")
ROWS["commit/small_fused"] = Row(_r, ("small_first",), ws=_ws)
_r, _ws = _commit_row("2p16")
ROWS["commit/general"] = Row(_r, ("unpack30", "ntt_pass_last", "tree_top"), ws=_ws)
_r, _ws = _proof_row("1KiB")
ROWS["prove/small_fused"] = Row(_r, ("small_first", "fri_tail"), ws=_ws)
ROWS["prove/small_general"] = Row(_r, ("unpack30", "fri_tail"), options={"FRIEDA_NO_SMALL_FUSED": 1}, ws=_ws)
_r, _ws = _proof_row("2p16")
ROWS["prove/general"] = Row(_r, ("unpack30", "ntt_pass_last", "tree5_leaf", "tree5_fold_circle", "tree5_fold_line", "fri_tail", "grind", "decommit"), ws=_ws)
ROWS["prove/general/host_channel"] = Row(_r, ("unpack30", "ntt_pass_last", "fold_circle", "fold_line", "grind", "gather"), host_channel=True, ws=_ws)
ROWS["prove/general/host_decommit"] = Row(_r, ("unpack30", "fri_tail", "gather"), options={"FRIEDA_HOST_DECOMMIT": 1}, ws=_ws)
ROWS["prove/general/host_decommit_copy"] = Row(_r, ("unpack30", "fri_tail", "gather"), options={"FRIEDA_HOST_DECOMMIT": 1, "FRIEDA_GATHER_COPY": 1}, ws=_ws)
ROWS["prove/general/tree_levels_skipped"] = Row(_r, ("unpack30", "fri_tail", "decommit"), options={"FRIEDA_TREE_SKIP_LOG": 10, "FRIEDA_TREE_SKIP_LONE_LOG": 10}, ws=_ws)
ROWS["prove/general/tree_levels_skipped/host_decommit"] = Row(
    _r, ("unpack30", "fri_tail", "gather"), options={"FRIEDA_TREE_SKIP_LOG": 10, "FRIEDA_TREE_SKIP_LONE_LOG": 10, "FRIEDA_HOST_DECOMMIT": 1}, ws=_ws)
_r, _ws = _proof_row("30000B")
ROWS["prove/nine_inner_layers"] = Row(_r, ("small_first", "tree5_fold_circle", "tree5_fold_line", "fri_tail", "grind", "decommit"), ws=_ws)


def _grind_retry(ctx, oracle):
    """test_gpu_parity.test_grind_retry_loop's shape: 18 bits of work, first window 2^10 nonces — a lone proof and a batch of six"""
    cfg = cfg_of(18, 4, 0, 8)
    blobs = [splitmix64_bytes(9500 + i, 900).tobytes() for i in range(6)]

    def want():
        out = [oracle.commit_and_generate_proof(b, i, oracle.make_config(18, 4, 0, 8)) for i, b in enumerate(blobs)]
        assert min(p.c.proof_of_work for _, p in out) >= 1 << 10, "no proof leaves the first window"
        return [(bytes(r), p.serialize()) for r, p in out]

    exp = cached("grind retry", want)
    got = [(r, p.serialize()) for r, p in ctx.commit_and_generate_proof_batch(blobs, list(range(6)), cfg)]
    r, p = ctx.commit_and_generate_proof(blobs[0], 0, cfg)
    assert got == exp and (r, p.serialize()) == exp[0]
    return norm((got, r, p))


ROWS["prove/grind_retry"] = Row(_grind_retry, ("small_first", "fri_tail"), grind_first_log=10, ws=(900, 4, 0, 1))


def _batch_row(log_domain):
    """three blobs of cells_util.BLOB_LEN[(log_domain, 4)] proved in one call: at 2^11 the first fold feeds the one-workgroup tail, at 2^12
    a multi-workgroup line fold runs in between (both domains take the fused small-domain first launch)"""
    length = U.BLOB_LEN[(log_domain, 4)]
    blobs = [splitmix64_bytes(4200 + i, length).tobytes() for i in range(3)]
    seeds = [7, 8, 9]

    def run(ctx, oracle):
        def want():
            out = [oracle.commit_and_generate_proof(b, s, oracle.make_config(5, 4, 0, 20)) for b, s in zip(blobs, seeds)]
            return [(bytes(r), p.serialize()) for r, p in out]

        got = [(r, p.serialize()) for r, p in ctx.commit_and_generate_proof_batch(blobs, seeds, cfg_of(5, 4, 0, 20))]
        assert got == cached(("batch", log_domain), want)
        return norm(got)

    return run, (length, 4, 0, 1)


_r, _ws = _batch_row(11)
ROWS["prove_batch/2p11"] = Row(_r, ("small_first", "tree5_fold_circle", "fri_tail", "grind", "decommit"), ws=_ws)
_r, _ws = _batch_row(12)
ROWS["prove_batch/2p12"] = Row(_r, ("small_first", "tree5_fold_circle", "tree5_fold_line", "fri_tail", "grind", "decommit"), ws=_ws)


def _begin_finish(ctx, oracle):
    import test_gpu_value_edges as VE

    n_bytes, (pow_bits, blowup, last, nq) = VE.PROOF_SHAPES["2p16"]
    ctx.prove_begin(BLOBS["ff_then_00"](n_bytes), SEED, cfg_of(pow_bits, blowup, last, nq))
    root, proof = ctx.prove_finish()
    assert (root, proof.serialize()) == VE.oracle_proof(oracle, "ff_then_00", "2p16")
    return root, proof.serialize()


ROWS["prove_begin_finish"] = Row(_begin_finish, ("unpack30", "fri_tail"), ws=(blob_len_for(16), 4, 0, 1))


def _commit_batch_fused(ctx, oracle):
    """test_gpu_value_edges.test_commit_batch_2p16_fused_encode_and_tree's launch: 16 blobs of a 2^16 domain"""
    import test_gpu_value_edges as VE

    kinds = list(BLOBS) * 4
    roots = ctx.commit_batch([BLOBS[k](blob_len_for(16)) for k in kinds], 4)
    assert roots == [VE.oracle_proof(oracle, k, "2p16")[0] for k in kinds]
    return norm(roots)


ROWS["commit_batch/fused_encode_tree"] = Row(_commit_batch_fused, ("unpack30", "ntt_last_tree7"), ws=(blob_len_for(16), 4, 0, 0))


def _prove_batch_fused(ctx, oracle):
    import test_gpu_value_edges as VE

    kinds = list(BLOBS) * 4
    got = ctx.commit_and_generate_proof_batch([BLOBS[k](blob_len_for(16)) for k in kinds], [SEED] * 16, cfg_of(4, 4, 0, 20))
    got = [(r, p.serialize()) for r, p in got]
    assert got == [VE.oracle_proof(oracle, k, "2p16") for k in kinds]
    return norm(got)


ROWS["prove_batch/fused_encode_tree"] = Row(_prove_batch_fused, ("ntt_last_tree7", "fri_tail"), options={"FRIEDA_ENCODE_TREE_FUSION_PROVE": 1},
                                            ws=(blob_len_for(16), 4, 0, 1))


# ---- one blob under many seeds ---------------------------------------------------------------------------------------------------------
def _seeds_row(shape, n_seeds):
    import test_gpu_value_edges as VE

    n_bytes, (pow_bits, blowup, last, nq) = VE.PROOF_SHAPES[shape]
    seeds = list(range(SEED, SEED + n_seeds))

    def run(ctx, oracle):
        data = BLOBS["ff_then_00"](n_bytes)
        with ctx.encode(data, blowup) as enc:
            commitment = enc.commitment
            got = [p.serialize() for p in ctx.prove_seeds(enc, seeds, cfg_of(pow_bits, blowup, last, nq))]
        assert commitment == VE.oracle_proof(oracle, "ff_then_00", shape)[0]
        assert got == [VE.oracle_proof(oracle, "ff_then_00", shape, s)[1] for s in seeds]
        return norm((commitment, got))

    return run


ROWS["prove_seeds/2p16"] = Row(_seeds_row("2p16", 8), ("unpack30", "seeds_first_alpha", "fri_tail"))
ROWS["prove_seeds/2p16/fold_group"] = Row(_seeds_row("2p16", 8), ("unpack30", "seeds_first_alpha", "tree5s_fold_circle", "fri_tail"),
                                          options={"FRIEDA_SEEDS_FOLD_GROUP": 3})
ROWS["prove_seeds/2p16/tree_levels_skipped"] = Row(_seeds_row("2p16", 8), ("unpack30", "seeds_first_alpha", "fri_tail"),
                                                   options={"FRIEDA_TREE_SKIP_LOG": 10, "FRIEDA_TREE_SKIP_LONE_LOG": 10})
ROWS["prove_seeds/2p16/tree_levels_skipped/host_decommit"] = Row(
    _seeds_row("2p16", 8), ("unpack30", "seeds_first_alpha", "fri_tail", "tree5_leaf", "gather"),
    options={"FRIEDA_TREE_SKIP_LOG": 10, "FRIEDA_TREE_SKIP_LONE_LOG": 10, "FRIEDA_HOST_DECOMMIT": 1})
ROWS["prove_seeds/small_fused"] = Row(_seeds_row("1KiB", 8), ("small_first", "seeds_first_alpha", "fri_tail"))


# ---- verify and rebuild ----------------------------------------------------------------------------------------------------------------
def _kib_proofs(oracle, n_seeds=16):
    """the 1 KiB ff_then_00 blob under seeds 1 .. n from the oracle (test_gpu_value_edges.test_1kib_seeds_and_reconstruction's pool), the
    second proof with one evaluation word bumped: (data, root, seeds, proofs)"""
    import frieda_amd
    import test_gpu_value_edges as VE

    def make():
        data = BLOBS["ff_then_00"](1024)
        seeds = list(range(1, n_seeds + 1))
        images = [VE.oracle_proof(oracle, "ff_then_00", "1KiB", s) for s in seeds]
        proofs = [frieda_amd.Proof.deserialize(im) for _, im in images]
        return data, images[0][0], seeds, proofs

    return cached(("kib", n_seeds), make)


def _verify_many(ctx, oracle):
    import test_gpu_value_edges as VE
    import test_gpu_verify_many as VM

    _, root, seeds, proofs = _kib_proofs(oracle)
    mixed = list(proofs)
    mixed[1] = cached("kib bad", lambda: VE._bump_evaluation(proofs[1]))
    st = VM.check_against_host(ctx, mixed, seeds)  # verify_many and verify_samples_many against the host verifier, proof by proof
    assert list(st) == [1, 0] + [1] * (len(seeds) - 2)
    st2, pos = ctx.verify_samples_many(mixed, seeds, expected_commitment=root)
    return norm((st, st2, [p if p is not None else b"" for p in pos]))


def _verify_pairs(ctx, oracle):
    import pairs_util as PU
    import test_gpu_value_edges as VE

    _, root, seeds, proofs = _kib_proofs(oracle)
    mixed = list(proofs)
    mixed[1] = cached("kib bad", lambda: VE._bump_evaluation(proofs[1]))
    rc, status, pos, val, npts = PU.raw_pairs_many(ctx, mixed, seeds, commitment=root)
    assert rc == 0
    for i, (p, s) in enumerate(zip(mixed, seeds)):
        want = cached(("restate", i), lambda: PU.restate(p, s))
        if want is None:
            assert status[i] == PU.REJECTED and npts[i] == 0 and (pos[i] == PU.SENTINEL).all() and (val[i] == PU.SENTINEL).all()
        else:
            k = len(want[0])
            assert status[i] == PU.ACCEPTED and npts[i] == k
            assert np.array_equal(pos[i, :k], want[0]) and np.array_equal(val[i, :k], want[1])
            assert (pos[i, k:] == PU.SENTINEL).all() and (val[i, k:] == PU.SENTINEL).all()
    return norm((status, pos, val, npts))


def _rebuild(pairs):
    def run(ctx, oracle):
        data, root, seeds, proofs = _kib_proofs(oracle)
        k = 8 if pairs else 16  # as test_1kib_seeds_and_reconstruction: 2^7 coefficients per column, 130 points needed
        fn = ctx.reconstruct_from_proof_pairs if pairs else ctx.reconstruct_from_proofs
        out, st, n_points = fn(proofs[:k], seeds[:k], root, len(data))
        assert out == data and set(st.tolist()) == {1} and n_points >= 130
        return norm((out, st, n_points))

    return run


ONE_PROOF = 3000  # bytes of staging budget: below two 1 KiB proofs, so every proof is a pass of its own
ROWS["verify_many"] = Row(_verify_many, ("verify_many",))
ROWS["verify_many/passes"] = Row(_verify_many, ("verify_many",), pass_bytes=ONE_PROOF)
ROWS["verify_pairs_many"] = Row(_verify_pairs, ("verify_many", "verify_pairs_gather"))
ROWS["verify_pairs_many/passes"] = Row(_verify_pairs, ("verify_many", "verify_pairs_gather"), pass_bytes=ONE_PROOF)
ROWS["reconstruct_from_proofs"] = Row(_rebuild(False), ("verify_many", "erasure_sample_lists", "pack30", "small_first"))
ROWS["reconstruct_from_proof_pairs"] = Row(_rebuild(True), ("verify_many", "verify_pairs_gather", "erasure_sample_lists", "pack30", "small_first"))
ROWS["reconstruct_from_proof_pairs/passes"] = Row(_rebuild(True), ("verify_many", "verify_pairs_gather", "erasure_sample_lists", "pack30"), pass_bytes=ONE_PROOF)


def _open_cells(shape):
    """test_gpu_cells.OPEN_SHAPES: encode, then cells of 2^c entries with their paths against the oracle's codeword and tree"""
    import test_gpu_cells as GC

    length, blowup, _ = GC.OPEN_SHAPES[shape]

    def run(ctx, oracle):
        data, ev, layers, n, L = U.codeword(length, blowup)
        out = []
        with ctx.encode(data, blowup) as enc:
            assert enc.commitment == layers[0][0].tobytes()
            for c in (0, 3, 6):
                idx = U.cell_list(n, c, 65, seed=65)
                values, paths = enc.open_cells(ctx, c, idx)
                want_v, want_p = U.open_oracle(ev, layers, c, idx)
                assert values.tobytes() == want_v.tobytes() and paths.tobytes() == want_p.tobytes(), c
                out.append((values, paths))
        return norm(out)

    return run, GC.OPEN_SHAPES[shape][2]


_r, _o = _open_cells("1k")
ROWS["open_cells/small_fused"] = Row(_r, ("small_first", "cells_open_values", "cells_open_paths"), options=_o)
_r, _o = _open_cells("d12_levels_skipped")
ROWS["open_cells/tree_levels_skipped"] = Row(_r, ("small_first", "cells_open_values", "cells_open_paths"), options=_o)
_r, _o = _open_cells("d12_full_tree")
ROWS["open_cells/full_tree"] = Row(_r, ("small_first", "cells_open_values", "cells_open_paths"), options=_o)


def _verify_cells(ctx, oracle):
    """test_gpu_cells.test_verify_many_on_random_bit_flips: 300 cells at 2^12, 200 with a flipped bit — device == host == independent"""
    import test_gpu_cells as GC

    n, c = 12, 3
    root, idx, values, paths = cached("flipped cells", lambda: GC.flipped_call(n, c, 300, 200, seed=2024))
    want = cached("flipped want", lambda: (U.independent_status(root, n, c, idx, values, paths), GC.host_status(root, n, c, idx, values, paths)))
    rc, st = GC.raw_verify_many(ctx, root, n, c, idx, values, paths)
    assert rc == 0 and st.tolist() == want[0].tolist() == want[1].tolist()
    return norm(st)


ROWS["verify_cells_many"] = Row(_verify_cells, ("cells_walk", "cells_roots"))
ROWS["verify_cells_many/passes"] = Row(_verify_cells, ("cells_walk", "cells_roots"), pass_bytes=40000)


def _rebuild_cells(c):
    """test_gpu_cells.test_reconstruct_from_opened_cells at 2^11: the minimum number of cells plus one, one of them corrupted"""
    import test_gpu_cells as GC

    def run(ctx, oracle):
        data, ev, layers, n, L = GC.reconstruct_case(11)
        root = layers[0][0].tobytes()
        need = (1 << (L - c)) + 1 if c else (1 << L) + 2
        rng = np.random.default_rng(300 + n + c)
        pick = rng.choice(1 << (n - c), size=need + 1, replace=False).astype(np.uint32)
        values, paths = U.open_oracle(ev, layers, c, pick)
        t = int(rng.integers(0, need))
        vbad = values.copy()
        vbad[t, 1, 0] ^= 2
        rc, out, st, used = GC.raw_reconstruct(ctx, root, 4, len(data), c, pick, vbad, paths)
        assert rc == 0 and out == data and used == need and np.flatnonzero(st != U.ACCEPTED).tolist() == [t]
        rc2, out2, st2, used2 = GC.raw_reconstruct(ctx, root, 4, len(data), c, pick[:need], vbad[:need], paths[:need])  # too few: refused
        assert rc2 == U.ERR_ARG and used2 == need - 1
        return norm((out, st, used, st2, used2))

    return run


ROWS["reconstruct_from_opened_cells/points"] = Row(_rebuild_cells(0), ("cells_walk", "cells_gather", "erasure_sample_lists", "pack30"))
ROWS["reconstruct_from_opened_cells/cells"] = Row(_rebuild_cells(3), ("cells_walk", "cells_roots", "cells_gather", "erasure_sample_lists", "erasure_zeval_cells", "pack30"))
ROWS["reconstruct_from_opened_cells/passes"] = Row(_rebuild_cells(3), ("cells_walk", "cells_roots", "cells_gather", "erasure_sample_lists", "pack30"), pass_bytes=4000)


def _open_blobs(ctx, oracle):
    """frieda_open_cells_blobs over three blobs of a 2^11 domain (test_cells_blobs_host.block) against each blob's own codeword and tree"""
    import frieda_amd

    n = 11
    blobs = H.block(n, 4)
    encs = [ctx.encode(bl[0], 4) for bl in blobs]
    out = []
    try:
        for c in (0, 3, 6):
            bidx, idx = H.pair_list(n, c, 65, seed=65)
            values, paths = frieda_amd.open_cells_blobs(ctx, encs, c, bidx, idx)
            want_v, want_p = H.open_pairs(blobs, c, bidx, idx)
            assert values.tobytes() == want_v.tobytes() and paths.tobytes() == want_p.tobytes(), c
            out.append((values, paths))
    finally:
        for e in encs:
            e.close()
    return norm(out)


ROWS["open_cells_blobs"] = Row(_open_blobs, ("small_first", "cells_open_blobs_values", "cells_open_blobs_paths"))


def _verify_blobs(ctx, oracle):
    """test_gpu_cells_blobs.test_verify_blobs_many_on_random_bit_flips' call: device == host == independent"""
    import test_gpu_cells_blobs as GB

    n, c = 12, 3
    coms, bidx, idx, values, paths = cached("flipped pairs", lambda: GB.flipped_pairs(n, c, 3, 300, 200, seed=2024))
    return norm(GB.three_way(ctx, coms, n, c, bidx, idx, values, paths))  # (asserts the three agree; returns the status)


ROWS["verify_cells_blobs_many"] = Row(_verify_blobs, ("cells_walk_blobs", "cells_roots"))
ROWS["verify_cells_blobs_many/passes"] = Row(_verify_blobs, ("cells_walk_blobs", "cells_roots"), pass_bytes=40000)


def _stripes(multi_pass):
    """test_gpu_cells_blobs.STRIPE_CASES (11, 4, 3, 3): the minimum number of stripes plus one, one cell of one blob corrupted"""
    import test_gpu_cells_blobs as GB

    n, blowup, k, c = 11, 4, 3, 3
    assert (n, blowup, k, c) in GB.STRIPE_CASES

    def run(ctx, oracle):
        blobs = H.block(n, blowup, k=k)
        coms = H.commitments_of(blobs)
        length, L = len(blobs[0][0]), n - blowup
        need = (1 << (L - c)) + 1
        rng = np.random.default_rng(400 + n + c + k)
        pick = rng.choice(1 << (n - c), size=need + 1, replace=False).astype(np.uint32)
        values, paths = cached("stripes opened", lambda: GB.open_stripes_oracle(blobs, c, pick))
        t, b = int(rng.integers(0, need)), int(rng.integers(0, k))
        vbad = values.copy()
        vbad[t, b, 1, 0] ^= 2
        rc, out, st, used = GB.raw_stripes(ctx, coms, blowup, length, c, pick, vbad, paths)
        assert rc == 0 and out == [bl[0] for bl in blobs] and used == need and np.argwhere(st != U.ACCEPTED).tolist() == [[t, b]]
        rc2, _, st2, used2 = GB.raw_stripes(ctx, coms, blowup, length, c, pick[:need], vbad[:need], paths[:need])
        assert rc2 == U.ERR_ARG and used2 == need - 1
        return norm((out, st, used, st2, used2))

    per = max(1, ((1 << (n - blowup - c)) + 1) // 3)
    return run, (per * k * (8 + (16 << c) + 32 * (n - c)) if multi_pass else 0)


_STRIPE_KERNELS = ("cells_walk_blobs", "cells_roots", "cells_stripe_accept", "cells_stripe_gather", "erasure_sample_lists", "pack30", "small_first")
_r, _pb = _stripes(False)
ROWS["reconstruct_blobs_from_opened_stripes"] = Row(_r, _STRIPE_KERNELS)
_r, _pb = _stripes(True)
ROWS["reconstruct_blobs_from_opened_stripes/passes"] = Row(_r, _STRIPE_KERNELS, pass_bytes=_pb)
