"""GPU: the buffer contract of the C ABI's device pointers (include/frieda_hip.h, above Level B) — every entry point that takes a
device pointer, with every device argument inside a red-zoned, poisoned allocation (util.GuardedBuf) and at the smallest offsets its
alignment class allows.

One table (TABLE) names, per entry point, every device-pointer parameter with its role (in / out / inout) and alignment class:

    byte    any address                       offsets +1, +2, +3
    word    4-byte aligned                    offsets +4, +8
    hash16  16-byte aligned (32-byte hashes)  offset +16; +4 must be refused with FRIEDA_ERR_ARG and nothing written
    u64     8-byte aligned (64-bit indices)   offset +8;  +4 refused likewise

For every row and shape the call runs with all offsets 0 (the red-zone check of the fast routes), the inputs only offset, the outputs
only, and both — the dispatch sites OR the input and output addresses together, so the mixed cases reach other kernels than the
both-offset case — and after every call: (a) outputs bit-equal to the CPU oracle, (b) both zones (and the offset slack) of every buffer
still poison, (c) every `in` payload unchanged, (d) — through the poison — outputs independent of what the output buffer held before.

tests/test_buffer_contract_table.py (no GPU) checks the table against the header: this module must import without a GPU."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass, field

import numpy as np
import pytest

from conftest import splitmix64_bytes
from test_levelb_opening_symbols import stwo_decommit_walk
from util import ZONE, GuardedBuf, poison_bytes

P = (1 << 31) - 1
ERR_ARG = 1

OFFSETS = {"byte": (1, 2, 3), "word": (4, 8), "hash16": (16,), "u64": (8,)}
REFUSED_OFFSET = {"hash16": 4, "u64": 4}  # classes whose header text asks for more than a word: a word offset is an argument error

# entry point -> device-pointer parameters -> (role, alignment class).  A key may carry a "[variant]" suffix (same function, other
# aliasing); the part before it is the function's name in the header.
TABLE = {
    "frieda_unpack30": {"d_bytes": ("in", "byte"), "d_coef": ("out", "word")},
    "frieda_pack30": {"d_felts": ("in", "word"), "d_bytes": ("out", "byte")},
    "frieda_circle_evaluate": {"d_coef": ("in", "word"), "d_out": ("out", "word")},
    "frieda_circle_interpolate": {"d_block": ("in", "word"), "d_coef": ("out", "word")},
    "frieda_circle_interpolate_cells": {"d_cells": ("in", "word"), "d_coef": ("out", "word")},
    "frieda_circle_interpolate_cells_any": {"d_cells": ("in", "word"), "d_coef": ("out", "word")},
    "frieda_circle_interpolate_points": {"d_cells": ("in", "word"), "d_coef": ("out", "word")},
    "frieda_reconstruct_device": {"d_block": ("in", "word"), "d_out_bytes": ("out", "byte")},
    "frieda_reconstruct_cells_device": {"d_cells": ("in", "word"), "d_out_bytes": ("out", "byte")},
    "frieda_reconstruct_points_device": {"d_cells": ("in", "word"), "d_out_bytes": ("out", "byte")},
    "frieda_merkle_commit": {"d_cols": ("in", "word"), "d_layers": ("out", "hash16")},
    "frieda_merkle_root": {"d_cols": ("in", "word"), "d_root": ("out", "word")},  # (the header's exception: the root is stored by words)
    "frieda_merkle_commit_layer": {"d_prev": ("in", "hash16"), "d_cols": ("in", "word"), "d_out": ("out", "hash16")},
    "frieda_fold_circle_into_line": {"d_dst": ("inout", "word"), "d_src": ("in", "word")},
    "frieda_fold_line": {"d_src": ("in", "word"), "d_dst": ("out", "word")},
    "frieda_circle_evaluate_fold2": {"d_coeffs": ("in", "word"), "d_evals": ("out", "word"), "d_line1": ("inout", "word"), "d_line2": ("out", "word")},
    "frieda_bit_reverse_column": {"d_cols": ("inout", "word")},
    "frieda_circle_extend": {"d_coef": ("in", "word"), "d_out": ("out", "word")},
    "frieda_circle_eval_at_point": {"d_coef": ("in", "word")},
    "frieda_fri_decompose": {"d_eval": ("in", "word"), "d_g": ("out", "word")},
    "frieda_fri_decompose[in place]": {"d_eval": ("inout", "word")},  # d_g = d_eval
    "frieda_dev_gather_device": {"d_cols": ("in", "word"), "d_idx": ("in", "u64"), "d_out": ("out", "word")},
    "frieda_dev_gather_hashes": {"d_layer": ("in", "hash16")},
    "frieda_merkle_decommit_device": {"d_layers": ("in", "hash16"), "d_cols": ("in", "word"), "d_positions": ("in", "word"),
                                      "d_out_values": ("out", "word"), "d_out_hashes": ("out", "hash16"), "d_n_hashes": ("out", "word")},
    "frieda_commit_device": {"d_data": ("in", "byte"), "d_out_root": ("out", "word")},
    "frieda_commit_and_generate_proof_device": {"d_data": ("in", "byte")},
    "frieda_commit_batch_device": {"d_data": ("in", "byte")},
    "frieda_prove_batch_begin_device": {"d_data": ("in", "byte")},
}


def offset_combinations(params, k_max=3):
    """[(label, {param: byte offset})]: all 0; inputs only; outputs only; both — at every offset of the parameters' classes (an inout
    parameter moves with either side); combinations that coincide are run once."""
    seen, out = set(), []
    for which in ("none", "in", "out", "both"):
        for k in range(k_max):
            offs = {}
            for name, (role, cls) in params.items():
                hit = which == "both" or (which == "in" and role != "out") or (which == "out" and role != "in")
                lst = OFFSETS[cls]
                offs[name] = lst[min(k, len(lst) - 1)] if hit and which != "none" else 0
            key = tuple(sorted(offs.items()))
            if key not in seen:
                seen.add(key)
                out.append((f"{which}+{k}" if which != "none" else "aligned", offs))
    return out


@dataclass
class Case:
    """One call: `inputs[param]` = [(byte offset in the payload, array)] uploaded before it, `size[param]` the payload bytes of every
    device argument, `call(ctx, addr, host)` -> status with addr[param] the device address and `host` a dict for host-side results,
    `expect[param]` = [(byte offset, array)] the payload must hold afterwards, `expect_host` what `host` must hold; everything of an
    out / inout payload outside `expect` must still be poison."""
    size: dict
    call: object
    inputs: dict = field(default_factory=dict)
    expect: dict = field(default_factory=dict)
    expect_host: dict = field(default_factory=dict)
    only: tuple = ()  # labels of the offset combinations to run (empty: all)
    k_max: int = 3


def rand_m31(rng, shape):
    return rng.integers(0, P, shape, dtype=np.uint32)


def _oracle_cols(fn, n_items):
    """oracle work per column on a few host threads (the C oracle releases the GIL)"""
    with ThreadPoolExecutor(max_workers=6) as ex:
        return list(ex.map(fn, range(n_items)))


def _gaps(nbytes, segments):
    """byte ranges of [0, nbytes) outside the (offset, array) segments"""
    gaps, pos = [], 0
    for at, arr in sorted(((a, np.ascontiguousarray(x)) for a, x in segments), key=lambda s: s[0]):
        if at > pos:
            gaps.append((pos, at))
        pos = max(pos, at + arr.nbytes)
    if pos < nbytes:
        gaps.append((pos, nbytes))
    return gaps


def run_case(ctx, name, case, offs, label):
    from frieda_amd.api import _check

    params = TABLE[name]
    bufs = {}
    for p in params:
        if p not in case.size:
            continue  # an optional argument this shape passes as NULL
        bufs[p] = GuardedBuf(ctx, case.size[p], offs.get(p, 0))
        for at, arr in case.inputs.get(p, []):
            bufs[p].upload(arr, at)
    host = {}
    rc = case.call(ctx, {p: b.ptr.value for p, b in bufs.items()}, host)
    _check(rc, ctx._h)
    ctx.synchronize()
    tag = f"{name} [{label}: {offs}]"
    for p, segs in case.expect.items():  # (a) + (d)
        for at, exp in segs:
            exp = np.ascontiguousarray(exp)
            got = bufs[p]._download(at, at + exp.nbytes)
            assert np.array_equal(got, exp.reshape(-1).view(np.uint8)), f"{tag}: {p} differs from the oracle"
    for k, exp in case.expect_host.items():
        assert np.array_equal(host[k], exp) if isinstance(exp, np.ndarray) else host[k] == exp, f"{tag}: host result {k} differs from the oracle"
    for p, b in bufs.items():  # (b), (c)
        role = params[p][0]
        b.assert_zones_intact(f"{tag}: {p}")
        if role == "in":
            for at, arr in case.inputs.get(p, []):
                assert at == 0
                b.assert_payload_equals(arr, f"{tag}: {p}")
            b.assert_poison_inside(_gaps(case.size[p], case.inputs.get(p, [])), f"{tag}: {p} (bytes of the input buffer no one uploaded)")
        else:
            b.assert_poison_inside(_gaps(case.size[p], case.expect.get(p, [])), f"{tag}: {p} (bytes the call does not document as written)")
    for b in bufs.values():
        b.free()


def run_refusals(ctx, name, case):
    """(iii): a parameter the header wants 8 / 16-byte aligned, 4 bytes off: FRIEDA_ERR_ARG before any launch, outputs untouched"""
    params = TABLE[name]
    for bad, (_, cls) in params.items():
        if cls not in REFUSED_OFFSET or bad not in case.size:
            continue
        bufs = {p: GuardedBuf(ctx, case.size[p], REFUSED_OFFSET[cls] if p == bad else 0) for p in params if p in case.size}
        for p, b in bufs.items():
            for at, arr in case.inputs.get(p, []):
                b.upload(arr, at)
        rc = case.call(ctx, {p: b.ptr.value for p, b in bufs.items()}, {})
        ctx.synchronize()
        assert rc == ERR_ARG, f"{name}: {bad} at +{REFUSED_OFFSET[cls]} bytes gave status {rc}, not FRIEDA_ERR_ARG"
        for p, b in bufs.items():
            b.assert_zones_intact(f"{name} refused ({bad} misaligned): {p}")
            b.assert_poison_inside(_gaps(case.size[p], case.inputs.get(p, [])), f"{name} refused ({bad} misaligned): {p}")
            for at, arr in case.inputs.get(p, []):
                got = b._download(at, at + np.ascontiguousarray(arr).nbytes)
                assert np.array_equal(got, np.ascontiguousarray(arr).reshape(-1).view(np.uint8)), f"{name} refused: {p} modified"
            b.free()


def drive(ctx, name, case):
    ran = 0
    for label, offs in offset_combinations(TABLE[name], case.k_max):
        if case.only and label not in case.only:
            continue
        run_case(ctx, name, case, offs, label)
        ran += 1
    assert ran >= 1, f"{name}: no offset combination selected by only={case.only}"
    run_refusals(ctx, name, case)


# ---- the rows ------------------------------------------------------------------------------------------------------------------------
BUILDERS, SHAPES = {}, {}


def row(name, shapes):
    def deco(fn):
        BUILDERS[name], SHAPES[name] = fn, shapes
        return fn

    return deco


# transforms straddle the pass planner's thresholds (last pass of <= 12 layers, strided passes above it, fast kernels from 12 layers on)
TRANSFORM_LN = [(3, 5), (11, 12), (12, 16), (13, 17), (16, 20), (17, 18)]
TRANSFORM_SHAPES = [(L, n, c) for L, n in TRANSFORM_LN for c in (1, 3, 4)] + [(18, 22, 4)]  # 2^22: the large unaligned route, word offset only
TREE_LOGS = [0, 1, 5, 9, 10, 12, 16, 18]
FOLD_LOGS = [2, 3, 12, 16, 20]


def _trim(n, big=None):
    """offset combinations of a shape on a 2^n domain: all of them up to 2^20; the 2^22 shapes (one transform, one tree) run with
    every pointer at its word offset only — the large unaligned routes, which run nowhere else"""
    return {"only": ("both+0",)} if n >= 22 else {}


@row("frieda_unpack30", [4096, 4097, 4098, 4099, 262147])
def _unpack30(oracle, n_bytes):
    data = splitmix64_bytes(11 + n_bytes, n_bytes)
    coef, _ = oracle.polynomial_from_bytes(data)
    coef = coef.ravel()
    return Case(size={"d_bytes": n_bytes, "d_coef": coef.nbytes}, inputs={"d_bytes": [(0, data)]}, expect={"d_coef": [(0, coef)]},
                call=lambda ctx, a, h: ctx._L.frieda_unpack30(ctx._h, a["d_bytes"], n_bytes, a["d_coef"], coef.size))


@row("frieda_pack30", [4096, 4097, 4098, 4099, 65539])
def _pack30(oracle, n_bytes):
    rng = np.random.default_rng(n_bytes)
    felts = rng.integers(0, 1 << 30, (8 * n_bytes + 29) // 30, dtype=np.uint32)
    exp = np.frombuffer(oracle.felts_to_bytes(felts, n_bytes), dtype=np.uint8)
    return Case(size={"d_felts": felts.nbytes, "d_bytes": n_bytes}, inputs={"d_felts": [(0, felts)]}, expect={"d_bytes": [(0, exp)]},
                call=lambda ctx, a, h: ctx._L.frieda_pack30(ctx._h, a["d_felts"], felts.size, a["d_bytes"], n_bytes))


@row("frieda_circle_evaluate", TRANSFORM_SHAPES)
def _evaluate(oracle, shape):
    L, n, ncols = shape
    coef = rand_m31(np.random.default_rng(100 * L + n + ncols), (ncols, 1 << L))
    tw, _ = oracle.precompute_twiddles(n)
    exp = np.concatenate(_oracle_cols(lambda c: oracle.circle_evaluate(coef[c : c + 1], n, tw), ncols))
    return Case(size={"d_coef": coef.nbytes, "d_out": exp.nbytes}, inputs={"d_coef": [(0, coef)]}, expect={"d_out": [(0, exp)]},
                call=lambda ctx, a, h: ctx._L.frieda_circle_evaluate(ctx._h, a["d_coef"], ncols, L, n, a["d_out"]), **_trim(n))


@row("frieda_circle_interpolate", TRANSFORM_SHAPES)
def _interpolate(oracle, shape):
    L, n, ncols = shape
    block = rand_m31(np.random.default_rng(200 * L + n + ncols), (ncols, 1 << L))
    k = (1 << (n - L)) - 1
    _, itw = oracle.precompute_twiddles(n)
    exp = np.concatenate(_oracle_cols(lambda c: oracle.circle_interpolate_block(block[c : c + 1], n, k, itw), ncols))
    return Case(size={"d_block": block.nbytes, "d_coef": exp.nbytes}, inputs={"d_block": [(0, block)]}, expect={"d_coef": [(0, exp)]},
                call=lambda ctx, a, h: ctx._L.frieda_circle_interpolate(ctx._h, a["d_block"], ncols, L, n, k, a["d_coef"]), **_trim(n))


def _cells_of(oracle, L, n, m, n_cells, seed, ncols=4, coef=None):
    rng = np.random.default_rng(seed)
    if coef is None:
        coef = rand_m31(rng, (ncols, 1 << L))
    ev = oracle.circle_evaluate(coef, n)
    idx = rng.permutation(1 << (n - m))[:n_cells].astype(np.uint32)
    cells = np.ascontiguousarray(np.stack([ev[:, int(c) << m : (int(c) + 1) << m] for c in idx]))  # [n_cells, ncols, 2^m]
    return coef, cells, idx


@row("frieda_circle_interpolate_cells", [(3, 5, 1), (10, 14, 5)])
def _cells(oracle, shape):
    L, n, m = shape
    coef, cells, idx = _cells_of(oracle, L, n, m, 1 << (L - m), 300 + L)
    exp = oracle.reconstruct_cells(cells, idx, n, L)
    assert np.array_equal(exp, coef)
    return Case(size={"d_cells": cells.nbytes, "d_coef": exp.nbytes}, inputs={"d_cells": [(0, cells)]}, expect={"d_coef": [(0, exp)]},
                call=lambda ctx, a, h: ctx._L.frieda_circle_interpolate_cells(ctx._h, a["d_cells"], idx.ctypes.data, idx.size, 4, m, L, n, a["d_coef"]))


@row("frieda_circle_interpolate_cells_any", [(3, 5, 1), (8, 12, 3)])
def _cells_any(oracle, shape):
    L, n, m = shape
    R = 1 << (L - m)
    coef, cells, idx = _cells_of(oracle, L, n, m, R + 2, 350 + L)
    exp = oracle.reconstruct_cells(cells[:R], idx[:R], n, L)  # with whole cells (m >= 1) any R distinct ones are independent: the first R are taken
    return Case(size={"d_cells": cells.nbytes, "d_coef": exp.nbytes}, inputs={"d_cells": [(0, cells)]}, expect={"d_coef": [(0, exp)]},
                call=lambda ctx, a, h: ctx._L.frieda_circle_interpolate_cells_any(ctx._h, a["d_cells"], idx.ctypes.data, idx.size, 4, m, L, n, a["d_coef"], None))


def _points_expected(oracle, cells, idx, n, L):
    vals = np.ascontiguousarray(cells[:, :, 0])  # log_cell 0: [n_pts, ncols]
    return oracle.reconstruct_points(vals, idx, n, L)


@row("frieda_circle_interpolate_points", [(3, 5, 0), (8, 11, 0)])
def _points(oracle, shape):
    L, n, m = shape
    coef, cells, idx = _cells_of(oracle, L, n, m, (1 << L) + 2, 400 + L)
    exp = _points_expected(oracle, cells, idx, n, L)
    assert np.array_equal(exp, coef)
    return Case(size={"d_cells": cells.nbytes, "d_coef": exp.nbytes}, inputs={"d_cells": [(0, cells)]}, expect={"d_coef": [(0, exp)]},
                call=lambda ctx, a, h: ctx._L.frieda_circle_interpolate_points(ctx._h, a["d_cells"], idx.ctypes.data, idx.size, 4, m, L, n, a["d_coef"]))


def _blob_poly(oracle, n_bytes, seed):
    data = splitmix64_bytes(seed, n_bytes)
    coef, L = oracle.polynomial_from_bytes(data)
    return data, coef, L


@row("frieda_reconstruct_device", [1001, 61443])  # len % 4 = 1, 3
def _reconstruct(oracle, n_bytes):
    data, coef, L = _blob_poly(oracle, n_bytes, 500 + n_bytes)
    n = L + 2
    ev = oracle.circle_evaluate(coef, n)
    k = 2
    block = np.ascontiguousarray(ev[:, k << L : (k + 1) << L])
    exp = np.frombuffer(oracle.felts_to_bytes(oracle.circle_interpolate_block(block, n, k), n_bytes), dtype=np.uint8)
    assert np.array_equal(exp, data)
    return Case(size={"d_block": block.nbytes, "d_out_bytes": n_bytes}, inputs={"d_block": [(0, block)]}, expect={"d_out_bytes": [(0, exp)]},
                call=lambda ctx, a, h: ctx._L.frieda_reconstruct_device(ctx._h, a["d_block"], L, n, k, n_bytes, a["d_out_bytes"]))


@row("frieda_reconstruct_cells_device", [1001, 30003])  # len % 4 = 1, 3
def _reconstruct_cells(oracle, n_bytes):
    data, coef, L = _blob_poly(oracle, n_bytes, 600 + n_bytes)
    n, m = L + 2, L - 3
    _, cells, idx = _cells_of(oracle, L, n, m, 8, 610 + L, coef=coef)
    exp = np.frombuffer(oracle.felts_to_bytes(oracle.reconstruct_cells(cells, idx, n, L), n_bytes), dtype=np.uint8)
    assert np.array_equal(exp, data)
    return Case(size={"d_cells": cells.nbytes, "d_out_bytes": n_bytes}, inputs={"d_cells": [(0, cells)]}, expect={"d_out_bytes": [(0, exp)]},
                call=lambda ctx, a, h: ctx._L.frieda_reconstruct_cells_device(ctx._h, a["d_cells"], idx.ctypes.data, 8, m, L, n, n_bytes, a["d_out_bytes"]))


@row("frieda_reconstruct_points_device", [117, 3001])  # (the oracle's point route is quadratic in the domain: small blobs)
def _reconstruct_points(oracle, n_bytes):
    data, coef, L = _blob_poly(oracle, n_bytes, 700 + n_bytes)
    n = L + 2
    _, cells, idx = _cells_of(oracle, L, n, 0, (1 << L) + 2, 710 + L, coef=coef)
    exp = np.frombuffer(oracle.felts_to_bytes(_points_expected(oracle, cells, idx, n, L), n_bytes), dtype=np.uint8)
    assert np.array_equal(exp, data)
    return Case(size={"d_cells": cells.nbytes, "d_out_bytes": n_bytes}, inputs={"d_cells": [(0, cells)]}, expect={"d_out_bytes": [(0, exp)]},
                call=lambda ctx, a, h: ctx._L.frieda_reconstruct_points_device(ctx._h, a["d_cells"], idx.ctypes.data, idx.size, 0, L, n, n_bytes, a["d_out_bytes"]))


def _tree_image(oracle, cols):
    """frieda_merkle_commit's buffer from the oracle's layers: leaves first, root last"""
    layers = oracle.merkle_commit(cols)
    return np.concatenate([layers[l].reshape(-1) for l in range(len(layers) - 1, -1, -1)]), layers


@row("frieda_merkle_commit", TREE_LOGS)
def _merkle_commit(oracle, m):
    cols = rand_m31(np.random.default_rng(800 + m), (4, 1 << m))
    image, _ = _tree_image(oracle, cols)
    return Case(size={"d_cols": cols.nbytes, "d_layers": image.nbytes}, inputs={"d_cols": [(0, cols)]}, expect={"d_layers": [(0, image)]},
                call=lambda ctx, a, h: ctx._L.frieda_merkle_commit(ctx._h, a["d_cols"], m, a["d_layers"]), **_trim(m))


@row("frieda_merkle_root", TREE_LOGS + [22])  # 2^22: the unaligned tree route at size, word offset only
def _merkle_root(oracle, m):
    cols = rand_m31(np.random.default_rng(900 + m), (4, 1 << m))
    root = oracle.merkle_commit(cols)[0].reshape(-1)
    return Case(size={"d_cols": cols.nbytes, "d_root": 32}, inputs={"d_cols": [(0, cols)]}, expect={"d_root": [(0, root)]},
                call=lambda ctx, a, h: ctx._L.frieda_merkle_root(ctx._h, a["d_cols"], m, a["d_root"]), **_trim(m))


@row("frieda_merkle_commit_layer", [(m, prev) for m in (0, 1, 2, 3, 7, 12) for prev in (False, True)])
def _merkle_layer(oracle, shape):
    """the four columns are sub-slices of ONE SecureColumn buffer [4][2^log_size], as an stwo caller passes them: at log_size 0 and 1
    column c starts 4 c and 8 c bytes into it"""
    m, with_prev = shape
    rng = np.random.default_rng(1000 + 2 * m + with_prev)
    cols = rand_m31(rng, (4, 1 << m))
    prev = rng.integers(0, 256, (2 << m, 32), dtype=np.uint8) if with_prev else None
    exp = oracle.merkle_commit_layer(m, prev, cols)
    size = {"d_cols": cols.nbytes, "d_out": exp.nbytes}
    inputs = {"d_cols": [(0, cols)]}
    if with_prev:
        size["d_prev"], inputs["d_prev"] = prev.nbytes, [(0, prev)]

    def call(ctx, a, h):
        ptrs = (C.c_void_p * 4)(*[a["d_cols"] + (4 * c << m) for c in range(4)])
        return ctx._L.frieda_merkle_commit_layer(ctx._h, m, a.get("d_prev"), ptrs, 4, a["d_out"])

    return Case(size=size, inputs=inputs, expect={"d_out": [(0, exp)]}, call=call)


@row("frieda_fold_circle_into_line", FOLD_LOGS)
def _fold_circle(oracle, n):
    rng = np.random.default_rng(1100 + n)
    src, dst0, alpha = rand_m31(rng, (4, 1 << n)), rand_m31(rng, (4, 1 << (n - 1))), rand_m31(rng, (4,))
    exp = oracle.fold_circle_into_line(src, alpha, dst0.copy())
    return Case(size={"d_dst": dst0.nbytes, "d_src": src.nbytes}, inputs={"d_dst": [(0, dst0)], "d_src": [(0, src)]}, expect={"d_dst": [(0, exp)]},
                call=lambda ctx, a, h: ctx._L.frieda_fold_circle_into_line(ctx._h, a["d_dst"], a["d_src"], n, alpha.ctypes.data), **_trim(n))


@row("frieda_fold_line", FOLD_LOGS)
def _fold_line(oracle, n):
    m = n - 1
    rng = np.random.default_rng(1200 + n)
    src, alpha = rand_m31(rng, (4, 1 << m)), rand_m31(rng, (4,))
    exp = oracle.fold_line(src, n, alpha)
    return Case(size={"d_src": src.nbytes, "d_dst": exp.nbytes}, inputs={"d_src": [(0, src)]}, expect={"d_dst": [(0, exp)]},
                call=lambda ctx, a, h: ctx._L.frieda_fold_line(ctx._h, a["d_src"], m, n, alpha.ctypes.data, a["d_dst"]), **_trim(n))


@row("frieda_circle_evaluate_fold2", [(5, 9), (12, 14), (13, 17), (16, 20)])
def _fold2(oracle, shape):
    """expected: the three separate operations of the oracle — an unaligned buffer takes the three-call route and must give the same"""
    L, n = shape
    rng = np.random.default_rng(1300 + 32 * L + n)
    coef, line1_0, a0, a1 = rand_m31(rng, (4, 1 << L)), rand_m31(rng, (4, 1 << (n - 1))), rand_m31(rng, (4,)), rand_m31(rng, (4,))
    tw, _ = oracle.precompute_twiddles(n)
    ev = np.concatenate(_oracle_cols(lambda c: oracle.circle_evaluate(coef[c : c + 1], n, tw), 4))
    l1 = oracle.fold_circle_into_line(ev, a0, line1_0.copy())
    l2 = oracle.fold_line(l1, n, a1)
    return Case(size={"d_coeffs": coef.nbytes, "d_evals": ev.nbytes, "d_line1": l1.nbytes, "d_line2": l2.nbytes},
                inputs={"d_coeffs": [(0, coef)], "d_line1": [(0, line1_0)]}, expect={"d_evals": [(0, ev)], "d_line1": [(0, l1)], "d_line2": [(0, l2)]},
                call=lambda ctx, a, h: ctx._L.frieda_circle_evaluate_fold2(ctx._h, a["d_coeffs"], L, n, a["d_evals"], a0.ctypes.data, 1, a["d_line1"],
                                                                           a1.ctypes.data, a["d_line2"]), **_trim(n))


@row("frieda_bit_reverse_column", [(5, 3, 40), (12, 4, 5000), (13, 2, 8200), (16, 1, 1 << 16)])
def _bit_reverse(oracle, shape):
    """stride > 2^log_size: the gap words between the columns are red zones too (nothing is uploaded there and nothing may be written)"""
    log_size, ncols, stride = shape
    cols = rand_m31(np.random.default_rng(1400 + log_size), (ncols, 1 << log_size))
    segs_in = [(4 * c * stride, cols[c]) for c in range(ncols)]
    segs_out = [(4 * c * stride, oracle.bit_reverse_column(cols[c])) for c in range(ncols)]
    return Case(size={"d_cols": 4 * ((ncols - 1) * stride + (1 << log_size))}, inputs={"d_cols": segs_in}, expect={"d_cols": segs_out},
                call=lambda ctx, a, h: ctx._L.frieda_bit_reverse_column(ctx._h, a["d_cols"], stride, ncols, log_size))


@row("frieda_circle_extend", [(4, 5, 9), (3, 10, 14), (1, 0, 5), (1, 12, 20)])
def _extend(oracle, shape):
    ncols, log_coef, log_size = shape
    coef = rand_m31(np.random.default_rng(1500 + log_size), (ncols, 1 << log_coef))
    exp = np.stack([oracle.circle_extend(coef[c], log_size) for c in range(ncols)])
    return Case(size={"d_coef": coef.nbytes, "d_out": exp.nbytes}, inputs={"d_coef": [(0, coef)]}, expect={"d_out": [(0, exp)]},
                call=lambda ctx, a, h: ctx._L.frieda_circle_extend(ctx._h, a["d_coef"], ncols, log_coef, log_size, a["d_out"]), **_trim(log_size))


@row("frieda_circle_eval_at_point", [(3, 5), (4, 12), (4, 13), (1, 17)])
def _eval_at_point(oracle, shape):
    ncols, log_coef = shape
    rng = np.random.default_rng(1600 + log_coef)
    coef, px, py = rand_m31(rng, (ncols, 1 << log_coef)), rand_m31(rng, 4), rand_m31(rng, 4)
    exp = np.stack([oracle.circle_eval_at_point(coef[c], px, py) for c in range(ncols)])

    def call(ctx, a, h):
        h["out"] = np.zeros((ncols, 4), dtype=np.uint32)
        return ctx._L.frieda_circle_eval_at_point(ctx._h, a["d_coef"], ncols, log_coef, px.ctypes.data, py.ctypes.data, h["out"].ctypes.data)

    return Case(size={"d_coef": coef.nbytes}, inputs={"d_coef": [(0, coef)]}, expect_host={"out": exp}, call=call)


DECOMPOSE_LOGS = [1, 5, 12, 13, 17]


def _decompose_case(oracle, log_size, in_place):
    ev = rand_m31(np.random.default_rng(1700 + log_size), (4, 1 << log_size))
    g, lam = oracle.fri_decompose(ev)

    def call(ctx, a, h):
        h["lambda"] = np.zeros(4, dtype=np.uint32)
        return ctx._L.frieda_fri_decompose(ctx._h, a["d_eval"], log_size, a["d_eval"] if in_place else a["d_g"], h["lambda"].ctypes.data)

    if in_place:
        return Case(size={"d_eval": ev.nbytes}, inputs={"d_eval": [(0, ev)]}, expect={"d_eval": [(0, g)]}, expect_host={"lambda": lam}, call=call)
    return Case(size={"d_eval": ev.nbytes, "d_g": g.nbytes}, inputs={"d_eval": [(0, ev)]}, expect={"d_g": [(0, g)]}, expect_host={"lambda": lam}, call=call)


row("frieda_fri_decompose", DECOMPOSE_LOGS)(lambda oracle, s: _decompose_case(oracle, s, False))
row("frieda_fri_decompose[in place]", DECOMPOSE_LOGS)(lambda oracle, s: _decompose_case(oracle, s, True))


@row("frieda_dev_gather_device", [(4, 37), (4, 4096), (1, 1000), (3, 100)])
def _gather(oracle, shape):
    ncols, n = shape
    rng = np.random.default_rng(1800 + n)
    stride = 1 << 14
    cols = rand_m31(rng, (ncols, stride))
    idx = rng.integers(0, stride, n, dtype=np.uint64)
    idx[:2] = [0, stride - 1]
    exp = np.ascontiguousarray(cols[:, idx].T)  # Column::at per index: plain indexing is the reference
    return Case(size={"d_cols": cols.nbytes, "d_idx": idx.nbytes, "d_out": exp.nbytes}, inputs={"d_cols": [(0, cols)], "d_idx": [(0, idx)]},
                expect={"d_out": [(0, exp)]},
                call=lambda ctx, a, h: ctx._L.frieda_dev_gather_device(ctx._h, a["d_cols"], stride, ncols, a["d_idx"], n, a["d_out"]))


@row("frieda_dev_gather_hashes", [(5, 7), (12, 300)])
def _gather_hashes(oracle, shape):
    log_len, n = shape
    rng = np.random.default_rng(1850 + n)
    layer = rng.integers(0, 256, (1 << log_len, 32), dtype=np.uint8)
    idx = rng.integers(0, 1 << log_len, n, dtype=np.uint64)
    idx[:2] = [0, (1 << log_len) - 1]

    def call(ctx, a, h):
        h["out"] = np.full((n, 32), 0x5A, dtype=np.uint8)
        return ctx._L.frieda_dev_gather_hashes(ctx._h, a["d_layer"], 1 << log_len, idx.ctypes.data, n, h["out"].ctypes.data)

    return Case(size={"d_layer": layer.nbytes}, inputs={"d_layer": [(0, layer)]}, expect_host={"out": layer[idx]}, call=call)  # plain indexing is the reference


@row("frieda_merkle_decommit_device", [(10, 20), (12, 600)])  # one launch (<= 512 positions) and the multi-block route
def _decommit(oracle, shape):
    m, n_pos = shape
    rng = np.random.default_rng(1900 + m)
    cols = rand_m31(rng, (4, 1 << m))
    image, layers = _tree_image(oracle, cols)
    pos = np.sort(rng.permutation(1 << m)[:n_pos]).astype(np.uint32)
    walk = stwo_decommit_walk([int(p) for p in pos], m)
    hashes = np.stack([layers[l][node] for l, node in walk]).reshape(-1)
    values = np.ascontiguousarray(cols[:, pos].T)

    def call(ctx, a, h):
        ptrs = (C.c_void_p * (m + 1))(*[a["d_layers"] + ctx._L.frieda_merkle_layer_offset(m, j) for j in range(m + 1)])
        return ctx._L.frieda_merkle_decommit_device(ctx._h, ptrs, m, a["d_cols"], 4, 1 << m, a["d_positions"], n_pos, a["d_out_values"],
                                                    a["d_out_hashes"], a["d_n_hashes"])

    return Case(size={"d_layers": image.nbytes, "d_cols": cols.nbytes, "d_positions": pos.nbytes, "d_out_values": values.nbytes,
                      "d_out_hashes": 32 * n_pos * m, "d_n_hashes": 4},
                inputs={"d_layers": [(0, image)], "d_cols": [(0, cols)], "d_positions": [(0, pos)]},
                expect={"d_out_values": [(0, values)], "d_out_hashes": [(0, hashes)], "d_n_hashes": [(0, np.array([len(walk)], dtype=np.uint32))]},
                call=call)


# Level A, device-resident blobs: d_data is a byte pointer.  One size of the fused small-domain route, one of >= 1 MB.
LEVEL_A_LENGTHS = [3001, (4 << 17) * 30 // 8 - 4321]


@row("frieda_commit_device", LEVEL_A_LENGTHS)
def _commit_device(oracle, n_bytes):
    data = splitmix64_bytes(2000 + n_bytes, n_bytes)
    root = np.frombuffer(oracle.commit(data.tobytes(), 1), dtype=np.uint8)
    return Case(size={"d_data": n_bytes, "d_out_root": 32}, inputs={"d_data": [(0, data)]}, expect={"d_out_root": [(0, root)]},
                call=lambda ctx, a, h: ctx._L.frieda_commit_device(ctx._h, a["d_data"], n_bytes, 1, a["d_out_root"]))


@row("frieda_commit_and_generate_proof_device", LEVEL_A_LENGTHS)
def _prove_device(oracle, n_bytes):
    import frieda_amd

    data = splitmix64_bytes(2100 + n_bytes, n_bytes)
    o_root, o_proof = oracle.commit_and_generate_proof(data.tobytes(), 7, oracle.make_config(6, 1, 0, 20))
    cfg = frieda_amd.PcsConfig(frieda_amd.FriConfig(1, 0, 20), 6)

    def call(ctx, a, h):
        h["root"], proof = ctx.commit_and_generate_proof_device(a["d_data"], n_bytes, 7, cfg)
        h["proof"] = proof.serialize()
        return 0

    return Case(size={"d_data": n_bytes}, inputs={"d_data": [(0, data)]}, expect_host={"root": o_root, "proof": o_proof.serialize()}, call=call)


def _batch_image(length, stride, count, seed):
    host = np.full(stride * (count - 1) + length, 0xA5, dtype=np.uint8)  # the padding between blobs must be ignored
    blobs = []
    for i in range(count):
        b = splitmix64_bytes(seed + i, length)
        host[i * stride : i * stride + length] = b
        blobs.append(b.tobytes())
    return host, blobs


# (length, stride, count): a stride that is no multiple of 4, one that is a multiple of 4 but not of 16
BATCH_SHAPES = [(3000, 3001, 5), (3000, 3012, 5), (70001, 70003, 3)]


@row("frieda_commit_batch_device", BATCH_SHAPES)
def _commit_batch(oracle, shape):
    length, stride, count = shape
    host, blobs = _batch_image(length, stride, count, 2200)
    exp = [oracle.commit(b, 2) for b in blobs]

    def call(ctx, a, h):
        h["roots"] = ctx.commit_batch_device(a["d_data"], stride, length, count, 2)
        return 0

    return Case(size={"d_data": host.nbytes}, inputs={"d_data": [(0, host)]}, expect_host={"roots": exp}, call=call)


@row("frieda_prove_batch_begin_device", BATCH_SHAPES)
def _prove_batch(oracle, shape):
    import frieda_amd

    length, stride, count = shape
    host, blobs = _batch_image(length, stride, count, 2300)
    seeds = [3 * i + 1 for i in range(count)]
    exp = []
    for b, s in zip(blobs, seeds):
        r, p = oracle.commit_and_generate_proof(b, s, oracle.make_config(5, 2, 1, 12))
        exp.append((r, p.serialize()))
    cfg = frieda_amd.PcsConfig(frieda_amd.FriConfig(2, 1, 12), 5)

    def call(ctx, a, h):
        ctx.prove_batch_begin_device(a["d_data"], stride, length, count, seeds, cfg)
        h["proofs"] = [(r, p.serialize()) for r, p in ctx.prove_batch_finish(count)]
        return 0

    return Case(size={"d_data": host.nbytes}, inputs={"d_data": [(0, host)]}, expect_host={"proofs": exp}, call=call)


ALL_CASES = [pytest.param(name, shape, id=f"{name}-{shape}".replace(" ", "")) for name in TABLE for shape in SHAPES[name]]


def test_every_table_row_has_shapes():
    """(no GPU) the table, the case builders and the shapes name the same entry points"""
    assert set(TABLE) == set(BUILDERS) == set(SHAPES)
    for name, params in TABLE.items():
        assert SHAPES[name], name
        for p, (role, cls) in params.items():
            assert role in ("in", "out", "inout") and cls in OFFSETS, (name, p)


@pytest.mark.gpu
@pytest.mark.parametrize("name,shape", ALL_CASES)
def test_buffer_contract(gpu_ctx, oracle, name, shape):
    drive(gpu_ctx, name, BUILDERS[name](oracle, shape))


# ---- the harness itself ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("offset", [0, 1, 4])
@pytest.mark.parametrize("nbytes", [4096, 4097, 3])
def test_guarded_buffer_reports_a_planted_byte(gpu_ctx, offset, nbytes):
    """One changed byte right behind the payload, and one right in front of it (both inside the buffer's own allocation), planted with
    frieda_dev_upload: assert_zones_intact must fail and name the payload-relative offset; an untouched buffer passes; a changed
    payload byte is not a zone failure but fails assert_payload_equals."""
    from frieda_amd.api import _check

    data = np.arange(nbytes, dtype=np.uint8)
    for where in (nbytes, -1):
        b = GuardedBuf(gpu_ctx, nbytes, offset).upload(data)
        assert b.ptr.value == b.base.value + ZONE + offset
        b.assert_zones_intact()
        b.assert_payload_equals(data)
        planted = (poison_bytes(b.start + where, b.start + where + 1) ^ 0x01).astype(np.uint8)
        _check(gpu_ctx._L.frieda_dev_upload(gpu_ctx._h, b.ptr.value + where, planted.ctypes.data, 1), gpu_ctx._h)
        with pytest.raises(AssertionError, match=rf"first at payload offset {where}, last at {where} "):
            b.assert_zones_intact()
        b.assert_payload_equals(data)
        b.free()
    b = GuardedBuf(gpu_ctx, nbytes, offset).upload(data)
    flipped = np.array([data[nbytes - 1] ^ 0x80], dtype=np.uint8)
    _check(gpu_ctx._L.frieda_dev_upload(gpu_ctx._h, b.ptr.value + nbytes - 1, flipped.ctypes.data, 1), gpu_ctx._h)
    b.assert_zones_intact()
    with pytest.raises(AssertionError, match=rf"first at payload offset {nbytes - 1}, last at {nbytes - 1}$"):
        b.assert_payload_equals(data)
    b.free()


def test_poison_is_position_dependent_and_never_canonical():
    """(no GPU) every poison word has bit 31 set; the pattern does not repeat with a small period and is the same however it is cut"""
    w = poison_bytes(0, 1 << 16).view("<u4")
    assert (w >> 31).all() and len(np.unique(w)) > 0.99 * w.size
    assert np.array_equal(poison_bytes(5, 1003), poison_bytes(0, 2000)[5:1003])


# ---- argument rules that belong to the contract -----------------------------------------------------------------------------------
@pytest.mark.gpu
def test_circle_extend_refuses_overlapping_buffers(gpu_ctx):
    """the header: "the buffers must not overlap" — FRIEDA_ERR_ARG before any launch, as frieda_circle_evaluate_fold2 does"""
    coef = rand_m31(np.random.default_rng(1), (2, 1 << 6))
    b = GuardedBuf(gpu_ctx, 4 * 2 * (1 << 10)).upload(coef)
    f = gpu_ctx._L.frieda_circle_extend
    for d_out in (b.ptr.value, b.ptr.value + 4, b.ptr.value + coef.nbytes - 4):  # same, shifted, last word
        assert f(gpu_ctx._h, b.ptr.value, 2, 6, 9, d_out) == ERR_ARG
    assert f(gpu_ctx._h, b.ptr.value + 1024, 1, 6, 9, b.ptr.value) == ERR_ARG  # the input inside the output's extent
    gpu_ctx.synchronize()
    b.assert_payload_equals(coef)
    b.assert_poison_inside([(coef.nbytes, b.nbytes)])
    b.assert_zones_intact()
    assert f(gpu_ctx._h, b.ptr.value, 2, 6, 8, b.ptr.value + coef.nbytes) == 0  # adjacent is fine
    gpu_ctx.synchronize()
    b.assert_zones_intact()


@pytest.mark.gpu
def test_interpolate_round_trip_on_the_generic_inverse_passes(oracle):
    """FRIEDA_INTT_GENERIC (the option no other test names) on a private context: evaluate, then interpolate every block shape through the
    generic inverse kernel, aligned and at a word offset — the coefficients come back, equal to the oracle's, zones intact."""
    import frieda_amd

    ctx = frieda_amd.Context(0)
    try:
        ctx.set_option("FRIEDA_INTT_GENERIC", 1)
        for L, n, ncols in ((12, 13, 3), (13, 13, 4), (16, 18, 4), (17, 18, 1)):
            rng = np.random.default_rng(40 + L)
            coef = rand_m31(rng, (ncols, 1 << L))
            tw, itw = oracle.precompute_twiddles(n)
            ev = np.concatenate(_oracle_cols(lambda c: oracle.circle_evaluate(coef[c : c + 1], n, tw), ncols))
            for off in (0, 4):
                d_c, d_e = GuardedBuf(ctx, coef.nbytes, off).upload(coef), GuardedBuf(ctx, ev.nbytes, off)
                assert ctx._L.frieda_circle_evaluate(ctx._h, d_c.ptr, ncols, L, n, d_e.ptr) == 0
                assert np.array_equal(d_e.payload(np.uint32, ev.shape), ev)
                for k in (0, (1 << (n - L)) - 1):
                    block = np.ascontiguousarray(ev[:, k << L : (k + 1) << L])
                    d_b, d_o = GuardedBuf(ctx, block.nbytes, off).upload(block), GuardedBuf(ctx, coef.nbytes, off)
                    assert ctx._L.frieda_circle_interpolate(ctx._h, d_b.ptr, ncols, L, n, k, d_o.ptr) == 0
                    ctx.synchronize()
                    got = d_o.payload(np.uint32, coef.shape)
                    assert np.array_equal(got, coef), (L, n, ncols, off, k)
                    assert np.array_equal(got, oracle.circle_interpolate_block(block, n, k, itw))
                    d_b.assert_payload_equals(block)
                    for b in (d_b, d_o):
                        b.assert_zones_intact(f"interpolate L={L} n={n} off={off}")
                        b.free()
                for b in (d_c, d_e):
                    b.assert_zones_intact(f"evaluate L={L} n={n} off={off}")
                    b.free()
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("no_cp", [0, 1])
def test_fold2_one_pass_form_with_and_without_side_by_side_columns(oracle, no_cp):
    """FRIEDA_NTT_NO_CP is read only where frieda_circle_evaluate_fold2 takes its one-pass form (16-byte aligned buffers, log_size >= 12,
    below 512 tiles): 0 runs the four columns side by side in one 1024-thread workgroup, 1 one after the other.  Aligned GuardedBufs on a
    private context, n = 14 .. 20, both accumulate modes, against the oracle's three separate operations; zones and the coefficients
    intact."""
    import frieda_amd

    ctx = frieda_amd.Context(0)
    try:
        ctx.set_option("FRIEDA_NTT_NO_CP", no_cp)
        for L, n in ((12, 14), (13, 17), (16, 20), (14, 14)):
            for accumulate in (0, 1):
                rng = np.random.default_rng(77 + 32 * L + n + accumulate)
                coef, line1_0, a0, a1 = rand_m31(rng, (4, 1 << L)), rand_m31(rng, (4, 1 << (n - 1))), rand_m31(rng, (4,)), rand_m31(rng, (4,))
                tw, _ = oracle.precompute_twiddles(n)
                ev = np.concatenate(_oracle_cols(lambda c: oracle.circle_evaluate(coef[c : c + 1], n, tw), 4))
                l1 = oracle.fold_circle_into_line(ev, a0, line1_0.copy() if accumulate else None)
                l2 = oracle.fold_line(l1, n, a1)
                d_c, d_e = GuardedBuf(ctx, coef.nbytes).upload(coef), GuardedBuf(ctx, ev.nbytes)
                d_1, d_2 = GuardedBuf(ctx, l1.nbytes).upload(line1_0), GuardedBuf(ctx, l2.nbytes)
                assert ctx._L.frieda_circle_evaluate_fold2(ctx._h, d_c.ptr, L, n, d_e.ptr, a0.ctypes.data, accumulate, d_1.ptr, a1.ctypes.data, d_2.ptr) == 0
                ctx.synchronize()
                what = (no_cp, L, n, accumulate)
                assert np.array_equal(d_e.payload(np.uint32, ev.shape), ev), what
                assert np.array_equal(d_1.payload(np.uint32, l1.shape), l1), what
                assert np.array_equal(d_2.payload(np.uint32, l2.shape), l2), what
                d_c.assert_payload_equals(coef)
                for b in (d_c, d_e, d_1, d_2):
                    b.assert_zones_intact(f"fold2 {what}")
                    b.free()
    finally:
        ctx.close()
