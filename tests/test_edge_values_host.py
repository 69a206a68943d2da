"""CPU: the oracle at the value edges, against Python integers.

The GPU tests of tests/test_gpu_value_edges.py compare the kernels with the oracle on the families of tests/edge_values.py.  The oracle
reduces with stwo's shift formula ("valid for v < P^2"), so at those inputs it needs a check of its own: (a) its field primitives over the
full cross product of the edge constants, (b) its operations against restatements in unbounded Python integers that share no code with
it (only point coordinates are taken from it: they are pinned by the reference's golden root and carry no edge arithmetic), and (c) that
the families produce the boundary events they are named for."""
import ctypes as C
import itertools

import numpy as np
import pytest

import edge_values as EV
from edge_values import ALPHAS, BLOBS, EDGE_CONSTANTS, EVAL_POINTS, FAMILIES, FOLD_INPUTS, FOLD_PAIRS, P, QM31_EDGE_CONSTANTS, SPARSE_TARGETS


# ---- Python-integer field arithmetic (QM31 = CM31[u] / (u^2 - 2 - i), CM31 = M31[i] / (i^2 + 1)) -------------------------------------
def cmul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def qmul(a, b):
    a0, a1, b0, b1 = a[:2], a[2:], b[:2], b[2:]
    lo, hi, rr = cmul(a0, b0), cmul(a1, b1), (2, 1)
    x0 = tuple((u + v) % P for u, v in zip(lo, cmul(rr, hi)))
    x1 = tuple((u + v) % P for u, v in zip(cmul(a0, b1), cmul(a1, b0)))
    return x0 + x1


def qadd(a, b):
    return tuple((u + v) % P for u, v in zip(a, b))


def qsub(a, b):
    return tuple((u - v) % P for u, v in zip(a, b))


def qscale(a, s):
    return tuple(u * s % P for u in a)


def inv(a):
    return pow(a, P - 2, P)


def qcol(cols, i):
    return tuple(int(cols[c][i]) for c in range(4))


def brev(i, bits):
    return int(format(i, f"0{bits}b")[::-1], 2) if bits else 0


# ---- (a) primitives ------------------------------------------------------------------------------------------------------------
def test_m31_primitives_over_the_edge_constants(oracle):
    L = oracle.lib()
    for a, b in itertools.product(EDGE_CONSTANTS, repeat=2):
        assert L.fo_m31_add(a, b) == (a + b) % P, (a, b)
        assert L.fo_m31_sub(a, b) == (a - b) % P, (a, b)
        assert L.fo_m31_mul(a, b) == a * b % P, (a, b)
    for a in EDGE_CONSTANTS:
        if a:
            assert a * L.fo_m31_inv(a) % P == 1, a


def test_qm31_mul_over_the_edge_constants(oracle):
    L = oracle.lib()
    elems = list(itertools.product(QM31_EDGE_CONSTANTS, repeat=4))
    arrs = [(C.c_uint32 * 4)(*e) for e in elems]
    out = (C.c_uint32 * 4)()
    for a, ca in zip(elems, arrs):
        for b, cb in zip(elems, arrs):
            L.fo_qm31_mul(ca, cb, out)
            assert tuple(out) == qmul(a, b), (a, b)


# ---- (b) operations ------------------------------------------------------------------------------------------------------------
def domain_point(oracle, n, i):
    """the point behind entry i of a bit-reversed evaluation on the 2^n domain"""
    L = oracle.lib()
    x, y = C.c_uint32(), C.c_uint32()
    L.fo_circle_domain_at(n, L.fo_bit_reverse_index(i, n), C.byref(x), C.byref(y))
    return x.value, y.value


_BASIS = {}


def basis(oracle, L, n):
    """B[i][k] = y^(k_0) * prod_j pi^j(x)^(k_(j+1)) at the point of entry i, pi(x) = 2 x^2 - 1, k < 2^L"""
    if (L, n) not in _BASIS:
        rows = []
        for i in range(1 << n):
            x, y = domain_point(oracle, n, i)
            factors = [y]
            for _ in range(max(L - 1, 0)):
                factors.append(x)
                x = (2 * x * x - 1) % P
            row = [1]
            for f in factors[:L]:  # bit b of k doubles the row
                row = row + [v * f % P for v in row]
            rows.append(row)
        _BASIS[(L, n)] = rows
    return _BASIS[(L, n)]


def evaluate_direct(oracle, coef, n):
    L = len(coef).bit_length() - 1
    c = [int(v) for v in coef]
    return [sum(ck * bk for ck, bk in zip(c, row)) % P for row in basis(oracle, L, n)]


EVAL_SHAPES = [(0, 4), (1, 1), (2, 2), (3, 3), (2, 6), (5, 5), (5, 6), (6, 6)]


@pytest.mark.parametrize("L,n", EVAL_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("family", FAMILIES)
def test_circle_evaluate_is_the_direct_sum(oracle, family, L, n):
    coef = FAMILIES[family]((2, 1 << L), seed=n)
    got = oracle.circle_evaluate(coef, n)
    for c in range(2):
        assert got[c].tolist() == evaluate_direct(oracle, coef[c], n)


def line_x(oracle, m, j):
    """x of point j of the line domain of log size m under any circle domain: the coset half_odds(m) = 2^(29-m) + j 2^(31-m)"""
    x, y = C.c_uint32(), C.c_uint32()
    oracle.lib().fo_point_from_index(((1 << (29 - m)) + (j << (31 - m))) & P, C.byref(x), C.byref(y))
    return x.value


def fold_restated(src, alpha, t_of_pair, dst=None):
    """(x + y) + alpha (x - y) / t per pair (2i, 2i+1), plus dst alpha^2 when accumulating"""
    alpha = tuple(int(a) for a in alpha)
    out = []
    for i in range(src.shape[1] // 2):
        x, y = qcol(src, 2 * i), qcol(src, 2 * i + 1)
        v = qadd(qadd(x, y), qmul(alpha, qscale(qsub(x, y), inv(t_of_pair(i)))))
        if dst is not None:
            v = qadd(qmul(qcol(dst, i), qmul(alpha, alpha)), v)
        out.append(v)
    return np.array(out, dtype=np.uint32).T


@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("family", FOLD_INPUTS)
def test_fold_circle_into_line_restated(oracle, family, alpha):
    for n in (1, 2, 6):
        src = FOLD_INPUTS[family]((4, 1 << n), seed=n)
        for dst in (None, EV.edge_rich((4, 1 << (n - 1)), 5), EV.pmax((4, 1 << (n - 1)))):
            got = oracle.fold_circle_into_line(src, EV.alpha_array(alpha), None if dst is None else dst.copy())
            exp = fold_restated(src, ALPHAS[alpha], lambda i: domain_point(oracle, n, 2 * i)[1], dst)
            assert np.array_equal(got, exp), (n, dst is None)


@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("family", FOLD_INPUTS)
def test_fold_line_restated(oracle, family, alpha):
    for n, m in ((2, 1), (6, 5), (6, 1), (7, 6)):
        src = FOLD_INPUTS[family]((4, 1 << m), seed=m)
        got = oracle.fold_line(src, n, EV.alpha_array(alpha))
        exp = fold_restated(src, ALPHAS[alpha], lambda i: line_x(oracle, m, brev(2 * i, m)))
        assert np.array_equal(got, exp), (n, m)


def decompose_restated(ev):
    n = ev.shape[1]
    cols = [[int(v) for v in ev[c]] for c in range(4)]
    lam = tuple((sum(col[: n // 2]) - sum(col[n // 2 :])) * inv(n % P) % P for col in cols)
    g = [[(v - lam[c]) % P if i < n // 2 else (v + lam[c]) % P for i, v in enumerate(cols[c])] for c in range(4)]
    return np.array(g, dtype=np.uint32), lam


@pytest.mark.parametrize("family", FAMILIES)
def test_fri_decompose_restated(oracle, family):
    for log_size in (1, 2, 5, 6):
        ev = FAMILIES[family]((4, 1 << log_size), seed=log_size)
        g, lam = oracle.fri_decompose(ev)
        eg, elam = decompose_restated(ev)
        assert tuple(lam.tolist()) == elam and np.array_equal(g, eg), log_size


@pytest.mark.parametrize("point", EVAL_POINTS)
@pytest.mark.parametrize("family", ["pmax", "alt", "onehot_last_pmax", "edge_rich"])
def test_eval_at_point_is_the_direct_sum(oracle, family, point):
    px, py = EVAL_POINTS[point]
    for log_coef in (1, 2, 5, 6):
        coef = FAMILIES[family]((1 << log_coef,), seed=log_coef)
        factors, x = [py], px
        for _ in range(log_coef - 1):
            factors.append(x)
            x = qsub(qscale(qmul(x, x), 2), (1, 0, 0, 0))
        row = [(1, 0, 0, 0)]
        for f in factors:
            row = row + [qmul(v, f) for v in row]
        exp = (0, 0, 0, 0)
        for ck, bk in zip(coef.tolist(), row):
            exp = qadd(exp, qscale(bk, ck))
        assert tuple(oracle.circle_eval_at_point(coef, px, py).tolist()) == exp, log_coef


@pytest.mark.parametrize("blob", BLOBS)
def test_codec_is_the_30_bit_little_endian_stream(oracle, blob):
    for n_bytes in (1, 4, 15, 16, 58, 119, 1000):
        data = BLOBS[blob](n_bytes)
        stream = int.from_bytes(data, "little")
        n_felts = (8 * n_bytes + 29) // 30
        felts = oracle.bytes_to_felt_le(data)
        assert felts.tolist() == [(stream >> (30 * k)) & (2**30 - 1) for k in range(n_felts)]
        assert oracle.felts_to_bytes(felts, n_bytes) == data
    # felts with bit 30 set: the packer keeps the low 30 bits
    for felts in (EV.pmax(64), EV.edge_rich(64, 3), np.full(64, 2**30, dtype=np.uint32)):
        stream = sum((int(v) & (2**30 - 1)) << (30 * k) for k, v in enumerate(felts.tolist()))
        for n_bytes in (240, 239, 7):
            assert oracle.felts_to_bytes(felts, n_bytes) == (stream & ((1 << (8 * n_bytes)) - 1)).to_bytes(n_bytes, "little")


# ---- (c) the families do what they are named for ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [5, 12, 16])
@pytest.mark.parametrize("target", SPARSE_TARGETS)
def test_sparse_targets_put_zeros_at_the_last_butterflies(oracle, target, n):
    """coefficients = interpolate(E) evaluate back to E, at least half of it 0: each zero is a last-layer v + t == P or v - t == 0"""
    E = FAMILIES[target]((1, 1 << n))
    coef = oracle.circle_interpolate_block(E, n, 0)
    assert coef.max() < P
    back = oracle.circle_evaluate(coef, n)
    assert np.array_equal(back, E) and 2 * np.count_nonzero(back == 0) >= back.size
    if n == 5:
        assert back[0].tolist() == evaluate_direct(oracle, coef[0], n)


def test_fold_pairs_hit_the_boundaries(oracle):
    for n in (2, 6, 12):
        src = FOLD_PAIRS["x+y==0"]((4, 1 << n), seed=n)
        assert not oracle.fold_circle_into_line(src, EV.alpha_array("zero")).any()
        assert not oracle.fold_line(src, n + 1, EV.alpha_array("zero")).any()
        src = FOLD_PAIRS["x==y"]((4, 1 << n), seed=n)
        twice = (2 * src[:, 0::2].astype(np.uint64) % P).astype(np.uint32)
        for alpha in ALPHAS:  # x - y == 0: alpha drops out
            assert np.array_equal(oracle.fold_circle_into_line(src, EV.alpha_array(alpha)), twice)
            assert np.array_equal(oracle.fold_line(src, n + 1, EV.alpha_array(alpha)), twice)


def test_families_are_canonical_and_deterministic():
    for name, f in {**FAMILIES, **FOLD_PAIRS}.items():
        a, b = f((4, 64), 7), f((4, 64), 7)
        assert a.dtype == np.uint32 and a.shape == (4, 64) and a.max() < P and np.array_equal(a, b), name
    rich = EV.edge_rich((4, 4096), 1)
    assert all((rich == c).any() for c in EDGE_CONSTANTS)
    for name, a in ALPHAS.items():
        assert len(a) == 4 and max(a) < P
    for name, f in BLOBS.items():
        assert len(f(1)) == 1 and len(f(1024)) == 1024 and len(f(15)) == 15
