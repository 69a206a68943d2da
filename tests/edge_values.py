"""Value-edge input families for the field kernels: deterministic `(shape, seed) -> uint32 array` functions of canonical M31 words
that make the boundary events of modular arithmetic happen on purpose — a sum that lands exactly on P, a difference that is exactly
0, operands 0 and P - 1, accumulators at the top of their stated bound.  On uniform words each of these has probability ~2^-31 per
operation.  Pure numpy: no GPU, no oracle.  `shape` is (columns, words) or (words,); every pattern runs along the last axis."""
import numpy as np

P = 2**31 - 1

# the constants every modular routine has a branch or a carry at
EDGE_CONSTANTS = (0, 1, 2, P - 2, P - 1, 2**30 - 1, 2**30, (P - 1) // 2, (P + 1) // 2)
QM31_EDGE_CONSTANTS = (0, 1, P - 1, 2**30)


def _shape(shape):
    return (shape,) if isinstance(shape, int) else tuple(shape)


def zeros(shape, seed=0):
    return np.zeros(_shape(shape), dtype=np.uint32)


def pmax(shape, seed=0):
    return np.full(_shape(shape), P - 1, dtype=np.uint32)


def alt(shape, seed=0):
    """0 at even indices, P - 1 at odd ones"""
    out = zeros(shape)
    out[..., 1::2] = P - 1
    return out


def halves(shape, seed=0):
    """first half 0, second half P - 1: fri_decompose's +/- pattern (extreme lambda, constant g)"""
    out = zeros(shape)
    out[..., out.shape[-1] // 2 :] = P - 1
    return out


def halves_swapped(shape, seed=0):
    out = zeros(shape)
    out[..., : out.shape[-1] // 2] = P - 1
    return out


def onehot(where, v):
    """a single v at index 0 ("first"), size // 2 ("middle") or size - 1 ("last") of every column"""

    def family(shape, seed=0):
        out = zeros(shape)
        k = {"first": 0, "middle": out.shape[-1] // 2, "last": out.shape[-1] - 1}[where]
        out[..., k] = v
        return out

    family.__name__ = f"onehot_{where}_{'1' if v == 1 else 'pmax'}"
    return family


def edge_rich(shape, seed=0):
    """each word with probability 1/2 one of EDGE_CONSTANTS, else uniform in [0, P)"""
    rng = np.random.default_rng(0xED6E + seed)
    shape = _shape(shape)
    uniform = rng.integers(0, P, shape, dtype=np.uint32)
    const = np.array(EDGE_CONSTANTS, dtype=np.uint32)[rng.integers(0, len(EDGE_CONSTANTS), shape)]
    return np.where(rng.integers(0, 2, shape).astype(bool), const, uniform).astype(np.uint32)


ONEHOTS = {f.__name__: f for f in (onehot(w, v) for w in ("first", "middle", "last") for v in (1, P - 1))}
FAMILIES = {"zeros": zeros, "pmax": pmax, "alt": alt, "halves": halves, "halves_swapped": halves_swapped, **ONEHOTS, "edge_rich": edge_rich}

# fold inputs: SoA QM31 columns [4, N]; the fold kernels (and the oracle's fold_line / fold_circle_into_line) pair entries 2i and 2i + 1
# of the bit-reversed evaluation: x = src[:, 2i], y = src[:, 2i + 1]
FOLD_PAIR_KINDS = ("x==y", "x+y==0", "0,pmax", "pmax,0", "pmax,pmax")


def fold_pairs(kind):
    def family(shape, seed=0):
        shape = _shape(shape)
        assert shape[-1] % 2 == 0
        out = np.zeros(shape, dtype=np.uint32)
        half = shape[:-1] + (shape[-1] // 2,)
        if kind == "x==y":  # x - y is exactly 0
            x = edge_rich(half, seed)
            x[..., 0] = P - 1  # 2x = 2P - 2: the largest sum there is
            out[..., 0::2], out[..., 1::2] = x, x
        elif kind == "x+y==0":  # x + y lands exactly on P in every coordinate (or is 0 + 0)
            x = edge_rich(half, seed)
            out[..., 0::2], out[..., 1::2] = x, (P - x.astype(np.uint64)) % P
        elif kind == "0,pmax":
            out[..., 1::2] = P - 1
        elif kind == "pmax,0":
            out[..., 0::2] = P - 1
        elif kind == "pmax,pmax":
            out[...] = P - 1
        else:
            raise ValueError(kind)
        return out

    family.__name__ = f"fold_pairs[{kind}]"
    return family


FOLD_PAIRS = {k: fold_pairs(k) for k in FOLD_PAIR_KINDS}
# what the fold tests run, host and GPU alike: every family and every pair kind
FOLD_INPUTS = {**FAMILIES, **{f"pairs[{k}]": f for k, f in FOLD_PAIRS.items()}}
# evaluation vectors that are mostly 0: transformed onto them, every zero is a last-layer butterfly whose v + t is exactly P or whose
# v - t is exactly 0
SPARSE_TARGETS = ("zeros", "halves", "halves_swapped") + tuple(ONEHOTS)
# QM31 points (x, y) for eval_at_point: 0, 1 and P - 1 in each of the four slots; the last pairs an edge x with a random y
EVAL_POINTS = {
    "zero": ((0, 0, 0, 0), (0, 0, 0, 0)),
    "one": ((1, 0, 0, 0), (1, 0, 0, 0)),
    "pmax4": ((P - 1,) * 4, (P - 1,) * 4),
    "x_last_pmax": ((0, 0, 0, P - 1), tuple(int(v) for v in np.random.default_rng(0xE7A1).integers(0, P, 4))),
}

ALPHAS = {
    "zero": (0, 0, 0, 0),
    "one": (1, 0, 0, 0),
    "pmax4": (P - 1,) * 4,
    "last_pmax": (0, 0, 0, P - 1),
    "pmax_1_pmax_1": (P - 1, 1, P - 1, 1),
    "random": tuple(int(v) for v in np.random.default_rng(0xA1FA).integers(0, P, 4)),
}


def alpha_array(name):
    return np.array(ALPHAS[name], dtype=np.uint32)


BLOBS = {
    "00": lambda n: bytes(n),
    "ff": lambda n: b"\xff" * n,
    "00ff": lambda n: (b"\x00\xff" * (n // 2 + 1))[:n],
    "ff_then_00": lambda n: b"\xff" * (n // 2) + bytes(n - n // 2),
}
