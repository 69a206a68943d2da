"""Shared by the stripe-bundle tests: stripe bundles of a block built by the CPU oracle alone, one bundles_util.Call per blob laid out
as the header pins it (values stripe-major; bundle b's witness block at hash K * witness_first[b], blob j's piece at j * W_b inside it),
the independent status per piece (bundles_util.independent_status on blob j's piece alone) and the mutation matrix of
bundles_util.mutations applied to ONE blob's piece.  Nothing here calls the library under test except raw_verify at the end."""
import ctypes as C

import numpy as np

import bundles_util as B
from bundles_util import ACCEPTED, MALFORMED, REJECTED  # noqa: F401
from cells_util import POISON


class StripeCall:
    """one call over K blobs: bundles (stripe index lists), values [S, K, 4, 2^c], witness [K * H, 32], witness_first [n_bundles + 1] per blob"""

    def __init__(self, n, c, commitments, bundles, values, witness, wfirst):
        self.n, self.c, self.commitments = n, c, [bytes(x) for x in commitments]
        self.bundles = [np.asarray(b, dtype=np.uint32) for b in bundles]
        self.values, self.witness, self.wfirst = values, witness, np.asarray(wfirst, dtype=np.uint64)

    @property
    def k(self):
        return len(self.commitments)

    @property
    def first(self):
        return np.concatenate([[0], np.cumsum([len(b) for b in self.bundles])]).astype(np.uint32)

    def replace(self, **kw):
        d = dict(n=self.n, c=self.c, commitments=self.commitments, bundles=self.bundles, values=self.values, witness=self.witness, wfirst=self.wfirst)
        d.update(kw)
        return StripeCall(**d)

    def piece(self, b, j):
        """blob j's W_b hashes of bundle b: a view into the witness"""
        w0, w1 = int(self.wfirst[b]), int(self.wfirst[b + 1])
        at = self.k * w0 + j * (w1 - w0)
        return self.witness[at:at + (w1 - w0)]

    def blob_call(self, j):
        """blob j's pieces alone, as the single-blob bundle call they are"""
        wits = [self.piece(b, j) for b in range(len(self.bundles))]
        witness = np.concatenate(wits) if wits else np.zeros((0, 32), np.uint8)
        return B.Call(self.n, self.c, self.commitments[j], self.bundles, np.ascontiguousarray(self.values[:, j]), np.ascontiguousarray(witness), self.wfirst)


def assemble(calls, bundles=None, wfirst=None):
    """K single-blob calls over the same bundles -> the stripe call.  bundles / wfirst: taken from calls[0] unless given; a blob whose
    piece of a bundle has another length than W_b is cut or padded with 0x5A (the row is malformed then anyway)."""
    bundles = calls[0].bundles if bundles is None else bundles
    wfirst = np.asarray(calls[0].wfirst if wfirst is None else wfirst, dtype=np.uint64)
    rows = []
    for b in range(len(bundles)):
        w = int(wfirst[b + 1]) - int(wfirst[b])
        for cj in calls:
            p = cj.witness[int(cj.wfirst[b]):int(cj.wfirst[b + 1])][:w]
            rows.append(np.concatenate([p, np.full((w - len(p), 32), 0x5A, np.uint8)]))
    witness = np.concatenate(rows) if rows else np.zeros((0, 32), np.uint8)
    values = np.ascontiguousarray(np.stack([cj.values for cj in calls], axis=1))
    return StripeCall(calls[0].n, calls[0].c, [cj.commitment for cj in calls], bundles, values, np.ascontiguousarray(witness), wfirst)


def blob_calls(blobs, c, bundles):
    """[(data, ev, layers)] -> one bundles_util.Call per blob on the same bundles, all from the oracle"""
    return [B.build_call(ev, layers, c, bundles) for _, ev, layers in blobs]


def build(blobs, c, bundles):
    return assemble(blob_calls(blobs, c, bundles))


def independent(call):
    """uint8 [n_bundles, K]: byte (b, j) is bundles_util.independent_status of blob j's piece of bundle b alone"""
    return np.stack([B.independent_status(call.blob_call(j)) for j in range(call.k)], axis=1) if call.bundles else np.zeros((0, call.k), np.uint8)


def mutations(calls, j):
    """bundles_util.mutations applied to blob j's call, every mutant embedded in the block: [(label, rows hit, must_be_malformed,
    touches_all_blobs, StripeCall)].  A mutant that moves an index or a witness length changes what all blobs of the bundle share."""
    out = []
    for label, hit, must, mutant in B.mutations(calls[j]):
        shared = any(len(a) != len(b) or (a != b).any() for a, b in zip(mutant.bundles, calls[j].bundles)) or mutant.wfirst.tolist() != calls[j].wfirst.tolist()
        out.append((label, hit, must, shared, assemble(calls[:j] + [mutant] + calls[j + 1:], bundles=mutant.bundles, wfirst=mutant.wfirst)))
    return out


def check_mutation(label, hit, must, shared, j, want):
    """what the independent check must say about a mutated block before a verifier is asked: a mutant of blob j's piece alone changes
    byte (b, j) only; a malformed bundle marks its whole row and leaves the other rows alone"""
    nb, k = want.shape
    for b in range(nb):
        if b not in hit:
            assert (want[b] == ACCEPTED).all(), (label, b)
        elif must:
            assert (want[b] == MALFORMED).all(), (label, b)
        elif not shared:
            assert want[b, j] == REJECTED and (np.delete(want[b], j) == ACCEPTED).all(), (label, b)
        else:
            assert (want[b] != ACCEPTED).all(), (label, b)


def table(commitments):
    return np.frombuffer(b"".join(commitments), dtype=np.uint8).copy()


def host_arrays(call):
    idx = np.ascontiguousarray(np.concatenate(call.bundles) if call.bundles else np.zeros(1, np.uint32), dtype=np.uint32)
    return (table(call.commitments), idx, np.ascontiguousarray(call.first, dtype=np.uint32), np.ascontiguousarray(call.values, dtype=np.uint32),
            np.ascontiguousarray(call.witness, dtype=np.uint8), np.ascontiguousarray(call.wfirst, dtype=np.uint64))


# ---- the library under test ---------------------------------------------------------------------------------------------------------------
def raw_verify(call, ctx=None, n_blobs=None):
    """frieda_verify_stripe_bundles (ctx None) or frieda_verify_stripe_bundles_many into a poison-filled status array: (rc, status [n_bundles, K])"""
    from frieda_amd import _lib

    L = _lib.lib()
    com, idx, first, values, witness, wfirst = host_arrays(call)
    nb, k = len(call.bundles), call.k
    status = np.full(nb * k + 8, POISON, dtype=np.uint8)
    args = (com.ctypes.data, k if n_blobs is None else n_blobs, call.n, call.c, idx.ctypes.data, first.ctypes.data, nb, values.ctypes.data if values.size else None,
            witness.ctypes.data if witness.size else None, wfirst.ctypes.data, status.ctypes.data)
    rc = L.frieda_verify_stripe_bundles(*args) if ctx is None else L.frieda_verify_stripe_bundles_many(ctx._h, *args)
    assert (status[nb * k:] == POISON).all(), "red zone behind out_status"
    return rc, status[: nb * k].reshape(nb, k)
