"""Shared helpers for the parity tests."""
import json
import os

import numpy as np

from conftest import GOLDEN, pattern_bytes


def load_vectors():
    with open(os.path.join(GOLDEN, "vectors.json")) as f:
        return json.load(f)


def resolve_input(spec, blob):
    if spec == "blob":
        return blob
    kind, arg = spec.split(":", 1)
    if kind == "pattern":
        return pattern_bytes(int(arg)).tobytes()
    if kind == "ascii":
        return arg.encode()
    raise ValueError(spec)


def blob_len_for(log_domain, log_blowup=4):
    """Byte length whose felts exactly fill a 2^log_domain domain: 4*2^L felts of 30 bits."""
    L = log_domain - log_blowup
    return (4 << L) * 30 // 8


class DevBuf:
    """Device memory through the C ABI's Column storage (frieda_dev_alloc / upload / download)."""

    def __init__(self, ctx, nbytes):
        import ctypes as C

        self.ctx = ctx
        self.nbytes = nbytes
        self.ptr = C.c_void_p()
        from frieda_amd.api import _check

        _check(ctx._L.frieda_dev_alloc(ctx._h, nbytes, C.byref(self.ptr)), ctx._h)

    @classmethod
    def from_array(cls, ctx, arr):
        arr = np.ascontiguousarray(arr)
        b = cls(ctx, max(arr.nbytes, 1))
        from frieda_amd.api import _check

        if arr.nbytes:
            _check(ctx._L.frieda_dev_upload(ctx._h, b.ptr, arr.ctypes.data, arr.nbytes), ctx._h)
        return b

    def to_array(self, dtype, shape):
        from frieda_amd.api import _check

        out = np.zeros(shape, dtype=dtype)
        assert out.nbytes <= self.nbytes
        if out.nbytes:
            _check(self.ctx._L.frieda_dev_download(self.ctx._h, out.ctypes.data, self.ptr, out.nbytes), self.ctx._h)
        return out

    def free(self):
        if self.ptr:
            self.ctx._L.frieda_dev_free(self.ctx._h, self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


ZONE = 256 << 10  # red zone on each side of a GuardedBuf payload: four times the widest tile a kernel writes (2^12 words x 4 columns)


def poison_bytes(start, stop):
    """Bytes [start, stop) of the position-dependent poison pattern: the little-endian word at byte offset 4 k is a hash of k with
    bit 31 set (never a canonical M31), so neither a constant fill nor a stale copy from elsewhere reproduces it."""
    w0, w1 = start // 4, (stop + 3) // 4
    x = np.arange(w0, w1, dtype=np.uint64) * np.uint64(0x9E3779B1) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(15)
    x = x * np.uint64(0x85EBCA6B) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(13)
    x = x * np.uint64(0xC2B2AE35) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16)
    words = (x | np.uint64(0x80000000)).astype("<u4")
    return words.view(np.uint8)[start - 4 * w0 : stop - 4 * w0]


class GuardedBuf:
    """A device payload of `nbytes` bytes at byte `offset` past a red zone, with a second red zone right behind its last byte, all
    inside ONE frieda_dev_alloc of ZONE + offset + nbytes + ZONE bytes (rounded up to a word) filled with poison_bytes: an overrun of
    up to ZONE bytes either way lands in this allocation and is reported by assert_zones_intact instead of corrupting a neighbour."""

    def __init__(self, ctx, nbytes, offset=0):
        import ctypes as C

        from frieda_amd.api import _check

        self.ctx, self.nbytes, self.offset = ctx, int(nbytes), int(offset)
        self.start = ZONE + self.offset  # payload, relative to the allocation
        self.total = (self.start + self.nbytes + ZONE + 3) & ~3
        self.base = C.c_void_p()
        _check(ctx._L.frieda_dev_alloc(ctx._h, self.total, C.byref(self.base)), ctx._h)
        self.ptr = C.c_void_p(self.base.value + self.start)
        fill = np.ascontiguousarray(poison_bytes(0, self.total))
        _check(ctx._L.frieda_dev_upload(ctx._h, self.base, fill.ctypes.data, self.total), ctx._h)

    def upload(self, arr, at=0):
        """host array -> payload bytes [at, at + arr.nbytes)"""
        from frieda_amd.api import _check

        arr = np.ascontiguousarray(arr)
        assert 0 <= at and at + arr.nbytes <= self.nbytes
        if arr.nbytes:
            _check(self.ctx._L.frieda_dev_upload(self.ctx._h, self.ptr.value + at, arr.ctypes.data, arr.nbytes), self.ctx._h)
        return self

    def _download(self, rel_start, rel_stop):
        """bytes [rel_start, rel_stop) relative to the payload start (negative: the front zone)"""
        from frieda_amd.api import _check

        out = np.zeros(rel_stop - rel_start, dtype=np.uint8)
        if out.size:
            _check(self.ctx._L.frieda_dev_download(self.ctx._h, out.ctypes.data, self.ptr.value + rel_start, out.size), self.ctx._h)
        return out

    def payload(self, dtype, shape):
        out = np.zeros(shape, dtype=dtype)
        assert out.nbytes <= self.nbytes
        if out.nbytes:
            out.reshape(-1).view(np.uint8)[:] = self._download(0, out.nbytes)
        return out

    def _assert_poison(self, rel_start, rel_stop, what):
        got = self._download(rel_start, rel_stop)
        want = poison_bytes(self.start + rel_start, self.start + rel_stop)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (
            f"{what}: {bad.size} byte(s) written outside the payload [0, {self.nbytes}): first at payload offset {rel_start + int(bad[0])}, "
            f"last at {rel_start + int(bad[-1])} (payload at byte {self.offset} past the front zone)"
        )

    def assert_zones_intact(self, what="buffer"):
        """both red zones and the `offset` slack, byte for byte: the back zone begins at the byte after the payload"""
        self._assert_poison(-self.start, 0, what)
        self._assert_poison(self.nbytes, self.total - self.start, what)

    def assert_poison_inside(self, ranges, what="buffer"):
        """payload byte ranges [(start, stop)] the call must leave alone (gaps between strided columns, an untouched output)"""
        for a, b in ranges:
            self._assert_poison(a, b, what)

    def assert_payload_equals(self, arr, what="input"):
        arr = np.ascontiguousarray(arr)
        got = self._download(0, arr.nbytes)
        bad = np.nonzero(got != arr.reshape(-1).view(np.uint8))[0]
        assert bad.size == 0, f"{what}: payload modified, {bad.size} byte(s), first at payload offset {int(bad[0])}, last at {int(bad[-1])}"

    def free(self):
        if self.base:
            self.ctx._L.frieda_dev_free(self.ctx._h, self.base)
            self.base = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass
