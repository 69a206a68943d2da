"""Host-side mirror of frieda's public API over the C ABI (include/frieda_hip.h).

Same names, argument meaning and error behaviour as /root/reference/src/lib.rs:22-44:

    commit(data, log_blowup_factor) -> bytes[32]
    generate_proof(data, seed, pcs_config) -> Proof
    commit_and_generate_proof(data, seed, pcs_config) -> (bytes[32], Proof)      (src/proof.rs:32)
    verify(proof, seed) -> bool

Where the reference panics (assert!/unwrap, e.g. src/proof.rs:166-173) `FriedaPanic` is raised; verifier
rejections return False.  Every call runs on the MI355X through libfrieda_hip.so; there is no CPU path.
"""
import ctypes as C
import threading
import time
from dataclasses import dataclass

import numpy as np

from . import _lib


class FriedaError(RuntimeError):
    def __init__(self, status, detail=""):
        self.status = status
        msg = _lib.lib().frieda_status_string(status).decode()
        super().__init__(f"frieda_hip status {status} ({msg}){': ' + detail if detail else ''}")


class FriedaPanic(FriedaError):
    """The reference implementation panics on this input (FRIEDA_ERR_INVARIANT)."""


def _check(status, ctx=None):
    if status == _lib.OK:
        return
    detail = ""
    if ctx is not None:
        detail = _lib.lib().frieda_last_error(ctx).decode(errors="replace")
    raise (FriedaPanic if status == _lib.ERR_INVARIANT else FriedaError)(status, detail)


@dataclass(frozen=True)
class FriConfig:
    """stwo FriConfig as constructed at src/proof.rs:110-114."""

    log_blowup_factor: int = 4
    log_last_layer_degree_bound: int = 0
    n_queries: int = 20


@dataclass(frozen=True)
class PcsConfig:
    """stwo PcsConfig as constructed at src/proof.rs:109-116, benches/proof.rs:5-12."""

    fri_config: FriConfig = FriConfig()
    pow_bits: int = 20

    def _c(self):
        f = self.fri_config
        return _lib.PcsConfigC(self.pow_bits, f.log_blowup_factor, f.log_last_layer_degree_bound, f.n_queries)


def _seed_ptr(seed):
    return C.byref(C.c_uint64(seed)) if seed is not None else None


def _ptr(p):
    """a device pointer given as int, c_void_p or None -> int or None"""
    return p.value if isinstance(p, C.c_void_p) else p


def _as_bytes(data):
    if isinstance(data, np.ndarray):
        return np.ascontiguousarray(data, dtype=np.uint8)
    return np.frombuffer(bytes(data), dtype=np.uint8)


class Context:
    """One device + one stream + twiddle cache + workspace (frieda_ctx).  Not thread-safe; use one per GPU/thread."""

    def __init__(self, device=0, stream=None):
        self._h = C.c_void_p()
        self._L = _lib.lib()
        _check(self._L.frieda_ctx_create(device, C.c_void_p(stream) if stream else None, C.byref(self._h)))
        self.device = device

    def close(self):
        if self._h:
            self._L.frieda_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def synchronize(self):
        _check(self._L.frieda_ctx_synchronize(self._h), self._h)

    def release_workspace(self):
        """Free the device workspace, the pinned staging block and the twiddle tables (they are re-created on demand)."""
        _check(self._L.frieda_ctx_release_workspace(self._h), self._h)

    def set_twiddle_cache(self, enabled):
        _check(self._L.frieda_ctx_set_twiddle_cache(self._h, int(bool(enabled))), self._h)

    def set_option(self, name, value):
        """A tuning / A-B option of this context alone (frieda_ctx_set_option): `name` is the environment variable that sets its default
        at context creation, e.g. "FRIEDA_HOST_DECOMMIT"; every option selects another kernel or plan for the same result."""
        _check(self._L.frieda_ctx_set_option(self._h, name.encode(), int(value)), self._h)

    def set_host_channel(self, enabled):
        """Evaluate the Fiat-Shamir channel on the host between layers instead of inside the device kernels."""
        _check(self._L.frieda_ctx_set_host_channel(self._h, int(bool(enabled))), self._h)

    def set_kernel_timing(self, enabled):
        _check(self._L.frieda_ctx_set_kernel_timing(self._h, int(bool(enabled))), self._h)

    def last_prove_phases(self):
        """Host wall-clock marks (ms since entry) of the last generate_proof: enqueued, device done, queries, gather, assembled."""
        a = (C.c_double * 8)()
        _check(self._L.frieda_ctx_last_prove_phases(self._h, a), self._h)
        return dict(zip(["enqueued", "device_done", "queries", "gathered", "assembled", "first_launch_after_entry"], list(a)[:6]))

    def blake2s_ceiling(self):
        """(leaf, node) compressions per second this device sustains right now on register-resident data (measurement aid)."""
        a, b = C.c_double(), C.c_double()
        _check(self._L.frieda_ctx_blake2s_ceiling(self._h, C.byref(a), C.byref(b)), self._h)
        return a.value, b.value

    def blake2s_ceiling_ex(self):
        """The ceiling with the in-kernel clock: {leaf_per_s, node_per_s, leaf_clock_ghz, leaf_cycles, node_clock_ghz, node_cycles}
        (cycles = SIMD cycles per wave-compression)."""
        a = (C.c_double * 6)()
        _check(self._L.frieda_ctx_blake2s_ceiling_ex(self._h, a), self._h)
        return dict(zip(["leaf_per_s", "node_per_s", "leaf_clock_ghz", "leaf_cycles_per_wave_compression", "node_clock_ghz", "node_cycles_per_wave_compression"], list(a)))

    def last_transcript(self):
        """Diagnostic: alphas drawn per FRI layer and the channel digest the grind was keyed by, of the last finished proof."""
        n = C.c_uint32()
        alphas = (C.c_uint32 * (4 * 64))()
        digest = (C.c_uint8 * 32)()
        _check(self._L.frieda_ctx_last_transcript(self._h, C.byref(n), alphas, 64, digest), self._h)
        return {"alphas": [[int(alphas[4 * i + c]) for c in range(4)] for i in range(min(n.value, 64))], "digest_before_grind": bytes(digest)}

    def kernel_timing_report(self, reset=True):
        """Per-kernel HIP-event timings accumulated since the last reset: list of dicts."""
        import json

        n = self._L.frieda_ctx_kernel_timing_report(self._h, None, 0, 0)
        buf = C.create_string_buffer(n + 16)
        self._L.frieda_ctx_kernel_timing_report(self._h, buf, n + 16, int(bool(reset)))
        return json.loads(buf.value.decode())["kernels"]

    # ---- Level A ----
    def commit(self, data, log_blowup_factor):
        a = _as_bytes(data)
        root = (C.c_uint8 * 32)()
        _check(self._L.frieda_commit(self._h, a.ctypes.data if a.size else None, a.size, log_blowup_factor, root), self._h)
        return bytes(root)

    def commit_device(self, d_ptr, length, log_blowup_factor, d_root_ptr):
        """Blob and 32-byte root both in device memory; asynchronous on the context stream."""
        _check(self._L.frieda_commit_device(self._h, d_ptr, length, log_blowup_factor, d_root_ptr), self._h)

    # ---- Level B openings over caller device buffers (pointers as int or c_void_p; host arrays in, numpy / bytes out) ----
    def dev_gather(self, d_cols, stride, ncols, idx):
        """Batched Column::at (frieda_dev_gather): uint32[n, ncols], row r = the values of the ncols columns (`stride` words apart,
        `stride` words long) at idx[r].  Any order, repeats allowed; an index >= stride raises FriedaError."""
        ix = np.ascontiguousarray(idx, dtype=np.uint64).reshape(-1)
        out = np.zeros((ix.size, ncols), dtype=np.uint32)
        _check(self._L.frieda_dev_gather(self._h, _ptr(d_cols), stride, ncols, ix.ctypes.data, ix.size, out.ctypes.data), self._h)
        return out

    def dev_gather_hashes(self, d_layer, layer_len, idx):
        """The 32-byte hashes at idx of a layer of layer_len hashes (frieda_dev_gather_hashes), concatenated."""
        ix = np.ascontiguousarray(idx, dtype=np.uint64).reshape(-1)
        out = np.zeros(32 * ix.size, dtype=np.uint8)
        _check(self._L.frieda_dev_gather_hashes(self._h, _ptr(d_layer), layer_len, ix.ctypes.data, ix.size, out.ctypes.data), self._h)
        return out.tobytes()

    def merkle_decommit(self, d_layers, log_size, d_cols, ncols, stride, positions):
        """MerkleProver::decommit of a tree whose columns all sit on the leaf layer (frieda_merkle_decommit).  d_layers: log_size + 1
        device pointers by layer log; positions strictly ascending, < 2^log_size.  -> (values uint32[n_pos, ncols], hash witness bytes
        in stwo's order)."""
        pos = np.ascontiguousarray(positions, dtype=np.uint32).reshape(-1)
        layers = (C.c_void_p * (log_size + 1))(*[_ptr(p) for p in d_layers])
        vals = np.zeros((pos.size, ncols), dtype=np.uint32)
        n = C.c_size_t(0)

        def call(buf, cap):
            return self._L.frieda_merkle_decommit(
                self._h, layers, log_size, _ptr(d_cols), ncols, stride, pos.ctypes.data, pos.size, vals.ctypes.data, buf, cap, C.byref(n)
            )

        # no witness is longer than sum_s min(n_pos, 2^(log_size - s)); where that bound is large (dense lists, whose witness is short)
        # the length is asked for first
        cap = sum(min(pos.size, 1 << (log_size - s)) for s in range(1, log_size + 1))
        if cap > (1 << 21):
            st = call(None, 0)
            if st != _lib.ERR_ARG:
                _check(st, self._h)
            cap = n.value
        hashes = np.zeros(max(32 * cap, 1), dtype=np.uint8)
        _check(call(hashes.ctypes.data, cap), self._h)
        return vals, hashes[: 32 * n.value].tobytes()

    # ---- reconstruction side (host arrays in, bytes out; the device entry points are frieda_reconstruct_*_device) ----
    def _dev_call_with_upload(self, host_arr, n_out_bytes, call):
        """uploads a uint32 array, runs call(d_in, d_out), downloads n_out_bytes"""
        import numpy as np

        a = np.ascontiguousarray(host_arr, dtype=np.uint32)
        d_in, d_out = C.c_void_p(), C.c_void_p()
        _check(self._L.frieda_dev_alloc(self._h, a.nbytes, C.byref(d_in)), self._h)
        try:
            _check(self._L.frieda_dev_alloc(self._h, n_out_bytes + 16, C.byref(d_out)), self._h)
            _check(self._L.frieda_dev_upload(self._h, d_in, a.ctypes.data, a.nbytes), self._h)
            call(d_in, d_out)
            out = (C.c_uint8 * max(n_out_bytes, 1))()
            if n_out_bytes:
                _check(self._L.frieda_dev_download(self._h, out, d_out, n_out_bytes), self._h)
            return bytes(out)[:n_out_bytes]
        finally:
            self._L.frieda_dev_free(self._h, d_in)
            if d_out:
                self._L.frieda_dev_free(self._h, d_out)

    def reconstruct_from_block(self, block, log_domain, block_index, n_bytes):
        """block: uint32[4, 2^L] = entries block_index * 2^L .. of the four bit-reversed evaluation columns -> the blob."""
        L = int(block.shape[1]).bit_length() - 1
        return self._dev_call_with_upload(
            block, n_bytes, lambda d_in, d_out: _check(self._L.frieda_reconstruct_device(self._h, d_in, L, log_domain, block_index, n_bytes, d_out), self._h)
        )

    def reconstruct_from_cells(self, cells, cell_index, log_coef, log_domain, n_bytes):
        """cells: uint32[R, 4, 2^m] (cell r = entries cell_index[r] * 2^m .. of every column), R = 2^(log_coef - m) <= 4096
        distinct cells anywhere in the codeword -> the blob."""
        import numpy as np

        R, m = int(cells.shape[0]), int(cells.shape[2]).bit_length() - 1
        idx = np.ascontiguousarray(cell_index, dtype=np.uint32)
        return self._dev_call_with_upload(
            cells,
            n_bytes,
            lambda d_in, d_out: _check(
                self._L.frieda_reconstruct_cells_device(self._h, d_in, idx.ctypes.data, R, m, log_coef, log_domain, n_bytes, d_out), self._h
            ),
        )

    def reconstruct_from_points(self, cells, cell_index, log_coef, log_domain, n_bytes):
        """cells: uint32[R, 4, 2^m] as in reconstruct_from_cells, but ANY number of distinct cells holding at least 2^log_coef + 2
        points in all (single sampled points: m = 0) — no linear system, no bound on R (frieda_reconstruct_points_device)."""
        import numpy as np

        R, m = int(cells.shape[0]), int(cells.shape[2]).bit_length() - 1
        idx = np.ascontiguousarray(cell_index, dtype=np.uint32)
        return self._dev_call_with_upload(
            cells,
            n_bytes,
            lambda d_in, d_out: _check(
                self._L.frieda_reconstruct_points_device(self._h, d_in, idx.ctypes.data, R, m, log_coef, log_domain, n_bytes, d_out), self._h
            ),
        )

    def commit_and_generate_proof(self, data, seed, pcs_config):
        a = _as_bytes(data)
        root = (C.c_uint8 * 32)()
        out = C.c_void_p()
        _check(
            self._L.frieda_commit_and_generate_proof(
                self._h, a.ctypes.data if a.size else None, a.size, _seed_ptr(seed), pcs_config._c(), root, C.byref(out)
            ),
            self._h,
        )
        return bytes(root), Proof(out)

    def commit_and_generate_proof_device(self, d_ptr, length, seed, pcs_config):
        root = (C.c_uint8 * 32)()
        out = C.c_void_p()
        _check(
            self._L.frieda_commit_and_generate_proof_device(self._h, d_ptr, length, _seed_ptr(seed), pcs_config._c(), root, C.byref(out)),
            self._h,
        )
        return bytes(root), Proof(out)

    def generate_proof(self, data, seed, pcs_config):
        return self.commit_and_generate_proof(data, seed, pcs_config)[1]

    # ---- split form: overlap several proofs on one GPU with one Context per in-flight proof ----
    def prove_begin(self, data, seed, pcs_config):
        a = _as_bytes(data)
        self._keep = a  # the host blob must outlive the asynchronous upload
        _check(self._L.frieda_prove_begin(self._h, a.ctypes.data if a.size else None, a.size, _seed_ptr(seed), pcs_config._c()), self._h)

    def prove_begin_device(self, d_ptr, length, seed, pcs_config):
        _check(self._L.frieda_prove_begin_device(self._h, d_ptr, length, _seed_ptr(seed), pcs_config._c()), self._h)

    # ---- batches of equal-length blobs: every kernel handles the whole batch (include/frieda_hip.h) ----
    def _seeds_array(self, seeds, count):
        if seeds is None:
            return None
        if len(seeds) != count:
            raise ValueError("one seed per blob")
        return (C.c_uint64 * count)(*[int(s) for s in seeds])

    def commit_and_generate_proof_batch(self, blobs, seeds, pcs_config):
        """blobs: equal-length bytes-like objects; seeds: None or one int per blob.  Returns [(commitment, Proof), ...]."""
        count = len(blobs)
        if count == 0:
            return []
        length = len(blobs[0])
        if any(len(b) != length for b in blobs):
            raise ValueError("a batch holds blobs of one length")
        flat = b"".join(bytes(b) for b in blobs)
        buf = (C.c_uint8 * max(len(flat), 1)).from_buffer_copy(flat or b"\0")
        return self._prove_batch(self._L.frieda_commit_and_generate_proof_batch, buf, length, length, count, seeds, pcs_config)

    def commit_and_generate_proof_batch_device(self, d_ptr, stride, length, count, seeds, pcs_config):
        return self._prove_batch(self._L.frieda_commit_and_generate_proof_batch_device, d_ptr, stride, length, count, seeds, pcs_config)

    def prove_batch_begin_device(self, d_ptr, stride, length, count, seeds, pcs_config):
        """Enqueue the commit phase of a batch; the blobs must stay valid until prove_batch_finish(count) returns."""
        _check(self._L.frieda_prove_batch_begin_device(self._h, d_ptr, stride, length, count, self._seeds_array(seeds, count), pcs_config._c()), self._h)

    def prove_batch_finish(self, count):
        roots = (C.c_uint8 * (32 * count))()
        outs = (C.c_void_p * count)()
        _check(self._L.frieda_prove_batch_finish(self._h, count, roots, outs), self._h)
        rb = bytes(roots)
        return [(rb[32 * i : 32 * i + 32], Proof(C.c_void_p(outs[i]))) for i in range(count)]

    def _prove_batch(self, fn, data, stride, length, count, seeds, pcs_config):
        roots = (C.c_uint8 * (32 * count))()
        outs = (C.c_void_p * count)()
        _check(fn(self._h, data, stride, length, count, self._seeds_array(seeds, count), pcs_config._c(), roots, outs), self._h)
        rb = bytes(roots)
        return [(rb[32 * i : 32 * i + 32], Proof(C.c_void_p(outs[i]))) for i in range(count)]

    # ---- one blob under many seeds: encode once, prove per seed (a provider serving sampling clients) ----
    def encode(self, data, log_blowup_factor):
        """Unpack + encode + first-layer tree of `data`, kept on the device: an Encoded to prove from under any number of seeds."""
        a = _as_bytes(data)
        out = C.c_void_p()
        _check(self._L.frieda_encode(self._h, a.ctypes.data if a.size else None, a.size, log_blowup_factor, C.byref(out)), self._h)
        return Encoded(out, a.size, log_blowup_factor)

    def encode_device(self, d_ptr, length, log_blowup_factor):
        out = C.c_void_p()
        _check(self._L.frieda_encode_device(self._h, d_ptr, length, log_blowup_factor, C.byref(out)), self._h)
        return Encoded(out, length, log_blowup_factor)

    def prove_seeds_begin(self, encoded, seeds, pcs_config):
        """Enqueue len(seeds) proofs of the encoded blob; `encoded` must stay open until prove_seeds_finish() returns."""
        seeds = [int(x) for x in seeds]
        arr = (C.c_uint64 * max(1, len(seeds)))(*seeds)
        _check(self._L.frieda_prove_seeds_begin(self._h, encoded._handle(), arr, len(seeds), pcs_config._c()), self._h)
        self._seeds_in_flight = len(seeds)

    def prove_seeds_finish(self):
        count = getattr(self, "_seeds_in_flight", 0)
        self._seeds_in_flight = 0
        outs = (C.c_void_p * max(1, count))()
        _check(self._L.frieda_prove_seeds_finish(self._h, outs), self._h)
        return [Proof(C.c_void_p(outs[i])) for i in range(count)]

    def prove_seeds(self, encoded, seeds, pcs_config):
        """[Proof]: proof i is commit_and_generate_proof(data, seeds[i], pcs_config)[1], byte for byte."""
        self.prove_seeds_begin(encoded, seeds, pcs_config)
        return self.prove_seeds_finish()

    # ---- a block under many seeds: K handles x S seeds in one call ----
    def prove_seeds_blobs_begin(self, encs, seeds, pcs_config):
        """Enqueue len(encs) * len(seeds) proofs: every encoded blob of the block under every seed of the one list.  The handles must stay
        open until prove_seeds_blobs_finish() returns."""
        encs = list(encs)
        seeds = [int(x) for x in seeds]
        handles = (C.c_void_p * max(1, len(encs)))(*[e._handle() for e in encs])
        arr = (C.c_uint64 * max(1, len(seeds)))(*seeds)
        _check(self._L.frieda_prove_seeds_blobs_begin(self._h, handles, len(encs), arr, len(seeds), pcs_config._c()), self._h)
        self._seeds_blobs_in_flight = (len(encs), len(seeds))

    def prove_seeds_blobs_finish(self):
        n_blobs, n_seeds = getattr(self, "_seeds_blobs_in_flight", (0, 0))
        self._seeds_blobs_in_flight = (0, 0)
        count = n_blobs * n_seeds
        outs = (C.c_void_p * max(1, count))()
        _check(self._L.frieda_prove_seeds_blobs_finish(self._h, outs), self._h)
        return [[Proof(C.c_void_p(outs[b * n_seeds + s])) for s in range(n_seeds)] for b in range(n_blobs)]

    def prove_seeds_blobs(self, encs, seeds, pcs_config):
        """[[Proof]]: proofs[b][s] is prove_seeds(encs[b], [seeds[s]], pcs_config)[0], byte for byte — one call for the whole block."""
        self.prove_seeds_blobs_begin(encs, seeds, pcs_config)
        return self.prove_seeds_blobs_finish()

    # ---- any list of (blob, seed) jobs over a block of handles ----
    @staticmethod
    def _jobs_arrays(encs, jobs):
        encs = list(encs)
        jobs = [(int(b), int(s)) for b, s in jobs]
        handles = (C.c_void_p * max(1, len(encs)))(*[e._handle() for e in encs])
        bidx = (C.c_uint32 * max(1, len(jobs)))(*[b for b, _ in jobs])
        seeds = (C.c_uint64 * max(1, len(jobs)))(*[s for _, s in jobs])
        return len(encs), len(jobs), handles, bidx, seeds

    def prove_jobs_begin(self, encs, jobs, pcs_config):
        """Enqueue one proof per job of `jobs`, a list of (blob_index, seed): encs[blob_index] under seed, all in one pass.  The handles
        must stay open until prove_jobs_finish() returns."""
        n_blobs, n_jobs, handles, bidx, seeds = self._jobs_arrays(encs, jobs)
        _check(self._L.frieda_prove_jobs_begin(self._h, handles, n_blobs, bidx, seeds, n_jobs, pcs_config._c()), self._h)
        self._jobs_in_flight = n_jobs

    def prove_jobs_finish(self):
        count = getattr(self, "_jobs_in_flight", 0)
        self._jobs_in_flight = 0
        outs = (C.c_void_p * max(1, count))()
        _check(self._L.frieda_prove_jobs_finish(self._h, outs), self._h)
        return [Proof(C.c_void_p(outs[i])) for i in range(count)]

    def prove_jobs(self, encs, jobs, pcs_config):
        """[Proof] in the caller's order: proof j is prove_seeds(encs[jobs[j][0]], [jobs[j][1]], pcs_config)[0], byte for byte.  The call
        cuts itself into passes (prove_jobs_plan)."""
        n_blobs, n_jobs, handles, bidx, seeds = self._jobs_arrays(encs, jobs)
        outs = (C.c_void_p * max(1, n_jobs))()
        _check(self._L.frieda_prove_jobs(self._h, handles, n_blobs, bidx, seeds, n_jobs, pcs_config._c(), outs), self._h)
        return [Proof(C.c_void_p(outs[i])) for i in range(n_jobs)]

    # ---- block proofs: one FRI proof for all blobs of a block (this project's own protocol: include/frieda_hip.h) ----
    def aggregate_encoded(self, encs, rho=None):
        """The seed-independent aggregate handle of a block: an Encoded whose evaluation is sum over k of rho^k * encs[k]'s, rho =
        block_challenge of the handles' commitments.  rho given (four canonical M31 words): the testing hook, for the value edges."""
        encs = list(encs)
        handles = (C.c_void_p * max(1, len(encs)))(*[e._handle() for e in encs])
        out = C.c_void_p()
        if rho is None:
            _check(self._L.frieda_aggregate_encoded(self._h, handles, len(encs), C.byref(out)), self._h)
        else:
            r = (C.c_uint32 * 4)(*[int(x) for x in rho])
            _check(self._L.frieda_test_aggregate_with_rho(self._h, handles, len(encs), r, C.byref(out)), self._h)
        return Encoded(out, encs[0].length, encs[0].log_blowup_factor)

    def prove_block_seeds(self, agg, encs, seeds, pcs_config):
        """[BlockProof], one per seed: the proof of the aggregate under that seed and the K blobs opened where it was queried."""
        encs = list(encs)
        seeds = [int(x) for x in seeds]
        handles = (C.c_void_p * max(1, len(encs)))(*[e._handle() for e in encs])
        arr = (C.c_uint64 * max(1, len(seeds)))(*seeds)
        outs = (C.c_void_p * max(1, len(seeds)))()
        _check(self._L.frieda_prove_block_seeds(self._h, agg._handle(), handles, len(encs), arr, len(seeds), pcs_config._c(), outs), self._h)
        return [BlockProof(C.c_void_p(outs[i])) for i in range(len(seeds))]

    def commit_and_generate_proofs_for_seeds(self, data, seeds, pcs_config):
        """(commitment, [Proof]) for a caller that has every seed at once: encode, prove, free."""
        a = _as_bytes(data)
        seeds = [int(x) for x in seeds]
        arr = (C.c_uint64 * max(1, len(seeds)))(*seeds)
        root = (C.c_uint8 * 32)()
        outs = (C.c_void_p * max(1, len(seeds)))()
        _check(
            self._L.frieda_commit_and_generate_proofs_for_seeds(
                self._h, a.ctypes.data if a.size else None, a.size, arr, len(seeds), pcs_config._c(), root, outs
            ),
            self._h,
        )
        return bytes(root), [Proof(C.c_void_p(outs[i])) for i in range(len(seeds))]

    def commit_batch(self, blobs, log_blowup_factor):
        count = len(blobs)
        if count == 0:
            return []
        length = len(blobs[0])
        if any(len(b) != length for b in blobs):
            raise ValueError("a batch holds blobs of one length")
        flat = b"".join(bytes(b) for b in blobs)
        buf = (C.c_uint8 * max(len(flat), 1)).from_buffer_copy(flat or b"\0")
        roots = (C.c_uint8 * (32 * count))()
        _check(self._L.frieda_commit_batch(self._h, buf, length, length, count, log_blowup_factor, roots), self._h)
        rb = bytes(roots)
        return [rb[32 * i : 32 * i + 32] for i in range(count)]

    def commit_batch_device(self, d_ptr, stride, length, count, log_blowup_factor):
        roots = (C.c_uint8 * (32 * count))()
        _check(self._L.frieda_commit_batch_device(self._h, d_ptr, stride, length, count, log_blowup_factor, roots), self._h)
        rb = bytes(roots)
        return [rb[32 * i : 32 * i + 32] for i in range(count)]

    def prove_finish(self):
        root = (C.c_uint8 * 32)()
        out = C.c_void_p()
        _check(self._L.frieda_prove_finish(self._h, root, C.byref(out)), self._h)
        self._keep = None
        return bytes(root), Proof(out)

    # ---- many proofs verified in one call on the device (frieda_verify_many*, verify.hip) ----
    def _proof_array(self, proofs):
        return (C.c_void_p * len(proofs))(*[p._h.value if isinstance(p._h, C.c_void_p) else p._h for p in proofs])

    def verify_many(self, proofs, seeds=None, expected_commitment=None):
        """One status byte per proof (numpy uint8: VERIFY_REJECTED / _ACCEPTED / _INVARIANT / _WRONG_COMMITMENT), each the result
        verify() gives for that proof.  seeds: None or one int per proof; expected_commitment: 32 bytes or None."""
        import numpy as np

        count = len(proofs)
        status = np.zeros(count, dtype=np.uint8)
        if count == 0:
            return status
        com = (C.c_uint8 * 32)(*expected_commitment) if expected_commitment is not None else None
        _check(self._L.frieda_verify_many(self._h, self._proof_array(proofs), self._seeds_array(seeds, count), count, com, status.ctypes.data), self._h)
        return status

    def verify_blobs_many(self, proofs, commitments, blob_index=None, seeds=None):
        """frieda_verify_blobs_many: the proofs of a block against a table of commitments.  Returns (status, accepted_per_blob): status[i]
        is exactly what verify_many gives for proof i alone with expected_commitment = commitments[blob_index[i]] (VERIFY_WRONG_COMMITMENT
        included, on every route); accepted_per_blob[b] (numpy uint32) is the number of ACCEPTED proofs that name blob b, so "proximity
        checked" reads > 0.  blob_index None: proof i belongs to commitment i and len(proofs) must be len(commitments).  FriedaError
        (ERR_ARG) before anything runs: an index >= len(commitments), blob_index None with a different count, proofs but no commitments,
        a proof in flight on the context."""
        import numpy as np

        count, n_blobs = len(proofs), len(commitments)
        if blob_index is not None and len(blob_index) != count:
            raise ValueError("one blob index per proof")
        if any(len(c) != 32 for c in commitments):
            raise ValueError("a commitment is 32 bytes")
        status = np.zeros(count, dtype=np.uint8)
        accepted = np.zeros(n_blobs, dtype=np.uint32)
        table = np.frombuffer(b"".join(bytes(c) for c in commitments) or b"\0", dtype=np.uint8).copy()
        bidx = None if blob_index is None else np.ascontiguousarray(blob_index, dtype=np.uint32)
        _check(
            self._L.frieda_verify_blobs_many(
                self._h, self._proof_array(proofs) if count else None, self._seeds_array(seeds, count), count, table.ctypes.data, n_blobs,
                None if bidx is None else bidx.ctypes.data, status.ctypes.data, accepted.ctypes.data
            ),
            self._h,
        )
        return status, accepted

    def verify_samples_many(self, proofs, seeds=None, expected_commitment=None, pitch=None):
        """(status, positions): positions[i] is the numpy uint32 array verify_samples() returns for proof i, None unless it is accepted."""
        import numpy as np

        count = len(proofs)
        status = np.zeros(count, dtype=np.uint8)
        if count == 0:
            return status, []
        if pitch is None:
            pitch = max(1, max(int(p.pcs_config.fri_config.n_queries) for p in proofs))
        pos = np.zeros((count, max(1, pitch)), dtype=np.uint32)
        npos = np.zeros(count, dtype=np.uint32)
        com = (C.c_uint8 * 32)(*expected_commitment) if expected_commitment is not None else None
        _check(
            self._L.frieda_verify_samples_many(
                self._h, self._proof_array(proofs), self._seeds_array(seeds, count), count, com, status.ctypes.data, pos.ctypes.data, pitch, npos.ctypes.data
            ),
            self._h,
        )
        return status, [pos[i, : npos[i]].copy() if status[i] == _lib.VERIFY_ACCEPTED else None for i in range(count)]

    def reconstruct_from_proofs(self, proofs, seeds, expected_commitment, n_bytes):
        """Verify the proofs against the commitment, pool the verified samples and rebuild the blob: (bytes, status, n_points).  Raises
        FriedaError (with .n_points and .proof_status set) when the verified points do not suffice or the result does not commit to
        expected_commitment."""
        import numpy as np

        count = len(proofs)
        status = np.zeros(max(count, 1), dtype=np.uint8)
        out = np.zeros(max(n_bytes, 1), dtype=np.uint8)
        n = C.c_size_t(0)
        com = (C.c_uint8 * 32)(*expected_commitment)
        try:
            _check(
                self._L.frieda_reconstruct_from_proofs(
                    self._h, self._proof_array(proofs) if count else None, self._seeds_array(seeds, count), count, com, n_bytes, out.ctypes.data,
                    status.ctypes.data, C.byref(n)
                ),
                self._h,
            )
        except FriedaError as e:
            e.n_points = n.value
            e.proof_status = status[:count]
            raise
        return out[:n_bytes].tobytes(), status[:count], n.value

    # ---- the pair forms: every point an accepted proof authenticates (frieda_verify_pairs_many, frieda_reconstruct_from_proof_pairs) ----
    def verify_pairs_many(self, proofs, seeds=None, expected_commitment=None, pitch=None):
        """(status, points): points[i] is the (positions uint32 [n], values uint32 [n, 4]) pair verify_pairs() returns for proof i, None
        unless it is accepted."""
        import numpy as np

        count = len(proofs)
        status = np.zeros(count, dtype=np.uint8)
        if count == 0:
            return status, []
        if pitch is None:
            pitch = max(1, 2 * max(int(p.pcs_config.fri_config.n_queries) for p in proofs))
        pos = np.zeros((count, max(1, pitch)), dtype=np.uint32)
        val = np.zeros((count, max(1, pitch), 4), dtype=np.uint32)
        npts = np.zeros(count, dtype=np.uint32)
        com = (C.c_uint8 * 32)(*expected_commitment) if expected_commitment is not None else None
        _check(
            self._L.frieda_verify_pairs_many(
                self._h, self._proof_array(proofs), self._seeds_array(seeds, count), count, com, status.ctypes.data, pos.ctypes.data, val.ctypes.data,
                pitch, npts.ctypes.data
            ),
            self._h,
        )
        return status, [(pos[i, : npts[i]].copy(), val[i, : npts[i]].copy()) if status[i] == _lib.VERIFY_ACCEPTED else None for i in range(count)]

    def reconstruct_from_proof_pairs(self, proofs, seeds, expected_commitment, n_bytes):
        """reconstruct_from_proofs with the pair points as the pool — both members of every first-layer pair an accepted proof opened, so
        about half as many proofs suffice: (bytes, status, n_points).  Raises FriedaError (with .n_points and .proof_status set) as
        reconstruct_from_proofs does."""
        import numpy as np

        count = len(proofs)
        status = np.zeros(max(count, 1), dtype=np.uint8)
        out = np.zeros(max(n_bytes, 1), dtype=np.uint8)
        n = C.c_size_t(0)
        com = (C.c_uint8 * 32)(*expected_commitment)
        try:
            _check(
                self._L.frieda_reconstruct_from_proof_pairs(
                    self._h, self._proof_array(proofs) if count else None, self._seeds_array(seeds, count), count, com, n_bytes, out.ctypes.data,
                    status.ctypes.data, C.byref(n)
                ),
                self._h,
            )
        except FriedaError as e:
            e.n_points = n.value
            e.proof_status = status[:count]
            raise
        return out[:n_bytes].tobytes(), status[:count], n.value


    # ---- authenticated cells (frieda_verify_cells_many, frieda_reconstruct_from_opened_cells; Encoded.open_cells is the provider's half) ----
    def verify_cells_many(self, commitment, log_domain, log_cell, cell_index, values, paths):
        """One status byte per cell (numpy uint8: CELL_ACCEPTED / CELL_REJECTED), verified on the device; the bytes verify_cells() gives."""
        idx, val, pth = _cell_arrays(log_domain, log_cell, cell_index, values, paths)
        status = np.zeros(len(idx), dtype=np.uint8)
        com = (C.c_uint8 * 32)(*commitment)
        _check(
            self._L.frieda_verify_cells_many(self._h, com, log_domain, log_cell, idx.ctypes.data, len(idx), val.ctypes.data, pth.ctypes.data, status.ctypes.data),
            self._h,
        )
        return status

    def reconstruct_from_opened_cells(self, commitment, log_blowup_factor, n_bytes, log_cell, cell_index, values, paths):
        """Verify the cells against the commitment, drop the rejected ones and rebuild the blob from the rest: (bytes, status,
        n_cells_used).  Raises FriedaError (with .n_cells_used and .cell_status set) when the accepted cells do not suffice or the result
        does not commit to `commitment`."""
        log_domain = codec_log_size(n_bytes) + log_blowup_factor
        idx, val, pth = _cell_arrays(log_domain, log_cell, cell_index, values, paths)
        count = len(idx)
        status = np.zeros(max(count, 1), dtype=np.uint8)
        out = np.zeros(max(n_bytes, 1), dtype=np.uint8)
        n = C.c_size_t(0)
        com = (C.c_uint8 * 32)(*commitment)
        try:
            _check(
                self._L.frieda_reconstruct_from_opened_cells(
                    self._h, com, log_blowup_factor, n_bytes, log_cell, idx.ctypes.data, count, val.ctypes.data, pth.ctypes.data, out.ctypes.data,
                    status.ctypes.data, C.byref(n)
                ),
                self._h,
            )
        except FriedaError as e:
            e.n_cells_used = n.value
            e.cell_status = status[:count]
            raise
        return out[:n_bytes].tobytes(), status[:count], n.value

    # ---- cell bundles: many cells under one shared Merkle witness (Encoded.open_cell_bundles is the provider's half) ----
    def verify_cell_bundles_many(self, commitment, log_domain, log_cell, bundles, values, witness, witness_first):
        """One status byte per bundle (numpy uint8: BUNDLE_REJECTED / BUNDLE_ACCEPTED / BUNDLE_MALFORMED), verified on the device; the
        bytes verify_cell_bundles() gives.  bundles: one ascending index list per bundle; values / witness / witness_first as
        Encoded.open_cell_bundles returns them."""
        idx, first, val, wit, wfirst = _bundle_arrays(log_cell, bundles, values, witness, witness_first)
        status = np.zeros(max(len(first) - 1, 1), dtype=np.uint8)
        com = (C.c_uint8 * 32)(*commitment)
        _check(
            self._L.frieda_verify_cell_bundles_many(self._h, com, log_domain, log_cell, idx.ctypes.data, first.ctypes.data, len(first) - 1, val.ctypes.data,
                                                    wit.ctypes.data, wfirst.ctypes.data, status.ctypes.data),
            self._h,
        )
        return status[: len(first) - 1]

    def reconstruct_from_cell_bundles(self, commitment, log_blowup_factor, n_bytes, log_cell, bundles, values, witness, witness_first):
        """Verify the bundles against the commitment, pool the cells of the accepted ones and rebuild the blob: (bytes, status,
        n_cells_used).  Raises FriedaError (with .n_cells_used and .bundle_status set) when the cells of the accepted bundles do not
        suffice or the result does not commit to `commitment`."""
        idx, first, val, wit, wfirst = _bundle_arrays(log_cell, bundles, values, witness, witness_first)
        count = len(first) - 1
        status = np.zeros(max(count, 1), dtype=np.uint8)
        out = np.zeros(max(n_bytes, 1), dtype=np.uint8)
        n = C.c_size_t(0)
        com = (C.c_uint8 * 32)(*commitment)
        try:
            _check(
                self._L.frieda_reconstruct_from_cell_bundles(
                    self._h, com, log_blowup_factor, n_bytes, log_cell, idx.ctypes.data, first.ctypes.data, count, val.ctypes.data, wit.ctypes.data,
                    wfirst.ctypes.data, out.ctypes.data, status.ctypes.data, C.byref(n)
                ),
                self._h,
            )
        except FriedaError as e:
            e.n_cells_used = n.value
            e.bundle_status = status[:count]
            raise
        return out[:n_bytes].tobytes(), status[:count], n.value

    # ---- the cells of a block: many blobs of one shape in one call (cell i is cell cell_index[i] of blob blob_index[i]) ----
    def verify_cells_blobs_many(self, commitments, log_domain, log_cell, blob_index, cell_index, values, paths):
        """One status byte per (blob, cell) pair, verified on the device in one call; the bytes verify_cells_blobs() gives."""
        com = _commitment_table(commitments)
        bidx, idx, val, pth = _blob_cell_arrays(log_domain, log_cell, blob_index, cell_index, values, paths)
        status = np.zeros(len(idx), dtype=np.uint8)
        _check(
            self._L.frieda_verify_cells_blobs_many(self._h, com.ctypes.data, len(com) // 32, log_domain, log_cell, bidx.ctypes.data, idx.ctypes.data, len(idx),
                                                   val.ctypes.data, pth.ctypes.data, status.ctypes.data),
            self._h,
        )
        return status

    def reconstruct_blobs_from_opened_stripes(self, commitments, log_blowup_factor, n_bytes, log_cell, stripe_index, values, paths):
        """A block sampled by stripes (stripe j = cell j of every blob): values [S, K, 4, 2^log_cell], paths [S, K, log_domain - log_cell, 32].
        Verifies every cell, uses the stripes whose K cells are all accepted and rebuilds all K blobs in one reconstruction:
        (list of K bytes, status uint8 [S, K], n_stripes_used).  Raises FriedaError (with .n_stripes_used and .cell_status set) when the
        fully accepted stripes do not suffice or a blob does not commit to its commitment."""
        com = _commitment_table(commitments)
        K = len(com) // 32
        log_domain = codec_log_size(n_bytes) + log_blowup_factor
        stripes = np.ascontiguousarray(stripe_index, dtype=np.uint32).reshape(-1)
        S = len(stripes)
        _, val, pth = _cell_arrays(log_domain, log_cell, np.zeros(S * K, dtype=np.uint32), values, paths)
        status = np.zeros(max(S * K, 1), dtype=np.uint8)
        out = np.zeros(max(n_bytes * K, 1), dtype=np.uint8)
        n = C.c_size_t(0)
        try:
            _check(
                self._L.frieda_reconstruct_blobs_from_opened_stripes(
                    self._h, com.ctypes.data, K, log_blowup_factor, n_bytes, log_cell, stripes.ctypes.data, S, val.ctypes.data, pth.ctypes.data,
                    out.ctypes.data, status.ctypes.data, C.byref(n)
                ),
                self._h,
            )
        except FriedaError as e:
            e.n_stripes_used = n.value
            e.cell_status = status[: S * K].reshape(S, K)
            raise
        return [out[b * n_bytes : (b + 1) * n_bytes].tobytes() for b in range(K)], status[: S * K].reshape(S, K), n.value

    # ---- stripe bundles: a block's stripes under one shared witness per blob (open_stripe_bundles is the provider's half) ----
    def verify_stripe_bundles_many(self, commitments, log_domain, log_cell, bundles, values, witness, witness_first):
        """One status byte per (bundle, blob), numpy uint8 [n_bundles, K], verified on the device; the bytes verify_stripe_bundles()
        gives.  bundles: one ascending stripe index list per bundle; values / witness / witness_first as open_stripe_bundles returns them."""
        com = _commitment_table(commitments)
        K = len(com) // 32
        idx, first, val, wit, wfirst = _stripe_bundle_arrays(K, log_cell, bundles, values, witness, witness_first)
        count = len(first) - 1
        status = np.zeros(max(count * K, 1), dtype=np.uint8)
        _check(
            self._L.frieda_verify_stripe_bundles_many(self._h, com.ctypes.data, K, log_domain, log_cell, idx.ctypes.data, first.ctypes.data, count,
                                                      val.ctypes.data, wit.ctypes.data, wfirst.ctypes.data, status.ctypes.data),
            self._h,
        )
        return status[: count * K].reshape(count, K)

    def reconstruct_blobs_from_stripe_bundles(self, commitments, log_blowup_factor, n_bytes, log_cell, bundles, values, witness, witness_first):
        """Verify the stripe bundles of a block, use the bundles whose K pieces are all accepted and rebuild all K blobs in one
        reconstruction: (list of K bytes, status uint8 [n_bundles, K], n_stripes_used).  Raises FriedaError (with .n_stripes_used and
        .bundle_status set) when the stripes of the used bundles do not suffice or a blob does not commit to its commitment."""
        com = _commitment_table(commitments)
        K = len(com) // 32
        idx, first, val, wit, wfirst = _stripe_bundle_arrays(K, log_cell, bundles, values, witness, witness_first)
        count = len(first) - 1
        status = np.zeros(max(count * K, 1), dtype=np.uint8)
        out = np.zeros(max(n_bytes * K, 1), dtype=np.uint8)
        n = C.c_size_t(0)
        try:
            _check(
                self._L.frieda_reconstruct_blobs_from_stripe_bundles(
                    self._h, com.ctypes.data, K, log_blowup_factor, n_bytes, log_cell, idx.ctypes.data, first.ctypes.data, count, val.ctypes.data,
                    wit.ctypes.data, wfirst.ctypes.data, out.ctypes.data, status.ctypes.data, C.byref(n)
                ),
                self._h,
            )
        except FriedaError as e:
            e.n_stripes_used = n.value
            e.bundle_status = status[: count * K].reshape(count, K)
            raise
        return [out[b * n_bytes : (b + 1) * n_bytes].tobytes() for b in range(K)], status[: count * K].reshape(count, K), n.value

    # ---- encoded handles for a block in one call, and straight from a rebuild (frieda_encode_batch, frieda_rebuild_encoded_*) ----
    def encode_batch(self, blobs, log_blowup_factor, stride=None):
        """Context.encode of every blob of a block in one call: a list of Encoded sharing one device allocation, each closed on its own.
        blobs: equal-length byte strings; stride (optional, >= the length): the distance of the blobs in the array handed to the library."""
        count = len(blobs)
        if count == 0:
            return []
        length = len(blobs[0])
        if any(len(b) != length for b in blobs):
            raise ValueError("a batch holds blobs of one length")
        stride = length if stride is None else int(stride)
        if stride < length:
            raise ValueError("stride smaller than the blob length")
        flat = b"".join(bytes(b) + b"\xa5" * (stride - length) for b in blobs)
        buf = (C.c_uint8 * max(len(flat), 1)).from_buffer_copy(flat or b"\0")
        outs = (C.c_void_p * count)()
        _check(self._L.frieda_encode_batch(self._h, buf, stride, length, count, log_blowup_factor, outs), self._h)
        return [Encoded(C.c_void_p(outs[b]), length, log_blowup_factor) for b in range(count)]

    def _rebuild_encoded(self, fn, args_before, n_bytes, n_blobs, status, log_blowup_factor, want_bytes):
        """the shared tail of the four rebuild_encoded_* methods: (out array or None, list of Encoded, n_used); raises with .n set"""
        out = np.zeros(max(n_bytes * n_blobs, 1), dtype=np.uint8) if want_bytes else None
        n = C.c_size_t(0)
        encs = (C.c_void_p * n_blobs)()
        try:
            _check(fn(self._h, *args_before, out.ctypes.data if want_bytes else None, status.ctypes.data, C.byref(n), encs), self._h)
        except FriedaError as e:
            e.n_used = n.value
            raise
        return out, [Encoded(C.c_void_p(encs[b]), n_bytes, log_blowup_factor) for b in range(n_blobs)], n.value

    def rebuild_encoded_from_opened_cells(self, commitment, log_blowup_factor, n_bytes, log_cell, cell_index, values, paths, want_bytes=True):
        """reconstruct_from_opened_cells that also returns the rebuilt blob as an Encoded, without encoding the bytes again: (bytes, status,
        n_cells_used, Encoded); bytes is None with want_bytes=False (nothing is packed or downloaded).  Raises FriedaError as the twin does
        (with .n_cells_used and .cell_status set)."""
        log_domain = codec_log_size(n_bytes) + log_blowup_factor
        idx, val, pth = _cell_arrays(log_domain, log_cell, cell_index, values, paths)
        count = len(idx)
        status = np.zeros(max(count, 1), dtype=np.uint8)
        com = (C.c_uint8 * 32)(*commitment)
        try:
            out, encs, n = self._rebuild_encoded(
                self._L.frieda_rebuild_encoded_from_opened_cells,
                (com, log_blowup_factor, n_bytes, log_cell, idx.ctypes.data, count, val.ctypes.data, pth.ctypes.data), n_bytes, 1, status, log_blowup_factor, want_bytes
            )
        except FriedaError as e:
            e.n_cells_used = e.n_used
            e.cell_status = status[:count]
            raise
        return (out[:n_bytes].tobytes() if want_bytes else None), status[:count], n, encs[0]

    def rebuild_encoded_from_cell_bundles(self, commitment, log_blowup_factor, n_bytes, log_cell, bundles, values, witness, witness_first, want_bytes=True):
        """reconstruct_from_cell_bundles + the Encoded: (bytes or None, status, n_cells_used, Encoded); errors as the twin (.n_cells_used,
        .bundle_status)."""
        idx, first, val, wit, wfirst = _bundle_arrays(log_cell, bundles, values, witness, witness_first)
        count = len(first) - 1
        status = np.zeros(max(count, 1), dtype=np.uint8)
        com = (C.c_uint8 * 32)(*commitment)
        try:
            out, encs, n = self._rebuild_encoded(
                self._L.frieda_rebuild_encoded_from_cell_bundles,
                (com, log_blowup_factor, n_bytes, log_cell, idx.ctypes.data, first.ctypes.data, count, val.ctypes.data, wit.ctypes.data, wfirst.ctypes.data),
                n_bytes, 1, status, log_blowup_factor, want_bytes
            )
        except FriedaError as e:
            e.n_cells_used = e.n_used
            e.bundle_status = status[:count]
            raise
        return (out[:n_bytes].tobytes() if want_bytes else None), status[:count], n, encs[0]

    def rebuild_encoded_blobs_from_opened_stripes(self, commitments, log_blowup_factor, n_bytes, log_cell, stripe_index, values, paths, want_bytes=True):
        """reconstruct_blobs_from_opened_stripes + one Encoded per blob (sharing one allocation): (list of K bytes or None, status [S, K],
        n_stripes_used, list of K Encoded); errors as the twin (.n_stripes_used, .cell_status)."""
        com = _commitment_table(commitments)
        K = len(com) // 32
        log_domain = codec_log_size(n_bytes) + log_blowup_factor
        stripes = np.ascontiguousarray(stripe_index, dtype=np.uint32).reshape(-1)
        S = len(stripes)
        _, val, pth = _cell_arrays(log_domain, log_cell, np.zeros(S * K, dtype=np.uint32), values, paths)
        status = np.zeros(max(S * K, 1), dtype=np.uint8)
        try:
            out, encs, n = self._rebuild_encoded(
                self._L.frieda_rebuild_encoded_blobs_from_opened_stripes,
                (com.ctypes.data, K, log_blowup_factor, n_bytes, log_cell, stripes.ctypes.data, S, val.ctypes.data, pth.ctypes.data), n_bytes, K, status,
                log_blowup_factor, want_bytes
            )
        except FriedaError as e:
            e.n_stripes_used = e.n_used
            e.cell_status = status[: S * K].reshape(S, K)
            raise
        blobs = [out[b * n_bytes : (b + 1) * n_bytes].tobytes() for b in range(K)] if want_bytes else None
        return blobs, status[: S * K].reshape(S, K), n, encs

    def rebuild_encoded_blobs_from_stripe_bundles(self, commitments, log_blowup_factor, n_bytes, log_cell, bundles, values, witness, witness_first, want_bytes=True):
        """reconstruct_blobs_from_stripe_bundles + one Encoded per blob: (list of K bytes or None, status [n_bundles, K], n_stripes_used,
        list of K Encoded); errors as the twin (.n_stripes_used, .bundle_status)."""
        com = _commitment_table(commitments)
        K = len(com) // 32
        idx, first, val, wit, wfirst = _stripe_bundle_arrays(K, log_cell, bundles, values, witness, witness_first)
        count = len(first) - 1
        status = np.zeros(max(count * K, 1), dtype=np.uint8)
        try:
            out, encs, n = self._rebuild_encoded(
                self._L.frieda_rebuild_encoded_blobs_from_stripe_bundles,
                (com.ctypes.data, K, log_blowup_factor, n_bytes, log_cell, idx.ctypes.data, first.ctypes.data, count, val.ctypes.data, wit.ctypes.data,
                 wfirst.ctypes.data), n_bytes, K, status, log_blowup_factor, want_bytes
            )
        except FriedaError as e:
            e.n_stripes_used = e.n_used
            e.bundle_status = status[: count * K].reshape(count, K)
            raise
        blobs = [out[b * n_bytes : (b + 1) * n_bytes].tobytes() for b in range(K)] if want_bytes else None
        return blobs, status[: count * K].reshape(count, K), n, encs


def codec_log_size(n_bytes):
    """log2 of the coefficients per column of a blob of n_bytes (frieda_codec_shape)."""
    a, b, lg = C.c_size_t(0), C.c_size_t(0), C.c_uint32(0)
    _check(_lib.lib().frieda_codec_shape(n_bytes, C.byref(a), C.byref(b), C.byref(lg)))
    return int(lg.value)


def _cell_arrays(log_domain, log_cell, cell_index, values, paths):
    """the three host arrays of a cells call, contiguous and of the shapes the C ABI reads: a short array must not reach the library"""
    if not 0 <= log_cell <= log_domain:
        raise FriedaError(_lib.ERR_ARG, "log_cell out of range")
    idx = np.ascontiguousarray(cell_index, dtype=np.uint32).reshape(-1)
    val = np.ascontiguousarray(values, dtype=np.uint32).reshape(-1)
    pth = np.ascontiguousarray(paths, dtype=np.uint8).reshape(-1)
    if val.size != (len(idx) * 4) << log_cell or pth.size != len(idx) * 32 * (log_domain - log_cell):
        raise FriedaError(_lib.ERR_ARG, "values / paths do not have the shape of the cell list")
    if pth.size == 0:
        pth = np.zeros(1, dtype=np.uint8)
    if val.size == 0:
        val = np.zeros(1, dtype=np.uint32)
    if idx.size == 0:
        idx = np.zeros(0, dtype=np.uint32)
    return idx, val, pth


def _bundle_index_arrays(bundles):
    """one index list per bundle -> (the indices back to back, bundle_first[n_bundles + 1])"""
    lists = [np.ascontiguousarray(b, dtype=np.uint32).reshape(-1) for b in bundles]
    first = np.zeros(len(lists) + 1, dtype=np.uint32)
    if lists:
        first[1:] = np.cumsum([len(x) for x in lists])
    idx = np.concatenate(lists) if lists else np.zeros(0, dtype=np.uint32)
    return np.ascontiguousarray(idx, dtype=np.uint32), first


def _bundle_arrays(log_cell, bundles, values, witness, witness_first):
    """the host arrays of a bundles call, contiguous and of the sizes the C ABI reads: a short array must not reach the library (what the
    arrays SAY — order, range, witness lengths — is the library's to judge: a bad bundle gets its own status)"""
    if not 0 <= log_cell <= _lib.MAX_LOG_OPEN_CELL:
        raise FriedaError(_lib.ERR_ARG, "log_cell out of range")
    idx, first = _bundle_index_arrays(bundles)
    val = np.ascontiguousarray(values, dtype=np.uint32).reshape(-1)
    wit = np.ascontiguousarray(witness, dtype=np.uint8).reshape(-1)
    wfirst = np.ascontiguousarray(witness_first, dtype=np.uint64).reshape(-1)
    if val.size != (len(idx) * 4) << log_cell:
        raise FriedaError(_lib.ERR_ARG, "values do not have the shape of the cell list")
    if len(wfirst) != len(first) or (len(wfirst) and wit.size < 32 * int(wfirst.max())):
        raise FriedaError(_lib.ERR_ARG, "witness_first: one entry per bundle and one more, none beyond the witness")
    if wit.size == 0:
        wit = np.zeros(1, dtype=np.uint8)
    if val.size == 0:
        val = np.zeros(1, dtype=np.uint32)
    if idx.size == 0:
        idx = np.zeros(1, dtype=np.uint32)
    return idx, first, val, wit, wfirst


def _stripe_bundle_arrays(n_blobs, log_cell, bundles, values, witness, witness_first):
    """the host arrays of a stripe-bundles call: as _bundle_arrays with K blobs behind every stripe and every witness hash"""
    if not 0 <= log_cell <= _lib.MAX_LOG_OPEN_CELL:
        raise FriedaError(_lib.ERR_ARG, "log_cell out of range")
    if n_blobs < 1:
        raise FriedaError(_lib.ERR_ARG, "no commitments")
    idx, first = _bundle_index_arrays(bundles)
    val = np.ascontiguousarray(values, dtype=np.uint32).reshape(-1)
    wit = np.ascontiguousarray(witness, dtype=np.uint8).reshape(-1)
    wfirst = np.ascontiguousarray(witness_first, dtype=np.uint64).reshape(-1)
    if val.size != (len(idx) * n_blobs * 4) << log_cell:
        raise FriedaError(_lib.ERR_ARG, "values do not have the shape of the stripe list")
    if len(wfirst) != len(first) or (len(wfirst) and wit.size < 32 * n_blobs * int(wfirst.max())):
        raise FriedaError(_lib.ERR_ARG, "witness_first: one entry per bundle and one more, none beyond the witness")
    if wit.size == 0:
        wit = np.zeros(1, dtype=np.uint8)
    if val.size == 0:
        val = np.zeros(1, dtype=np.uint32)
    if idx.size == 0:
        idx = np.zeros(1, dtype=np.uint32)
    return idx, first, val, wit, wfirst


def _commitment_table(commitments):
    """[K][32] commitments -> one contiguous uint8 array of 32 K bytes"""
    rows = [bytes(c) for c in commitments]
    if not rows or any(len(r) != 32 for r in rows):
        raise FriedaError(_lib.ERR_ARG, "commitments: need at least one, 32 bytes each")
    return np.frombuffer(b"".join(rows), dtype=np.uint8).copy()


def _blob_cell_arrays(log_domain, log_cell, blob_index, cell_index, values, paths):
    """_cell_arrays plus the blob numbers: one per cell"""
    idx, val, pth = _cell_arrays(log_domain, log_cell, cell_index, values, paths)
    bidx = np.ascontiguousarray(blob_index, dtype=np.uint32).reshape(-1)
    if len(bidx) != len(idx):
        raise FriedaError(_lib.ERR_ARG, "blob_index / cell_index: one blob number per cell")
    return bidx, idx, val, pth


class Encoded:
    """An encoded blob on the device (frieda_encoded): evaluations + first-layer tree + root, in an allocation of its own that outlives
    the context's workspace.  Only read by proving: several contexts of its device may prove from it at once.  close() frees it."""

    def __init__(self, handle, length, log_blowup_factor):
        self._h = handle
        self.length = int(length)
        self.log_blowup_factor = int(log_blowup_factor)

    def _handle(self):
        if not self._h:
            raise ValueError("the encoded blob is closed")
        return self._h

    @property
    def commitment(self):
        root = (C.c_uint8 * 32)()
        _check(_lib.lib().frieda_encoded_commitment(self._handle(), root))
        return bytes(root)

    @property
    def nbytes(self):
        return int(_lib.lib().frieda_encoded_bytes(self._handle()))

    @property
    def shape(self):
        """(log_size_bound, log_domain) of the encoded codeword (frieda_encoded_shape)"""
        a, b = C.c_uint32(0), C.c_uint32(0)
        _check(_lib.lib().frieda_encoded_shape(self._handle(), C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    @property
    def aggregate_of(self):
        """the number of blobs an aggregate handle (Context.aggregate_encoded) combines; 0 for a blob's own handle"""
        return int(_lib.lib().frieda_encoded_aggregate_of(self._handle()))

    def open_cells(self, ctx, log_cell, cell_index):
        """Cells of the codeword with their Merkle paths to `commitment` (frieda_open_cells, on `ctx`, which must be on the blob's
        device): (values uint32 [n, 4, 2^log_cell], paths uint8 [n, log_domain - log_cell, 32])."""
        log_domain = self.shape[1]
        if not 0 <= log_cell <= log_domain:
            raise FriedaError(_lib.ERR_ARG, "log_cell out of range")
        idx = np.ascontiguousarray(cell_index, dtype=np.uint32).reshape(-1)
        values = np.zeros((len(idx), 4, 1 << log_cell), dtype=np.uint32)
        paths = np.zeros((len(idx), log_domain - log_cell, 32), dtype=np.uint8)
        _check(
            _lib.lib().frieda_open_cells(ctx._h, self._handle(), log_cell, idx.ctypes.data, len(idx), values.ctypes.data if values.size else None,
                                         paths.ctypes.data if paths.size else None),
            ctx._h,
        )
        return values, paths

    def open_cell_bundles(self, ctx, log_cell, bundles):
        """Cells of the codeword in bundles, each bundle (one strictly ascending index list) under ONE shared Merkle witness
        (frieda_open_cell_bundles on `ctx`): (values uint32 [n, 4, 2^log_cell] over all cells of the call, witness uint8 [H, 32] of all
        bundles back to back, witness_first uint64 [n_bundles + 1] in hashes)."""
        idx, first = _bundle_index_arrays(bundles)
        nb = len(first) - 1
        wfirst = np.zeros(nb + 1, dtype=np.uint64)
        if nb == 0:
            return np.zeros((0, 4, 1 << log_cell), dtype=np.uint32), np.zeros((0, 32), dtype=np.uint8), wfirst
        L = _lib.lib()
        iptr = idx.ctypes.data if idx.size else None
        _check(L.frieda_open_cell_bundles(ctx._h, self._handle(), log_cell, iptr, first.ctypes.data, nb, None, None, 0, wfirst.ctypes.data), ctx._h)
        total = int(wfirst[-1])
        values = np.zeros((len(idx), 4, 1 << log_cell), dtype=np.uint32)
        witness = np.zeros((max(total, 1), 32), dtype=np.uint8)
        _check(L.frieda_open_cell_bundles(ctx._h, self._handle(), log_cell, iptr, first.ctypes.data, nb, values.ctypes.data, witness.ctypes.data, total,
                                          wfirst.ctypes.data), ctx._h)
        return values, witness[:total], wfirst

    def close(self):
        if self._h:
            _lib.lib().frieda_encoded_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class Proof:
    """frieda::proof::Proof (src/proof.rs:19-26).  Fields are public upstream, so they are readable and writable here."""

    def __init__(self, handle):
        self._h = handle
        self._L = _lib.lib()

    def __del__(self):
        try:
            if self._h:
                self._L.frieda_proof_free(self._h)
                self._h = None
        except Exception:
            pass

    def clone(self):
        out = C.c_void_p()
        _check(self._L.frieda_proof_clone(self._h, C.byref(out)))
        return Proof(out)

    @property
    def proof_of_work(self):
        return self._L.frieda_proof_proof_of_work(self._h)

    @proof_of_work.setter
    def proof_of_work(self, v):
        self._L.frieda_proof_set_proof_of_work(self._h, v)

    @property
    def pcs_config(self):
        c = self._L.frieda_proof_pcs_config(self._h)
        return PcsConfig(FriConfig(c.log_blowup_factor, c.log_last_layer_degree_bound, c.n_queries), c.pow_bits)

    @property
    def log_size_bound(self):
        return self._L.frieda_proof_log_size_bound(self._h)

    @property
    def evaluations(self):
        """uint32[n, 4] copy of Vec<QM31>."""
        n = self._L.frieda_proof_n_evaluations(self._h)
        if n == 0:
            return np.zeros((0, 4), dtype=np.uint32)
        p = self._L.frieda_proof_evaluations(self._h)
        return np.ctypeslib.as_array(p, shape=(n, 4)).copy()

    @evaluations.setter
    def evaluations(self, arr):
        arr = np.ascontiguousarray(arr, dtype=np.uint32).reshape(-1, 4)
        _check(self._L.frieda_proof_resize_evaluations(self._h, arr.shape[0]))
        if arr.shape[0]:
            p = self._L.frieda_proof_evaluations(self._h)
            C.memmove(p, arr.ctypes.data, arr.nbytes)

    @property
    def n_inner_layers(self):
        return self._L.frieda_proof_n_inner_layers(self._h)

    def layer(self, i):
        """Layer 0 = first_layer, 1.. = inner_layers[i-1] -> dict(commitment, fri_witness, hash_witness, column_witness)."""
        n = C.c_size_t()
        com = bytes(self._L.frieda_proof_layer_commitment(self._h, i)[:32])
        p = self._L.frieda_proof_layer_fri_witness(self._h, i, C.byref(n))
        fw = np.ctypeslib.as_array(p, shape=(n.value, 4)).copy() if n.value else np.zeros((0, 4), np.uint32)
        p = self._L.frieda_proof_layer_hash_witness(self._h, i, C.byref(n))
        hw = [bytes(p[32 * j : 32 * j + 32]) for j in range(n.value)]
        p = self._L.frieda_proof_layer_column_witness(self._h, i, C.byref(n))
        cw = np.ctypeslib.as_array(p, shape=(n.value,)).copy() if n.value else np.zeros((0,), np.uint32)
        return {"commitment": com, "fri_witness": fw, "hash_witness": hw, "column_witness": cw}

    @property
    def commitment(self):
        return bytes(self._L.frieda_proof_layer_commitment(self._h, 0)[:32])

    @property
    def last_layer_poly(self):
        n = C.c_size_t()
        p = self._L.frieda_proof_last_layer_poly(self._h, C.byref(n))
        return np.ctypeslib.as_array(p, shape=(n.value, 4)).copy() if n.value else np.zeros((0, 4), np.uint32)

    def serialize(self):
        n = self._L.frieda_proof_serialize(self._h, None, 0)
        buf = (C.c_uint8 * n)()
        self._L.frieda_proof_serialize(self._h, buf, n)
        return bytes(buf)

    @staticmethod
    def deserialize(blob):
        a = np.frombuffer(bytes(blob), dtype=np.uint8)
        out = C.c_void_p()
        _check(_lib.lib().frieda_proof_deserialize(a.ctypes.data, a.size, C.byref(out)))
        return Proof(out)


from ._lib import BLOCK_BUNDLE, BLOCK_COMBINATION, BLOCK_FRI, BLOCK_INDICES, BLOCK_OK, BLOCK_SHAPE  # noqa: E402,F401  (frieda_verify_block's reasons)


class BlockProof:
    """frieda_block_proof: ONE FRI proof for all blobs of a block — the proof of the aggregate under a seed (`fri`) and the blobs opened
    where it was queried, as one stripe bundle at log_cell 1 (`stripe_index`, `values`, `witness`, in the layouts of
    verify_stripe_bundles).  A protocol of this project, not of the reference."""

    def __init__(self, handle):
        self._h = handle
        self._L = _lib.lib()

    def __del__(self):
        try:
            if self._h:
                self._L.frieda_block_proof_free(self._h)
                self._h = None
        except Exception:
            pass

    @property
    def fri(self):
        """a copy of the FRI part as an ordinary Proof"""
        out = C.c_void_p()
        _check(self._L.frieda_proof_clone(self._L.frieda_block_proof_fri(self._h), C.byref(out)))
        return Proof(out)

    @property
    def n_blobs(self):
        return int(self._L.frieda_block_proof_n_blobs(self._h))

    @property
    def n_stripes(self):
        return int(self._L.frieda_block_proof_n_stripes(self._h))

    @property
    def witness_hashes(self):
        """witness hashes per blob"""
        return int(self._L.frieda_block_proof_witness_hashes(self._h))

    def _array(self, ptr, ctype, dtype, count, shape):
        if count == 0:
            return np.zeros(shape, dtype=dtype)
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ctype)), shape=(count,)).copy().reshape(shape)

    @property
    def stripe_index(self):
        n = self.n_stripes
        return self._array(self._L.frieda_block_proof_stripe_index(self._h), C.c_uint32, np.uint32, n, (n,))

    @property
    def values(self):
        """uint32 [n_stripes, n_blobs, 4, 2]"""
        n, k = self.n_stripes, self.n_blobs
        return self._array(self._L.frieda_block_proof_values(self._h), C.c_uint32, np.uint32, 8 * n * k, (n, k, 4, 2))

    @property
    def witness(self):
        """uint8 [n_blobs, witness_hashes, 32]"""
        k, w = self.n_blobs, self.witness_hashes
        return self._array(self._L.frieda_block_proof_witness(self._h), C.c_uint8, np.uint8, 32 * k * w, (k, w, 32))

    def serialize(self):
        n = self._L.frieda_block_proof_serialize(self._h, None, 0)
        buf = (C.c_uint8 * n)()
        self._L.frieda_block_proof_serialize(self._h, buf, n)
        return bytes(buf)

    @staticmethod
    def from_bytes(blob):
        a = np.frombuffer(bytes(blob), dtype=np.uint8)
        out = C.c_void_p()
        _check(_lib.lib().frieda_block_proof_deserialize(a.ctypes.data if a.size else None, a.size, C.byref(out)))
        return BlockProof(out)

    @staticmethod
    def from_parts(fri, stripe_index, values, witness):
        """A block proof from its parts (a relay that re-bundles, a test that tampers): `fri` a Proof, values [n_stripes, n_blobs, 4, 2],
        witness [n_blobs, W, 32] — assembled as the wire image and read back, so the rules of from_bytes apply."""
        img = fri.serialize()
        idx = np.ascontiguousarray(stripe_index, dtype="<u4").reshape(-1)
        val = np.ascontiguousarray(values, dtype="<u4").reshape(len(idx), -1, 4, 2)
        k = val.shape[1]
        wit = np.ascontiguousarray(witness, dtype=np.uint8).reshape(-1)
        head = np.array([0x31504246, 1, k, len(idx)], dtype="<u4").tobytes() + np.array([wit.size // (32 * max(k, 1)), len(img)], dtype="<u8").tobytes()
        return BlockProof.from_bytes(head + img + idx.tobytes() + val.tobytes() + wit.tobytes())


def block_challenge(commitments):
    """rho of a block as four M31 words: a default channel, mix_u64(K), mix_root of every commitment in order, one draw_felt (host only)"""
    tab = _commitment_table(commitments)
    out = (C.c_uint32 * 4)()
    _check(_lib.lib().frieda_block_challenge(tab.ctypes.data, len(tab) // 32, out))
    return tuple(int(x) for x in out)


def verify_block(commitments, block_proof, seed):
    """(ok, reason): the client's check of a block proof against the block's commitments (host only); reason is BLOCK_OK or the first
    failing step, BLOCK_SHAPE / _FRI / _INDICES / _BUNDLE / _COMBINATION."""
    tab = _commitment_table(commitments)
    ok, reason = C.c_int(0), C.c_uint32(0)
    _check(_lib.lib().frieda_verify_block(tab.ctypes.data, len(tab) // 32, block_proof._h, _seed_ptr(seed), C.byref(ok), C.byref(reason)))
    return bool(ok.value), int(reason.value)


class MultiContext:
    """A batch of independent blobs across the GPUs of one node from ONE process (frieda_multi, include/frieda_hip.h): blob i runs
    on devices[i mod n] (one host thread + two contexts per device), the 32-byte roots are gathered with ncclAllGather on a
    single-process RCCL communicator.  The one-process-per-GPU launch model (bench.py, torch.distributed) lives in batch.py."""

    def __init__(self, devices):
        self._L = _lib.lib()
        self._h = C.c_void_p()
        devs = (C.c_int * len(devices))(*[int(d) for d in devices])
        st = self._L.frieda_multi_create(devs, len(devices), C.byref(self._h))
        if st != _lib.OK:
            raise FriedaError(st, f"frieda_multi_create({list(devices)})")

    def _check(self, st):
        if st != _lib.OK:
            detail = self._L.frieda_multi_last_error(self._h).decode(errors="replace")
            raise (FriedaPanic if st == _lib.ERR_INVARIANT else FriedaError)(st, detail)

    def close(self):
        if self._h:
            self._L.frieda_multi_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def release_workspace(self):
        """Frees the device workspaces (two per device, up to the batch budget each) and upload rings the handle keeps between calls."""
        self._check(self._L.frieda_multi_release_workspace(self._h))

    @property
    def device_count(self):
        return self._L.frieda_multi_device_count(self._h)

    @property
    def uses_rccl(self):
        return bool(self._L.frieda_multi_uses_rccl(self._h))

    @property
    def gather_count(self):
        return int(self._L.frieda_multi_gather_count(self._h))

    def _blob_table(self, blobs):
        arrs = [_as_bytes(b) for b in blobs]
        ptrs = (C.c_void_p * len(arrs))(*[a.ctypes.data if a.size else None for a in arrs])
        lens = (C.c_size_t * len(arrs))(*[a.size for a in arrs])
        return arrs, ptrs, lens

    def commit_many(self, blobs, log_blowup_factor):
        if not blobs:
            return []
        arrs, ptrs, lens = self._blob_table(blobs)
        roots = (C.c_uint8 * (32 * len(arrs)))()
        self._check(self._L.frieda_commit_many(self._h, ptrs, lens, len(arrs), log_blowup_factor, roots))
        rb = bytes(roots)
        return [rb[32 * i : 32 * i + 32] for i in range(len(arrs))]

    def prove_many(self, blobs, seeds, pcs_config):
        """-> [(commitment, Proof)] in blob order; seeds: None or one per blob"""
        if not blobs:
            return []
        arrs, ptrs, lens = self._blob_table(blobs)
        n = len(arrs)
        if seeds is not None and len(seeds) != n:
            raise ValueError("one seed per blob")
        sd = (C.c_uint64 * n)(*seeds) if seeds is not None else None
        roots = (C.c_uint8 * (32 * n))()
        outs = (C.c_void_p * n)()
        self._check(self._L.frieda_prove_many(self._h, ptrs, lens, n, sd, pcs_config._c(), roots, outs))
        rb = bytes(roots)
        return [(rb[32 * i : 32 * i + 32], Proof(C.c_void_p(outs[i]))) for i in range(n)]


class ProofPipeline:
    """Keeps up to `depth` proofs in flight on one GPU (one Context = stream + workspace each), so that the latency-bound
    tail of one proof (tree tops, small FRI layers, host round trips) overlaps the throughput-bound kernels of the next.
    submit() returns the oldest finished (commitment, proof) once the pipeline is full, else None; drain() flushes."""

    def __init__(self, device=0, depth=2):
        self.ctxs = [Context(device) for _ in range(depth)]
        self.inflight = []  # contexts with a proof in flight, oldest first
        self.free = list(self.ctxs)

    def submit_device(self, d_ptr, length, seed, pcs_config):
        done = None
        if not self.free:
            ctx = self.inflight.pop(0)
            done = ctx.prove_finish()
            self.free.append(ctx)
        ctx = self.free.pop(0)
        ctx.prove_begin_device(d_ptr, length, seed, pcs_config)
        self.inflight.append(ctx)
        return done

    def drain(self):
        out = []
        while self.inflight:
            ctx = self.inflight.pop(0)
            out.append(ctx.prove_finish())
            self.free.append(ctx)
        return out

    def close(self):
        self.drain()
        for c in self.ctxs:
            c.close()


class BatchPipeline:
    """ProofPipeline for batches: up to `depth` batches of equal-length blobs in flight on one GPU (frieda_prove_batch_begin_device /
    _finish on one Context each).  The Fiat-Shamir chain is paid once per batch AND runs under the other batch's wide kernels —
    the highest-throughput way through a stream of blobs.  submit returns the oldest finished batch's [(commitment, proof)] or None."""

    def __init__(self, device=0, depth=2):
        self.ctxs = [Context(device) for _ in range(depth)]
        self.inflight = []  # (ctx, count, time of _begin), oldest first
        self.free = list(self.ctxs)
        self.call_latencies = []  # (blobs, seconds from _begin to the return of _finish) of every finished call; callers may clear it

    def plan(self, length, count, pcs_config, prove=True):
        """The library's cut of `count` equal-length blobs into calls for this pipeline's depth (frieda_batch_plan: workspace bytes in
        flight; the options FRIEDA_BATCH_BUDGET_MB / FRIEDA_BATCH_CALLS_PER_CTX of the first context apply)."""
        return batch_plan(length, count, pcs_config, in_flight=len(self.ctxs), prove=prove, ctx=self.ctxs[0])

    def run_stream_device(self, d_ptr, stride, length, count, seeds, pcs_config):
        """`count` device-resident blobs of one length (blob i at d_ptr + i * stride) through the pipeline, cut into calls by the library's
        batch policy; returns [(commitment, proof)] in blob order (the caller loop of benches/proof.rs:30-44 over many blobs)."""
        out = []
        i = 0
        for cnt in self.plan(length, count, pcs_config):
            sd = None if seeds is None else seeds[i : i + cnt]
            r = self.submit_device(d_ptr + i * stride, stride, length, cnt, sd, pcs_config)
            if r is not None:
                out.extend(r)
            i += cnt
        out.extend(self.drain())
        return out

    def submit_device(self, d_ptr, stride, length, count, seeds, pcs_config):
        done = None
        if not self.free:
            done = self._finish_oldest()
        ctx = self.free.pop(0)
        t0 = time.perf_counter()
        ctx.prove_batch_begin_device(d_ptr, stride, length, count, seeds, pcs_config)
        self.inflight.append((ctx, count, t0))
        return done

    def _finish_oldest(self):
        ctx, cnt, t0 = self.inflight.pop(0)
        done = ctx.prove_batch_finish(cnt)
        self.call_latencies.append((cnt, time.perf_counter() - t0))
        self.free.append(ctx)
        return done

    def drain(self):
        out = []
        while self.inflight:
            out.extend(self._finish_oldest())
        return out

    def close(self):
        self.drain()
        for c in self.ctxs:
            c.close()


def workspace_bytes(length, log_blowup_factor, log_last_layer_degree_bound=0, prove=True):
    """Device workspace one blob of `length` bytes adds to a batched call (frieda_workspace_bytes); 0: shape out of range."""
    return int(_lib.lib().frieda_workspace_bytes(length, log_blowup_factor, log_last_layer_degree_bound, int(bool(prove))))


def seeds_workspace_bytes(length, pcs_config, n_seeds):
    """Workspace a prove_seeds call of n_seeds seeds asks of its context, the Encoded excluded (frieda_seeds_workspace_bytes); 0: refused shape."""
    return int(_lib.lib().frieda_seeds_workspace_bytes(length, pcs_config._c(), n_seeds))


def seeds_blobs_workspace_bytes(length, pcs_config, n_blobs, n_seeds):
    """Workspace a prove_seeds_blobs call of n_blobs handles under n_seeds seeds asks of its context, the handles excluded
    (frieda_seeds_blobs_workspace_bytes); 0: refused shape.  At n_blobs == 1: seeds_workspace_bytes."""
    return int(_lib.lib().frieda_seeds_blobs_workspace_bytes(length, pcs_config._c(), n_blobs, n_seeds))


def prove_jobs_workspace_bytes(length, pcs_config, n_blobs, n_jobs):
    """Workspace one pass of n_jobs jobs over n_blobs handles asks of its context, the handles excluded (frieda_prove_jobs_workspace_bytes);
    0: refused shape.  At n_blobs == 1: seeds_workspace_bytes; at (K, K * S): seeds_blobs_workspace_bytes(K, S)."""
    return int(_lib.lib().frieda_prove_jobs_workspace_bytes(length, pcs_config._c(), n_blobs, n_jobs))


def prove_jobs_plan(length, pcs_config, n_blobs, n_jobs, ctx=None):
    """(jobs_per_pass, n_passes): how prove_jobs cuts n_jobs jobs over n_blobs handles into passes (frieda_prove_jobs_plan); ctx None:
    the default options."""
    per, n = C.c_uint32(0), C.c_uint32(0)
    h = ctx._h if ctx is not None else None
    _check(_lib.lib().frieda_prove_jobs_plan(h, length, pcs_config._c(), n_blobs, n_jobs, C.byref(per), C.byref(n)))
    return int(per.value), int(n.value)


def batch_plan(length, count, pcs_config=None, in_flight=2, prove=True, ctx=None, log_blowup_factor=None):
    """The library's batch policy (frieda_batch_plan, include/frieda_hip.h "batch policy"): the blob count of each call, in order, for
    `count` equal-length blobs and `in_flight` contexts taking turns.  pcs_config for proofs, log_blowup_factor for commits."""
    L = _lib.lib()
    if pcs_config is not None:
        B, last = pcs_config.fri_config.log_blowup_factor, pcs_config.fri_config.log_last_layer_degree_bound
    else:
        B, last = int(log_blowup_factor), 0
    n = C.c_uint32(0)
    h = ctx._h if ctx is not None else None
    _check(L.frieda_batch_plan(h, length, B, last, int(bool(prove)), count, in_flight, None, 0, C.byref(n)))
    out = (C.c_uint32 * max(1, n.value))()
    _check(L.frieda_batch_plan(h, length, B, last, int(bool(prove)), count, in_flight, out, n.value, C.byref(n)))
    return [int(out[i]) for i in range(n.value)]


# ---- module-level API with an implicit per-thread default context (frieda's free functions) ----
_tls = threading.local()


def _default_device():
    """The GPU of this process: torch's current device when torch has initialised one (one process per GPU under
    torch.distributed), else LOCAL_RANK, else 0."""
    import os
    import sys

    torch = sys.modules.get("torch")
    if torch is not None and torch.cuda.is_available() and torch.cuda.is_initialized():
        return int(torch.cuda.current_device())
    return int(os.environ.get("LOCAL_RANK", "0"))


def default_context():
    ctx = getattr(_tls, "ctx", None)
    if ctx is None:
        ctx = _tls.ctx = Context(_default_device())
    return ctx


def commit(data, log_blowup_factor):
    """api::commit (src/lib.rs:31)."""
    return default_context().commit(data, log_blowup_factor)


def generate_proof(data, seed, pcs_config):
    """api::generate_proof (src/lib.rs:36)."""
    return default_context().generate_proof(data, seed, pcs_config)


def commit_and_generate_proof(data, seed, pcs_config):
    """proof::commit_and_generate_proof (src/proof.rs:32)."""
    return default_context().commit_and_generate_proof(data, seed, pcs_config)


def commit_and_generate_proofs_for_seeds(data, seeds, pcs_config):
    """One blob, many seeds: (commitment, [Proof]) with proof i == commit_and_generate_proof(data, seeds[i], pcs_config)[1]."""
    return default_context().commit_and_generate_proofs_for_seeds(data, seeds, pcs_config)


def verify(proof, seed):
    """api::verify (src/lib.rs:41): bool; raises FriedaPanic where the reference panics.  Host-only."""
    ok = C.c_int(0)
    _check(_lib.lib().frieda_verify(proof._h, _seed_ptr(seed), C.byref(ok)))
    return bool(ok.value)


def verify_samples(proof, seed):
    """verify + where the accepted proof sampled: (ok, positions) with positions[i] the index in the bit-reversed codeword whose four
    column values are proof.evaluations[i] (frieda_verify_samples); positions is None when the proof is rejected."""
    import numpy as np

    ok = C.c_int(0)
    n = C.c_size_t(0)
    cap = max(1, int(proof.pcs_config.fri_config.n_queries))
    buf = np.zeros(cap, dtype=np.uint32)
    _check(_lib.lib().frieda_verify_samples(proof._h, _seed_ptr(seed), C.byref(ok), buf.ctypes.data, cap, C.byref(n)))
    if not ok.value:
        return False, None
    return True, buf[: n.value].copy()


def verify_pairs(proof, seed):
    """verify + every point the accepted proof authenticates (frieda_verify_pairs, host-only): (ok, positions, values) with positions the
    ascending distinct positions of both members of every opened first-layer pair and values[i] the four column words at positions[i]
    — from proof.evaluations where the position was queried, from the first layer's fri_witness otherwise; (False, None, None) when the
    proof is rejected."""
    import numpy as np

    ok = C.c_int(0)
    n = C.c_size_t(0)
    cap = max(1, 2 * int(proof.pcs_config.fri_config.n_queries))
    pos = np.zeros(cap, dtype=np.uint32)
    val = np.zeros((cap, 4), dtype=np.uint32)
    _check(_lib.lib().frieda_verify_pairs(proof._h, _seed_ptr(seed), C.byref(ok), pos.ctypes.data, val.ctypes.data, cap, C.byref(n)))
    if not ok.value:
        return False, None, None
    return True, pos[: n.value].copy(), val[: n.value].copy()


def verify_pairs_many(proofs, seeds=None, expected_commitment=None):
    """frieda_verify_pairs_many on the default context: (status, [(positions, values) or None])."""
    return default_context().verify_pairs_many(proofs, seeds, expected_commitment)


def reconstruct_from_proof_pairs(proofs, seeds, expected_commitment, n_bytes):
    """frieda_reconstruct_from_proof_pairs on the default context: (bytes, status, n_points)."""
    return default_context().reconstruct_from_proof_pairs(proofs, seeds, expected_commitment, n_bytes)


def verify_many(proofs, seeds=None, expected_commitment=None):
    """frieda_verify_many on the default context: one status byte per proof, verified in one call on the device."""
    return default_context().verify_many(proofs, seeds, expected_commitment)


def verify_blobs_many(proofs, commitments, blob_index=None, seeds=None):
    """frieda_verify_blobs_many on the default context: (status, accepted_per_blob), proof i against commitments[blob_index[i]]."""
    return default_context().verify_blobs_many(proofs, commitments, blob_index, seeds)


def verify_samples_many(proofs, seeds=None, expected_commitment=None):
    """frieda_verify_samples_many on the default context: (status, [positions or None])."""
    return default_context().verify_samples_many(proofs, seeds, expected_commitment)


def reconstruct_from_proofs(proofs, seeds, expected_commitment, n_bytes):
    """frieda_reconstruct_from_proofs on the default context: (bytes, status, n_points)."""
    return default_context().reconstruct_from_proofs(proofs, seeds, expected_commitment, n_bytes)


def open_cells(encoded, log_cell, cell_index):
    """Encoded.open_cells on the default context: (values, paths)."""
    return encoded.open_cells(default_context(), log_cell, cell_index)


def verify_cells(commitment, log_domain, log_cell, cell_index, values, paths):
    """The host verifier of opened cells (frieda_verify_cells: no context, one core): one status byte per cell (numpy uint8), CELL_ACCEPTED
    when every word is a canonical M31 and the cell's subtree root, carried up its path, equals the commitment."""
    idx, val, pth = _cell_arrays(log_domain, log_cell, cell_index, values, paths)
    status = np.zeros(len(idx), dtype=np.uint8)
    com = (C.c_uint8 * 32)(*commitment)
    _check(_lib.lib().frieda_verify_cells(com, log_domain, log_cell, idx.ctypes.data, len(idx), val.ctypes.data, pth.ctypes.data, status.ctypes.data))
    return status


def verify_cells_many(commitment, log_domain, log_cell, cell_index, values, paths):
    """frieda_verify_cells_many on the default context: one status byte per cell, verified on the device."""
    return default_context().verify_cells_many(commitment, log_domain, log_cell, cell_index, values, paths)


def reconstruct_from_opened_cells(commitment, log_blowup_factor, n_bytes, log_cell, cell_index, values, paths):
    """frieda_reconstruct_from_opened_cells on the default context: (bytes, status, n_cells_used)."""
    return default_context().reconstruct_from_opened_cells(commitment, log_blowup_factor, n_bytes, log_cell, cell_index, values, paths)


def cell_bundle_witness_count(log_domain, log_cell, cell_index):
    """The witness length, in hashes, of one bundle of the strictly ascending cells `cell_index` (frieda_cell_bundle_witness_count: host
    only).  Raises FriedaError for a malformed bundle."""
    idx = np.ascontiguousarray(cell_index, dtype=np.uint32).reshape(-1)
    n = C.c_size_t(0)
    _check(_lib.lib().frieda_cell_bundle_witness_count(log_domain, log_cell, idx.ctypes.data if idx.size else None, len(idx), C.byref(n)))
    return int(n.value)


def open_cell_bundles(encoded, log_cell, bundles):
    """Encoded.open_cell_bundles on the default context: (values, witness, witness_first)."""
    return encoded.open_cell_bundles(default_context(), log_cell, bundles)


def verify_cell_bundles(commitment, log_domain, log_cell, bundles, values, witness, witness_first):
    """The host verifier of cell bundles (frieda_verify_cell_bundles: no context, one core): one status byte per bundle (numpy uint8),
    BUNDLE_REJECTED / BUNDLE_ACCEPTED / BUNDLE_MALFORMED."""
    idx, first, val, wit, wfirst = _bundle_arrays(log_cell, bundles, values, witness, witness_first)
    status = np.zeros(max(len(first) - 1, 1), dtype=np.uint8)
    com = (C.c_uint8 * 32)(*commitment)
    _check(_lib.lib().frieda_verify_cell_bundles(com, log_domain, log_cell, idx.ctypes.data, first.ctypes.data, len(first) - 1, val.ctypes.data, wit.ctypes.data,
                                                 wfirst.ctypes.data, status.ctypes.data))
    return status[: len(first) - 1]


def verify_cell_bundles_many(commitment, log_domain, log_cell, bundles, values, witness, witness_first):
    """frieda_verify_cell_bundles_many on the default context: one status byte per bundle, verified on the device."""
    return default_context().verify_cell_bundles_many(commitment, log_domain, log_cell, bundles, values, witness, witness_first)


def reconstruct_from_cell_bundles(commitment, log_blowup_factor, n_bytes, log_cell, bundles, values, witness, witness_first):
    """frieda_reconstruct_from_cell_bundles on the default context: (bytes, status, n_cells_used)."""
    return default_context().reconstruct_from_cell_bundles(commitment, log_blowup_factor, n_bytes, log_cell, bundles, values, witness, witness_first)


def open_cells_blobs(ctx, encs, log_cell, blob_index, cell_index):
    """Cells of many encoded blobs of one shape in ONE call (frieda_open_cells_blobs on `ctx`): pair i is cell cell_index[i] of
    encs[blob_index[i]].  (values uint32 [n, 4, 2^log_cell], paths uint8 [n, log_domain - log_cell, 32])."""
    encs = list(encs)
    if not encs:
        raise FriedaError(_lib.ERR_ARG, "open_cells_blobs: no blobs")
    log_domain = encs[0].shape[1]
    if not 0 <= log_cell <= log_domain:
        raise FriedaError(_lib.ERR_ARG, "log_cell out of range")
    bidx = np.ascontiguousarray(blob_index, dtype=np.uint32).reshape(-1)
    idx = np.ascontiguousarray(cell_index, dtype=np.uint32).reshape(-1)
    if len(bidx) != len(idx):
        raise FriedaError(_lib.ERR_ARG, "blob_index / cell_index: one blob number per cell")
    handles = (C.c_void_p * len(encs))(*[e._handle() for e in encs])
    values = np.zeros((len(idx), 4, 1 << log_cell), dtype=np.uint32)
    paths = np.zeros((len(idx), log_domain - log_cell, 32), dtype=np.uint8)
    _check(
        _lib.lib().frieda_open_cells_blobs(ctx._h, handles, len(encs), log_cell, bidx.ctypes.data, idx.ctypes.data, len(idx),
                                           values.ctypes.data if values.size else None, paths.ctypes.data if paths.size else None),
        ctx._h,
    )
    return values, paths


def prove_jobs(ctx, encs, jobs, pcs_config):
    """Any list of (blob_index, seed) jobs over a block of encoded blobs in ONE call (frieda_prove_jobs on `ctx`): a flat list of Proof
    in the caller's order."""
    return ctx.prove_jobs(encs, jobs, pcs_config)


def prove_seeds_blobs(ctx, encs, seeds, pcs_config):
    """Every encoded blob of a block under every seed of one list in ONE call (frieda_prove_seeds_blobs on `ctx`): a list of
    len(encs) lists of len(seeds) Proofs."""
    return ctx.prove_seeds_blobs(encs, seeds, pcs_config)


def aggregate_encoded(ctx, encs):
    """The aggregate handle of a block (frieda_aggregate_encoded on `ctx`): once per block, whatever the seeds."""
    return ctx.aggregate_encoded(encs)


def prove_block_seeds(ctx, agg, encs, seeds, pcs_config):
    """One BlockProof per seed for the whole block (frieda_prove_block_seeds on `ctx`): len(seeds) fold chains instead of
    len(encs) * len(seeds)."""
    return ctx.prove_block_seeds(agg, encs, seeds, pcs_config)


def open_stripes(ctx, encs, log_cell, stripe_index):
    """Stripe j of a block = cell j of each of its K blobs.  One open_cells_blobs call: (values uint32 [S, K, 4, 2^log_cell],
    paths uint8 [S, K, log_domain - log_cell, 32]) — what Context.reconstruct_blobs_from_opened_stripes takes."""
    encs = list(encs)
    stripes = np.ascontiguousarray(stripe_index, dtype=np.uint32).reshape(-1)
    S, K = len(stripes), len(encs)
    values, paths = open_cells_blobs(ctx, encs, log_cell, np.tile(np.arange(K, dtype=np.uint32), S), np.repeat(stripes, K))
    return values.reshape(S, K, 4, -1), paths.reshape(S, K, -1, 32)


def verify_cells_blobs(commitments, log_domain, log_cell, blob_index, cell_index, values, paths):
    """The host verifier over (blob, cell) pairs (frieda_verify_cells_blobs: no context): one status byte per pair (numpy uint8)."""
    com = _commitment_table(commitments)
    bidx, idx, val, pth = _blob_cell_arrays(log_domain, log_cell, blob_index, cell_index, values, paths)
    status = np.zeros(len(idx), dtype=np.uint8)
    _check(_lib.lib().frieda_verify_cells_blobs(com.ctypes.data, len(com) // 32, log_domain, log_cell, bidx.ctypes.data, idx.ctypes.data, len(idx),
                                                val.ctypes.data, pth.ctypes.data, status.ctypes.data))
    return status


def verify_cells_blobs_many(commitments, log_domain, log_cell, blob_index, cell_index, values, paths):
    """frieda_verify_cells_blobs_many on the default context."""
    return default_context().verify_cells_blobs_many(commitments, log_domain, log_cell, blob_index, cell_index, values, paths)


def reconstruct_blobs_from_opened_stripes(commitments, log_blowup_factor, n_bytes, log_cell, stripe_index, values, paths):
    """frieda_reconstruct_blobs_from_opened_stripes on the default context: (list of bytes, status [S, K], n_stripes_used)."""
    return default_context().reconstruct_blobs_from_opened_stripes(commitments, log_blowup_factor, n_bytes, log_cell, stripe_index, values, paths)


def open_stripe_bundles(ctx, encs, log_cell, bundles):
    """Stripes of a block of K encoded blobs in bundles (one strictly ascending stripe index list each), every bundle under ONE shared
    Merkle witness per blob (frieda_open_stripe_bundles on `ctx`): (values uint32 [S, K, 4, 2^log_cell] over all stripes of the call,
    witness uint8 [K * H, 32] — bundle b's block starts at hash K * witness_first[b], blob j's piece at j * W_b inside it —,
    witness_first uint64 [n_bundles + 1] in hashes per blob)."""
    encs = list(encs)
    if not encs:
        raise FriedaError(_lib.ERR_ARG, "open_stripe_bundles: no blobs")
    K = len(encs)
    idx, first = _bundle_index_arrays(bundles)
    nb = len(first) - 1
    L = _lib.lib()
    handles = (C.c_void_p * K)(*[e._handle() for e in encs])
    wfirst = np.zeros(nb + 1, dtype=np.uint64)
    values = np.zeros((len(idx), K, 4, 1 << log_cell), dtype=np.uint32)
    if nb == 0:
        return values, np.zeros((0, 32), dtype=np.uint8), wfirst
    iptr = idx.ctypes.data if idx.size else None
    _check(L.frieda_open_stripe_bundles(ctx._h, handles, K, log_cell, iptr, first.ctypes.data, nb, None, None, 0, wfirst.ctypes.data), ctx._h)
    total = K * int(wfirst[-1])
    witness = np.zeros((max(total, 1), 32), dtype=np.uint8)
    _check(L.frieda_open_stripe_bundles(ctx._h, handles, K, log_cell, iptr, first.ctypes.data, nb, values.ctypes.data, witness.ctypes.data, total,
                                        wfirst.ctypes.data), ctx._h)
    return values, witness[:total], wfirst


def verify_stripe_bundles(commitments, log_domain, log_cell, bundles, values, witness, witness_first):
    """The host verifier of stripe bundles (frieda_verify_stripe_bundles: no context, one core): one status byte per (bundle, blob),
    numpy uint8 [n_bundles, K]."""
    com = _commitment_table(commitments)
    K = len(com) // 32
    idx, first, val, wit, wfirst = _stripe_bundle_arrays(K, log_cell, bundles, values, witness, witness_first)
    count = len(first) - 1
    status = np.zeros(max(count * K, 1), dtype=np.uint8)
    _check(_lib.lib().frieda_verify_stripe_bundles(com.ctypes.data, K, log_domain, log_cell, idx.ctypes.data, first.ctypes.data, count, val.ctypes.data,
                                                   wit.ctypes.data, wfirst.ctypes.data, status.ctypes.data))
    return status[: count * K].reshape(count, K)


def verify_stripe_bundles_many(commitments, log_domain, log_cell, bundles, values, witness, witness_first):
    """frieda_verify_stripe_bundles_many on the default context: status [n_bundles, K], verified on the device."""
    return default_context().verify_stripe_bundles_many(commitments, log_domain, log_cell, bundles, values, witness, witness_first)


def reconstruct_blobs_from_stripe_bundles(commitments, log_blowup_factor, n_bytes, log_cell, bundles, values, witness, witness_first):
    """frieda_reconstruct_blobs_from_stripe_bundles on the default context: (list of bytes, status [n_bundles, K], n_stripes_used)."""
    return default_context().reconstruct_blobs_from_stripe_bundles(commitments, log_blowup_factor, n_bytes, log_cell, bundles, values, witness, witness_first)


def encode_batch(blobs, log_blowup_factor):
    """frieda_encode_batch on the default context: one Encoded per blob, sharing one allocation."""
    return default_context().encode_batch(blobs, log_blowup_factor)


def rebuild_encoded_from_opened_cells(commitment, log_blowup_factor, n_bytes, log_cell, cell_index, values, paths, want_bytes=True):
    """frieda_rebuild_encoded_from_opened_cells on the default context: (bytes, status, n_cells_used, Encoded)."""
    return default_context().rebuild_encoded_from_opened_cells(commitment, log_blowup_factor, n_bytes, log_cell, cell_index, values, paths, want_bytes)


def rebuild_encoded_from_cell_bundles(commitment, log_blowup_factor, n_bytes, log_cell, bundles, values, witness, witness_first, want_bytes=True):
    """frieda_rebuild_encoded_from_cell_bundles on the default context: (bytes, status, n_cells_used, Encoded)."""
    return default_context().rebuild_encoded_from_cell_bundles(commitment, log_blowup_factor, n_bytes, log_cell, bundles, values, witness, witness_first, want_bytes)


def rebuild_encoded_blobs_from_opened_stripes(commitments, log_blowup_factor, n_bytes, log_cell, stripe_index, values, paths, want_bytes=True):
    """frieda_rebuild_encoded_blobs_from_opened_stripes on the default context: (list of bytes, status [S, K], n_stripes_used, list of Encoded)."""
    return default_context().rebuild_encoded_blobs_from_opened_stripes(commitments, log_blowup_factor, n_bytes, log_cell, stripe_index, values, paths, want_bytes)


def rebuild_encoded_blobs_from_stripe_bundles(commitments, log_blowup_factor, n_bytes, log_cell, bundles, values, witness, witness_first, want_bytes=True):
    """frieda_rebuild_encoded_blobs_from_stripe_bundles on the default context: (list of bytes, status [n_bundles, K], n_stripes_used, list of Encoded)."""
    return default_context().rebuild_encoded_blobs_from_stripe_bundles(commitments, log_blowup_factor, n_bytes, log_cell, bundles, values, witness, witness_first,
                                                                       want_bytes)
