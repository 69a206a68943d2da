"""Times all openings of one proof (every FRI layer: decommitment values + Merkle hash witness, plus the first layer's evaluations)
through Level B, three ways, on one GPU:
  loop   — what Level B offered before the batched calls: frieda_dev_at_secure per value, one 32-byte frieda_dev_download per hash
  sync   — one frieda_merkle_decommit per layer + one frieda_dev_gather for the evaluations
  async  — one upload of every layer's positions, frieda_merkle_decommit_device per layer + frieda_dev_gather_device, one download
The layers and trees are rebuilt with Level B calls from a Level A proof of the same blob (as tests/test_gpu_levelb_opening.py does),
and all three results are checked against that proof before any timing is reported.  Prints one JSON line.

    python tools/levelb_opening.py [--log-domain 24] [--queries 20] [--reps 30]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-domain", type=int, default=24)
    ap.add_argument("--queries", type=int, default=20)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--loop-reps", type=int, default=3)
    args = ap.parse_args()
    import torch  # noqa: F401  (loads the HIP runtime first, see frieda_amd/_lib.py)

    import frieda_amd
    from frieda_amd.api import _check
    from test_levelb_opening_symbols import stwo_decommit_walk
    from util import DevBuf, blob_len_for

    ctx = frieda_amd.Context(0)
    L_, h = ctx._L, ctx._h
    B, seed = 4, 7
    n_bytes = blob_len_for(args.log_domain, B)
    data = (np.arange(n_bytes, dtype=np.uint64) % 256).astype(np.uint8)
    root, proof = ctx.commit_and_generate_proof(data.tobytes(), seed, frieda_amd.PcsConfig(frieda_amd.FriConfig(B, 0, args.queries), 20))
    alphas = ctx.last_transcript()["alphas"]
    ok, q = frieda_amd.verify_samples(proof, seed)
    assert ok
    q = np.asarray(q, dtype=np.int64)
    n = args.log_domain
    nl = proof.n_inner_layers + 1

    # the layers and their trees, Level B calls only
    d_in = DevBuf.from_array(ctx, data)
    d_coef = DevBuf(ctx, 16 << (n - B))
    _check(L_.frieda_unpack30(h, d_in.ptr, n_bytes, d_coef.ptr, 4 << (n - B)), h)
    layers, trees, tree_ptrs = [DevBuf(ctx, 16 << n)], [], []
    _check(L_.frieda_circle_evaluate(h, d_coef.ptr, 4, n - B, n, layers[0].ptr), h)
    for li in range(nl):
        m = n - li
        t = DevBuf(ctx, 32 * ((2 << m) - 1))
        _check(L_.frieda_merkle_commit(h, layers[li].ptr, m, t.ptr), h)
        trees.append(t)
        tree_ptrs.append([t.ptr.value + L_.frieda_merkle_layer_offset(m, j) for j in range(m + 1)])
        nxt = DevBuf.from_array(ctx, np.zeros((4, 1 << (m - 1)), np.uint32))
        a = np.array(alphas[li], dtype=np.uint32)
        if li == 0:
            _check(L_.frieda_fold_circle_into_line(h, nxt.ptr, layers[0].ptr, n, a.ctypes.data), h)
        else:
            _check(L_.frieda_fold_line(h, layers[li].ptr, m, n, a.ctypes.data, nxt.ptr), h)
        layers.append(nxt)
    ctx.synchronize()
    dpos = []
    for li in range(nl):
        pairs = np.unique(q >> (li + 1))
        dpos.append(np.unique(np.concatenate([2 * pairs, 2 * pairs + 1])).astype(np.uint32))
    walks = [stwo_decommit_walk(dpos[li].tolist(), n - li) for li in range(nl)]
    expect_h = [b"".join(proof.layer(li)["hash_witness"]) for li in range(nl)]
    expect_ev = proof.evaluations

    # ---- loop: one synchronised copy per value / hash ----
    def run_loop():
        ev = np.zeros((q.size, 4), np.uint32)
        v4 = (C.c_uint32 * 4)()
        for i, x in enumerate(q.tolist()):
            _check(L_.frieda_dev_at_secure(h, layers[0].ptr, 1 << n, x, v4), h)
            ev[i] = list(v4)
        out_v, out_h = [], []
        hb = (C.c_uint8 * 32)()
        for li in range(nl):
            vals = np.zeros((dpos[li].size, 4), np.uint32)
            for i, x in enumerate(dpos[li].tolist()):
                _check(L_.frieda_dev_at_secure(h, layers[li].ptr, 1 << (n - li), x, v4), h)
                vals[i] = list(v4)
            hs = []
            for layer, node in walks[li]:
                _check(L_.frieda_dev_download(h, hb, C.c_void_p(tree_ptrs[li][layer] + 32 * node), 32), h)
                hs.append(bytes(hb))
            out_v.append(vals)
            out_h.append(b"".join(hs))
        return ev, out_v, out_h

    # ---- sync: one decommit per layer ----
    def run_sync():
        ev = ctx.dev_gather(layers[0].ptr, 1 << n, 4, q.astype(np.uint64))
        out_v, out_h = [], []
        for li in range(nl):
            v, hs = ctx.merkle_decommit(tree_ptrs[li], n - li, layers[li].ptr, 4, 1 << (n - li), dpos[li])
            out_v.append(v)
            out_h.append(hs)
        return ev, out_v, out_h

    # ---- async: everything queued, one download ----
    pos_all = np.concatenate(dpos + [np.zeros(0, np.uint32)])
    q64 = q.astype(np.uint64)
    pos_off = np.concatenate([[0], np.cumsum([p.size for p in dpos])]).astype(np.int64)
    h_bound = [dpos[li].size * (n - li) for li in range(nl)]
    # output image: [counts: nl words, padded to 256 B | evaluations | values of every layer | hashes of every layer (by bound)]
    cnt_b = 256
    ev_b = 16 * q.size
    val_off = cnt_b + ((ev_b + 255) & ~255)
    val_offs = [val_off + 16 * int(pos_off[li]) for li in range(nl)]
    hash_base = (val_off + 16 * int(pos_off[-1]) + 255) & ~255
    hash_offs = list(hash_base + 32 * np.concatenate([[0], np.cumsum(h_bound)[:-1]]).astype(np.int64))
    out_bytes = int(hash_base + 32 * sum(h_bound))
    in_img = np.concatenate([q64.view(np.uint32), pos_all])
    d_inimg = DevBuf(ctx, 4 * in_img.size)
    d_out = DevBuf(ctx, out_bytes)
    host_out = np.zeros(out_bytes, np.uint8)
    layer_tabs = [(C.c_void_p * (n - li + 1))(*tree_ptrs[li]) for li in range(nl)]
    base_in, base_out = d_inimg.ptr.value, d_out.ptr.value
    pos_dev = [base_in + 8 * q.size + 4 * int(pos_off[li]) for li in range(nl)]

    def run_async():
        _check(L_.frieda_dev_upload(h, d_inimg.ptr, in_img.ctypes.data, in_img.nbytes), h)
        _check(L_.frieda_dev_gather_device(h, layers[0].ptr, 1 << n, 4, C.c_void_p(base_in), q.size, C.c_void_p(base_out + cnt_b)), h)
        for li in range(nl):
            m = n - li
            _check(
                L_.frieda_merkle_decommit_device(h, layer_tabs[li], m, layers[li].ptr, 4, 1 << m, C.c_void_p(pos_dev[li]), dpos[li].size,
                                                 C.c_void_p(base_out + val_offs[li]), C.c_void_p(base_out + int(hash_offs[li])),
                                                 C.c_void_p(base_out + 4 * li)),
                h,
            )
        _check(L_.frieda_dev_download(h, host_out.ctypes.data, d_out.ptr, out_bytes), h)
        cnt = host_out[: 4 * nl].view(np.uint32)
        ev = host_out[cnt_b : cnt_b + ev_b].view(np.uint32).reshape(-1, 4)
        out_v = [host_out[val_offs[li] : val_offs[li] + 16 * dpos[li].size].view(np.uint32).reshape(-1, 4) for li in range(nl)]
        out_h = [host_out[int(hash_offs[li]) : int(hash_offs[li]) + 32 * int(cnt[li])].tobytes() for li in range(nl)]
        return ev, out_v, out_h

    def check(res, name):
        ev, vs, hs = res
        assert np.array_equal(ev, expect_ev), name
        for li in range(nl):
            assert hs[li] == expect_h[li], (name, li)
            exp_v = layers[li].to_array(np.uint32, (4, 1 << (n - li)))[:, dpos[li]].T if li < 2 else vs_ref[li]
            assert np.array_equal(vs[li], exp_v), (name, li)

    vs_ref = run_sync()[1]
    for fn, name in ((run_loop, "loop"), (run_sync, "sync"), (run_async, "async")):
        check(fn(), name)

    def timed(fn, reps):
        fn()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts)), float(np.min(ts))

    res = {"log_domain": n, "queries": int(args.queries), "unique_queries": int(q.size), "layers": nl,
           "positions": int(pos_all.size), "hashes": int(sum(len(x) for x in expect_h) // 32)}
    res["loop_ms"], res["loop_min_ms"] = timed(run_loop, args.loop_reps)
    res["sync_ms"], res["sync_min_ms"] = timed(run_sync, args.reps)
    res["async_ms"], res["async_min_ms"] = timed(run_async, args.reps)
    res["loop_over_async"] = res["loop_ms"] / res["async_ms"]
    # per-layer breakdown of the synchronous form
    per = []
    for li in range(nl):
        def one(li=li):
            ctx.merkle_decommit(tree_ptrs[li], n - li, layers[li].ptr, 4, 1 << (n - li), dpos[li])
        per.append(round(timed(one, args.reps)[0], 4))
    res["sync_per_layer_ms"] = per
    res["calls_loop"] = int(q.size + pos_all.size + res["hashes"])
    print(json.dumps(res))
    ctx.close()


if __name__ == "__main__":
    main()
