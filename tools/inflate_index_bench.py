#!/usr/bin/env python3
"""The seek index of ordinary streams on the GPU (a standalone tool; bench.py is the project's yardstick and does not run this).

    python tools/inflate_index_bench.py [--scale 1.0] [--steps 5] [--warmup 2] [--span 0] [--only batch] [--out FILE]

The workload is DESIGN.md section 17's S3: 64 x 16 MiB text, each one ordinary gzip stream from Python's zlib (nothing to split).
  floor     zwz_inflate_streams_dev on the batch: one wave a stream
  build     zwz_inflate_streams_index_dev on the batch: the same decode that also writes every stream's index
  indexed   zwz_inflate_indexed_dev, one call a stream, the indexes on the device
  indexed_batch   the same batch through ONE zwz_inflate_indexed_batch_dev call, the indexes on the device.  The gate: its time is at
            most a tenth of floor's, both measured in this run
  one       one stream of the batch alone: zwz_inflate_streams_dev against zwz_inflate_indexed_dev
  ranges    4 096 ranges of 4 KiB out of one stream through zwz_inflate_read_ranges_dev
  ranges_batch    4 096 ranges of 4 KiB spread over all streams in one zwz_inflate_read_ranges_batch_dev call, against the same ranges
            through one zwz_inflate_read_ranges_dev call a stream
--only batch runs floor, indexed_batch and ranges_batch alone (what a second span is measured with).
--scale multiplies the number of streams.  Every figure is decoded bytes over the wall time of synchronised calls, median of --steps
after --warmup, the variants alternating in one process, with the spread (max - min) / median; every output is compared with the
input on the device.  One JSON line on stdout (and in --out).
"""
import argparse
import concurrent.futures as cf
import importlib
import json
import os
import random
import statistics
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PKG = "parallel-data-compression-and-decompression_amd"
THREADS = 16


def alternate(variants, steps, warmup):
    ts = {k: [] for k in variants}
    for it in range(warmup + steps):
        for k, fn in variants.items():
            t0 = time.perf_counter()
            fn()
            dt = time.perf_counter() - t0
            if it >= warmup:
                ts[k].append(dt)
    return {k: (statistics.median(v), (max(v) - min(v)) / statistics.median(v)) for k, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--span", type=int, default=0)
    ap.add_argument("--only", default="", choices=["", "batch"])
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    torch.zeros(1, device="cuda")
    dev = torch.device("cuda", 0)
    z = importlib.import_module(PKG)
    import corpus
    codec = z.Codec(0)
    L = z.lib()
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    n, k = 16 << 20, max(1, int(64 * a.scale))
    span = a.span or (1 << 20)
    pool = np.frombuffer(corpus.text_like(7, 32 << 20), dtype=np.uint8)
    host = np.concatenate([np.roll(pool, 7919 * (r + 1)) for r in range((n * k + len(pool) - 1) // len(pool))])[:n * k]
    d_src = t(host)

    def one(i):
        c = zlib.compressobj(6, zlib.DEFLATED, 31)
        return c.compress(host[i * n:(i + 1) * n].tobytes()) + c.flush()
    with cf.ThreadPoolExecutor(THREADS) as ex:
        streams = list(ex.map(one, range(k)))
    c_len = np.array([len(s) for s in streams], dtype=np.int64)
    c_off = np.zeros(k, dtype=np.int64)
    c_off[1:] = np.cumsum((c_len[:-1] + 15) // 16 * 16)
    blob = np.zeros(int(c_off[-1] + c_len[-1] + 32), dtype=np.uint8)
    for i, s in enumerate(streams):
        blob[c_off[i]:c_off[i] + len(s)] = np.frombuffer(s, dtype=np.uint8)
    d_comp = t(blob)
    s_off = np.arange(k, dtype=np.int64) * n
    bound = int(L.zwz_inflate_index_bound(n, span))
    i_off = np.arange(k, dtype=np.int64) * bound
    d_coff, d_clen, d_ooff, d_cap, d_ioff, d_icap = t(c_off), t(c_len), t(s_off), t(np.full(k, n, dtype=np.int64)), t(i_off), t(np.full(k, bound, dtype=np.int64))
    d_out = torch.empty(n * k + 16, dtype=torch.uint8, device=dev)
    d_idx = torch.zeros(bound * k, dtype=torch.uint8, device=dev)
    d_olen = torch.zeros(k, dtype=torch.int64, device=dev)
    d_ilen = torch.zeros(k, dtype=torch.int64, device=dev)
    d_st = torch.zeros(k, dtype=torch.int32, device=dev)
    d_seg = torch.zeros(k, dtype=torch.int32, device=dev)

    def check(m=k):
        ok = bool((d_st[:m] == 0).all()) and bool((d_olen[:m] == n).all()) and torch.equal(d_out[:n * m], d_src[:n * m])
        d_out.zero_(); d_st.fill_(-1); d_olen.fill_(-1)
        return ok

    def floor(m=k):
        codec.inflate_streams_dev("gzip", d_comp, d_coff[:m], d_clen[:m], d_out, d_ooff[:m], d_cap[:m], d_olen[:m], d_st[:m])
        codec.sync()

    def build():
        codec.inflate_streams_index_dev("gzip", d_comp, d_coff, d_clen, d_out, d_ooff, d_cap, d_olen, d_st, d_idx, d_ioff, d_icap, d_ilen, span)
        codec.sync()

    build()
    ok = check()
    i_len = d_ilen.cpu().numpy()
    ok = ok and bool((i_len > 0).all())
    idx_host = [d_idx[i_off[i]:i_off[i] + i_len[i]].cpu().numpy().tobytes() for i in range(k)]
    segs = [int.from_bytes(x[32:36], "little") for x in idx_host]

    def indexed(m=k):
        for i in range(m):
            codec.inflate_indexed_dev(d_comp[c_off[i]:], int(c_len[i]), idx_host[i], d_out[s_off[i]:], n, d_olen[i:i + 1], d_st[i:i + 1], d_seg[i:i + 1],
                                      d_idx[i_off[i]:])
        codec.sync()

    pk = z.pack_indexes(idx_host, i_off)                     # (the host copy of d_idx's layout, made once)
    caps = np.full(k, n, dtype=np.uint64)

    def indexed_batch():
        codec.inflate_indexed_batch_dev(d_comp, c_off, c_len, pk, d_out, s_off, caps, d_olen, d_st, d_seg, d_idx)
        codec.sync()

    d_seg.fill_(-1)
    indexed_batch()
    ok = ok and check() and [int(x) for x in d_seg.cpu().numpy()] == segs
    d_seg.fill_(-1)
    indexed()
    ok = ok and check() and [int(x) for x in d_seg.cpu().numpy()] == segs
    res = {"tool": "inflate_index_bench", "scale": a.scale, "steps": a.steps, "warmup": a.warmup, "span": span, "streams": k, "decoded_bytes": n * k,
           "compressed_bytes": int(c_len.sum()), "segments_per_stream": [min(segs), max(segs)], "index_bytes": int(i_len.sum()),
           "index_share_of_decoded": round(float(i_len.sum()) / (n * k), 4)}
    variants = {"floor": floor, "indexed_batch": indexed_batch} if a.only else {"floor": floor, "build": build, "indexed": indexed, "indexed_batch": indexed_batch}
    times = alternate(variants, a.steps, a.warmup)
    for name, (med, spread) in times.items():
        res[name + "_wall_ms"], res[name + "_gbps"], res[name + "_spread"] = round(med * 1e3, 3), round(n * k / med / 1e9, 3), round(spread, 3)
    indexed_batch()
    ok = ok and check()
    res["indexed_batch_over_floor"] = round(res["floor_wall_ms"] / res["indexed_batch_wall_ms"], 2)
    res["gate_10x_floor"] = res["indexed_batch_wall_ms"] * 10.0 <= res["floor_wall_ms"]
    # 4 096 ranges of 4 KiB over all streams: one batched call against one call a stream
    rng = random.Random(6)
    trip = z._ranges(np, [(rng.randrange(k), rng.randrange(n - 4096), 4096) for _ in range(4096)], 3)
    d_rng = torch.zeros(4096 * 4096, dtype=torch.uint8, device=dev)
    d_one = torch.zeros(4096 * 4096, dtype=torch.uint8, device=dev)
    per = [np.flatnonzero(trip[:, 0] == i) for i in range(k)]
    starts = np.concatenate([[0], np.cumsum([4096 * len(p) for p in per])]).astype(np.int64)

    def ranges_batch():
        codec.read_ranges_batch_dev(d_comp, c_off, c_len, pk, trip, d_rng, d_idx)

    def ranges_each():
        for i in range(k):
            if len(per[i]):
                codec.read_ranges_dev(d_comp[c_off[i]:], int(c_len[i]), idx_host[i], np.ascontiguousarray(trip[per[i], 1:]), d_one[starts[i]:], d_idx[i_off[i]:])

    times = alternate({"ranges_batch": ranges_batch, "ranges_each": ranges_each}, a.steps, a.warmup)
    want = torch.cat([d_src[int(s) * n + int(o):int(s) * n + int(o) + 4096] for s, o, _ in trip])
    ok = ok and torch.equal(d_rng, want)
    order = np.concatenate(per)
    ok = ok and torch.equal(d_one.view(-1, 4096), want.view(-1, 4096)[torch.from_numpy(order).to(dev)])
    for name, (med, spread) in times.items():
        res[name + "_wall_ms"], res[name + "_per_s"], res[name + "_spread"] = round(med * 1e3, 3), round(4096 / med), round(spread, 3)
    res["ranges_batch_over_each"] = round(res["ranges_each_wall_ms"] / res["ranges_batch_wall_ms"], 2)
    if not a.only:
        res["indexed_over_floor"] = round(res["indexed_gbps"] / res["floor_gbps"], 2)
        res["build_over_floor_time"] = round(res["build_wall_ms"] / res["floor_wall_ms"], 3)
        # one stream alone
        times = alternate({"one_floor": lambda: floor(1), "one_indexed": lambda: indexed(1)}, a.steps, a.warmup)
        for name, (med, spread) in times.items():
            res[name + "_wall_ms"], res[name + "_gbps"], res[name + "_spread"] = round(med * 1e3, 3), round(n / med / 1e9, 3), round(spread, 3)
        indexed(1)
        ok = ok and check(1)
        res["one_indexed_over_floor"] = round(res["one_indexed_gbps"] / res["one_floor_gbps"], 2)
        # 4 096 ranges of 4 KiB out of stream 0
        rng = random.Random(5)
        ranges = z._ranges(np, [(rng.randrange(n - 4096), 4096) for _ in range(4096)])
        d_rng = torch.zeros(4096 * 4096, dtype=torch.uint8, device=dev)

        def read():
            codec.read_ranges_dev(d_comp, int(c_len[0]), idx_host[0], ranges, d_rng, d_idx)
        med, spread = alternate({"ranges": read}, a.steps, a.warmup)["ranges"]
        want = torch.cat([d_src[int(o):int(o) + 4096] for o in ranges[:, 0]])
        ok = ok and torch.equal(d_rng, want)
        res["ranges_wall_ms"], res["ranges_per_s"], res["ranges_spread"] = round(med * 1e3, 3), round(4096 / med), round(spread, 3)
    codec.close()
    res["ok"] = bool(ok)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
