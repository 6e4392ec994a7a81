#!/usr/bin/env python3
"""BGZF against the bare codec on the same bytes (a standalone tool; bench.py is the project's yardstick and does not run this).

    python tools/bgzf_bench.py [--mib 256] [--steps 5] [--warmup 2] [--workload text|random|both]

For each workload: zwz_bgzf_compress_dev over n contiguous bytes against zwz_deflate_batch_dev over the same bytes cut into the
same 65 280-byte blocks, and zwz_bgzf_decompress_dev over the BGZF stream against zwz_inflate_batch_dev over the bare payloads.
Rates are raw bytes / wall time of a call synchronised on the context's stream (median of --steps).  The BGZF output is checked:
Python's gzip reads it back to the input, and the device decompression returns the input.  One JSON line on stdout.
"""
import argparse
import ctypes
import gzip
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

BLOCK, STRIDE = 65280, 65536


def make_data(torch, dev, workload, nbytes):
    import workloads
    rows = max(1, nbytes // (4 << 20))
    seeds = list(range(workloads.TEXT_SEED0 if workload == "text" else workloads.RANDOM_SEED0,
                       (workloads.TEXT_SEED0 if workload == "text" else workloads.RANDOM_SEED0) + rows))
    if workload == "text":
        t = workloads.text_rows_device(torch, seeds, 4 << 20, dev)
    else:
        t = workloads.random_files_device(torch, torch.tensor(seeds, dtype=torch.int64), 4 << 20, dev)
    flat = torch.zeros(rows * (4 << 20) + 16, dtype=torch.uint8, device=dev)
    flat[:rows * (4 << 20)] = t.reshape(-1)
    return flat, rows * (4 << 20)


def timed(fn, sync, steps, warmup):
    for _ in range(warmup):
        fn()
    sync()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def run(z, torch, codec, workload, nbytes, steps, warmup):
    L = z.lib()
    dev = torch.device("cuda", 0)
    d_in, n = make_data(torch, dev, workload, nbytes)
    nb = (n + BLOCK - 1) // BLOCK
    cap = L.zwz_bgzf_bound(n)
    d_gz = torch.empty(cap, dtype=torch.uint8, device=dev)
    d_gzlen = torch.zeros(1, dtype=torch.int64, device=dev)
    # the bare codec's view of the same bytes: block i at i * 65280, results in 65 536-byte slots
    d_off = torch.arange(nb, dtype=torch.int64, device=dev) * BLOCK
    d_len = torch.clamp(n - d_off, max=BLOCK).to(torch.int32)
    d_slots = torch.empty(nb * STRIDE, dtype=torch.uint8, device=dev)
    d_olen = torch.zeros(nb, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()

    def bgzf_c():
        z._check(L.zwz_bgzf_compress_dev(codec.handle, d_in.data_ptr(), n, d_gz.data_ptr(), cap, d_gzlen.data_ptr()), "bgzf_compress_dev")

    def bare_c():
        z._check(L.zwz_deflate_batch_dev(codec.handle, d_in.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), nb, d_slots.data_ptr(), STRIDE,
                                         d_olen.data_ptr()), "deflate_batch_dev")

    t_bc = timed(bgzf_c, codec.sync, steps, warmup)
    t_dc = timed(bare_c, codec.sync, steps, warmup)
    gz_len = int(d_gzlen.item())
    gz = d_gz[:gz_len].cpu().numpy().tobytes()
    host = d_in[:n].cpu().numpy().tobytes()
    verified = gzip.decompress(gz) == host
    # decompression: BGZF members vs the bare payloads (each a zlib stream in its slot)
    offs, raw = z.bgzf_index(gz)
    d_moff = torch.tensor(offs, dtype=torch.int64, device=dev)
    d_gzin = torch.zeros(gz_len + 16, dtype=torch.uint8, device=dev)
    d_gzin[:gz_len] = d_gz[:gz_len]
    d_back = torch.empty(raw + 16, dtype=torch.uint8, device=dev)
    d_blen = torch.zeros(1, dtype=torch.int64, device=dev)
    d_st = torch.zeros(len(offs), dtype=torch.int32, device=dev)
    p_off = torch.arange(nb, dtype=torch.int64, device=dev) * STRIDE
    d_iback = torch.empty(nb * STRIDE, dtype=torch.uint8, device=dev)
    d_ilen = torch.zeros(nb, dtype=torch.int32, device=dev)
    d_ist = torch.zeros(nb, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()

    def bgzf_d():
        z._check(L.zwz_bgzf_decompress_dev(codec.handle, d_gzin.data_ptr(), gz_len, d_moff.data_ptr(), len(offs), d_back.data_ptr(),
                                           d_blen.data_ptr(), d_st.data_ptr()), "bgzf_decompress_dev")

    def bare_d():
        z._check(L.zwz_inflate_batch_dev(codec.handle, d_slots.data_ptr(), p_off.data_ptr(), d_olen.data_ptr(), nb, d_iback.data_ptr(), STRIDE,
                                         d_ilen.data_ptr(), d_ist.data_ptr()), "inflate_batch_dev")

    t_bd = timed(bgzf_d, codec.sync, steps, warmup)
    t_dd = timed(bare_d, codec.sync, steps, warmup)
    verified = verified and int(d_blen.item()) == n and int(d_st.abs().sum().item()) == 0 and torch.equal(d_back[:n], d_in[:n])
    gbps = lambda t: round(n / t / 1e9, 2)
    return {"workload": workload, "bytes": n, "members": nb, "gz_bytes": gz_len, "ratio": round(gz_len / n, 4),
            "bgzf_compress_GBps": gbps(t_bc), "deflate_GBps": gbps(t_dc), "compress_vs_bare": round(t_dc / t_bc, 3),
            "bgzf_decompress_GBps": gbps(t_bd), "inflate_GBps": gbps(t_dd), "decompress_vs_bare": round(t_dd / t_bd, 3),
            "verified": bool(verified)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workload", default="both", choices=["text", "random", "both"])
    a = ap.parse_args()
    import torch
    torch.zeros(1, device="cuda")          # torch's HIP runtime opens the GPU before the codec's library does
    z = importlib.import_module("parallel-data-compression-and-decompression_amd")
    codec = z.Codec(0)
    res = [run(z, torch, codec, w, a.mib << 20, a.steps, a.warmup) for w in (["text", "random"] if a.workload == "both" else [a.workload])]
    codec.close()
    print(json.dumps({"tool": "bgzf_bench", "results": res, "verified": all(r["verified"] for r in res)}))
    return 0 if all(r["verified"] for r in res) else 1


if __name__ == "__main__":
    sys.exit(main())
