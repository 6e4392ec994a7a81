#!/usr/bin/env python3
"""Deflate under libz's search-free strategies (Z_HUFFMAN_ONLY, Z_RLE) against levels 6 and 4 on the GPU: kernel-scope throughput,
per-stage milliseconds and compressed size on bench.py's text and random workloads (a standalone tool; bench.py is the project's
yardstick and does not run this).  Fails without a GPU.

    python tools/deflate_strategies_bench.py [--files 10000] [--file-bytes 262144] [--steps 3] [--out FILE]

Per workload (tests/workloads.py: build_equal_files, the chunks resident on the device as in bench.py) the modes -- level 6,
level 4, huffman, rle -- alternate in one process: every mode is warmed once, then two rounds over the four, each round timing
--steps synchronised zwz_deflate_batch_dev calls (both rounds are reported, so the spread is visible), then one profiled call per
mode for the stages' milliseconds (zwz_ctx_stage_ms; under a strategy the one kernel that stands in for search and parse reports
as lz_parse, and lz_links and lz_match are empty).  The compressed size is the sum of the chunks' payload lengths; a sample of
chunks per mode is compared with libz in that mode, byte for byte.  One JSON line on stdout (and in --out).
"""
import argparse
import importlib
import json
import os
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PKG = "parallel-data-compression-and-decompression_amd"
MODES = (("level6", 6, 0), ("level4", 4, 0), ("huffman", 6, 2), ("rle", 6, 3))      # name, level, libz's strategy number
CHUNK, STRIDE = 65535, 65536


def run_workload(args, torch, z, codec, dev, name):
    import workloads
    d_in, d_off, d_len, n, raw_bytes, _ = workloads.build_equal_files(torch, dev, name, args.files, args.file_bytes, 0)
    d_out = torch.empty(n * STRIDE, dtype=torch.uint8, device=dev)
    d_olen = torch.zeros(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()

    def deflate(mode, times=1):
        _, level, strategy = mode
        codec.set_level(level)
        codec.set_strategy(strategy)
        t0 = time.perf_counter()
        for _ in range(times):
            codec.deflate_dev(d_in, d_off, d_len, d_out, d_olen)
        codec.sync()
        return time.perf_counter() - t0

    def libz(raw, mode):
        c = zlib.compressobj(mode[1], zlib.DEFLATED, 15, 8, mode[2])
        return (c.compress(raw) + c.flush())[:CHUNK]

    res = {"chunks": n, "raw_bytes": raw_bytes, "modes": {}}
    sample = sorted({int(i) for i in torch.linspace(0, n - 1, args.sample).tolist()})
    lens = d_len.cpu().numpy()
    for mode in MODES:                                                     # warm-up, size and the check against libz
        deflate(mode)
        olen = d_olen.cpu().numpy()
        for i in sample:
            raw = d_in[i * STRIDE:i * STRIDE + int(lens[i])].cpu().numpy().tobytes()
            got = d_out[i * STRIDE:i * STRIDE + int(olen[i])].cpu().numpy().tobytes()
            if got != libz(raw, mode):
                raise SystemExit("%s: chunk %d in mode %s is not libz's stream" % (name, i, mode[0]))
        res["modes"][mode[0]] = {"compressed_bytes": int(olen.astype("int64").sum()), "ratio": round(float(olen.astype("int64").sum()) / raw_bytes, 5),
                                "GBps": [], "ms_per_call": []}
    for _ in range(2):                                                     # two timed rounds, the modes alternating
        for mode in MODES:
            dt = deflate(mode, args.steps)
            res["modes"][mode[0]]["GBps"].append(round(raw_bytes * args.steps / dt / 1e9, 3))
            res["modes"][mode[0]]["ms_per_call"].append(round(dt / args.steps * 1e3, 3))
    codec.set_profiling(True)
    for mode in MODES:                                                     # the stages, one profiled call each
        codec.stage_ms(reset=True)
        deflate(mode)
        st = codec.stage_ms(reset=True)
        res["modes"][mode[0]]["stage_ms"] = {k: round(v, 3) for k, v in st.items() if k != "inflate"}
    codec.set_profiling(False)
    codec.set_level(0)
    codec.set_strategy(0)
    del d_in, d_out
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=10000, help="files of --file-bytes each (bench.py's default: 10 000 x 256 KiB = 50 000 chunks)")
    ap.add_argument("--file-bytes", type=int, default=262144)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--sample", type=int, default=24, help="chunks per mode and workload compared with libz")
    ap.add_argument("--max-batch", type=int, default=51200)
    ap.add_argument("--workloads", default="text,random")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures the HIP kernels")
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    z = importlib.import_module(PKG)
    codec = z.Codec(0, max_batch_chunks=args.max_batch)
    line = {"tool": "deflate_strategies_bench", "device": torch.cuda.get_device_name(0), "steps": args.steps,
            "scope": "zwz_deflate_batch_dev on device-resident chunks, synchronised; GB/s of raw input", "workloads": {}}
    for name in args.workloads.split(","):
        line["workloads"][name] = run_workload(args, torch, z, codec, dev, name)
    codec.close()
    text = json.dumps(line)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
