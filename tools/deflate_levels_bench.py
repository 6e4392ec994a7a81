#!/usr/bin/env python3
"""Deflate at compression levels 4, 5 and 6 on the GPU: kernel-scope throughput, per-stage milliseconds and compressed size on
bench.py's text and random workloads (a standalone tool; bench.py is the project's yardstick and does not run this).  Fails
without a GPU.

    python tools/deflate_levels_bench.py [--files 10000] [--file-bytes 262144] [--steps 3] [--match auto] [--out FILE]

Per workload (tests/workloads.py: build_equal_files, the chunks resident on the device as in bench.py) the levels alternate in
one process: every level is warmed once, then two rounds of 4, 5, 6, each round timing --steps synchronised zwz_deflate_batch_dev
calls (both rounds are reported, so the spread is visible), then one profiled call per level for the stages' milliseconds
(zwz_ctx_stage_ms).  The compressed size is the sum of the chunks' payload lengths; a sample of chunks per level is compared
with libz at that level, byte for byte.  One JSON line on stdout (and in --out).
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
LEVELS = (4, 5, 6)
CHUNK, STRIDE = 65535, 65536


def run_workload(args, torch, z, codec, dev, name):
    import workloads
    d_in, d_off, d_len, n, raw_bytes, _ = workloads.build_equal_files(torch, dev, name, args.files, args.file_bytes, 0)
    d_out = torch.empty(n * STRIDE, dtype=torch.uint8, device=dev)
    d_olen = torch.zeros(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()

    def deflate(level, times=1):
        codec.set_level(level)
        t0 = time.perf_counter()
        for _ in range(times):
            codec.deflate_dev(d_in, d_off, d_len, d_out, d_olen)
        codec.sync()
        return time.perf_counter() - t0

    res = {"chunks": n, "raw_bytes": raw_bytes, "levels": {}}
    sample = sorted({int(i) for i in torch.linspace(0, n - 1, args.sample).tolist()})
    lens = d_len.cpu().numpy()
    for level in LEVELS:                                                   # warm-up, size and the check against libz
        deflate(level)
        olen = d_olen.cpu().numpy()
        for i in sample:
            raw = d_in[i * STRIDE:i * STRIDE + int(lens[i])].cpu().numpy().tobytes()
            got = d_out[i * STRIDE:i * STRIDE + int(olen[i])].cpu().numpy().tobytes()
            if got != zlib.compress(raw, level)[:CHUNK]:
                raise SystemExit("%s: chunk %d at level %d is not libz's stream" % (name, i, level))
        res["levels"][level] = {"compressed_bytes": int(olen.astype("int64").sum()), "ratio": round(float(olen.astype("int64").sum()) / raw_bytes, 5),
                                "GBps": [], "ms_per_call": []}
    for _ in range(2):                                                     # two timed rounds, the levels alternating
        for level in LEVELS:
            dt = deflate(level, args.steps)
            res["levels"][level]["GBps"].append(round(raw_bytes * args.steps / dt / 1e9, 3))
            res["levels"][level]["ms_per_call"].append(round(dt / args.steps * 1e3, 3))
    codec.set_profiling(True)
    for level in LEVELS:                                                   # the stages, one profiled call each
        codec.stage_ms(reset=True)
        deflate(level)
        st = codec.stage_ms(reset=True)
        res["levels"][level]["stage_ms"] = {k: round(v, 3) for k, v in st.items() if k != "inflate"}
    codec.set_profiling(False)
    codec.set_level(0)
    del d_in, d_out
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=10000, help="files of --file-bytes each (bench.py's default: 10 000 x 256 KiB = 50 000 chunks)")
    ap.add_argument("--file-bytes", type=int, default=262144)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--sample", type=int, default=24, help="chunks per level and workload compared with libz")
    ap.add_argument("--match", default="auto", help="the context's match option (auto | walk | band | lazy | autoband | autolazy)")
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
    codec.set_option("match", args.match)
    line = {"tool": "deflate_levels_bench", "device": torch.cuda.get_device_name(0), "match": args.match, "steps": args.steps,
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
