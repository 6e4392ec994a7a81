#!/usr/bin/env python3
"""Batched deflate into raw / zlib / gzip streams on the GPU against the bare codec and BGZF on the same bytes (a standalone tool;
bench.py is the project's yardstick and does not run this).  Fails without a GPU.

    python tools/deflate_streams_bench.py [--scale 1.0] [--steps 5] [--warmup 2] [--only w1,w2,w3,w4] [--out FILE]
    python tools/deflate_streams_bench.py --trace-summary DIR     (condenses a rocprofv3 --kernel-trace run of this tool; no GPU)

  W1   16 384 x 256 KiB text, gzip
  W2a  one 1 GiB text stream, gzip          W2b  64 x 16 MiB text, gzip
  W3   100 000 zlib streams of text, log-normal sizes with a 32 KiB median, at most 4 MiB
  W4   256 MiB of random bytes as one raw stream
--scale multiplies stream counts (W1, W2b, W3) and sizes (W2a, W4).  The text is workloads.text_rows_device (corpus.text_like's
language, made on the device); streams are windows of one buffer.  Per workload the variants alternate in one process -- streams
(zwz_deflate_streams_dev), dep (zwz_deflate_dep_streams_dev: the same call on dependent pieces, into buffers of its own), bare
(zwz_deflate_batch_dev on the same 65 280-byte pieces) and, where the input is one buffer, bgzf (zwz_bgzf_compress_dev) -- each a
synchronised call, --warmup rounds untimed, then --steps rounds: the median per variant, and its
spread (max - min) / median over the same rounds.  Every status must be 0; on a sample of at most 256 MiB per workload the output of
streams and of dep must be what Python's zlib inflates back to the input, the same sample gives the zlib rate on 16 threads (level 6, one window per stream)
and the size against that one-window stream.  One JSON line on stdout (and in --out).
"""
import argparse
import collections
import concurrent.futures as cf
import csv
import glob
import importlib
import json
import os
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
PIECE, STRIDE = 65280, 65536
SAMPLE = 256 << 20
WBITS = {"raw": -15, "zlib": 15, "gzip": 31}


def trace_summary(root):
    """Per-kernel totals of the codec's kernels from a rocprofv3 --kernel-trace --stats run of this tool (its *kernel_stats.csv, or
    the *kernel_trace.csv), and the share of the kernels that only the stream path runs."""
    rows = {}                                          # name -> [calls, total us, max us]
    clean = lambda n: n.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0].replace("zwz::", "")
    stats = glob.glob(os.path.join(root, "**", "*kernel_stats.csv"), recursive=True)
    if stats:
        for f in stats:
            for r in csv.DictReader(open(f)):
                if "zwz::" in r["Name"]:
                    e = rows.setdefault(clean(r["Name"]), [0, 0.0, 0.0])
                    e[0] += int(r["Calls"]); e[1] += int(r["TotalDurationNs"]) / 1e3; e[2] = max(e[2], int(r["MaxNs"]) / 1e3)
    else:
        for f in glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True):
            for r in csv.DictReader(open(f)):
                if "zwz::" in r["Kernel_Name"]:
                    d = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
                    e = rows.setdefault(clean(r["Kernel_Name"]), [0, 0.0, 0.0])
                    e[0] += 1; e[1] += d; e[2] = max(e[2], d)
    if not rows:
        print("no kernel statistics under %s" % root)
        return 1
    total = sum(e[1] for e in rows.values())
    print("%-44s %7s %13s %11s %11s %8s" % ("kernel", "calls", "total us", "mean us", "max us", "share"))
    for k, e in sorted(rows.items(), key=lambda kv: -kv[1][1]):
        print("%-44s %7d %13.1f %11.1f %11.1f %7.3f%%" % (k[:44], e[0], e[1], e[1] / e[0], e[2], 100 * e[1] / total))
    is_extra = lambda k: k.startswith("dstream_") or k.startswith("crc32_blocks") or k.startswith("bgzf_scan")
    extra = sum(e[1] for k, e in rows.items() if is_extra(k))
    mine = sum(e[1] for k, e in rows.items() if k.startswith("dstream_"))
    # the streams and the bare variant alternate, one call each a round: half of the codec's own kernel time belongs to each
    codec_half = (total - extra) / 2
    print("\nkernels only the stream path runs (dstream_*, crc32_blocks, bgzf_scan): %.1f us, %.2f %% of a streams call's GPU time"
          % (extra, 100 * extra / (extra + codec_half)))
    print("of which splice, scan and combine (dstream_*, bgzf_scan): %.1f us, %.2f %%; crc32_blocks: %.2f %%"
          % (mine + sum(e[1] for k, e in rows.items() if k.startswith("bgzf_scan")),
             100 * (mine + sum(e[1] for k, e in rows.items() if k.startswith("bgzf_scan"))) / (extra + codec_half),
             100 * sum(e[1] for k, e in rows.items() if k.startswith("crc32_blocks")) / (extra + codec_half)))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="w1,w2,w3,w4")
    ap.add_argument("--out", default="")
    ap.add_argument("--trace-summary", default="")
    a = ap.parse_args()
    if a.trace_summary:
        return trace_summary(a.trace_summary)
    only = set(a.only.split(","))
    import torch
    if not torch.cuda.is_available():
        print("deflate_streams_bench: no GPU", file=sys.stderr)
        return 2
    torch.zeros(1, device="cuda")          # torch's HIP runtime opens the GPU before the codec's library does
    import workloads
    z = importlib.import_module(PKG)
    L = z.lib()
    dev = torch.device("cuda", 0)
    codec = z.Codec(0)
    rng = np.random.default_rng(2026)
    res = {"tool": "deflate_streams_bench", "scale": a.scale, "steps": a.steps, "warmup": a.warmup, "cpu_threads": THREADS}

    def text_buffer(nbytes):
        rows = (nbytes + (4 << 20) - 1) // (4 << 20)
        flat = torch.zeros(rows * (4 << 20) + 16, dtype=torch.uint8, device=dev)
        for r0 in range(0, rows, 64):
            r1 = min(rows, r0 + 64)
            t = workloads.text_rows_device(torch, list(range(workloads.TEXT_SEED0 + r0, workloads.TEXT_SEED0 + r1)), 4 << 20, dev)
            flat[r0 * (4 << 20):r1 * (4 << 20)] = t.reshape(-1)
            del t
        return flat

    def random_buffer(nbytes):
        rows = (nbytes + (4 << 20) - 1) // (4 << 20)
        seeds = torch.tensor(list(range(workloads.RANDOM_SEED0, workloads.RANDOM_SEED0 + rows)), dtype=torch.int64)
        flat = torch.zeros(rows * (4 << 20) + 16, dtype=torch.uint8, device=dev)
        flat[:rows * (4 << 20)] = workloads.random_files_device(torch, seeds, 4 << 20, dev).reshape(-1)
        return flat

    def workload(name, wrap, d_in, offs, lens, one_buffer):
        """offs / lens: numpy int64 windows of d_in, offsets multiples of 16."""
        n = len(lens)
        total = int(lens.sum())
        caps = np.array([z.deflate_stream_bound(int(k), wrap) for k in lens], dtype=np.int64)
        ooff = np.zeros(n, dtype=np.int64)
        ooff[1:] = np.cumsum((caps[:-1] + 15) // 16 * 16)
        d_out = torch.empty(int(ooff[-1] + caps[-1] + 16), dtype=torch.uint8, device=dev)
        d_olen = torch.zeros(n, dtype=torch.int64, device=dev)
        d_st = torch.zeros(n, dtype=torch.int32, device=dev)
        # the same pieces for the bare codec
        npieces = (lens + PIECE - 1) // PIECE
        first = np.concatenate([[0], np.cumsum(npieces)])
        nb = int(first[-1])
        owner = np.repeat(np.arange(n), npieces)
        k = np.arange(nb) - first[owner]
        p_off = offs[owner] + k * PIECE
        p_len = np.minimum(lens[owner] - k * PIECE, PIECE).astype(np.int32)
        d_poff, d_plen = torch.from_numpy(p_off).to(dev), torch.from_numpy(p_len).to(dev)
        d_slots = torch.empty(nb * STRIDE, dtype=torch.uint8, device=dev)
        d_polen = torch.zeros(nb, dtype=torch.int32, device=dev)
        variants = collections.OrderedDict()

        def streams():
            codec.deflate_streams_dev(wrap, d_in, offs, lens, d_out, ooff, caps, d_olen, d_st)
        variants["streams"] = streams
        # the same call shape on dependent pieces
        dcaps = np.array([z.deflate_dep_stream_bound(int(k), wrap) for k in lens], dtype=np.int64)
        doff = np.zeros(n, dtype=np.int64)
        doff[1:] = np.cumsum((dcaps[:-1] + 15) // 16 * 16)
        d_dout = torch.empty(int(doff[-1] + dcaps[-1] + 16), dtype=torch.uint8, device=dev)
        d_dlen = torch.zeros(n, dtype=torch.int64, device=dev)
        d_dst = torch.zeros(n, dtype=torch.int32, device=dev)

        def dep():
            codec.deflate_dep_streams_dev(wrap, d_in, offs, lens, d_dout, doff, dcaps, d_dlen, d_dst)
        variants["dep"] = dep

        def bare():
            z._check(L.zwz_deflate_batch_dev(codec.handle, d_in.data_ptr(), d_poff.data_ptr(), d_plen.data_ptr(), nb, d_slots.data_ptr(), STRIDE,
                                             d_polen.data_ptr()), "deflate_batch_dev")
        variants["bare"] = bare
        if one_buffer:
            gcap = L.zwz_bgzf_bound(total)
            d_gz = torch.empty(gcap, dtype=torch.uint8, device=dev)
            d_gzlen = torch.zeros(1, dtype=torch.int64, device=dev)

            def bgzf():
                z._check(L.zwz_bgzf_compress_dev(codec.handle, d_in.data_ptr() + int(offs[0]), total, d_gz.data_ptr(), gcap, d_gzlen.data_ptr()),
                         "bgzf_compress_dev")
            variants["bgzf"] = bgzf
        torch.cuda.synchronize()
        times = {v: [] for v in variants}
        for step in range(a.warmup + a.steps):
            for v, fn in variants.items():
                t0 = time.perf_counter()
                fn()
                codec.sync()
                if step >= a.warmup:
                    times[v].append(time.perf_counter() - t0)
        r = {"wrap": wrap, "streams": n, "pieces": nb, "bytes": total}
        med = {v: statistics.median(t) for v, t in times.items()}
        for v, t in times.items():
            r[v + "_ms"] = round(med[v] * 1e3, 3)
            r[v + "_GBps"] = round(total / med[v] / 1e9, 2)
            r[v + "_spread"] = round((max(t) - min(t)) / med[v], 4)
        r["streams_over_bare"] = round(med["bare"] / med["streams"], 3)
        if one_buffer:
            r["bgzf_over_bare"] = round(med["bare"] / med["bgzf"], 3)
            r["streams_over_bgzf"] = round(med["bgzf"] / med["streams"], 3)
        st, olen = d_st.cpu().numpy(), d_olen.cpu().numpy()
        r["out_bytes"] = int(olen.sum())
        ok = bool((st == 0).all()) and bool((olen <= caps).all())
        dst, dlen = d_dst.cpu().numpy(), d_dlen.cpu().numpy()
        r["dep_out_bytes"] = int(dlen.sum())
        ok = ok and bool((dst == 0).all()) and bool((dlen <= dcaps).all())
        # sample: the first streams up to SAMPLE input bytes (at least one; a longer single stream is cut to its first SAMPLE bytes' pieces)
        m = max(1, int(np.searchsorted(np.cumsum(lens), SAMPLE, side="right")))
        hin = d_in[int(offs[:m].min()):int((offs[:m] + lens[:m]).max())].cpu().numpy()
        base = int(offs[:m].min())
        hout = [d_out[int(ooff[i]):int(ooff[i] + olen[i])].cpu().numpy().tobytes() for i in range(m)]
        hdep = [d_dout[int(doff[i]):int(doff[i] + dlen[i])].cpu().numpy().tobytes() for i in range(m)]
        srcs = [hin[int(offs[i]) - base:int(offs[i]) - base + int(lens[i])].tobytes() for i in range(m)]
        if m == 1 and len(srcs[0]) > SAMPLE:              # one long stream: libz on its first SAMPLE bytes only
            srcs_cpu = [srcs[0][:SAMPLE]]
        else:
            srcs_cpu = srcs

        def one(b):
            c = zlib.compressobj(6, zlib.DEFLATED, WBITS[wrap])
            return len(c.compress(b) + c.flush())
        with cf.ThreadPoolExecutor(THREADS) as ex:
            t0 = time.perf_counter()
            one_window = sum(ex.map(one, srcs_cpu, chunksize=max(1, len(srcs_cpu) // (4 * THREADS))))
            dt = time.perf_counter() - t0
            back = list(ex.map(lambda s: zlib.decompress(s, WBITS[wrap]), hout, chunksize=max(1, m // (4 * THREADS))))
            dback = list(ex.map(lambda s: zlib.decompress(s, WBITS[wrap]), hdep, chunksize=max(1, m // (4 * THREADS))))
        ok = ok and back == srcs and dback == srcs
        cpu_bytes = sum(len(s) for s in srcs_cpu)
        r["cpu16_GBps"] = round(cpu_bytes / dt / 1e9, 3)
        r["streams_over_cpu16"] = round(r["streams_GBps"] / r["cpu16_GBps"], 1)
        r["sample_streams"], r["sample_bytes"] = m, cpu_bytes
        if srcs_cpu is srcs:
            r["size_over_one_window"] = round(sum(len(h) for h in hout) / one_window, 4)
        else:
            r["size_over_one_window"] = round((r["out_bytes"] / total) / (one_window / cpu_bytes), 4)
        r["ok"] = ok
        res[name] = r
        print(name, r, file=sys.stderr, flush=True)
        torch.cuda.empty_cache()

    text = None
    if only & {"w1", "w2", "w3"}:
        text = text_buffer(max(int((4 << 30) * min(a.scale, 1.0)), 64 << 20))
    tbytes = (text.numel() - 16) if text is not None else 0
    if "w1" in only:
        n1 = max(1, min(int(16384 * a.scale), tbytes // (256 << 10)))
        workload("W1", "gzip", text, np.arange(n1, dtype=np.int64) * (256 << 10), np.full(n1, 256 << 10, dtype=np.int64), False)
    if "w2" in only:
        n2 = min(int((1 << 30) * a.scale), tbytes)
        workload("W2a", "gzip", text, np.zeros(1, dtype=np.int64), np.array([n2], dtype=np.int64), True)
        k2 = max(1, min(int(64 * a.scale), tbytes // (16 << 20)))
        workload("W2b", "gzip", text, np.arange(k2, dtype=np.int64) * (16 << 20), np.full(k2, 16 << 20, dtype=np.int64), False)
    if "w3" in only:
        n3 = max(1, int(100000 * a.scale))
        sizes = np.minimum(np.exp(rng.normal(np.log(32 << 10), 0.8, size=n3)).astype(np.int64) + 1, 4 << 20)
        starts = rng.integers(0, (tbytes - (4 << 20)) // 16, size=n3).astype(np.int64) * 16
        workload("W3", "zlib", text, starts, sizes, False)
    del text
    torch.cuda.empty_cache()
    if "w4" in only:
        n4 = max(int((256 << 20) * a.scale), 4 << 20)
        workload("W4", "raw", random_buffer(n4), np.zeros(1, dtype=np.int64), np.array([n4], dtype=np.int64), True)
    codec.close()
    res["ok"] = all(v["ok"] for k, v in res.items() if k.startswith("W"))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if res["ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
