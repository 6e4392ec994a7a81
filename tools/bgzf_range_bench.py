#!/usr/bin/env python3
"""BGZF random access on the GPU (a standalone tool; bench.py is the project's yardstick and does not run this).

    python tools/bgzf_range_bench.py [--mib 1024] [--steps 5] [--warmup 2] [--only w1,w2,w3,w4] [--w4-copies 4] [--out FILE]

A `text` BGZF stream of --mib MiB is made and held on the device (zwz_bgzf_compress_dev), then:
  W1  one range covering the whole stream (zwz_bgzf_read_ranges_dev) against zwz_bgzf_decompress_dev on the same stream, the two
      alternated in one process;
  W2  4 096 seeded ranges of 4 KiB: touched members, touched decoded bytes and their rate;
  W3  1 000 000 seeded ranges of 100 B: ranges/s;
  W4  the stream written --w4-copies times into one file (concatenated BGZF), its .gzi by zwz_bgzf_gzi_file, and one 1 MiB range in the
      middle by zwz_bgzf_read_ranges_file with the .gzi: wall time and the bytes the process read (/proc/self/io rchar, less the
      tool's own read of that file), against
      `main bgunzip` of the whole file.
Times are wall clock around calls that return after the GPU work (median of --steps, after --warmup).  Every output is compared with
the Python slice of the input.  One JSON line on stdout (and in --out).
"""
import argparse
import ctypes
import importlib
import json
import os
import random
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
BLOCK = 65280


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def rchar():
    with open("/proc/self/io") as f:
        for line in f:
            if line.startswith("rchar:"):
                return int(line.split()[1])
    return -1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="w1,w2,w3,w4")
    ap.add_argument("--w4-copies", type=int, default=4)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    only = set(a.only.split(","))
    import numpy as np
    import torch
    import bgzf_bench
    z = importlib.import_module("parallel-data-compression-and-decompression_amd")
    L = z.lib()
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    codec = z.Codec(0)
    d_in, n = bgzf_bench.make_data(torch, dev, "text", a.mib << 20)
    d_in = d_in[:n]
    d_gz = codec.bgzf_compress(d_in)
    gz_len = d_gz.numel()
    gz = d_gz.cpu().numpy().tobytes()
    data = d_in.cpu().numpy().tobytes()
    gzi = z.bgzf_gzi(gz)
    offs, raw = z.bgzf_index(gz)
    assert raw == n
    d_gz = z._device_input(torch, d_gz, 0)
    res = {"metric": "bgzf_range_reads", "stream_bytes": n, "gz_bytes": gz_len, "members": len(offs), "steps": a.steps, "warmup": a.warmup}

    def read_dev(ranges, d_out):
        rng = np.ascontiguousarray(np.array(ranges, dtype=np.uint64).reshape(-1, 2))
        return lambda: z._check(L.zwz_bgzf_read_ranges_dev(codec.handle, d_gz.data_ptr(), gz_len, gzi, len(gzi), rng.ctypes.data, len(rng),
                                                           d_out.data_ptr()), "zwz_bgzf_read_ranges_dev")

    def touched(ranges):
        ms = set()
        for o, k in ranges:
            if k:
                ms.update(range(o // BLOCK, (o + k - 1) // BLOCK + 1))
        return len(ms), sum(min(BLOCK, n - m * BLOCK) for m in ms)

    if "w1" in only:
        d_out = torch.empty(n, dtype=torch.uint8, device=dev)
        f = read_dev([(0, n)], d_out)
        d_moff = torch.tensor(np.array(offs, dtype=np.uint64).view(np.int64), device=dev)
        d_dec = torch.empty(n, dtype=torch.uint8, device=dev)
        d_len = torch.zeros(1, dtype=torch.int64, device=dev)
        d_st = torch.zeros(len(offs), dtype=torch.int32, device=dev)

        def g():
            z._check(L.zwz_bgzf_decompress_dev(codec.handle, d_gz.data_ptr(), gz_len, d_moff.data_ptr(), len(offs), d_dec.data_ptr(), d_len.data_ptr(),
                                               d_st.data_ptr()), "zwz_bgzf_decompress_dev")
            codec.sync()
        for _ in range(a.warmup):
            f(); g()
        tr, td = [], []
        for _ in range(a.steps):          # alternated
            t0 = time.perf_counter(); f(); tr.append(time.perf_counter() - t0)
            t0 = time.perf_counter(); g(); td.append(time.perf_counter() - t0)
        tr, td = statistics.median(tr), statistics.median(td)
        ok = bool(torch.equal(d_out, d_in)) and bool(torch.equal(d_dec[:n], d_in)) and int(d_st.abs().sum().item()) == 0
        res["w1"] = {"ranges": 1, "s": tr, "GBps": n / tr / 1e9, "decompress_dev_s": td, "decompress_dev_GBps": n / td / 1e9,
                     "ratio_to_decompress_dev": td / tr, "target": 0.9, "verified": ok}
        del d_out, d_dec
    for key, k, size, seed in (("w2", 4096, 4096, 2), ("w3", 1000000, 100, 3)):
        if key not in only:
            continue
        rnd = random.Random(seed)
        ranges = [(o, size) for o in (rnd.randrange(0, n - size + 1) for _ in range(k))]
        d_out = torch.empty(k * size, dtype=torch.uint8, device=dev)
        f = read_dev(ranges, d_out)
        t = timed(f, a.steps, a.warmup)
        got = d_out.cpu().numpy().tobytes()
        ok = all(got[i * size:(i + 1) * size] == data[o:o + size] for i, (o, _) in enumerate(ranges))
        tm, tb = touched(ranges)
        res[key] = {"ranges": k, "range_bytes": size, "s": t, "ranges_per_s": k / t, "touched_members": tm, "touched_decoded_bytes": tb,
                    "touched_GBps": tb / t / 1e9, "host_planning_s": "not measured (in the call's wall time; see the rocprofv3 summary for GPU time)",
                    "verified": ok}
        if key == "w2" and "w1" in res:
            res[key]["ratio_to_w1_rate"] = (tb / t) / (n / res["w1"]["s"])
            res[key]["target"] = 0.8
        del d_out
    if "w4" in only:
        tmp = tempfile.mkdtemp(prefix="bgzf_range_")
        try:
            free = shutil.disk_usage(tmp).free
            path = os.path.join(tmp, "big.gz")
            body = gz[:-28]                                      # the copies' EOF members dropped but for the last
            need = a.w4_copies * len(body) + 28
            if free < 2 * need + a.w4_copies * n + (1 << 30):
                res["w4"] = "not measured (%d bytes free)" % free
            else:
                with open(path, "wb") as fo:
                    for _ in range(a.w4_copies):
                        fo.write(body)
                    fo.write(gz[-28:])
                t0 = time.perf_counter()
                z.bgzf_gzi_file(path, path + ".gzi")
                t_gzi = time.perf_counter() - t0
                total = a.w4_copies * n
                mid = total // 2 + 12345
                want = data[(mid % n):(mid % n) + (1 << 20)]
                own = -(rchar() - rchar())                       # what one read of /proc/self/io adds to rchar itself
                r0 = rchar(); t0 = time.perf_counter()
                got = codec.bgzf_read_ranges_file(path, [(mid, 1 << 20)], gzi=path + ".gzi")[0]
                t_cold = time.perf_counter() - t0; read = rchar() - r0 - own
                t_warm = timed(lambda: codec.bgzf_read_ranges_file(path, [(mid, 1 << 20)], gzi=path + ".gzi"), a.steps, 1)
                ms = sorted({(mid % n + i) // BLOCK for i in (0, (1 << 20) - 1)})
                touched_c = sum((offs[m + 1] if m + 1 < len(offs) else gz_len) - offs[m] for m in range(ms[0], ms[-1] + 1))
                out = os.path.join(tmp, "whole")
                t0 = time.perf_counter()
                r = subprocess.run([os.path.join(ROOT, "parallel-data-compression-and-decompression_amd", "main"), "bgunzip", path, out],
                                   capture_output=True, text=True, timeout=900)
                t_whole = time.perf_counter() - t0
                whole_ok = r.returncode == 0 and os.path.getsize(out) == total
                res["w4"] = {"file_bytes": os.path.getsize(path), "decoded_bytes": total, "gzi_bytes": os.path.getsize(path + ".gzi"), "gzi_file_s": t_gzi,
                             "range_bytes": 1 << 20, "first_call_s": t_cold, "s": t_warm, "bytes_read_first_call": read,
                             "touched_compressed_bytes": touched_c, "bound": touched_c + os.path.getsize(path + ".gzi"),
                             "within_bound": read <= touched_c + os.path.getsize(path + ".gzi"), "main_bgunzip_whole_s": t_whole,
                             "main_bgunzip_ok": whole_ok, "verified": got == want}
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    codec.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
