#!/usr/bin/env python3
"""The file loop of the decode in legs on the GPU (a standalone tool; bench.py is the project's yardstick and does not run this).

    python tools/inflate_legs_file_bench.py [--mib 256] [--steps 5] [--warmup 2] [--long] [--out profiles/inflate_legs_file_bench.json]

It measures no speed-up: one stream is decoded by ONE wave, about 36 s a decoded GiB, through the file call as through the device call.
  (a) one ordinary gzip text file of --mib MiB decoded (Python's zlib, level 6):
      file   zwz_inflate_legs_file at the default options: the file through the staging windows, dst and the index written
      dev    zwz_inflate_legs_dev on the same stream from device memory, with its index: the yardstick, unchanged by the file loop
      alternating in one process, median of --steps after --warmup, spread = max - min.  Expected: the decode dominates; reading and
      writing hide behind it except the last commit's copy and write, which is timed on its own (last_commit): a copy of as many bytes
      from the device to pinned memory and their write to a file.  How many bytes that is follows from the index: a rewound leg restarts
      at the last entry in front of its input window's end.
  (b) --long: a gzip file of more than 2^29 bytes (text, Python's zlib at level 1), `main gzindex`, then `main gunzip
      --index`, against plain `main gunzip` on the same file: wall times of the three commands, outputs compared by SHA-256.
One JSON line on stdout (and in --out).  A comparison that fails exits 1.
"""
import argparse
import hashlib
import importlib
import json
import os
import shutil
import statistics
import struct
import subprocess
import sys
import tempfile
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PKG = "parallel-data-compression-and-decompression_amd"
LEG_IN, LEG_OUT = 67108864, 268435456


def alternate(variants, steps, warmup):
    ts = {k: [] for k in variants}
    for it in range(warmup + steps):
        for k, fn in variants.items():
            t0 = time.perf_counter()
            fn()
            dt = time.perf_counter() - t0
            if it >= warmup:
                ts[k].append(dt)
    return {k: (statistics.median(v), max(v) - min(v)) for k, v in ts.items()}


def text(n):
    import corpus
    pool = np.frombuffer(corpus.text_like(7, 32 << 20), dtype=np.uint8)
    return np.concatenate([np.roll(pool, 7919 * (r + 1)) for r in range((n + len(pool) - 1) // len(pool))])[:n]


def legs_from_index(idx, stream_len):
    """The restart points of the file loop at the default windows, from the index: (legs, decoded offset where the last leg started)."""
    count = struct.unpack_from("<I", idx, 32)[0]
    ent = [struct.unpack_from("<QQ", idx, 64 + 24 * k) for k in range(count)]
    legs, base, start = 0, 0, 0
    while True:
        legs += 1
        end = base + LEG_IN
        if end >= stream_len:
            return legs, start
        bit, start = [e for e in ent if e[0] < 8 * end][-1]
        base = (bit >> 3) & ~15


def sha(path):
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for b in iter(lambda: f.read(1 << 24), b""):
            h.update(b)
    return h.hexdigest()


def one_file(a, z, torch, codec, tmp, res):
    n = a.mib << 20
    host = text(n)
    t0 = time.perf_counter()
    c = zlib.compressobj(6, zlib.DEFLATED, 31)
    stream = c.compress(host.tobytes()) + c.flush()
    res["a_compress_s"] = round(time.perf_counter() - t0, 1)
    src, dst, zwi = os.path.join(tmp, "a.gz"), os.path.join(tmp, "a.out"), os.path.join(tmp, "a.zwi")
    with open(src, "wb") as f:
        f.write(stream)
    span = 1 << 20
    blob = np.zeros((len(stream) + 31) // 16 * 16, dtype=np.uint8)
    blob[:len(stream)] = np.frombuffer(stream, dtype=np.uint8)
    d_in = torch.from_numpy(blob).cuda()
    cap = (n + 15) // 16 * 16
    icap = int(z.lib().zwz_inflate_index_bound(cap, span))
    d_out = torch.empty(cap + 16, dtype=torch.uint8, device="cuda")
    d_idx = torch.empty(icap, dtype=torch.uint8, device="cuda")
    d_len = torch.zeros(1, dtype=torch.int64, device="cuda")
    d_ilen = torch.zeros(1, dtype=torch.int64, device="cuda")
    d_st = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    legs = np.zeros(3, dtype=np.uint32)
    stats = {}

    def dev():
        codec.inflate_legs_dev("gzip", d_in, [0], [len(stream)], d_out, [0], [cap], d_len, d_st, span, d_idx, [0], [icap], d_ilen, legs)
        codec.sync()

    def file():
        stats.update(codec.inflate_legs_file(src, dst, zwi, "gzip"))

    dev()
    ok = int(d_st.item()) == 0 and int(d_len.item()) == n and bool(torch.equal(d_out[:n].cpu(), torch.from_numpy(host)))
    want_idx = d_idx[:int(d_ilen.item())].cpu().numpy().tobytes()
    file()
    with open(zwi, "rb") as f:
        ok = ok and f.read() == want_idx
    ok = ok and sha(dst) == hashlib.sha256(host.tobytes()).hexdigest()
    times = alternate({"file": file, "dev": dev}, a.steps, a.warmup)
    res.update({"a_decoded_bytes": n, "a_compressed_bytes": len(stream), "a_span": span, "a_dev_legs_run_rewound_grown": legs.tolist(), "a_file_stats": dict(stats)})
    for k, (med, spread) in times.items():
        res["a_%s_wall_ms" % k], res["a_%s_spread_ms" % k] = round(med * 1e3, 1), round(spread * 1e3, 1)
    res["a_file_over_dev"] = round(res["a_file_wall_ms"] / res["a_dev_wall_ms"], 4)
    res["a_dev_s_per_decoded_gib"] = round(res["a_dev_wall_ms"] / 1e3 / (n / 2**30), 2)
    # the last commit's copy and write on its own
    nlegs, last_start = legs_from_index(want_idx, len(stream))
    res["a_legs_from_index"] = nlegs                   # (equal to a_file_stats.legs when the restart points were read right)
    k = n - last_start
    pinned = torch.empty(k, dtype=torch.uint8).pin_memory()

    def last_commit():
        pinned.copy_(d_out[last_start:n])
        torch.cuda.synchronize()
        with open(dst, "wb") as f:
            f.write(pinned.numpy().data)
    med, spread = alternate({"c": last_commit}, a.steps, a.warmup)["c"]
    res.update({"a_last_commit_bytes": k, "a_last_commit_wall_ms": round(med * 1e3, 1), "a_last_commit_spread_ms": round(spread * 1e3, 1)})
    res["a_file_minus_dev_ms"] = round(res["a_file_wall_ms"] - res["a_dev_wall_ms"], 1)
    for p in (src, dst, zwi):
        os.unlink(p)
    del d_in, d_out, d_idx
    torch.cuda.empty_cache()
    return ok


def long_file(tmp, res):
    """A gzip file of more than 2^29 bytes through the three commands."""
    cli = os.path.join(ROOT, PKG, "main")
    src, zwi, out1, out2 = (os.path.join(tmp, x) for x in ("b.gz", "b.gz.zwi", "b.indexed", "b.plain"))
    t0 = time.perf_counter()
    txt = text(8 << 20).tobytes()
    c = zlib.compressobj(1, zlib.DEFLATED, 31)
    h, n, size, i = hashlib.sha256(), 0, 0, 0
    with open(src, "wb") as f:
        while size <= (1 << 29) + (8 << 20):
            piece = txt[i % 64:] + txt[:i % 64]
            i += 1
            h.update(piece)
            n += len(piece)
            size += f.write(c.compress(piece))
        size += f.write(c.flush())
    res.update({"b_compressed_bytes": size, "b_decoded_bytes": n, "b_compress_s": round(time.perf_counter() - t0, 1)})
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "ZWZ_NRANKS", "OMPI_COMM_WORLD_SIZE", "PMI_SIZE")}
    ok = size > 1 << 29
    for key, args, outp in (("b_gzindex", ["gzindex", src, zwi], None), ("b_gunzip_index", ["gunzip", src, out1, "--index", zwi], out1), ("b_gunzip_plain", ["gunzip", src, out2], out2)):
        t0 = time.perf_counter()
        r = subprocess.run([cli] + args, capture_output=True, text=True, timeout=900, env=env)
        res[key + "_wall_s"] = round(time.perf_counter() - t0, 2)
        ok = ok and r.returncode == 0
        if r.returncode != 0:
            res[key + "_error"] = r.stderr[-400:]
        elif outp:
            ok = ok and sha(outp) == h.hexdigest()
            os.unlink(outp)
    res["b_index_bytes"] = os.path.getsize(zwi) if os.path.exists(zwi) else 0
    res["b_plain_s_per_decoded_gib"] = round(res["b_gunzip_plain_wall_s"] / (n / 2**30), 2)
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--long", action="store_true")
    ap.add_argument("--no-one", action="store_true", help="skip (a)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    res = {"tool": "inflate_legs_file_bench", "steps": a.steps, "warmup": a.warmup}
    tmp = tempfile.mkdtemp(prefix="zwz_legs_file_bench_")
    ok = True
    try:
        if not a.no_one:
            import torch
            torch.zeros(1, device="cuda")
            z = importlib.import_module(PKG)
            codec = z.Codec(0)
            ok = one_file(a, z, torch, codec, tmp, res)
            codec.close()
        if a.long:
            ok = long_file(tmp, res) and ok
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    res["ok"] = bool(ok)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
