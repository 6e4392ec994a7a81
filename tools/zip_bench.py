#!/usr/bin/env python3
"""ZIP archives on the GPU against the calls they are built on, on the same buffers (a standalone tool; bench.py is the project's
yardstick and does not run this).  Fails without a GPU.

    python tools/zip_bench.py [--scale 1.0] [--steps 5] [--warmup 2] [--only w1,w3,big,zf] [--out profiles/zip_bench.json]

  W1   16 384 x 256 KiB text           W3   100 000 entries of text, log-normal sizes with a 32 KiB median, at most 4 MiB
  BIG  one 1 GiB text entry            RND  256 MiB of random bytes as one entry (the copy is all there is)
  ZF   2 048 x 256 KiB text, the archive written by Python's zipfile (level 6, one window per entry: nothing splits)
--scale multiplies entry counts and sizes.  The text is workloads.text_rows_device; entries are windows of one buffer.
Write: zip (zwz_zip_dev) against bare (zwz_deflate_streams_dev, raw, into bound-spaced ranges: the parent commit's path).
Read:  unzip (zwz_unzip_dev on the archive) against bare (zwz_inflate_split_streams_dev on the same raw streams, already aligned).
The variants of a workload alternate in one process, each a synchronised call; --warmup rounds untimed, then --steps rounds: the
median per variant and its spread (max - min) / median.  Every status must be 0 and every decoded entry equal to its input on the
device.  One JSON line on stdout (and in --out).
"""
import argparse
import importlib
import io
import json
import os
import statistics
import sys
import time
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PKG = "parallel-data-compression-and-decompression_amd"
up = lambda a: (a + 15) // 16 * 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="w1,w3,big,rnd,zf")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    only = set(a.only.split(","))
    import torch
    if not torch.cuda.is_available():
        print("zip_bench: no GPU", file=sys.stderr)
        return 2
    torch.zeros(1, device="cuda")          # torch's HIP runtime opens the GPU before the codec's library does
    import workloads
    z = importlib.import_module(PKG)
    dev = torch.device("cuda", 0)
    codec = z.Codec(0)
    rng = np.random.default_rng(2026)
    res = {"tool": "zip_bench", "scale": a.scale, "steps": a.steps, "warmup": a.warmup}

    def text_buffer(nbytes):
        rows = (nbytes + (4 << 20) - 1) // (4 << 20)
        flat = torch.zeros(rows * (4 << 20) + 16, dtype=torch.uint8, device=dev)
        for r0 in range(0, rows, 64):
            r1 = min(rows, r0 + 64)
            t = workloads.text_rows_device(torch, list(range(workloads.TEXT_SEED0 + r0, workloads.TEXT_SEED0 + r1)), 4 << 20, dev)
            flat[r0 * (4 << 20):r1 * (4 << 20)] = t.reshape(-1)
            del t
        return flat

    def timed(variants):
        torch.cuda.synchronize()
        times = {v: [] for v in variants}
        for step in range(a.warmup + a.steps):
            for v, fn in variants.items():
                t0 = time.perf_counter()
                fn()
                codec.sync()
                if step >= a.warmup:
                    times[v].append(time.perf_counter() - t0)
        return times

    def report(r, side, times, nbytes):
        med = {v: statistics.median(t) for v, t in times.items()}
        for v, t in times.items():
            r["%s_%s_ms" % (side, v)] = round(med[v] * 1e3, 3)
            r["%s_%s_GBps" % (side, v)] = round(nbytes / med[v] / 1e9, 2)
            r["%s_%s_spread" % (side, v)] = round((max(t) - min(t)) / med[v], 4)
        r["%s_over_bare" % side] = round(med["bare"] / med[side], 3)

    def read_side(r, blob_dev, blob_len, ents, d_in, offs, lens, bare_streams):
        """unzip of the archive against split inflate of the same streams aligned; bare_streams: (d_raw, off, len) device tensors."""
        n = len(ents)
        ooff = np.zeros(n, dtype=np.int64)
        ooff[1:] = np.cumsum(up(lens[:-1]))
        total = int(ooff[-1] + up(lens[-1]))
        d_out = torch.empty(total + 16, dtype=torch.uint8, device=dev)
        d_olen = torch.zeros(n, dtype=torch.int64, device=dev)
        d_st = torch.zeros(n, dtype=torch.int32, device=dev)
        d_seg = torch.zeros(n, dtype=torch.int32, device=dev)
        d_raw, d_roff, d_rlen = bare_streams
        d_ooff, d_cap = torch.from_numpy(ooff).to(dev), torch.from_numpy(lens.astype(np.int64)).to(dev)
        variants = {"unzip": lambda: codec.unzip_dev(blob_dev, blob_len, ents, d_out, ooff, d_olen, d_st, d_seg),
                    "bare": lambda: codec.inflate_split_streams_dev("raw", d_raw, d_roff, d_rlen, d_out, d_ooff, d_cap, d_olen, d_st, d_seg)}
        times = timed(variants)
        report(r, "unzip", times, int(lens.sum()))
        variants["unzip"]()
        codec.sync()
        ok = bool((d_st == 0).all().item())
        for i in range(0, n, max(1, n // 64)):          # a sample of entries, compared on the device
            ok = ok and torch.equal(d_out[int(ooff[i]):int(ooff[i] + lens[i])], d_in[int(offs[i]):int(offs[i] + lens[i])])
        r["segments"] = int(d_seg.sum().item())
        return ok

    def workload(name, d_in, offs, lens):
        n = len(lens)
        total = int(lens.sum())
        names = ["e/%07d.txt" % i for i in range(n)]
        cap = z.zip_bound(lens, names)
        d_zip = torch.empty(up(cap), dtype=torch.uint8, device=dev)
        d_zlen = torch.zeros(1, dtype=torch.int64, device=dev)
        d_zst = torch.zeros(1, dtype=torch.int32, device=dev)
        caps = np.array([z.deflate_stream_bound(int(k), "raw") for k in lens], dtype=np.int64)
        roff = np.zeros(n, dtype=np.int64)
        roff[1:] = np.cumsum(up(caps[:-1]))
        d_raw = torch.empty(int(roff[-1] + up(caps[-1])) + 16, dtype=torch.uint8, device=dev)
        d_rlen = torch.zeros(n, dtype=torch.int64, device=dev)
        d_rst = torch.zeros(n, dtype=torch.int32, device=dev)
        c_names = z._c_names(names)                     # (built once: the call itself takes char pointers)
        u_off, u_len = offs.astype(np.uint64), lens.astype(np.uint64)
        variants = {"zip": lambda: z._check(z.lib().zwz_zip_dev(codec.handle, d_in.data_ptr(), u_off.ctypes.data, u_len.ctypes.data, c_names, None, n, d_zip.data_ptr(),
                                                                  cap, d_zlen.data_ptr(), d_zst.data_ptr()), "zwz_zip_dev"),
                    "bare": lambda: codec.deflate_streams_dev("raw", d_in, offs, lens, d_raw, roff, caps, d_rlen, d_rst)}
        times = timed(variants)
        r = {"entries": n, "bytes": total}
        report(r, "zip", times, total)
        zlen = int(d_zlen.item())
        r["archive_bytes"] = zlen
        ok = int(d_zst.item()) == 0 and bool((d_rst == 0).all().item())
        blob = d_zip[:zlen].cpu().numpy().tobytes()
        ents = z.zip_index(blob)
        ok = ok and len(ents) == n
        ok = read_side(r, d_zip, zlen, ents, d_in, offs, lens, (d_raw, torch.from_numpy(roff).to(dev), d_rlen)) and ok
        r["ok"] = ok
        res[name] = r
        print(name, r, file=sys.stderr, flush=True)
        torch.cuda.empty_cache()

    def zipfile_workload(name, d_in, offs, lens):
        """The archive and the aligned raw streams both from Python's zlib at level 6, one window per entry."""
        n = len(lens)
        host = d_in.cpu().numpy()
        raw = io.BytesIO()
        with zipfile.ZipFile(raw, "w", zipfile.ZIP_DEFLATED) as zf:
            for i in range(n):
                zf.writestr("e/%07d.txt" % i, host[int(offs[i]):int(offs[i] + lens[i])].tobytes())
        blob = raw.getvalue()
        ents = z.zip_index(blob)
        clen = np.array([e.csize for e in ents], dtype=np.int64)
        roff = np.zeros(n, dtype=np.int64)
        roff[1:] = np.cumsum(up(clen[:-1]))
        packed = np.zeros(int(roff[-1] + up(clen[-1])) + 16, dtype=np.uint8)
        view = np.frombuffer(blob, dtype=np.uint8)
        for i, e in enumerate(ents):
            packed[roff[i]:roff[i] + e.csize] = view[e.data_off:e.data_off + e.csize]
        d_blob = torch.from_numpy(np.frombuffer(blob + b"\0" * 16, dtype=np.uint8).copy()).to(dev)
        r = {"entries": n, "bytes": int(lens.sum()), "archive_bytes": len(blob)}
        ok = read_side(r, d_blob, len(blob), ents, d_in, offs, lens, (torch.from_numpy(packed).to(dev), torch.from_numpy(roff).to(dev), torch.from_numpy(clen).to(dev)))
        r["ok"] = ok
        res[name] = r
        print(name, r, file=sys.stderr, flush=True)
        torch.cuda.empty_cache()

    text = text_buffer(max(int((4 << 30) * min(a.scale, 1.0)), 64 << 20))
    tbytes = text.numel() - 16
    if "w1" in only:
        n1 = max(1, min(int(16384 * a.scale), tbytes // (256 << 10)))
        workload("W1", text, np.arange(n1, dtype=np.int64) * (256 << 10), np.full(n1, 256 << 10, dtype=np.int64))
    if "w3" in only:
        n3 = max(1, int(100000 * a.scale))
        sizes = np.minimum(np.exp(rng.normal(np.log(32 << 10), 0.8, size=n3)).astype(np.int64) + 1, 4 << 20)
        starts = rng.integers(0, (tbytes - (4 << 20)) // 16, size=n3).astype(np.int64) * 16
        workload("W3", text, starts, sizes)
    if "big" in only:
        workload("BIG", text, np.zeros(1, dtype=np.int64), np.array([min(int((1 << 30) * a.scale), tbytes)], dtype=np.int64))
    if "zf" in only:
        nz = max(1, min(int(2048 * a.scale), tbytes // (256 << 10)))
        zipfile_workload("ZF", text, np.arange(nz, dtype=np.int64) * (256 << 10), np.full(nz, 256 << 10, dtype=np.int64))
    del text
    torch.cuda.empty_cache()
    if "rnd" in only:
        nr = max(int((256 << 20) * a.scale), 4 << 20) // (4 << 20) * (4 << 20)
        seeds = torch.tensor(list(range(workloads.RANDOM_SEED0, workloads.RANDOM_SEED0 + nr // (4 << 20))), dtype=torch.int64)
        flat = torch.zeros(nr + 16, dtype=torch.uint8, device=dev)
        flat[:nr] = workloads.random_files_device(torch, seeds, 4 << 20, dev).reshape(-1)
        workload("RND", flat, np.zeros(1, dtype=np.int64), np.array([nr], dtype=np.int64))
    codec.close()
    res["ok"] = all(v["ok"] for k, v in res.items() if isinstance(v, dict))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if res["ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
