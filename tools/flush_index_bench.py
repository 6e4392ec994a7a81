#!/usr/bin/env python3
"""The seek index at full-flush points on the GPU: what it costs the reader and the writer, and what it saves (a standalone tool;
bench.py is the project's yardstick and does not run this).

    python tools/flush_index_bench.py [--scale 1.0] [--steps 5] [--warmup 2] [--only a,b,c,d,e] [--span N] [--tmp DIR] [--out FILE [--merge]]

  a  reader cost: zwz_inflate_split_streams_index_dev against zwz_inflate_split_streams_dev on one 1 GiB text stream in 65 280-byte
     pieces (DESIGN.md section 17's S1) and on 64 x 16 MiB
  b  writer cost: zwz_deflate_streams_index_dev against zwz_deflate_streams_dev on the same inputs
  c  build comparison (reported, not gated): zwz_inflate_streams_index_dev, the one-wave marking build, against the split-index build
     of one 64 MiB flushed stream, and the two index sizes
  d  range reads: 4 096 ranges of 4 KiB out of the 1 GiB stream with the flush index against the marking index at the same span
  e  files: `main gzip --write-index` of a 4 GiB file against plain `main gzip` (the smaller of two runs each behind a warm-up pass,
     all four listed), and from there to the first `main gunzip --index --offset` byte.  The chain this replaces -- `main gzip` +
     `main gzindex` + the same read -- is not run: see DESIGN.md section 26
--scale multiplies the sizes and is recorded with every measurement.  Every figure is the wall time of a synchronised call, median of --steps after --warmup, the variants of
a workload alternating in one process, with the spread (max - min) / median; every output is checked on the device.  One JSON line on
stdout (and in --out).
"""
import argparse
import importlib
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PKG = "parallel-data-compression-and-decompression_amd"


def alternate(variants, steps, warmup):
    """{name: fn} -> {name: (median seconds, spread)}: one call of each in turn, steps + warmup times"""
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
    ap.add_argument("--only", default="a,b,c,d,e")
    ap.add_argument("--span", type=int, default=1 << 20)
    ap.add_argument("--tmp", default=None)
    ap.add_argument("--out", default="")
    ap.add_argument("--merge", action="store_true", help="keep the measurements --out already holds that this run does not take")
    a = ap.parse_args()
    only = set(a.only.split(","))
    import torch
    torch.zeros(1, device="cuda")
    dev = torch.device("cuda", 0)
    z = importlib.import_module(PKG)
    import corpus
    codec = z.Codec(0)
    span = a.span
    res = {"tool": "flush_index_bench", "scale": a.scale, "steps": a.steps, "warmup": a.warmup, "span": span}
    pool = torch.from_numpy(np.frombuffer(corpus.text_like(7, 32 << 20), dtype=np.uint8).copy()).to(dev)
    up = lambda x: (x + 15) // 16 * 16

    def text(n):
        reps = [torch.roll(pool, 7919 * (r + 1)) for r in range((n + pool.numel() - 1) // pool.numel())]
        return torch.cat(reps)[:n].contiguous()

    def layout(sizes):
        off = np.zeros(len(sizes), dtype=np.int64)
        off[1:] = np.cumsum(up(np.asarray(sizes[:-1], dtype=np.int64)))
        return off

    class Writer:
        """n inputs on the device; the stream and index ranges at their bounds"""
        def __init__(self, lens):
            self.lens = np.asarray(lens, dtype=np.int64)
            self.n = len(lens)
            self.s_off = layout(self.lens)
            self.d_src = text(int(self.s_off[-1] + up(self.lens[-1])))
            self.caps = np.array([up(z.deflate_stream_bound(int(k), "gzip")) for k in lens], dtype=np.int64)
            self.icaps = np.array([z.deflate_stream_index_bound(int(k), span) for k in lens], dtype=np.int64)
            self.c_off, self.i_off = layout(self.caps), layout(self.icaps)
            self.d_comp = torch.zeros(int(self.caps.sum()) + 16, dtype=torch.uint8, device=dev)
            self.d_idx = torch.zeros(int(self.icaps.sum()) + 16, dtype=torch.uint8, device=dev)
            self.d_olen = torch.zeros(self.n, dtype=torch.int64, device=dev)
            self.d_ilen = torch.zeros(self.n, dtype=torch.int64, device=dev)
            self.d_st = torch.zeros(self.n, dtype=torch.int32, device=dev)

        def run(self, index):
            torch.cuda.synchronize()                          # (torch fills and compares on a stream of its own)
            if index:
                codec.deflate_streams_index_dev("gzip", self.d_src, self.s_off, self.lens, self.d_comp, self.c_off, self.caps, self.d_olen, self.d_st,
                                                self.d_idx, self.i_off, self.icaps, self.d_ilen, span)
            else:
                codec.deflate_streams_dev("gzip", self.d_src, self.s_off, self.lens, self.d_comp, self.c_off, self.caps, self.d_olen, self.d_st)
            codec.sync()

    class Reader:
        """the writer's streams, one output range each of exactly the decoded size, index ranges at the one-wave bound"""
        def __init__(self, w):
            self.w = w
            w.run(True)
            self.c_len = w.d_olen.cpu().numpy().copy()
            self.w_idx = [w.d_idx[int(o):int(o) + int(k)].clone() for o, k in zip(w.i_off, w.d_ilen.cpu().numpy())]
            t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
            self.icaps = np.array([z.lib().zwz_inflate_index_bound(int(k), span) for k in w.lens], dtype=np.int64)
            self.i_off = layout(self.icaps)
            self.d_coff, self.d_clen, self.d_ooff, self.d_cap = t(w.c_off), t(self.c_len), t(w.s_off), t(w.lens)
            self.d_ioff, self.d_icap = t(self.i_off), t(self.icaps)
            self.d_out = torch.empty(int(w.d_src.numel()) + 16, dtype=torch.uint8, device=dev)
            self.d_idx = torch.zeros(int(self.icaps.sum()) + 16, dtype=torch.uint8, device=dev)
            self.d_olen = torch.zeros(w.n, dtype=torch.int64, device=dev)
            self.d_ilen = torch.zeros(w.n, dtype=torch.int64, device=dev)
            self.d_st = torch.zeros(w.n, dtype=torch.int32, device=dev)
            self.d_seg = torch.zeros(w.n, dtype=torch.int32, device=dev)

        def run(self, which):
            torch.cuda.synchronize()                          # (torch fills and compares on a stream of its own)
            args = ("gzip", self.w.d_comp, self.d_coff, self.d_clen, self.d_out, self.d_ooff, self.d_cap, self.d_olen, self.d_st)
            idx = (self.d_idx, self.d_ioff, self.d_icap, self.d_ilen, span)
            if which == "split":
                codec.inflate_split_streams_dev(*args, self.d_seg)
            elif which == "split_index":
                codec.inflate_split_streams_index_dev(*args, self.d_seg, *idx)
            else:
                codec.inflate_streams_index_dev(*args, *idx)
            codec.sync()

        def check(self, index=None):
            """the decoded bytes are the input's; index "writer": every index is the one the writer wrote"""
            w = self.w
            ok = bool((self.d_st == 0).all()) and bool((self.d_olen == self.d_cap).all())
            for i in range(w.n):
                ok = ok and torch.equal(self.d_out[int(w.s_off[i]):int(w.s_off[i] + w.lens[i])], w.d_src[int(w.s_off[i]):int(w.s_off[i] + w.lens[i])])
                if index == "writer":
                    k = int(self.d_ilen[i].item())
                    ok = ok and torch.equal(self.d_idx[int(self.i_off[i]):int(self.i_off[i]) + k], self.w_idx[i])
            self.d_out.zero_(); self.d_st.fill_(-1)
            return ok

    def pair(times, new, old):
        return {"%s_s" % new: times[new][0], "%s_spread" % new: times[new][1], "%s_s" % old: times[old][0], "%s_spread" % old: times[old][1],
                "ratio": times[new][0] / times[old][0]}

    shapes = {"one_stream": [int((1 << 30) * a.scale)], "64_streams": [int((16 << 20) * a.scale)] * 64}
    writers = {}

    def writer(name):
        if name not in writers:
            writers.clear()                                   # (one workload's buffers at a time)
            writers[name] = Writer(shapes[name])
        return writers[name]

    for name in shapes:
        if "b" in only:
            w = writer(name)
            tm = alternate({"index": lambda: w.run(True), "plain": lambda: w.run(False)}, a.steps, a.warmup)
            w.run(False); plain = w.d_comp.clone(); plain_len = w.d_olen.clone()
            w.run(True)
            ok = torch.equal(plain, w.d_comp) and torch.equal(plain_len, w.d_olen) and bool((w.d_st == 0).all()) and bool((w.d_ilen > 0).all())
            res["b_writer_" + name] = dict(pair(tm, "index", "plain"), bytes=int(w.lens.sum()), ok=ok, index_bytes=int(w.d_ilen.sum().item()))
            del plain
        if "a" in only:
            r = Reader(writer(name))
            tm = alternate({"split_index": lambda: r.run("split_index"), "split": lambda: r.run("split")}, a.steps, a.warmup)
            r.run("split"); ok = r.check()
            r.run("split_index"); ok = r.check("writer") and ok
            res["a_reader_" + name] = dict(pair(tm, "split_index", "split"), bytes=int(r.w.lens.sum()), ok=ok, segments=int(r.d_seg.sum().item()))
            del r
    if "c" in only:
        shapes["build"] = [int((64 << 20) * a.scale)]
        r = Reader(writer("build"))
        tm = alternate({"split_index": lambda: r.run("split_index"), "marking": lambda: r.run("marking")}, a.steps, a.warmup)
        r.run("marking"); ok = r.check(); mark_bytes = int(r.d_ilen.sum().item())
        r.run("split_index"); ok = r.check("writer") and ok
        res["c_build"] = dict(pair(tm, "split_index", "marking"), bytes=int(r.w.lens.sum()), ok=ok, flush_index_bytes=int(r.d_ilen.sum().item()),
                              marking_index_bytes=mark_bytes)
        del r
    if "d" in only:
        n = int((1 << 30) * a.scale)
        shapes["ranges"] = [n]
        r = Reader(writer("ranges"))
        r.run("split_index")
        flush_idx = r.d_idx[:int(r.d_ilen[0].item())].cpu().numpy().tobytes()
        r.run("marking")
        mark_idx = r.d_idx[:int(r.d_ilen[0].item())].cpu().numpy().tobytes()
        if not mark_idx or not flush_idx:
            raise RuntimeError("d: no index: marking status %d, decoded %d of %d, index bytes %d (flush index %d bytes, %d compressed bytes)"
                               % (int(r.d_st[0].item()), int(r.d_olen[0].item()), n, len(mark_idx), len(flush_idx), int(r.c_len[0])))
        rng = np.random.RandomState(5)
        ranges = np.stack([rng.randint(0, n - 4096, 4096).astype(np.uint64), np.full(4096, 4096, dtype=np.uint64)], axis=1)
        d_in = r.w.d_comp
        d_got = torch.zeros(4096 * 4096 + 16, dtype=torch.uint8, device=dev)
        c_len = int(r.c_len[0])
        d_f = torch.from_numpy(np.frombuffer(flush_idx, dtype=np.uint8).copy()).to(dev)
        d_m = torch.from_numpy(np.frombuffer(mark_idx, dtype=np.uint8).copy()).to(dev)
        torch.cuda.synchronize()
        tm = alternate({"flush": lambda: codec.read_ranges_dev(d_in, c_len, flush_idx, ranges, d_got, d_idx=d_f),
                        "marking": lambda: codec.read_ranges_dev(d_in, c_len, mark_idx, ranges, d_got, d_idx=d_m)}, a.steps, a.warmup)
        expect = torch.cat([r.w.d_src[int(o):int(o) + 4096] for o, _ in ranges])
        ok = True
        for idx, d_i in ((flush_idx, d_f), (mark_idx, d_m)):
            d_got.zero_()
            codec.read_ranges_dev(d_in, c_len, idx, ranges, d_got, d_idx=d_i)
            ok = ok and torch.equal(d_got[:expect.numel()], expect)
        res["d_ranges"] = dict(pair(tm, "flush", "marking"), ranges=4096, ok=ok, flush_index_bytes=len(flush_idx), marking_index_bytes=len(mark_idx))
        del r
    writers.clear()
    codec.close()
    if "e" in only:
        tmp = tempfile.mkdtemp(prefix="zwz_flush_index_", dir=a.tmp)
        try:
            n = int((4 << 30) * a.scale)
            src = os.path.join(tmp, "src.bin")
            host = text(min(n, 256 << 20)).cpu().numpy()
            with open(src, "wb") as f:
                for at in range(0, n, host.size):
                    f.write(host[:min(host.size, n - at)].tobytes())
            main_bin = os.path.join(ROOT, PKG, "main")

            def run(*args):
                t0 = time.perf_counter()
                out = subprocess.run([main_bin] + list(args), capture_output=True, text=True)
                if out.returncode:
                    raise RuntimeError("%s: %s" % (" ".join(args), out.stderr))
                return time.perf_counter() - t0

            gz, gz2, zwi, got = os.path.join(tmp, "a.gz"), os.path.join(tmp, "b.gz"), os.path.join(tmp, "b.zwi"), os.path.join(tmp, "got.bin")
            off, size = n // 2 + 12345, 1 << 20
            plain, indexed = [], []
            for it in range(3):                                # the two writers in turn; the first pass warms the file cache
                t1, t2 = run("gzip", src, gz), run("gzip", src, gz2, "--write-index", zwi, "--span", str(span))
                if it:
                    plain.append(t1); indexed.append(t2)
            e = {"bytes": n, "gzip_s": min(plain), "gzip_write_index_s": min(indexed), "runs": [plain, indexed]}
            e["ratio"] = e["gzip_write_index_s"] / e["gzip_s"]
            e["read_flush_s"] = run("gunzip", gz2, got, "--index", zwi, "--offset", str(off), "--size", str(size))
            e["flush_index_bytes"] = os.path.getsize(zwi)
            e["chain_flush_s"] = e["gzip_write_index_s"] + e["read_flush_s"]
            piece = open(got, "rb").read()
            at = off % host.size
            want = (host[at:at + size] if at + size <= host.size else np.concatenate([host[at:], host[:at + size - host.size]])).tobytes()
            same = os.path.getsize(gz) == os.path.getsize(gz2)
            with open(gz, "rb") as f1, open(gz2, "rb") as f2:
                while same:
                    b1, b2 = f1.read(1 << 24), f2.read(1 << 24)
                    same = b1 == b2
                    if not b1:
                        break
            e["ok"] = piece == want and same
            # the chain it replaces, plain `main gzip` + `main gzindex` + the same read, is not run here: `main gzindex` of a flushed file
            # of this size ended in a GPU memory fault when this tool was written
            e["chain_marking_s"] = None
            res["e_files"] = e
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    for k, v in res.items():                               # every measurement says at what scale it was taken
        if isinstance(v, dict):
            v["scale"] = a.scale
    if a.merge and a.out and os.path.exists(a.out):
        old = json.loads(open(a.out).read())
        old.update({k: v for k, v in res.items() if isinstance(v, dict)})
        old.pop("scale", None)
        res = old
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
