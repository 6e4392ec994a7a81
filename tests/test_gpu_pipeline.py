"""GPU parity tests, second file: the configurations and corners round 1 left without byte-level evidence -- the bench's
own workspace size, a mixed-content soak, reordered / damaged shards, decompression shared by several ranks, stale
rendezvous markers, the opt-in loss-free chunk size.  All through the C ABI; bit-exact."""
import hashlib
import importlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import corpus

pytestmark = pytest.mark.gpu
CHUNK, STRIDE = 65535, 65536
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def sha(b):
    return hashlib.sha256(b).hexdigest()


@pytest.fixture(scope="module")
def zwz():
    return importlib.import_module("parallel-data-compression-and-decompression_amd")


@pytest.fixture(scope="module")
def codec(zwz):
    c = zwz.Codec(0, 1024)
    yield c
    c.close()


def _cli():
    return os.path.join(ROOT, "parallel-data-compression-and-decompression_amd", "main")


def _tree_of(root):
    out = {}
    for d, _, names in os.walk(root):
        for n in names:
            b = open(os.path.join(d, n), "rb").read()
            out[os.path.relpath(os.path.join(d, n), root)] = {"size": len(b), "sha256": sha(b)}
    return out


def _write_tree(root):
    files = corpus.golden_tree()
    for rel, data in files.items():
        p = os.path.join(root, rel)
        os.makedirs(os.path.dirname(p), exist_ok=True)
        with open(p, "wb") as f:
            f.write(data)
    return files


# ---------------------------------------------------------------------------------------------- bench-sized batches
@pytest.mark.parametrize("workload", ["random", "text"])
def test_full_batch_at_bench_workspace_is_bit_identical(zwz, oracle, workload):
    """BASELINE configs[1] / [2] at full size (10 000 x 256 KiB = 50 000 chunks) the way bench.py runs them -- ONE launch
    per kernel over a 51 200-chunk workspace -- against the same chunks run in 1 024-chunk slices (the size every other
    parity test uses), byte for byte, plus an oracle sample and the device-side round-trip comparison."""
    torch = pytest.importorskip("torch")
    import bench
    import workloads
    dev = torch.device("cuda", 0)
    d_in, d_off, d_len, n, raw, host_file = workloads.build_equal_files(torch, dev, workload, 10000, 262144)
    assert n == 50000
    outs = []
    for max_batch in (51200, 1024):
        c = zwz.Codec(0, max_batch)
        try:
            d_out = torch.zeros(n * STRIDE, dtype=torch.uint8, device=dev)
            d_olen = torch.zeros(n, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()      # torch fills on ITS stream; the codec runs on its own (non-blocking) one
            c.deflate_dev(d_in, d_off, d_len, d_out, d_olen)
            c.sync()
            if max_batch == 51200:
                d_back = torch.zeros(n * STRIDE, dtype=torch.uint8, device=dev)
                d_blen = torch.zeros(n, dtype=torch.int32, device=dev)
                d_stat = torch.zeros(n, dtype=torch.int32, device=dev)
                torch.cuda.synchronize()
                c.inflate_dev(d_out, d_off, d_olen, d_back, d_blen, d_stat)
                c.sync()
                v = bench.verify_bytes(torch, d_in, d_len, d_olen, d_back, d_blen, d_stat)
                assert v["length_rule_ok"] and v["chunks_with_wrong_bytes"] == 0, v
                assert v["truncated_chunks"] == (40000 if workload == "random" else 0)
                o = bench.verify_oracle_sample(torch, 256, d_in, d_len, d_out, d_olen, d_back, d_blen)
                assert o["sampled"] >= 250 and o["payload_mismatches"] == 0 and o["decode_mismatches"] == 0, o
                del d_back
            outs.append((d_out, d_olen))
        finally:
            c.close()
    (a, alen), (b, blen) = outs
    assert torch.equal(alen, blen)
    col = torch.arange(STRIDE, device=dev, dtype=torch.int32).view(1, -1)
    av, bv = a.view(n, STRIDE), b.view(n, STRIDE)
    for c0 in range(0, n, 2048):
        live = col < alen[c0:c0 + 2048].view(-1, 1)
        assert not bool(((av[c0:c0 + 2048] != bv[c0:c0 + 2048]) & live).any().item()), c0


def test_soak_mixed_chunks(codec, oracle):
    """5 000 chunks of mixed kinds, sizes and stitched segments against the oracle, then corrupted / cut streams: lz_links'
    single-exchange insert stands on a lane order the ISA manual does not spell out, so the evidence is
    volume, every run."""
    N, seed = 5000, 11
    rs = corpus.splitmix64(seed, 6 * N)
    kinds = [k for k in corpus.KINDS if k != "lz"]
    chunks = []
    for i in range(N):
        r = int(rs[6 * i] % 100)
        if r < 60:
            kind = kinds[int(rs[6 * i + 1] % len(kinds))]
            n = int(rs[6 * i + 2] % 65536) if r < 45 else 65535 - int(rs[6 * i + 2] % 700)
            chunks.append(corpus.make(kind, seed * 100000 + i, n))
        else:
            parts, total = [], 0
            for j in range(2 + int(rs[6 * i + 1] % 4)):
                kind = kinds[int((rs[6 * i + 3] >> (7 * j)) % len(kinds))]
                n = 200 + int((rs[6 * i + 4] >> (11 * j)) % 30000)
                n = min(n, 65535 - total)
                if n <= 0:
                    break
                parts.append(corpus.make(kind, seed * 100000 + 7 * i + j, n)); total += n
            chunks.append(b"".join(parts))
    got = codec.deflate_chunks(chunks)
    back, _ = codec.inflate_chunks(got)
    bad = [(i, len(c)) for i, (c, g) in enumerate(zip(chunks, got)) if g != oracle.payload(c)]
    assert not bad, bad[:10]
    wrong = [i for i, (g, b) in enumerate(zip(got, back)) if b != oracle.inflate(g, 70000)[0]]
    assert not wrong, wrong[:10]
    import zlib
    rs2 = corpus.splitmix64(seed + 77, 4 * 1500)
    damaged = []
    for i in range(1500):
        z = bytearray(got[i]) if len(got[i]) > 8 else bytearray(zlib.compress(b"abcabcabc" * 50, 6))
        mode = int(rs2[4 * i] % 4)
        if mode == 0:
            z[2 + int(rs2[4 * i + 1] % (len(z) - 2))] ^= 1 << int(rs2[4 * i + 2] % 8)
        elif mode == 1:
            z = z[:2 + int(rs2[4 * i + 1] % (len(z) - 2))]
        elif mode == 2:
            for j in range(3):
                z[2 + int((rs2[4 * i + 1] >> (11 * j)) % (len(z) - 2))] ^= 0xff
        else:
            z += bytes(min(int(rs2[4 * i + 1] % 7), 65535 - len(z)))
        damaged.append(bytes(z))
    gb, _ = codec.inflate_chunks(damaged)
    off = []
    for i, (pl, g) in enumerate(zip(damaged, gb)):
        w, total, st = oracle.inflate(pl, 1 << 20)
        if total <= 65535 and g != w:
            off.append(i)
    assert not off, off[:10]


# ---------------------------------------------------------------------------------------------- container corners
def test_decompress_edge_shards_like_reference(zwz, codec, golden_dir, tmp_path):
    """Reordered and damaged shards through the GPU path against what the reference binary made of them (edges.json):
    records permuted within files (decompression.cpp:119-153), shards cut at a record boundary / inside an MD5 / inside a
    payload / inside a header, an empty shard.  A damaged shard decodes up to the damage like the reference and then
    reports ZWZ_E_FORMAT (the reference exits 0)."""
    import zwz_records
    edges = json.load(open(os.path.join(golden_dir, "edges.json")))
    good = open(os.path.join(golden_dir, "tree_N1", "compressed_0.zwz"), "rb").read()
    for name, blob in zwz_records.edge_shards(good).items():
        want = edges[name]
        assert sha(blob) == want["shard_sha256"]
        src, out = tmp_path / (name + "_in"), tmp_path / (name + "_out")
        src.mkdir(); out.mkdir()
        (src / "compressed_0.zwz").write_bytes(blob)
        if name in ("cut_md5", "cut_payload", "cut_header"):
            with pytest.raises(zwz.ZwzError) as ei:
                codec.do_decompression(str(src), str(out))
            assert ei.value.status == zwz.E_FORMAT, name
            bad = ei.value.md5_mismatches
        else:
            bad = codec.do_decompression(str(src), str(out))
        assert bad == want["md5_mismatches"], name
        assert _tree_of(str(out)) == want["decoded"], name


@pytest.mark.parametrize("nranks,nshards", [(2, 1), (3, 1), (2, 2), (2, 3)])
def test_cli_multirank_decompress_matches_reference_tree(golden_dir, tmp_path, nranks, nshards):
    """`main decompress` as N ranks on this box's GPU: ONE shard split into N record ranges (BASELINE
    configs[4]'s shape) with the decoded byte counts all-gathered, and whole shards round-robin.  The tree must be the
    reference's own (lossy) decoded tree; the MD5 mismatches it prints must be reported by some rank."""
    run = json.load(open(os.path.join(golden_dir, "tree.json")))["runs"][str(nshards)]
    zdir = tmp_path / "zwz"
    zdir.mkdir()
    if nshards == 1:
        shutil.copy(os.path.join(golden_dir, "tree_N1", "compressed_0.zwz"), zdir / "compressed_0.zwz")
    else:
        import oracle_binding
        src = tmp_path / "src"
        _write_tree(str(src))
        rec = tmp_path / "list.txt"
        rec.write_text(run["sorted_list"])
        o = oracle_binding.load()
        for r in range(nshards):
            assert o.compress_shard(str(src), str(zdir), str(rec), r, nshards) == 0
    back = tmp_path / "back"
    procs = []
    for r in range(nranks):
        env = dict(os.environ, ZWZ_RANK=str(r), ZWZ_NRANKS=str(nranks), ZWZ_DEVICE="0", ZWZ_RENDEZVOUS_TIMEOUT="120")
        procs.append(subprocess.Popen([_cli(), "decompress", str(zdir), str(back)], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.PIPE, text=True))
    outs = [p.communicate(timeout=300) for p in procs]
    assert all(p.returncode == 0 for p in procs), outs
    assert "Operation: decompress" in outs[0][0] and "Processor Count: %d" % nranks in outs[0][0]
    assert sum(o[1].count("MD5 mismatch for file:") for o in outs) == run["md5_mismatches"]
    for rel, want in run["decoded"].items():
        b = open(back / rel, "rb").read()
        assert {"size": len(b), "sha256": sha(b)} == want, rel
    assert not [n for n in os.listdir(back) if n.startswith(".zwz_")]          # rendezvous markers cleaned up


@pytest.mark.parametrize("nranks,budget", [(2, "0"), (2, "4"), (3, "1"), (3, "2")])
def test_cli_split_decode_streams_a_range_that_does_not_fit(golden_dir, tmp_path, nranks, budget):
    """One shard split over N ranks whose record ranges do NOT fit the device (BASELINE configs[4]: 64 GiB over few ranks; forced
    here by ZWZ_MAX_RANGE_CHUNKS, the number of chunks a rank may keep on the device between the two phases): the first slices
    stay resident, the others keep only their decoded lengths for the exchange and are inflated a second time when their
    bytes are written (decompression.cpp:65-154 streams by construction).  Same tree as the reference's, same MD5 verdicts."""
    run = json.load(open(os.path.join(golden_dir, "tree.json")))["runs"]["1"]
    zdir = tmp_path / "zwz"
    zdir.mkdir()
    shutil.copy(os.path.join(golden_dir, "tree_N1", "compressed_0.zwz"), zdir / "compressed_0.zwz")
    back = tmp_path / "back"
    procs = []
    for r in range(nranks):
        env = dict(os.environ, ZWZ_RANK=str(r), ZWZ_NRANKS=str(nranks), ZWZ_DEVICE="0", ZWZ_RENDEZVOUS_TIMEOUT="120", ZWZ_MAX_RANGE_CHUNKS=budget, ZWZ_VERBOSE="1")
        procs.append(subprocess.Popen([_cli(), "decompress", str(zdir), str(back)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    outs = [p.communicate(timeout=300) for p in procs]
    assert all(p.returncode == 0 for p in procs), outs
    held = [int(l.split("holds ")[1].split(" of its ")[0]) for o in outs for l in o[1].splitlines() if "split decode: rank" in l]
    total = [int(l.split(" of its ")[1].split(" chunks")[0]) for o in outs for l in o[1].splitlines() if "split decode: rank" in l]
    assert len(held) == nranks and all(h <= int(budget) for h in held) and any(h < t for h, t in zip(held, total)), (held, total)
    assert sum(o[1].count("MD5 mismatch for file:") for o in outs) == run["md5_mismatches"]
    for rel, want in run["decoded"].items():
        b = open(back / rel, "rb").read()
        assert {"size": len(b), "sha256": sha(b)} == want, rel


def test_cli_ignores_stale_markers_of_a_crashed_run(golden_dir, tmp_path):
    """A run that died leaves its rendezvous files in <dst>.  The next run -- even under the SAME run id -- must not take
    the dead run's list path, nor its completion markers, for its own (csrc/main.cpp: nonce handshake)."""
    run = json.load(open(os.path.join(golden_dir, "tree.json")))["runs"]["2"]
    src = tmp_path / "data" / "src"
    _write_tree(str(src))
    rec = tmp_path / "list.txt"
    rec.write_text(run["sorted_list"])
    wrong = tmp_path / "stale_list.txt"
    wrong.write_text("hello.txt\n")                                        # what a stale publication would point at
    dst = tmp_path / "zwz"
    dst.mkdir()
    stem = ".zwz_compress_FIXEDRUN"
    (dst / (stem + "_list_999s1")).write_text("999s1\n%s\n888s1\n" % wrong)   # dead rank 0's publication naming dead rank 1
    (dst / (stem + "_here_1_888s1")).write_text("888s1\n")
    (dst / (stem + "_done_1_999s1")).write_text("0\n")
    (dst / ".zwz_compress_list_ready").write_text("")                         # round-1 style markers
    (dst / ".zwz_compress_list").write_text(str(wrong))
    procs = []
    for r in (1, 0):                                                          # rank 1 first: it must wait for the live rank 0
        env = dict(os.environ, ZWZ_RANK=str(r), ZWZ_NRANKS="2", ZWZ_DEVICE="0", ZWZ_RUN_ID="FIXEDRUN", ZWZ_RENDEZVOUS_TIMEOUT="120")
        if r == 0:
            env["ZWZ_FILE_RECORD"] = str(rec)
        procs.append(subprocess.Popen([_cli(), "compress", str(src), str(dst)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    outs = [p.communicate(timeout=300) for p in procs]
    assert all(p.returncode == 0 for p in procs), outs
    got = {n: open(dst / n, "rb").read() for n in sorted(os.listdir(dst)) if n.endswith(".zwz")}
    assert {n: {"size": len(b), "sha256": sha(b)} for n, b in got.items()} == run["shards"]
    assert not [n for n in os.listdir(dst) if n.startswith(stem)]             # this run id's files are gone, stale ones included


def test_cli_reports_a_failed_rank(tmp_path):
    """Rank 0 must not report success when another rank failed (round 1: return codes of other ranks were ignored)."""
    src = tmp_path / "data" / "src"
    _write_tree(str(src))
    dst = tmp_path / "zwz"
    procs = []
    for r in range(2):
        env = dict(os.environ, ZWZ_RANK=str(r), ZWZ_NRANKS="2", ZWZ_DEVICE="0" if r == 0 else "4711", ZWZ_RENDEZVOUS_TIMEOUT="60")
        if r == 1:
            env["HIP_VISIBLE_DEVICES"] = "-1"                                # rank 1 finds no GPU: zwz_ctx_create fails
        procs.append(subprocess.Popen([_cli(), "compress", str(src), str(dst)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    outs = [p.communicate(timeout=300) for p in procs]
    assert procs[1].returncode != 0, outs[1]
    assert procs[0].returncode != 0 and "rank 1 failed" in outs[0][1], outs[0]


# ---------------------------------------------------------------------------------------------- opt-in loss-free mode
def test_lossless_chunk_size_roundtrips_incompressible_files(zwz, oracle, tmp_path):
    """SURVEY.md section 8 f4, opt-in: with 65 509-byte chunks no level-6 stream exceeds the reference's 65 535-byte payload buffer
    (compression.cpp:127-132), so incompressible files come back whole with a matching MD5 -- from this decoder AND from
    the reference's own, which reads the unchanged container.  The default stays bit-exact (every other test)."""
    src = tmp_path / "data" / "src"
    src.mkdir(parents=True)
    files = {"r1.bin": corpus.random_bytes(71, 262144), "r2.bin": corpus.random_bytes(72, 65509), "r3.bin": corpus.random_bytes(73, 65535),
             "r4.bin": corpus.random_bytes(74, 2 * 65509), "t.txt": corpus.text_like(75, 150000), "e.bin": b""}
    for n, d in files.items():
        (src / n).write_bytes(d)
    rec = tmp_path / "list.txt"
    rec.write_text("".join(n + "\n" for n in files))
    c = zwz.Codec(0, 256)
    try:
        lossy, loss_free = tmp_path / "lossy", tmp_path / "lossfree"
        lossy.mkdir(); loss_free.mkdir()
        c.do_compression(str(src), str(lossy), str(rec), 0, 1)
        c.set_chunk_size(zwz.LOSSLESS_CHUNK_SIZE)
        c.do_compression(str(src), str(loss_free), str(rec), 0, 1)
        c.set_chunk_size(0)
        b1, b2 = tmp_path / "b1", tmp_path / "b2"
        b1.mkdir(); b2.mkdir()
        assert c.do_decompression(str(lossy), str(b1)) == 3                   # the reference's behaviour: r1, r3, r4 come back short (r2 = 65509 B just fits)
        assert c.do_decompression(str(loss_free), str(b2)) == 0
        for n, d in files.items():
            assert open(b2 / n, "rb").read() == d, n
        import zwz_records
        recs = zwz_records.parse(open(loss_free / "compressed_0.zwz", "rb").read())
        assert max(len(r[3]) for r in recs) == 65535 and [r[1] for r in recs if r[0] == b"r4.bin"] == [0, 1, 2]   # 65509 + 65509 + empty
        for r in recs:                                                        # every payload is the oracle's stream of its 65 509-byte chunk
            data = files[r[0].decode()]
            assert r[3] == oracle.payload(data[r[1] * 65509:(r[1] + 1) * 65509])
    finally:
        c.close()
    ref = os.path.join(ROOT, "oracle", "_ref", "main")
    if os.path.exists(ref):                                                   # the reference's own decoder reads the loss-free shard
        b3 = tmp_path / "b3"
        r = subprocess.run([ref, "decompress", str(loss_free), str(b3)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "MD5 mismatch" not in r.stderr
        for n, d in files.items():
            assert open(b3 / n, "rb").read() == d, n


def test_lossless_env_switch_through_the_cli(tmp_path):
    src = tmp_path / "data" / "src"
    src.mkdir(parents=True)
    data = corpus.random_bytes(81, 200000)
    (src / "r.bin").write_bytes(data)
    dst, back = tmp_path / "zwz", tmp_path / "back"
    env = dict(os.environ, ZWZ_LOSSLESS="1")
    r = subprocess.run([_cli(), "compress", str(src), str(dst)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([_cli(), "decompress", str(dst), str(back)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "MD5 mismatch" not in r.stderr
    assert open(back / "r.bin", "rb").read() == data


def test_cli_rccl_collectives_single_rank(golden_dir, tmp_path):
    """csrc/main.cpp's RCCL path (list contents broadcast, status all-reduce, decompress all-gather) needs a GPU per rank, so a
    1-GPU box can only run it as a communicator of ONE rank (ZWZ_COMM=rccl forces it on): every RCCL call is made, the
    shard must still be the reference's.  With N > 1 ranks on N GPUs the same code runs with real peers."""
    run = json.load(open(os.path.join(golden_dir, "tree.json")))["runs"]["1"]
    src = tmp_path / "data" / "src"
    _write_tree(str(src))
    rec = tmp_path / "list.txt"
    rec.write_text(run["sorted_list"])
    dst, back = tmp_path / "zwz", tmp_path / "back"
    env = dict(os.environ, ZWZ_COMM="rccl", ZWZ_VERBOSE="1", ZWZ_FILE_RECORD=str(rec), ZWZ_GATHER="1")   # (+ the shard gather: sizes all-gathered, nothing to send with one rank)
    r = subprocess.run([_cli(), "compress", str(src), str(dst)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "over RCCL" in r.stderr and "shard gather over RCCL done" in r.stderr, r.stderr
    got = {n: open(dst / n, "rb").read() for n in sorted(os.listdir(dst))}
    assert {n: {"size": len(b), "sha256": sha(b)} for n, b in got.items()} == run["shards"]
    r = subprocess.run([_cli(), "decompress", str(dst), str(back)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "job status 0 over RCCL" in r.stderr, r.stderr
    for rel, want in run["decoded"].items():
        b = open(back / rel, "rb").read()
        assert {"size": len(b), "sha256": sha(b)} == want, rel


def test_parallel_consumers_write_records_out_of_order(zwz, tmp_path, monkeypatch):
    """SURVEY.md section 8 f4, opt-in: ZWZ_CONSUMERS=k emits a file's chunks the way k consumers might finish them (runs of k back to
    front, the file's last chunk behind all its others).  Same records as the default shard, in another order; this decoder
    and the reference's own (decompression.cpp:119-153 puts chunks back by sequence_id) restore the tree with matching MD5s."""
    import zwz_records
    src = tmp_path / "data" / "src"
    src.mkdir(parents=True)
    files = {"a.txt": corpus.text_like(81, 400000), "b.bin": corpus.low_entropy(82, 3 * 65535), "c.txt": corpus.text_like(83, 70000), "d.bin": corpus.skewed(84, 1000), "e.bin": b""}
    for n, d in files.items():
        (src / n).write_bytes(d)
    rec = tmp_path / "list.txt"
    rec.write_text("".join(n + "\n" for n in files))
    plain, mixed = tmp_path / "plain", tmp_path / "mixed"
    plain.mkdir(); mixed.mkdir()
    c = zwz.Codec(0, 256)
    try:
        c.do_compression(str(src), str(plain), str(rec), 0, 1)
        monkeypatch.setenv("ZWZ_CONSUMERS", "3")
        c.do_compression(str(src), str(mixed), str(rec), 0, 1)
        monkeypatch.delenv("ZWZ_CONSUMERS")
        r0 = zwz_records.parse(open(plain / "compressed_0.zwz", "rb").read())
        r1 = zwz_records.parse(open(mixed / "compressed_0.zwz", "rb").read())
        assert sorted(r0) == sorted(r1) and r0 != r1                           # the same records, another order
        seqs = [r[1] for r in r1 if r[0] == b"a.txt"]
        assert seqs[:6] == [2, 1, 0, 5, 4, 3] and seqs[-1] == max(seqs)        # runs of three back to front; the last chunk last
        back = tmp_path / "back"
        back.mkdir()
        assert c.do_decompression(str(mixed), str(back)) == 0
        for n, d in files.items():
            assert open(back / n, "rb").read() == d, n
    finally:
        c.close()
    ref = os.path.join(ROOT, "oracle", "_ref", "main")
    if os.path.exists(ref):
        b3 = tmp_path / "b3"
        r = subprocess.run([ref, "decompress", str(mixed), str(b3)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "MD5 mismatch" not in r.stderr and r.stdout.count("MD5 match") == len(files)
        for n, d in files.items():
            assert open(b3 / n, "rb").read() == d, n


def test_a_path_that_occurs_twice_in_a_shard_is_written_in_shard_order(zwz, codec, golden_dir, tmp_path):
    """A shard may hold a path as two instances (finalised, then seen again -- duplicate lines in the file list).  The reference
    takes records strictly in shard order: the second instance truncates and rewrites the file.  Here files are written by
    concurrent tasks, so instances that share a path are taken out of the concurrency: the tree must be the one
    a single instance gives, each instance verified."""
    import zwz_records
    good = open(os.path.join(golden_dir, "tree_N1", "compressed_0.zwz"), "rb").read()
    recs = zwz_records.parse(good)
    twice = [r for r in recs if r[0] in (b"hello.txt", b"text100k.txt")]
    assert len(twice) >= 3
    blob = zwz_records.serialise(recs + twice + [r for r in recs if r[0] == b"hello.txt"])
    src, out = tmp_path / "in", tmp_path / "out"
    src.mkdir(); out.mkdir()
    (src / "compressed_0.zwz").write_bytes(blob)
    want = json.load(open(os.path.join(golden_dir, "tree.json")))["runs"]["1"]
    bad = codec.do_decompression(str(src), str(out))
    assert _tree_of(str(out)) == want["decoded"]
    plain = tmp_path / "plain_in"; plain_out = tmp_path / "plain_out"
    plain.mkdir(); plain_out.mkdir()
    (plain / "compressed_0.zwz").write_bytes(good)
    assert bad == codec.do_decompression(str(plain), str(plain_out))          # the repeated files verify: no further mismatches


def test_cli_two_ranks_one_shard_with_a_repeated_path(golden_dir, tmp_path):
    """ONE shard for two ranks is split into record ranges -- unless a path occurs in it twice: the later instance must be written
    over the earlier in shard order, which ranks writing their ranges side by side cannot promise, so rank 0 decodes such a shard
    whole and the others only keep the exchanges company.  The tree must be what a single instance of every file gives."""
    import zwz_records
    good = open(os.path.join(golden_dir, "tree_N1", "compressed_0.zwz"), "rb").read()
    recs = zwz_records.parse(good)
    twice = [r for r in recs if r[0] in (b"hello.txt", b"text100k.txt")]
    zdir = tmp_path / "zwz"
    zdir.mkdir()
    (zdir / "compressed_0.zwz").write_bytes(zwz_records.serialise(recs + twice))
    run = json.load(open(os.path.join(golden_dir, "tree.json")))["runs"]["1"]
    back = tmp_path / "back"
    procs = []
    for r in range(2):
        env = dict(os.environ, ZWZ_RANK=str(r), ZWZ_NRANKS="2", ZWZ_DEVICE="0", ZWZ_RENDEZVOUS_TIMEOUT="120")
        procs.append(subprocess.Popen([_cli(), "decompress", str(zdir), str(back)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    outs = [p.communicate(timeout=300) for p in procs]
    assert all(p.returncode == 0 for p in procs), outs
    for rel, want in run["decoded"].items():
        b = open(back / rel, "rb").read()
        assert {"size": len(b), "sha256": sha(b)} == want, rel
    assert sum(o[1].count("MD5 mismatch for file:") for o in outs) == run["md5_mismatches"]      # the repeated files verify


# ---------------------------------------------------------------------------------------------- idle ranks
def _two_file_job(tmp_path):
    """A source tree of two files and its size-descending list: under three ranks the third has nothing to do."""
    src = tmp_path / "data" / "src"
    src.mkdir(parents=True)
    (src / "big.txt").write_bytes(corpus.text_like(71, 150_000))
    (src / "small.bin").write_bytes(corpus.random_bytes(72, 70_000))
    rec = tmp_path / "list.txt"
    rec.write_text("big.txt\nsmall.bin\n")
    return src, rec


def test_compress_dir_idle_rank_writes_nothing(codec, oracle, tmp_path):
    """main.cpp:44-51: a rank whose index is not below the number of listed files compresses nothing and creates NO shard.
    Through the HIP library (the CPU tests check the same guard with the oracle as codec)."""
    src, rec = _two_file_job(tmp_path)
    dst, want = tmp_path / "dst", tmp_path / "want"
    dst.mkdir()
    want.mkdir()
    for r in range(3):
        codec.do_compression(str(src), str(dst), str(rec), r, 3)            # rank 2: returns ZWZ_OK (no exception) ...
        assert oracle.compress_shard(str(src), str(want), str(rec), r, 3) == 0
    assert sorted(os.listdir(dst)) == ["compressed_0.zwz", "compressed_1.zwz"]      # ... and leaves no compressed_2.zwz
    for n in os.listdir(dst):
        assert open(dst / n, "rb").read() == open(want / n, "rb").read(), n
    codec.do_compression(str(src), str(dst), str(rec), 7, 8)                 # far beyond the list
    assert sorted(os.listdir(dst)) == ["compressed_0.zwz", "compressed_1.zwz"]


def test_cli_three_ranks_two_files_third_rank_is_idle(oracle, tmp_path):
    """`main compress` as three ranks over a two-file list: two shards, byte-identical with the oracle's three-rank run, the
    third rank prints the reference's "No file to compress" (main.cpp:50) and the job exits 0."""
    src, rec = _two_file_job(tmp_path)
    dst, want = tmp_path / "zwz", tmp_path / "want"
    want.mkdir()
    for r in range(3):
        assert oracle.compress_shard(str(src), str(want), str(rec), r, 3) == 0
    assert sorted(os.listdir(want)) == ["compressed_0.zwz", "compressed_1.zwz"]
    procs = []
    for r in range(3):
        env = dict(os.environ, ZWZ_RANK=str(r), ZWZ_NRANKS="3", ZWZ_DEVICE="0", ZWZ_FILE_RECORD=str(rec), ZWZ_RENDEZVOUS_TIMEOUT="120")
        procs.append(subprocess.Popen([_cli(), "compress", str(src), str(dst)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    outs = [p.communicate(timeout=300) for p in procs]
    assert all(p.returncode == 0 for p in procs), outs
    assert "Rank: 2 - No file to compress" in outs[2][0]
    assert "No file to compress" not in outs[0][0] and "No file to compress" not in outs[1][0]
    assert sorted(os.listdir(dst)) == ["compressed_0.zwz", "compressed_1.zwz"]      # no third shard, no markers left
    for n in os.listdir(dst):
        assert open(dst / n, "rb").read() == open(want / n, "rb").read(), n
    # and the two shards decode, as three ranks again (fewer shards than ranks: each shard's records are split three ways), to the tree
    # the oracle decodes
    back, wback = tmp_path / "back", tmp_path / "wback"
    wback.mkdir()
    for n in sorted(os.listdir(want)):
        oracle.decompress_shard(str(want / n), str(wback))
    procs = []
    for r in range(3):
        env = dict(os.environ, ZWZ_RANK=str(r), ZWZ_NRANKS="3", ZWZ_DEVICE="0", ZWZ_RENDEZVOUS_TIMEOUT="120")
        procs.append(subprocess.Popen([_cli(), "decompress", str(dst), str(back)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    outs = [p.communicate(timeout=300) for p in procs]
    assert all(p.returncode == 0 for p in procs), outs
    assert _tree_of(str(back)) == _tree_of(str(wback))


# ---------------------------------------------------------------------------------------------- the multi-rank bench path
def test_bench_two_ranks_rehearsal_on_one_gpu(tmp_path):
    """bench.py's N > 1 path (launcher, communicator self-check, per-rank times, job-wide verification) as two ranks on this
    box's one GPU over gloo -- the same code the driver's --gpus 8 run goes through, minus RCCL (main.cpp:24-41,131,144 are
    the collectives it stands in for).  Not a measurement."""
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--gpus", "2", "--rehearse-on-one-gpu", "--files", "200", "--steps", "2",
                        "--warmup", "1", "--no-cpu-baseline", "--max-batch", "2048", "--oracle-sample", "64"],
                       capture_output=True, text=True, timeout=900, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["comm"]["ranks_seen"] == 2 and d["comm"]["backend"] == "gloo"
    assert len(d["ms_per_step_by_rank"]) == 2 and all(t > 0 for t in d["ms_per_step_by_rank"])
    assert d["verified"]["ok"] and d["verified"]["ranks_failed"] == 0
    assert d["random"]["verified"]["ok"] and len(d["random"]["ms_per_step_by_rank"]) == 2        # (the line's own fields are the text configuration's)
    assert d["value"] > 0 and d["value"] == d["value_text"] and d["value_random"] == d["random"]["value"] and d["scaling"] == "weak"
    assert "e2e" not in d                                                                            # the CLI legs are a one-rank affair


def test_bench_plain_run_is_lean_and_dumps_the_timed_outputs(oracle, tmp_path):
    """A plain bench.py run times the headline (text) workload only and prints the headline fields, nothing of --full; with
    --dump-outputs the sampled chunks on disk are the oracle's payloads of the workload's own input bytes and decode back to them."""
    import sys
    import workloads
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--files", "200", "--steps", "3", "--warmup", "1",
                        "--max-batch", "2048", "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0 and d["unit"] == "GB/s"
    assert d["higher_is_better"] is True and d["dtype"] == "u8" and d["metric"].startswith("compress+decompress GB/s")
    assert not {"verified", "random", "e2e", "roofline", "cpu_baseline", "stage_ms_per_pass"} & set(d)
    files = sorted(os.listdir(out))
    assert files and all(f.startswith("text_") for f in files) and sum(os.path.getsize(out / f) for f in files) <= 64 << 20
    dump = {f[len("text_"):-4]: np.load(out / f) for f in files}
    per_file = 262144 // CHUNK + 1
    assert (dump["chunk_index"] == np.arange(200 * per_file)).all() and (dump["inflate_status"] == 0).all()
    for j, k in enumerate(dump["sample_index"].astype(np.int64)):
        f, part = divmod(int(k), per_file)
        chunk = corpus.text_like(workloads.TEXT_SEED0 + f, 262144)[part * CHUNK:(part + 1) * CHUNK]
        plen, blen = int(dump["payload_len"][k]), int(dump["decoded_len"][k])
        assert dump["payload_sample"][j, :plen].astype(np.uint8).tobytes() == oracle.payload(chunk), k
        assert blen == len(chunk) and dump["decoded_sample"][j, :blen].astype(np.uint8).tobytes() == chunk, k
