"""zwz_inflate_split_streams_dev on the GPU: the corpora of tests/stream_corpus.py and tests/split_corpus.py in shuffled mixed batches
against libz (tests/stream_ref.py), canary bytes around every output range, in both block-header forms; d_segments against how the
streams were made; agreement, stream by stream, with zwz_inflate_streams_dev in the same process on bytes, length and status; one
1 GiB text stream and one of 256 MiB random bytes written by Codec.deflate_streams_dev and read back; 64 x 16 MiB; pieces that meet
at every alignment mod 16; Codec.inflate_stream; invalid arguments; the file function and `main gunzip`: round trips over several
slices in all three wrappers, a file Python's gzip module wrote, empty files, cut and damaged files, destinations that cannot be written.

A stream of p pieces reports p + 1 segments: what follows the last marker -- the empty final block and nothing else in the streams
this codec writes -- is a chain segment of its own."""
import gzip
import importlib
import os
import random
import subprocess
import zlib

import numpy as np
import pytest

import corpus as kinds
import deflate_stream_ref
import split_corpus
import stream_corpus
import stream_ref
from stream_batch import CANARY, GAP, run_batch

pytestmark = pytest.mark.gpu

PKG = "parallel-data-compression-and-decompression_amd"
PIECE = deflate_stream_ref.PIECE


@pytest.fixture(scope="module")
def z():
    return importlib.import_module(PKG)


@pytest.fixture(scope="module")
def torch_first():
    """torch brings its own HIP runtime: it must have opened the GPU before a Codec does."""
    import torch
    torch.zeros(1, device="cuda")
    return torch


@pytest.fixture(scope="module")
def codec(z, torch_first):
    c = z.Codec(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def corpora():
    """{wrap: [(name, data, cap, group, chain, item)]}: both corpora"""
    out = {w: [] for w in (stream_ref.RAW, stream_ref.ZLIB, stream_ref.GZIP)}
    for w, streams in stream_corpus.corpus(2026, big=True).items():
        out[w] += [(s.name, s.data, s.cap, "s", 0, None) for s in streams]
    for it in split_corpus.corpus(2027, big=True):
        out[it.wrap].append((it.name, it.data, it.cap, it.group, it.chain, it))
    return out


@pytest.mark.parametrize("header", ["wave", "serial"])
@pytest.mark.parametrize("min_bytes", [split_corpus.MIN_BYTES, 0])
@pytest.mark.parametrize("wrap", ["raw", "zlib", "gzip"])
def test_corpora_mixed_batch(codec, torch_first, corpora, wrap, header, min_bytes):
    w = stream_ref.WRAPS[wrap]
    items = list(corpora[w])
    random.Random(len(items) + min_bytes).shuffle(items)
    streams, caps = [x[1] for x in items], [x[2] for x in items]
    codec.set_option("inflate_header", header)
    codec.set_option("split_min_bytes", str(min_bytes))
    try:
        st, out, seg = run_batch(codec, torch_first, wrap, streams, caps)
        st1, out1, _ = run_batch(codec, torch_first, wrap, streams, caps, split=False)
    finally:
        codec.set_option("inflate_header", "")
        codec.set_option("split_min_bytes", "")
    bad, fell_back, n_split, n_expected = [], [], 0, 0
    for i, (name, data, cap, group, chain, it) in enumerate(items):
        why = stream_ref.accept(w, data, cap, st[i], out[i])
        if why:
            bad.append("%s: %s" % (name, why))
        if (st[i], out[i]) != (st1[i], out1[i]):
            bad.append("%s: status %d, %d bytes; zwz_inflate_streams_dev: status %d, %d bytes%s" % (
                name, st[i], len(out[i]), st1[i], len(out1[i]), "" if len(out[i]) != len(out1[i]) else ", other bytes"))
        if group == "a":
            want = split_corpus.expected_segments(it, min_bytes)
            if seg[i] != want:
                (fell_back if want and not seg[i] else bad).append("%s: %d segments, %d expected" % (name, seg[i], want))
            n_split += seg[i] > 0
            n_expected += want > 0
        elif group == "s":
            if seg[i] < 0:
                bad.append("%s: segments not written" % name)
        elif seg[i] not in (0, chain):
            bad.append("%s: %d segments, 0 or %d expected" % (name, seg[i], chain))
    assert not fell_back, "clean split streams fell back: %s" % fell_back[:20]
    assert not bad, "%d of %d:\n%s" % (len(bad), len(items), "\n".join(bad[:40]))
    assert n_split == n_expected and n_expected > 0, (n_split, n_expected)     # (the batch does hold streams that must split)


def _deflate_on_gpu(z, codec, torch, d_src, lens, wrap):
    """len(lens) inputs laid out one after the other in d_src (16-byte aligned starts) -> (d_comp, offs, comp lens)"""
    dev = d_src.device
    n = len(lens)
    in_off = np.zeros(n, dtype=np.int64)
    in_off[1:] = np.cumsum((np.array(lens[:-1], dtype=np.int64) + 15) // 16 * 16)
    caps = np.array([(z.deflate_stream_bound(int(k), wrap) + 15) // 16 * 16 for k in lens], dtype=np.int64)
    out_off = np.zeros(n, dtype=np.int64)
    out_off[1:] = np.cumsum(caps[:-1])
    d_comp = torch.zeros(int(caps.sum()) + 16, dtype=torch.uint8, device=dev)
    d_olen = torch.zeros(n, dtype=torch.int64, device=dev)
    d_st = torch.full((n,), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    codec.deflate_streams_dev(wrap, d_src, in_off, np.array(lens, dtype=np.int64), d_comp, out_off, caps, d_olen, d_st)
    codec.sync()
    assert (d_st.cpu().numpy() == 0).all()
    return d_comp, in_off, out_off, d_olen.cpu().numpy()


def _read_back(z, codec, torch, d_src, lens, wrap):
    dev = d_src.device
    n = len(lens)
    d_comp, in_off, c_off, c_len = _deflate_on_gpu(z, codec, torch, d_src, lens, wrap)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    results = []
    for split in (True, False) if n > 1 else (True,):
        d_back = torch.full((int(d_src.numel()) + 16,), CANARY, dtype=torch.uint8, device=dev)
        d_olen = torch.full((n,), -1, dtype=torch.int64, device=dev)
        d_st = torch.full((n,), -1, dtype=torch.int32, device=dev)
        d_seg = torch.full((n,), -1, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        args = (wrap, d_comp, t(c_off), t(c_len), d_back, t(in_off), t(np.array(lens, dtype=np.int64)), d_olen, d_st)
        if split:
            codec.inflate_split_streams_dev(*args, d_seg)
        else:
            codec.inflate_streams_dev(*args)
        codec.sync()
        assert (d_st.cpu().numpy() == 0).all(), d_st.cpu().numpy()
        assert (d_olen.cpu().numpy() == np.array(lens)).all()
        for i in range(n):
            assert torch.equal(d_back[in_off[i]:in_off[i] + lens[i]], d_src[in_off[i]:in_off[i] + lens[i]]), i
            end = in_off[i] + lens[i]
            nxt = in_off[i + 1] if i + 1 < n else end + 16
            assert bool((d_back[end:nxt] == CANARY).all()), "bytes written behind stream %d" % i
        results.append([int(x) for x in d_seg.cpu().numpy()])
    return results[0]


def _text_on_gpu(torch, n, seed):
    base = torch.from_numpy(np.frombuffer(kinds.text_like(seed, 32 << 20), dtype=np.uint8).copy()).cuda()
    reps = [torch.roll(base, 7919 * (r + 1)) for r in range((n + base.numel() - 1) // base.numel())]
    return torch.cat(reps)[:n].contiguous()


@pytest.mark.parametrize("wrap", ["gzip", "zlib"])
def test_one_gib_text_stream(z, codec, torch_first, wrap):
    n = 1 << 30
    d_src = _text_on_gpu(torch_first, n, 7)
    seg = _read_back(z, codec, torch_first, d_src, [n], wrap)
    assert seg == [-(-n // PIECE) + 1]


def test_256_mib_random_stream(z, codec, torch_first):
    n = 256 << 20
    g = torch_first.Generator(device="cuda")
    g.manual_seed(5)
    d_src = torch_first.randint(0, 256, (n,), dtype=torch_first.uint8, device="cuda", generator=g)
    seg = _read_back(z, codec, torch_first, d_src, [n], "raw")
    assert seg == [-(-n // PIECE) + 1]


def test_64_streams_of_16_mib(z, codec, torch_first):
    n = 16 << 20
    d_src = _text_on_gpu(torch_first, 64 * n, 9)
    seg = _read_back(z, codec, torch_first, d_src, [n] * 64, "gzip")
    assert seg == [-(-n // PIECE) + 1] * 64


def test_pieces_meet_at_every_alignment(codec, torch_first):
    """Pieces of 65 521 + r decoded bytes: neighbours meet at every output address mod 16, and their compressed starts fall where
    they fall.  No byte of a neighbour may be touched: the result is exact and the canaries stand."""
    streams, srcs = [], []
    for r in range(16):
        src = kinds.text_like(40 + r, 5 * (65521 + r) + r)
        data, pieces = split_corpus.flushed(src, 65521 + r, 6, stream_ref.ZLIB)
        streams.append(data); srcs.append((src, pieces))
    st, out, seg = run_batch(codec, torch_first, "zlib", streams, [len(s) for s, _ in srcs])
    for i, (src, pieces) in enumerate(srcs):
        assert st[i] == 0 and out[i] == src and seg[i] == pieces, (i, st[i], seg[i], pieces)


def test_hostile_markers(codec, torch_first):
    plain = split_corpus.MARKER * (2 << 20)
    data = split_corpus._wrapped(stream_ref.ZLIB, split_corpus._stored(plain, final=True), plain)
    for opts in (("", ""), ("4096", str(1 << 23))):
        codec.set_option("split_budget", opts[0]); codec.set_option("split_max_candidates", opts[1])
        try:
            st, out, seg = run_batch(codec, torch_first, "zlib", [data], [len(plain)])
        finally:
            codec.set_option("split_budget", ""); codec.set_option("split_max_candidates", "")
        assert (st, seg) == ([0], [0]) and out[0] == plain


def test_inflate_stream_bytes(z, codec, torch_first):
    src = kinds.text_like(21, 3000000)
    for wrap in ("gzip", "zlib", "raw"):
        data = deflate_stream_ref.deflate_stream(src, wrap)
        assert codec.inflate_stream(data, wrap) == src
        assert codec.inflate_stream(data, wrap, out_size=len(src)) == src
    one = zlib.compress(src)                                    # nothing to split: the one-wave path
    assert codec.inflate_stream(one, "zlib") == src
    with pytest.raises(z.ZwzError) as e:
        codec.inflate_stream(deflate_stream_ref.deflate_stream(src, "gzip")[:-9], "gzip")
    assert e.value.stream_status == stream_ref.NEED_INPUT
    with pytest.raises(z.ZwzError) as e:
        bad = bytearray(deflate_stream_ref.deflate_stream(src, "gzip")); bad[-6] ^= 1
        codec.inflate_stream(bytes(bad), "gzip", out_size=len(src))
    assert e.value.stream_status == stream_ref.CHECKSUM


def test_invalid_arguments(z, codec, torch_first):
    torch = torch_first
    L = z.lib()
    d = torch.zeros(64, dtype=torch.uint8, device="cuda")
    i64 = torch.zeros(1, dtype=torch.int64, device="cuda")
    i32 = torch.zeros(1, dtype=torch.int32, device="cuda")
    ok = lambda wrap, din, dout, n=1: L.zwz_inflate_split_streams_dev(codec.handle, wrap, din, i64.data_ptr(), i64.data_ptr(), n, dout, i64.data_ptr(),
                                                                       i64.data_ptr(), i64.data_ptr(), i32.data_ptr(), None)
    assert ok(3, d.data_ptr(), d.data_ptr()) == z.E_INVALID
    assert ok(2, d.data_ptr() + 8, d.data_ptr()) == z.E_INVALID
    assert ok(2, d.data_ptr(), d.data_ptr() + 4) == z.E_INVALID
    assert ok(2, None, d.data_ptr()) == z.E_INVALID
    assert ok(2, None, None, 0) == 0
    assert L.zwz_inflate_split_streams_dev(None, 2, d.data_ptr(), i64.data_ptr(), i64.data_ptr(), 1, d.data_ptr(), i64.data_ptr(), i64.data_ptr(),
                                           i64.data_ptr(), i32.data_ptr(), None) == z.E_INVALID
    for name, value in (("split_budget", "x"), ("split_budget", "3"), ("split_max_candidates", "1"), ("split_min_bytes", "-1")):
        with pytest.raises(z.ZwzError):
            codec.set_option(name, value)
    codec.sync()


# ---- zwz_inflate_stream_file and `main gunzip` ----------------------------------------------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_IO = -4                           # ZWZ_E_IO (include/zwz.h); the package names only the codes its own callers test for
SLICE = 4 << 20                     # compressed bytes a slice: the 40 MB file below is 5 to 7 slices in every wrapper
DECODE = {"gzip": gzip.decompress, "zlib": zlib.decompress, "raw": lambda b: zlib.decompressobj(-15).decompress(b)}


def _file_data():
    return b"".join(kinds.text_like(70 + i, 4 << 20) for i in range(8)) + kinds.random_bytes(79, (8 << 20) + 3)


@pytest.fixture()
def small_slices(codec):
    codec.set_option("split_slice_bytes", str(SLICE))
    yield codec
    codec.set_option("split_slice_bytes", "")


@pytest.mark.parametrize("wrap", ["raw", "zlib", "gzip"])
def test_file_round_trip(small_slices, tmp_path, wrap):
    codec = small_slices
    data = _file_data()
    src, comp, back = tmp_path / "big", tmp_path / "big.z", tmp_path / "big.back"
    src.write_bytes(data)
    codec.deflate_stream_file(str(src), str(comp), wrap=wrap)
    assert comp.stat().st_size >= 3 * SLICE
    codec.inflate_stream_file(str(comp), str(back), wrap=wrap)
    got = back.read_bytes()
    assert got == DECODE[wrap](comp.read_bytes()) and got == data
    assert not (tmp_path / "big.back.part").exists()
    # an empty input's stream, and one piece exactly
    for n in (0, PIECE, PIECE + 1):
        src.write_bytes(data[:n])
        codec.deflate_stream_file(str(src), str(comp), wrap=wrap)
        codec.inflate_stream_file(str(comp), str(back), wrap=wrap)
        assert back.read_bytes() == data[:n]


def test_file_from_pythons_gzip_falls_back(small_slices, tmp_path):
    """One window, no flush points, longer than a slice: no piece ends in the first slice, nothing has been written, so the file goes
    through the one-stream path.  Also two members, which only that path reads."""
    codec = small_slices
    data = kinds.text_like(5, 14 << 20)
    p, back = tmp_path / "py.gz", tmp_path / "py.out"
    with gzip.open(p, "wb", compresslevel=6) as f:
        f.write(data)
    assert p.stat().st_size > SLICE
    codec.inflate_stream_file(str(p), str(back))
    assert back.read_bytes() == data
    p.write_bytes(gzip.compress(data[:100000]) + gzip.compress(data[100000:300000]))
    codec.inflate_stream_file(str(p), str(back))
    assert back.read_bytes() == data[:300000]
    p.write_bytes(zlib.compress(data[:500000]))
    codec.inflate_stream_file(str(p), str(back), wrap="zlib")
    assert back.read_bytes() == data[:500000]


def test_file_damage_and_failures(z, small_slices, tmp_path):
    codec = small_slices
    data = _file_data()
    src, comp, back = tmp_path / "big", tmp_path / "big.gz", tmp_path / "big.back"
    src.write_bytes(data)
    codec.deflate_stream_file(str(src), str(comp))
    good = comp.read_bytes()

    def fails(blob, status, wrap="gzip", path=None):
        bad = tmp_path / "bad.gz"
        bad.write_bytes(blob)
        with pytest.raises(z.ZwzError) as e:
            codec.inflate_stream_file(str(bad), str(path or back), wrap=wrap)
        assert e.value.status == status, (e.value.status, str(e.value))
        assert not (path or back).exists() and not os.path.exists(str(path or back) + ".part")
        return str(e.value)

    msg = fails(good[:SLICE + SLICE // 2], z.E_FORMAT)                          # cut in the second slice
    assert "offset" in msg
    crc = bytearray(good); crc[-7] ^= 0x10
    fails(bytes(crc), z.E_CHECKSUM)                                             # a wrong CRC-32
    isz = bytearray(good); isz[-2] ^= 1
    fails(bytes(isz), z.E_CHECKSUM)                                             # a wrong ISIZE
    fails(good[:-3], z.E_FORMAT)                                                # cut inside the trailer
    flip = bytearray(good); flip[3 * SLICE + 12345] ^= 0x40
    with pytest.raises(z.ZwzError) as e:                                        # a bit flipped in the fourth slice: a broken chain or a wrong checksum
        (tmp_path / "bad.gz").write_bytes(bytes(flip))
        codec.inflate_stream_file(str(tmp_path / "bad.gz"), str(back))
    assert e.value.status in (z.E_FORMAT, z.E_CHECKSUM) and not back.exists() and not os.path.exists(str(back) + ".part")
    fails(good + b"junk", z.E_FORMAT)                                           # bytes behind the member
    fails(b"", z.E_FORMAT)                                                      # an empty file is no stream
    fails(good, z.E_FORMAT, wrap="zlib")                                        # another wrapper
    codec.inflate_stream_file(str(comp), str(back))                             # zero padding behind the member is fine
    (tmp_path / "pad.gz").write_bytes(good + bytes(100))
    codec.inflate_stream_file(str(tmp_path / "pad.gz"), str(back))
    assert back.read_bytes() == data
    back.unlink()
    nowhere = tmp_path / "no" / "such" / "dir" / "out"
    fails(good, E_IO, path=nowhere)             # an unwritable destination
    with pytest.raises(z.ZwzError):
        codec.inflate_stream_file(str(tmp_path / "missing"), str(back))
    assert not back.exists() and not os.path.exists(str(back) + ".part")
    L = z.lib()
    assert L.zwz_inflate_stream_file(codec.handle, 3, b"a", b"b") == z.E_INVALID
    assert L.zwz_inflate_stream_file(codec.handle, 2, None, b"b") == z.E_INVALID
    assert L.zwz_inflate_stream_file(None, 2, b"a", b"b") == z.E_INVALID
    for value in ("100", "x", str((1 << 28) + 16)):
        with pytest.raises(z.ZwzError):
            codec.set_option("split_slice_bytes", value)
    codec.inflate_stream_file(str(comp), str(back))                             # the codec still works afterwards
    assert back.read_bytes() == data


def test_cli_gzip_gunzip(tmp_path):
    cli = os.path.join(ROOT, PKG, "main")
    data = _file_data()
    src = tmp_path / "big"
    src.write_bytes(data)
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "ZWZ_NRANKS", "OMPI_COMM_WORLD_SIZE", "PMI_SIZE")}
    env["ZWZ_SPLIT_SLICE_BYTES"] = str(SLICE)
    run = lambda *a, **kw: subprocess.run([cli] + [str(x) for x in a], capture_output=True, text=True, timeout=600, env=kw.get("env", env))
    for flags, wrap in (([], "gzip"), (["--zlib"], "zlib"), (["--raw"], "raw")):
        comp, back = tmp_path / ("big." + wrap), tmp_path / ("back." + wrap)
        r = run("gzip", src, comp, *flags)
        assert r.returncode == 0, r.stderr
        assert comp.stat().st_size >= 3 * SLICE
        r = run("gunzip", comp, back, *flags)
        assert r.returncode == 0, r.stderr
        got = back.read_bytes()
        assert got == DECODE[wrap](comp.read_bytes()) and got == data
    empty = tmp_path / "empty"
    empty.write_bytes(b"")
    assert run("gzip", empty, tmp_path / "empty.gz").returncode == 0
    r = run("gunzip", tmp_path / "empty.gz", tmp_path / "empty.back")
    assert r.returncode == 0 and (tmp_path / "empty.back").read_bytes() == b""
    cut = tmp_path / "cut.gz"
    cut.write_bytes((tmp_path / "big.gzip").read_bytes()[:SLICE + SLICE // 2])
    r = run("gunzip", cut, tmp_path / "cut.out")
    assert r.returncode == 1 and "offset" in r.stderr
    assert not (tmp_path / "cut.out").exists() and not (tmp_path / "cut.out.part").exists()
    nowhere = tmp_path / "no" / "dir" / "x"
    assert run("gunzip", tmp_path / "big.gzip", nowhere).returncode == 1 and not nowhere.exists()
    r = run("gunzip", tmp_path / "big.gzip", tmp_path / "x", "--fast")
    assert r.returncode == 1 and "gunzip <src> <dst> [--zlib|--raw]" in r.stderr
    r = run("gunzip", tmp_path / "big.gzip", tmp_path / "x", env=dict(env, WORLD_SIZE="2"))
    assert r.returncode == 1 and "single process" in r.stderr
