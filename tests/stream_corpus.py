"""The seeded corpus of zwz_inflate_streams_dev's tests: raw, zlib and gzip streams with their output capacities.  Test
infrastructure only.

corpus(seed, big=True) -> {wrap: [Stream]}, wrap in stream_ref.RAW / ZLIB / GZIP:
  - Python zlib at levels 0-9 and every strategy, windowBits 9..15 as zlib, -9..-15 as raw, 31 as gzip; Z_SYNC_FLUSH and
    Z_FULL_FLUSH in the middle of a stream
  - sizes 0, 1, 65 535, 65 536, 65 537, 1 MiB + 7 and 8 MiB (big=False: up to 65 537), a few settings each
  - hand-built gzip headers (FEXTRA with several subfields, a 3 KiB FNAME, FCOMMENT, FHCRC right and wrong, reserved flags, CM = 7)
  - gzip streams of 2, 3 and 300 members, empty members among them, 4 KiB of zeros between members; trailing garbage and a lone 1f
  - every cut inside the headers and trailers of small streams, bit flips in the CRC-32, ISIZE and Adler-32 fields
  - a second member whose first match reaches into the first; a bad CRC in one member followed by a bad ISIZE in the next
  - deflate_gen's conformance corpus as zlib and as raw (its payloads without their 2-byte header)
"""
import random
import struct
import zlib
from dataclasses import dataclass

import deflate_gen
from stream_ref import GZIP, RAW, ZLIB

STRATEGIES = [zlib.Z_DEFAULT_STRATEGY, zlib.Z_FILTERED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE, zlib.Z_FIXED]


@dataclass
class Stream:
    name: str
    data: bytes
    cap: int


def default_cap(n_in):
    return max(4 * n_in, 1 << 16)


def compress(data, level=6, wbits=15, strategy=zlib.Z_DEFAULT_STRATEGY, mem=8, flush_at=None, flush=zlib.Z_SYNC_FLUSH, zdict=None):
    c = zlib.compressobj(level, zlib.DEFLATED, wbits, mem, strategy, **({"zdict": zdict} if zdict else {}))
    if flush_at is None:
        return c.compress(data) + c.flush()
    return c.compress(data[:flush_at]) + c.flush(flush) + c.compress(data[flush_at:]) + c.flush()


def gz_member(data, level=6, flg=0, extra=b"", name=b"", comment=b"", hcrc=None, cm=8, body=None, crc=None, isize=None):
    """One gzip member written by hand: every header field explicit; hcrc None = right, an int = that value."""
    h = bytes([0x1f, 0x8b, cm, flg]) + b"\x00\x00\x00\x00" + b"\x00\xff"
    if flg & 4:
        h += struct.pack("<H", len(extra)) + extra
    if flg & 8:
        h += name + b"\x00"
    if flg & 16:
        h += comment + b"\x00"
    if flg & 2:
        h += struct.pack("<H", (zlib.crc32(h) & 0xffff) if hcrc is None else hcrc)
    if body is None:
        body = compress(data, level, -15)
    return h + body + struct.pack("<II", zlib.crc32(data) if crc is None else crc, len(data) & 0xffffffff if isize is None else isize)


def text(rng, n):
    return deflate_gen.text(rng, n)


def _flip(b, bit):
    b = bytearray(b)
    b[bit // 8] ^= 1 << (bit % 8)
    return bytes(b)


def corpus(seed=2026, big=True, n_conformance=300):
    rng = random.Random(seed)
    out = {RAW: [], ZLIB: [], GZIP: []}

    def add(wrap, name, data, cap=None):
        out[wrap].append(Stream(name, data, default_cap(len(data)) if cap is None else cap))

    # Python zlib: level x strategy x window, three wrappers
    for level in range(10):
        for strategy in STRATEGIES:
            for wb in range(9, 16):
                src = deflate_gen.mixed(rng, rng.choice([0, 100, 3000, 20000]))
                add(ZLIB, "zlib L%d s%d w%d" % (level, strategy, wb), compress(src, level, wb, strategy), len(src) + 64)
                add(RAW, "raw L%d s%d w-%d" % (level, strategy, wb), compress(src, level, -wb, strategy), len(src) + 64)
            src = deflate_gen.mixed(rng, rng.choice([0, 100, 3000, 20000]))
            add(GZIP, "gzip L%d s%d" % (level, strategy), compress(src, level, 31, strategy), len(src) + 64)
    for flush in (zlib.Z_SYNC_FLUSH, zlib.Z_FULL_FLUSH):
        for level in (1, 6, 9):
            src = deflate_gen.mixed(rng, 30000)
            for wrap, wb in ((ZLIB, 15), (RAW, -15), (GZIP, 31)):
                add(wrap, "flush %d L%d" % (flush, level), compress(src, level, wb, flush_at=rng.randrange(1, 30000), flush=flush),
                    len(src) + 16)

    # sizes
    sizes = [0, 1, 65535, 65536, 65537] + ([(1 << 20) + 7, 8 << 20] if big else [])
    for n in sizes:
        src = text(rng, n) if n < (1 << 20) else deflate_gen.mixed(rng, n)
        for level in ((0, 6) if n < (1 << 20) else (6,)):
            for wrap, wb in ((ZLIB, 15), (RAW, -15), (GZIP, 31)):
                add(wrap, "size %d L%d" % (n, level), compress(src, level, wb), n)     # the exact capacity

    # hand-built gzip headers
    src = text(rng, 5000)
    add(GZIP, "fextra", gz_member(src, flg=4, extra=b"AB\x02\x00xyCD\x00\x00EF\x05\x00hello"))
    add(GZIP, "fname 3 KiB", gz_member(src, flg=8, name=b"n" * 3072))
    add(GZIP, "fcomment", gz_member(src, flg=16, comment=b"a comment"))
    add(GZIP, "all fields + fhcrc", gz_member(src, flg=2 | 4 | 8 | 16 | 1, extra=b"QQ\x01\x00z", name=b"file.txt", comment=b"c"))
    add(GZIP, "fhcrc wrong", gz_member(src, flg=2 | 8, name=b"f", hcrc=0x1234))
    for bit in (0x20, 0x40, 0x80):
        add(GZIP, "reserved flag %x" % bit, gz_member(src, flg=bit))
    add(GZIP, "cm 7", gz_member(src, cm=7))
    add(GZIP, "not gzip", compress(src, 6, 15))
    add(GZIP, "leading zero", b"\x00" + gz_member(src))

    # members
    parts = [text(rng, rng.randrange(0, 4000)) for _ in range(300)]
    for k in (2, 3, 300):
        members = [gz_member(p, level=rng.randrange(10)) for p in parts[:k]]
        add(GZIP, "%d members" % k, b"".join(members))
    add(GZIP, "empty members", gz_member(b"") + gz_member(src) + gz_member(b"") + gz_member(b""))
    add(GZIP, "zeros between", gz_member(parts[1]) + b"\x00" * 4096 + gz_member(parts[2]) + b"\x00" * 17)
    add(GZIP, "only zeros", b"\x00" * 100)
    add(GZIP, "empty", b"")
    add(GZIP, "trailing garbage", gz_member(src) + b"garbage")
    add(GZIP, "lone 1f", gz_member(src) + b"\x1f")
    add(GZIP, "1f 8b then nothing", gz_member(src) + b"\x1f\x8b")
    add(ZLIB, "zlib trailing bytes", compress(src, 6, 15) + b"more")
    add(RAW, "raw trailing bytes", compress(src, 6, -15) + b"more")
    add(ZLIB, "fdict", bytes([0x78, 0xbb]) + b"\x00\x00\x00\x01" + compress(src, 6, -15))
    add(ZLIB, "fdict cut", bytes([0x78, 0xbb, 0, 0]))
    add(GZIP, "zlib level 0 in gzip", compress(src, 0, 31))

    # cuts inside headers and trailers of small streams
    small = text(rng, 300)
    g = gz_member(small, flg=2 | 4 | 8 | 16, extra=b"ab\x01\x00c", name=b"nm", comment=b"cm")
    z = compress(small, 6, 15)
    two = gz_member(small) + gz_member(small[:100])
    for i in range(len(g) + 1):
        if i < 40 or i > len(g) - 10:
            add(GZIP, "gzip cut %d" % i, g[:i])
    for i in list(range(0, 4)) + list(range(len(z) - 6, len(z) + 1)):
        add(ZLIB, "zlib cut %d" % i, z[:i])
    m1 = len(gz_member(small))
    for i in range(m1 - 8, m1 + 14):
        add(GZIP, "second member cut %d" % i, two[:i])

    # bit flips in the checksums and ISIZE
    for bit in range(0, 32, 5):
        add(GZIP, "crc flip %d" % bit, _flip(g, 8 * (len(g) - 8) + bit))
        add(GZIP, "isize flip %d" % bit, _flip(g, 8 * (len(g) - 4) + bit))
        add(ZLIB, "adler flip %d" % bit, _flip(z, 8 * (len(z) - 4) + bit))
    # a bad CRC in the first member, a bad ISIZE in the second: CHECKSUM (libz stops at the first)
    add(GZIP, "bad crc then bad isize", gz_member(small, crc=1) + gz_member(small, isize=7))
    add(GZIP, "bad isize then bad crc", gz_member(small, isize=7) + gz_member(small, crc=1))
    add(GZIP, "good then bad crc then data error", gz_member(small) + gz_member(small, crc=5) + gz_member(small, body=b"\xff\xff\xff"))
    # the second member's first match reaches into the first: a member starts with an empty window
    dict_body = compress(b"hello world, hello world", 6, -15, zdict=b"hello world, ")
    add(GZIP, "match into previous member", gz_member(b"hello world, ") + gz_member(b"hello world, hello world", body=dict_body))
    add(RAW, "match before the start", dict_body)

    # deflate_gen's conformance corpus
    for c in deflate_gen.conformance_corpus(seed, n_zlib=n_conformance):
        cap = len(c.data) if c.data is not None and rng.random() < 0.3 else deflate_gen.CHUNK
        add(ZLIB, "conf %s %s" % (c.group, c.name), c.payload, cap)
        add(RAW, "conf raw %s %s" % (c.group, c.name), c.payload[2:], cap)
    return out


def capacity_cases(rng):
    """(wrap, name, data, cap) pairs around the exact size: cap = size gives END, size - 1 gives OVERFLOW."""
    cases = []
    for n in (1, 1000, 65536, 300000):
        src = deflate_gen.mixed(rng, n)
        for wrap, wb in ((ZLIB, 15), (RAW, -15), (GZIP, 31)):
            for level in (0, 6):
                p = compress(src, level, wb)
                cases.append((wrap, "cap exact %d L%d" % (n, level), p, n))
                cases.append((wrap, "cap -1 %d L%d" % (n, level), p, n - 1))
    return cases
