"""The seeded corpus of zwz_inflate_split_streams_dev's tests, built with Python's zlib (libz 1.2.11) and hand-written stored
blocks in all three wrappers.  Test infrastructure only.

corpus(seed, big=True) -> [Item].  Item.group:
  "a"  clean split streams: Z_FULL_FLUSH after every k input bytes, k in {1, 100, 4 096, 65 280, 1 MiB} over corpus.KINDS at levels
       1, 6, 9 and 0; streams written by the codec's own reference (tests/deflate_stream_ref.py); two flushes in a row; a flush
       before any input; lengths 0, 1, k, k +- 1.  Item.chain is the number of pieces, known from how the stream was made:
       1 + the flush() calls that returned a marker (libz writes nothing for a repeated flush, so markers in a row are appended
       by hand as 00 00 00 ff ff, one piece each).
  "b"  must fall back and decode right: Z_SYNC_FLUSH and Z_PARTIAL_FLUSH streams of text (the pieces refer back), full flushes up to
       the middle and sync flushes after it, one-window streams, a gzip of two flushed members, a flushed member followed by garbage
  "c"  false candidates: stored blocks full of 00 00 ff ff; a stored block that holds the marker followed by a complete valid DEFLATE
       stream with a final block (a fake chain that must not be followed); 8 MiB of stored markers
  "d"  damage to streams of (a): a bit flipped in each of several pieces, cuts inside a piece, at a marker and inside the trailer, a
       wrong CRC-32 / Adler-32 / ISIZE, capacity exact, one less, 0
For (b), (c) and (d) Item.chain is the true chain's length where the stream could legitimately split, else 0; the segment count
reported must be 0 or exactly that.

expected_segments(item, min_bytes, max_candidates) is what group (a) must report: the documented rule, computed here from the
stream's bytes alone.
"""
import random
import struct
import zlib
from dataclasses import dataclass

import corpus as kinds
import deflate_stream_ref
from stream_ref import GZIP, RAW, ZLIB

MARKER = b"\x00\x00\xff\xff"
WBITS = {RAW: -15, ZLIB: 15, GZIP: 31}
HEADER = {RAW: 0, ZLIB: 2, GZIP: 10}
TRAILER = {RAW: 0, ZLIB: 4, GZIP: 8}
MIN_BYTES, BUDGET, MAX_CANDIDATES = 65536, 4 << 20, 1 << 17        # the documented defaults (include/zwz.h)


@dataclass
class Item:
    group: str
    name: str
    wrap: int
    data: bytes
    cap: int
    chain: int


def flushed(src, k, level, wrap, flush=zlib.Z_FULL_FLUSH, first_flush=False, doubled=()):
    """src compressed with a flush after every k input bytes -> (stream, pieces).  first_flush: a flush before any input.
    doubled: indices of flushes behind which a second marker is appended by hand."""
    c = zlib.compressobj(level, zlib.DEFLATED, WBITS[wrap])
    out, pieces = [], 1
    if first_flush:
        b = c.flush(flush)
        out.append(b)
        pieces += b.endswith(MARKER)
    for j, i in enumerate(range(0, len(src), k)):
        b = c.compress(src[i:i + k]) + c.flush(flush)
        out.append(b)
        pieces += b.endswith(MARKER)
        if j in doubled and b.endswith(MARKER):
            out.append(b"\x00" + MARKER)
            pieces += 1
    return b"".join(out) + c.flush(), pieces


def candidates(wrap, data):
    """The scan's count for a stream whose header is the plain one Python's zlib writes: the body's first byte and every offset
    p >= body + 4 behind the four marker bytes, p < len(data)."""
    body, n, i = HEADER[wrap], 1, data.find(MARKER, HEADER[wrap])
    while i >= 0:
        n += i + 4 < len(data)
        i = data.find(MARKER, i + 1)
    return n if body < len(data) else 0


def expected_segments(item, min_bytes=MIN_BYTES, max_candidates=MAX_CANDIDATES):
    if len(item.data) < min_bytes or candidates(item.wrap, item.data) > max_candidates or item.chain < 2:
        return 0
    return item.chain


def _flip(b, bit):
    b = bytearray(b)
    b[bit // 8] ^= 1 << (bit % 8)
    return bytes(b)


def _stored(data, final=False):
    out = b""
    for i in range(0, max(len(data), 1), 65535):
        part = data[i:i + 65535]
        last = final and i + 65535 >= len(data)
        out += bytes([1 if last else 0]) + struct.pack("<HH", len(part), len(part) ^ 0xffff) + part
    return out


def _wrapped(wrap, body, plain):
    if wrap == RAW:
        return body
    if wrap == ZLIB:
        return b"\x78\x9c" + body + struct.pack(">I", zlib.adler32(plain))
    return b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\x03" + body + struct.pack("<II", zlib.crc32(plain), len(plain) & 0xffffffff)


def corpus(seed=2027, big=True):
    rng = random.Random(seed)
    items = []
    wraps = (RAW, ZLIB, GZIP)

    def add(group, name, wrap, data, cap, chain):
        items.append(Item(group, "%s %s w%d" % (group, name, wrap), wrap, data, cap, chain))

    # ---- (a) clean split streams
    sizes = {1: 700, 100: 30000, 4096: 400000, 65280: 1200000, 1 << 20: (3 << 20) + 12345}
    a_items = []
    for k, n in sizes.items():
        if not big and k >= 65280:
            n = 3 * k + 17 if k == 65280 else 0
        if not n:
            continue
        for ki, kind in enumerate(sorted(kinds.KINDS)):
            levels = (1, 6, 9, 0) if k <= 65280 else (6,)
            for level in levels:
                if k >= 4096 and level != 6 and (ki + level) % 3:
                    continue                           # every kind at level 6; the other levels on a third of the kinds each
                src = kinds.make(kind, seed + ki, n)
                wrap = wraps[(ki + level + k) % 3]
                data, pieces = flushed(src, k, level, wrap)
                add("a", "k%d %s L%d" % (k, kind, level), wrap, data, len(src), pieces)
                a_items.append((items[-1], src))
    for wrap in wraps:
        src = kinds.text_like(seed, 5 * 65280 + 999)
        data = deflate_stream_ref.deflate_stream(src, wrap)
        add("a", "own reference", wrap, data, len(src) + 7, -(-len(src) // deflate_stream_ref.PIECE) + 1)
        a_items.append((items[-1], src))
        src = kinds.text_like(seed + 1, 300000)
        data, pieces = flushed(src, 50000, 6, wrap, doubled=(1, 3))
        add("a", "two flushes in a row", wrap, data, len(src), pieces)
        data, pieces = flushed(src, 50000, 6, wrap, first_flush=True)
        add("a", "flush before any input", wrap, data, len(src), pieces)
        for k in (100, 4096):
            for n in (0, 1, k - 1, k, k + 1):
                src = kinds.text_like(seed + n, n)
                data, pieces = flushed(src, k, 6, wrap)
                add("a", "length %d of k%d" % (n, k), wrap, data, n, pieces)
        # all 16 alignments of the place where two pieces meet, in the output and in the input
        for r in range(16):
            src = kinds.text_like(seed + r, 70000 + 3 * (4096 + r))
            data, pieces = flushed(src, 4096 + r, 6, wrap)
            add("a", "alignment %d" % r, wrap, data, len(src), pieces)

    # ---- (b) must fall back, and decode right
    text = kinds.text_like(seed + 5, 400000)
    for wrap in wraps:
        for flush, fname in ((zlib.Z_SYNC_FLUSH, "sync"), (zlib.Z_PARTIAL_FLUSH, "partial")):
            data, _ = flushed(text, 20000, 6, wrap, flush)
            add("b", "%s flush" % fname, wrap, data, len(text), 0)
        c = zlib.compressobj(6, zlib.DEFLATED, WBITS[wrap])
        parts = [c.compress(text[i:i + 20000]) + c.flush(zlib.Z_FULL_FLUSH if i < 200000 else zlib.Z_SYNC_FLUSH) for i in range(0, len(text), 20000)]
        add("b", "full then sync", wrap, b"".join(parts) + c.flush(), len(text), 0)
        c = zlib.compressobj(6, zlib.DEFLATED, WBITS[wrap])
        add("b", "one window", wrap, c.compress(text) + c.flush(), len(text), 0)
    m1, _ = flushed(text[:150000], 30000, 6, GZIP)
    m2, _ = flushed(text[150000:], 30000, 6, GZIP)
    add("b", "two flushed members", GZIP, m1 + m2, len(text), 0)
    add("b", "flushed member then garbage", GZIP, m1 + b"garbage", 150000, 0)
    add("b", "flushed member then zeros", GZIP, m1 + b"\x00" * 100, 150000, 6)
    add("b", "flushed member then 8 KiB of zeros", GZIP, m1 + b"\x00" * 8192, 150000, 0)
    add("b", "flushed raw then garbage", RAW, flushed(text[:150000], 30000, 6, RAW)[0] + b"garbage", 150000, 6)

    # ---- (c) false candidates
    for wrap in wraps:
        plain = MARKER * 30000 + b"\x00\x00\xff" + MARKER * 5000
        add("c", "stored markers", wrap, _wrapped(wrap, _stored(plain, final=True), plain), len(plain), 0)
        # a stored block whose data holds the marker and then a complete stream with a final block; the true stream goes on behind it
        fake = flushed(kinds.text_like(seed + 9, 90000), 30000, 6, RAW)[0]
        inner = b"abc" + MARKER + fake + b"tail" * 5000
        tail = kinds.text_like(seed + 10, 80000)
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        body = _stored(inner) + c.compress(tail) + c.flush()
        add("c", "fake chain in stored data", wrap, _wrapped(wrap, body, inner + tail), len(inner) + len(tail), 0)
        # the same behind a true flush: the true chain has two pieces, the fake one hangs off a false candidate
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        head = c.compress(tail) + c.flush(zlib.Z_FULL_FLUSH)
        c2 = zlib.compressobj(6, zlib.DEFLATED, -15)
        body = head + _stored(inner) + c2.compress(tail[:30000]) + c2.flush()
        add("c", "fake chain behind a true flush", wrap, _wrapped(wrap, body, tail + inner + tail[:30000]), len(tail) + len(inner) + 30000, 2)
    if big:
        plain = MARKER * (2 << 20)
        add("c", "8 MiB of stored markers", ZLIB, _wrapped(ZLIB, _stored(plain, final=True), plain), len(plain), 0)

    # ---- (d) damage to streams of (a)
    picks = [p for p in a_items if 150000 < len(p[0].data) < 1500000]
    rng.shuffle(picks)
    for it, src in picks[:9 if big else 3]:
        d, w = it.data, it.wrap
        marks = [i for i in range(len(d)) if d.startswith(MARKER, i)][:400]
        name = it.name[2:]
        for j in range(4):
            add("d", "bit flip %d in %s" % (j, name), w, _flip(d, rng.randrange(8 * HEADER[w], 8 * (len(d) - TRAILER[w]))), it.cap, it.chain)
        add("d", "cut inside a piece of %s" % name, w, d[:rng.randrange(len(d) // 4, len(d) // 2)], it.cap, 0)
        if marks:
            mk = marks[len(marks) // 2]
            for cut in (mk, mk + 2, mk + 4):
                add("d", "cut at a marker +%d of %s" % (cut - mk, name), w, d[:cut], it.cap, 0)
        for cut in range(1, TRAILER[w] + 1):
            add("d", "cut %d into the trailer of %s" % (TRAILER[w] - cut, name), w, d[:len(d) - cut], it.cap, 0)
        if w != RAW:
            add("d", "wrong checksum of %s" % name, w, _flip(d, 8 * (len(d) - TRAILER[w]) + 3), it.cap, it.chain)
        if w == GZIP:
            add("d", "wrong isize of %s" % name, w, _flip(d, 8 * (len(d) - 4) + 9), it.cap, 0)
        add("d", "capacity exact of %s" % name, w, d, len(src), it.chain)
        add("d", "capacity one less of %s" % name, w, d, len(src) - 1, 0)
        add("d", "capacity 0 of %s" % name, w, d, 0, 0)
    return items
