"""The seek index of ordinary DEFLATE streams (include/zwz.h) in plain Python: parsing, composing, the libz check of a checkpoint,
and reference indexes written without the product's code.  Test infrastructure only.

The libz check: a checkpoint says that a block header starts at bit `bit` of the stream, that `off` decoded bytes precede it and that
the `hist` bytes in front of it are `window`.  Shift the stream right by `bit` -- int.from_bytes(s, "little") >> bit -- and a raw
inflate primed with the window (zlib.decompressobj(-15, zdict=window)) must give data[off:].  (shifted() keeps the bits' places
within their bytes, which stored blocks depend on.)
"""
import struct
import zlib
from dataclasses import dataclass

MAGIC = b"ZWZIDX\x00\x01"
HEADER, ENTRY, WINDOW = 64, 24, 32768
RAW, ZLIB, GZIP = 0, 1, 2
STREAM_INDEX = 37


@dataclass
class Index:
    wrap: int
    span: int
    stream_len: int
    decoded_len: int
    end_bit: int
    check: int
    entries: list          # [(bit, off, hist)]
    windows: list          # [bytes], one per entry


def parse(idx):
    """bytes -> Index; AssertionError for anything the layout forbids."""
    assert idx[:8] == MAGIC and len(idx) % 16 == 0
    wrap, span, slen, dlen, count, flags, end_bit, check, crc, zero = struct.unpack_from("<IIQQIIQIIQ", idx, 8)
    assert flags == 0 and zero == 0 and count >= 1
    assert zlib.crc32(idx[HEADER:]) == crc
    entries, windows = [], []
    at = HEADER + ENTRY * count
    for k in range(count):
        bit, off, hist, z = struct.unpack_from("<QQII", idx, HEADER + ENTRY * k)
        assert z == 0 and hist <= min(WINDOW, off)
        entries.append((bit, off, hist))
        windows.append(idx[at:at + hist])
        at += hist
    assert (at + 15) // 16 * 16 == len(idx) and not any(idx[at:])
    assert entries[0][1] == 0 and entries[0][2] == 0
    for a, b in zip(entries, entries[1:]):
        assert b[0] > a[0] and b[1] >= a[1]
    assert entries[-1][0] < end_bit <= 8 * slen
    return Index(wrap, span, slen, dlen, end_bit, check, entries, windows)


def compose(ix, crc=None):
    """Index -> bytes.  crc: the index CRC field (None: the right one)."""
    body = b"".join(struct.pack("<QQII", b, o, h, 0) for b, o, h in ix.entries) + b"".join(ix.windows)
    body += bytes(-(HEADER + len(body)) % 16)
    head = MAGIC + struct.pack("<IIQQIIQIIQ", ix.wrap, ix.span, ix.stream_len, ix.decoded_len, len(ix.entries), 0, ix.end_bit, ix.check,
                               zlib.crc32(body) if crc is None else crc, 0)
    return head + body


def _bits(v, n):
    return [(v >> i) & 1 for i in range(n)]


# Two non-final blocks that decode to nothing: an empty fixed block (10 bits) and an empty dynamic block of 93 bits -- HLIT 257,
# HDIST 1, the code-length code {0: 1 bit, 1: 2 bits, 18: 2 bits}, lengths 18(138) 18(118) 1 0: only the end-of-block code, one bit.
_FIXED_EMPTY = [0] + _bits(1, 2) + [0] * 7
_DYN_EMPTY = ([0] + _bits(2, 2) + _bits(0, 5) + _bits(0, 5) + _bits(14, 4) + sum((_bits(v, 3) for v in [0, 0, 2, 1] + [0] * 13 + [2]), [])
              + [1, 1] + _bits(127, 7) + [1, 1] + _bits(107, 7) + [1, 0] + [0] + [0])
_PREFIX = {r: _DYN_EMPTY * (r & 1) + _FIXED_EMPTY * {0: 0, 2: 1, 4: 2, 6: 3, 1: 2, 3: 3, 5: 0, 7: 1}[r] for r in range(8)}
assert all(len(p) % 8 == r for r, p in _PREFIX.items())


def shifted(stream, bit):
    """The stream from bit `bit` on, as bytes libz reads: shifted right by `bit` -- and, where bit is no multiple of 8, pushed up again
    behind blocks that decode to nothing and end bit & 7 bits into a byte, so that the stream's bits keep their places within
    their bytes (a stored block pads to the ORIGINAL byte boundaries)."""
    pre = _PREFIX[bit & 7]
    v = (int.from_bytes(stream, "little") >> bit) << len(pre) | sum(x << i for i, x in enumerate(pre))
    return v.to_bytes((8 * len(stream) - bit + len(pre) + 7) // 8 or 1, "little")


def check_checkpoint(stream, data, bit, off, window):
    """The libz check of one checkpoint (module docstring)."""
    d = zlib.decompressobj(-15, zdict=window) if window else zlib.decompressobj(-15)
    got = d.decompress(shifted(stream, bit))
    assert got == data[off:], "checkpoint (bit %d, offset %d, hist %d) does not decode to data[off:]" % (bit, off, len(window))
    assert d.eof


def check_index(idx, stream, data, wrap=None):
    """Parses an index and puts every entry through the libz check; returns the Index."""
    ix = parse(idx)
    assert ix.stream_len == len(stream) and ix.decoded_len == len(data)
    if wrap is not None:
        assert ix.wrap == wrap
    if ix.wrap == GZIP:
        assert ix.check == zlib.crc32(data)
    elif ix.wrap == ZLIB:
        assert ix.check == zlib.adler32(data)
    else:
        assert ix.check == 0
    for (bit, off, hist), w in zip(ix.entries, ix.windows):
        assert w == data[off - hist:off]
        check_checkpoint(stream, data, bit, off, w)
    # the end bit: the bits from there to the next byte boundary are padding, and the trailer follows
    q = (ix.end_bit + 7) // 8
    if ix.wrap == GZIP:
        assert stream[q:q + 8] == struct.pack("<II", zlib.crc32(data), len(data) & 0xffffffff)
    elif ix.wrap == ZLIB:
        assert stream[q:q + 4] == struct.pack(">I", zlib.adler32(data))
    return ix


WBITS = {RAW: -15, ZLIB: 15, GZIP: 31}


def sync_flush_stream(data, cuts, wrap=GZIP, level=6, span=1 << 16):
    """A stream libz writes with a Z_SYNC_FLUSH after every data[:c], c in cuts, and its reference index composed here: after a sync
    flush (an empty stored block, 00 00 ff ff on a byte boundary) the next block starts on a byte boundary at decoded offset c.  The
    pieces refer back across the flushes: the stream has no cut a split decode could use.  -> (stream, index bytes)"""
    c = zlib.compressobj(level, zlib.DEFLATED, WBITS[wrap])
    out = b""
    body = {RAW: 0, ZLIB: 2, GZIP: 10}[wrap]          # libz's headers: 78 xx; 1f 8b 08 00 and six more bytes
    entries, prev = [(8 * body, 0, 0)], 0
    for cut in cuts:
        out += c.compress(data[prev:cut]) + c.flush(zlib.Z_SYNC_FLUSH)
        assert out[-4:] == b"\x00\x00\xff\xff"
        entries.append((8 * len(out), cut, min(WINDOW, cut)))
        prev = cut
    out += c.compress(data[prev:]) + c.flush()
    tail = {RAW: 0, ZLIB: 4, GZIP: 8}[wrap]
    # the final block ends somewhere in the last byte in front of the trailer: find the end bit with libz itself
    end_bit = None
    last_bit = entries[-1][0]
    d = zlib.decompressobj(-15, zdict=data[max(0, prev - WINDOW):prev]) if prev else zlib.decompressobj(-15)
    rest = out[last_bit // 8:len(out) - tail]
    d.decompress(rest)
    assert d.eof
    used = len(rest) - len(d.unused_data)
    # libz stops at the byte that holds the last bit and does not say which bit it was.  The first bit behind the final block is the
    # smallest eb in that byte for which the bits below eb alone end the stream whatever follows them: the same bytes with zeros
    # behind eb and with ones behind eb must both reach the end with the whole output (a code cut short reads one of the two wrong)
    hi = 8 * (last_bit // 8 + used)
    whole = int.from_bytes(out[:len(out) - tail], "little")

    def ends(eb, fill):
        piece = (whole & ((1 << eb) - 1)) | (((1 << (hi - eb)) - 1) << eb if fill else 0)
        dd = zlib.decompressobj(-15, zdict=data[max(0, prev - WINDOW):prev]) if prev else zlib.decompressobj(-15)
        try:
            got = dd.decompress((piece >> (last_bit & ~7)).to_bytes((hi - (last_bit & ~7)) // 8, "little"))
        except zlib.error:
            return False
        return dd.eof and got == data[prev:]

    for eb in range(hi - 7, hi + 1):
        if ends(eb, 0) and ends(eb, 1):
            end_bit = eb
            break
    assert end_bit is not None
    check = zlib.crc32(data) if wrap == GZIP else zlib.adler32(data) if wrap == ZLIB else 0
    ix = Index(wrap, span, len(out), len(data), end_bit, check, entries, [data[o - h:o] for _, o, h in entries])
    return out, compose(ix)
