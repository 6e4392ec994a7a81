"""The seek index at full-flush points (include/zwz.h: zwz_deflate_streams_index_dev) in plain Python, written without the product's
code: streams from libz through Python's zlib with Z_FULL_FLUSH at given cuts, the rule, and the index composed with
index_ref.compose.  Test infrastructure only.

The POINTS of a stream are its piece starts in stream order: the body's first block (bit 8 * body, offset 0) and every block that
starts behind a flush marker (bit 8 * p, decoded offset o).  Entry 0 is point 0; point k >= 1 is an entry when o_k < the decoded
length and floor(o_k / span) > floor(o_(k-1) / span), the point in front of it, not the entry.  Every entry has hist 0.
"""
import zlib

import index_ref
from index_ref import GZIP, RAW, WBITS, ZLIB

MARKER = b"\x00\x00\xff\xff"
BODY = {RAW: 0, ZLIB: 2, GZIP: 10}
TRAILER = {RAW: 0, ZLIB: 4, GZIP: 8}
PIECE = 65280


def flush_stream(data, cuts, wrap=GZIP, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, first_flush=False, doubled=()):
    """libz's stream of data with a Z_FULL_FLUSH after every data[:c], c in cuts (rising, the last may be len(data): an empty last
    piece).  first_flush: a flush before any input.  doubled: indices into cuts behind whose flush a second marker is appended by
    hand (libz writes nothing for a repeated flush).  -> (stream, points [(byte, offset)], end bit)"""
    c = zlib.compressobj(level, zlib.DEFLATED, WBITS[wrap], 8, strategy)
    out = b""
    points, prev = [(BODY[wrap], 0)], 0
    if first_flush:
        out += c.flush(zlib.Z_FULL_FLUSH)
        assert out.endswith(MARKER)
        points.append((len(out), 0))
    for j, cut in enumerate(cuts):
        b = c.compress(data[prev:cut]) + c.flush(zlib.Z_FULL_FLUSH)
        out += b
        if b.endswith(MARKER):
            points.append((len(out), cut))
        if j in doubled and b.endswith(MARKER):
            out += b"\x00" + MARKER
            points.append((len(out), cut))
        prev = cut
    last = len(out) or BODY[wrap]                 # (no flush yet: libz's header is still to come)
    out += c.compress(data[prev:]) + c.flush()
    tail = TRAILER[wrap]
    if prev == len(data) and out[last:len(out) - tail] == b"\x03\x00":
        # the final block is the 03 00 behind the last marker (an empty static block: 3 header bits and the 7 of its end code)
        return out, points, 8 * (len(out) - tail - 2) + 10
    return out, points, _end_bit(out, data, last, prev, tail)


def _end_bit(out, data, last, prev, tail):
    """index_ref.sync_flush_stream's search, restated: libz stops at the byte that holds the final block's last bit and does not say
    which bit it was.  The first bit behind the block is the smallest eb in that byte for which the bits below eb alone end the
    stream whatever follows: with zeros and with ones behind eb the decode from the last piece's start (an empty window: a full
    flush precedes it) must reach the end with the piece's whole output."""
    d = zlib.decompressobj(-15)
    rest = out[last:len(out) - tail]
    d.decompress(rest)
    assert d.eof
    hi = 8 * (last + len(rest) - len(d.unused_data))
    whole = int.from_bytes(out[:len(out) - tail], "little")

    def ends(eb, fill):
        piece = (whole & ((1 << eb) - 1)) | (((1 << (hi - eb)) - 1) << eb if fill else 0)
        dd = zlib.decompressobj(-15)
        try:
            got = dd.decompress((piece >> (8 * last)).to_bytes((hi - 8 * last) // 8, "little"))
        except zlib.error:
            return False
        return dd.eof and got == data[prev:]

    for eb in range(hi - 7, hi + 1):
        if ends(eb, 0) and ends(eb, 1):
            return eb
    raise AssertionError("no end bit found")


def points_of(stream, wrap):
    """The points of a stream from its bytes: libz decodes up to every byte behind the four marker bytes and counts, and the byte is
    a point if the rest of the stream, decoded from there with an empty window, is the rest of the data (marker bytes inside a
    stored block, or a sync flush, fail that)."""
    body, end = BODY[wrap], len(stream) - TRAILER[wrap]
    data = zlib.decompress(stream, WBITS[wrap])
    d = zlib.decompressobj(-15)
    points, pos, off = [(body, 0)], body, 0
    i = stream.find(MARKER, body, end)
    while i >= 0 and i + 4 < end and not d.eof:
        off += len(d.decompress(stream[pos:i + 4]))
        pos = i + 4
        alone = zlib.decompressobj(-15)
        try:
            if not d.eof and alone.decompress(stream[pos:end]) == data[off:] and alone.eof:
                points.append((pos, off))
        except zlib.error:
            pass
        i = stream.find(MARKER, i + 1, end)
    return points


def entries_of(points, decoded_len, span):
    """The rule (module docstring) -> [(bit, off, 0)]"""
    assert points[0][1] == 0
    entries = [(8 * points[0][0], 0, 0)]
    for (_, po), (p, o) in zip(points, points[1:]):
        if o < decoded_len and o // span > po // span:
            entries.append((8 * p, o, 0))
    return entries


def compose(stream, data, wrap, span, points, end_bit):
    """The reference index of a stream, checked with libz entry by entry (index_ref.check_index) -> bytes"""
    check = zlib.crc32(data) if wrap == GZIP else zlib.adler32(data) if wrap == ZLIB else 0
    entries = entries_of(points, len(data), span)
    idx = index_ref.compose(index_ref.Index(wrap, span, len(stream), len(data), end_bit, check, entries, [b""] * len(entries)))
    index_ref.check_index(idx, stream, data, wrap)
    return idx


def flush_index(data, cuts, wrap=GZIP, span=1 << 16, **how):
    """flush_stream and its reference index -> (stream, index bytes)"""
    stream, points, end_bit = flush_stream(data, cuts, wrap, **how)
    return stream, compose(stream, data, wrap, span, points, end_bit)


def writer_cuts(n):
    """Where zwz_deflate_streams_dev flushes: behind every piece of 65 280 input bytes, the last one included"""
    return [min(c + PIECE, n) for c in range(0, n, PIECE)]


def writer_index(data, wrap=GZIP, span=1 << 16, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    """What zwz_deflate_streams_index_dev must write, from libz -> (stream, index bytes)"""
    return flush_index(data, writer_cuts(len(data)), wrap, span, level=level, strategy=strategy)
