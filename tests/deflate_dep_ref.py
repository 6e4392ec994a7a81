"""What zwz_deflate_dep_streams_dev must write, from libz itself (Python's zlib is libz 1.2.11 here, as tests/libz_ref.py checks):
pieces of 32 768 input bytes, each a raw deflate stream of its own that was primed with the 32 512 bytes in front of it
(deflateSetDictionary on a raw stream: no FDICT bit anywhere) and closed with Z_SYNC_FLUSH; 03 00 behind the last.  The wrapper is the
project's own: zlib's 78 9c / 78 5e and Adler-32, or gzip's ten bytes with OS 3, CRC-32 and ISIZE, over the whole input.  pigz's default.

The index of such a stream (include/zwz.h: zwz_deflate_dep_streams_index_dev) is section 22's format: the points are the piece starts,
chosen by the rule of the index at flush points; entry 0 has hist 0, every later entry hist 32 512 and the input in front of it as its
window.  Test infrastructure only."""
import struct
import zlib

import index_ref
from index_ref import GZIP, RAW, ZLIB

P, D = 32768, 32512
WRAPS = ("raw", "zlib", "gzip")
WRAP_ID = {"raw": RAW, "zlib": ZLIB, "gzip": GZIP}
MARKER = b"\x00\x00\xff\xff"


def header(wrap, level=6):
    if wrap == "zlib":
        return b"\x78\x9c" if level == 6 else b"\x78\x5e"
    return bytes.fromhex("1f8b0800000000000003") if wrap == "gzip" else b""


def trailer(wrap, data):
    if wrap == "zlib":
        return struct.pack(">I", zlib.adler32(data))
    return struct.pack("<II", zlib.crc32(data), len(data) & 0xffffffff) if wrap == "gzip" else b""


def pieces(data, level=6):
    """The pieces' shares of the body, in order"""
    out = []
    for i in range(0, len(data), P):
        zd = data[max(0, i - D):i]
        c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, zlib.Z_DEFAULT_STRATEGY, zd) if zd \
            else zlib.compressobj(level, zlib.DEFLATED, -15, 8)
        out.append(c.compress(data[i:i + P]) + c.flush(zlib.Z_SYNC_FLUSH))
        assert out[-1].endswith(MARKER)
    return out


def deflate_dep_stream(data, wrap="gzip", level=6):
    return header(wrap, level) + b"".join(pieces(data, level)) + b"\x03\x00" + trailer(wrap, data)


def entries_of(data, wrap="gzip", level=6, span=1 << 20):
    """[(bit, off, hist)] by the rule: piece k is a point at decoded offset P k; entry 0 is point 0, point k >= 1 is an entry when
    bytes follow it and it is the first point in its span-sized bucket of the output"""
    at = len(header(wrap, level))
    entries = []
    for k, share in enumerate(pieces(data, level)):
        off = P * k
        if k == 0 or (off < len(data) and off // span > (off - P) // span):
            entries.append((8 * at, off, D if k else 0))
        at += len(share)
    return entries or [(8 * at, 0, 0)]


def dep_index(data, wrap="gzip", level=6, span=1 << 20):
    """The stream and its index -> (stream, index bytes); every checkpoint is checked with libz (index_ref.check_index)"""
    stream = deflate_dep_stream(data, wrap, level)
    entries = entries_of(data, wrap, level, span)
    w = WRAP_ID[wrap]
    check = zlib.crc32(data) if w == GZIP else zlib.adler32(data) if w == ZLIB else 0
    end_bit = 8 * (len(stream) - len(trailer(wrap, data)) - 2) + 10
    windows = [data[off - hist:off] for _, off, hist in entries]
    idx = index_ref.compose(index_ref.Index(w, span, len(stream), len(data), end_bit, check, entries, windows))
    index_ref.check_index(idx, stream, data, w)
    return stream, idx
