"""libz 1.2.11, the library behind Python's zlib module, as the reference for zwz_inflate_streams_dev.  Test infrastructure only.

reference(wrap, data, cap) -> (status, bytes): what one stream must decode to with an output capacity of `cap` bytes.
  raw   decompressobj(-15); bytes after the final block are ignored
  zlib  decompressobj(15); bytes after the Adler-32 are ignored
  gzip  the member loop of gzip.decompress, each member through decompressobj(31) (libz checks FHCRC, CRC-32 and ISIZE and starts
        every member with an empty window); zero bytes between and after members are skipped, a following 1f 8b starts another
        member, any other byte is TRAILING.  Unlike Python, an input with no member at all (empty, or zeros only) is status 1.
Statuses: libz's messages mapped -- header messages and Z_NEED_DICT -> BAD_HEADER, "incorrect data check" -> CHECKSUM, "incorrect
length check" -> LENGTH, any other data error -> 2, not at the end of the stream -> 1, and 3 when the output would pass `cap` before
libz stops for any other reason (decoded with max_length = cap + 1).  Each stream runs through libz's inflate with that output
budget, as Python's decompressobj(wbits).decompress(data, cap + 1) does, but on the z_stream itself: on an error the module raises
and drops the bytes decoded before it, which the acceptance compares, and which say whether the cap had been passed.
"""
import ctypes

import numpy as np

import libz_ref

RAW, ZLIB, GZIP = 0, 1, 2
WRAPS = {"raw": RAW, "zlib": ZLIB, "gzip": GZIP}
END, NEED_INPUT, DATA_ERROR, OVERFLOW = 0, 1, 2, 3
BAD_HEADER, CHECKSUM, LENGTH, TRAILING, TOO_LARGE = 32, 33, 34, 35, 36
MAX_IN, MAX_OUT = 1 << 29, 1 << 32

_HEADER_MESSAGES = ("incorrect header check", "unknown compression method", "invalid window size", "unknown header flags set",
                    "header crc mismatch")


def _status_of(msg):
    if any(m in msg for m in _HEADER_MESSAGES):
        return BAD_HEADER
    if "incorrect data check" in msg:
        return CHECKSUM
    if "incorrect length check" in msg:
        return LENGTH
    return DATA_ERROR


def _first_nonzero(data, start):
    """index of the first byte at or after start that is not zero, or len(data) (bytes.lstrip takes seconds over half a GiB)"""
    v = np.frombuffer(data, dtype=np.uint8)
    for o in range(start, len(data), 1 << 24):
        c = v[o:o + (1 << 24)]
        if c.any():
            return o + int((c != 0).argmax())
    return len(data)


def _decode_one(wbits, data, room, start=0):
    """One inflate stream over data[start:] with at most room + 1 bytes of output -> (status, bytes, where the unused input starts).
    libz's own z_stream (the library Python's zlib module maps, through libz_ref): on an error the module hides what was decoded
    before it, and whether the output had passed the cap by then decides between status 3 and the error.  libz reads the bytes
    object in place (no copy: the streams at the 2^29 limit are half a GiB)."""
    z = libz_ref.lib()
    s = libz_ref.ZStream()
    assert z.inflateInit2_(ctypes.byref(s), wbits, z.zlibVersion(), ctypes.sizeof(s)) == libz_ref.Z_OK
    inbuf = ctypes.c_char_p(data)                       # (kept alive, as `data` is, until the return)
    s.next_in = ctypes.cast(inbuf, ctypes.c_void_p).value + start
    s.avail_in = len(data) - start
    step = 1 << 20
    obuf = ctypes.create_string_buffer(step)
    out = bytearray()
    try:
        while True:
            want = min(step, room + 1 - len(out))
            s.next_out = ctypes.cast(obuf, ctypes.c_void_p)
            s.avail_out = want
            rc = z.inflate(ctypes.byref(s), 0)
            got = want - s.avail_out
            out += obuf.raw[:got]
            if len(out) > room:
                return OVERFLOW, bytes(out[:room]), len(data)
            if rc == libz_ref.Z_STREAM_END:
                return END, bytes(out), len(data) - s.avail_in
            if rc == libz_ref.Z_NEED_DICT:
                return BAD_HEADER, bytes(out), len(data)
            if rc == libz_ref.Z_DATA_ERROR:
                return _status_of((s.msg or b"").decode()), bytes(out), len(data)
            if rc == libz_ref.Z_BUF_ERROR or s.avail_in == 0 and got < want:
                return NEED_INPUT, bytes(out), len(data)
    finally:
        z.inflateEnd(ctypes.byref(s))


def reference(wrap, data, cap):
    data = bytes(data)
    if len(data) >= MAX_IN or cap >= MAX_OUT:
        return TOO_LARGE, b""
    if wrap == RAW:
        st, out, _ = _decode_one(-15, data, cap)
        return st, out
    if wrap == ZLIB:
        st, out, _ = _decode_one(15, data, cap)
        return st, out
    if _first_nonzero(data, 0) == len(data):
        return NEED_INPUT, b""
    out = b""
    pos = 0
    first = True
    while True:
        if not first:
            pos = _first_nonzero(data, pos)
            if pos == len(data):
                return END, out
            if data[pos:pos + 2] != b"\x1f\x8b":
                return TRAILING, out
        st, got, pos = _decode_one(31, data, cap - len(out), pos)
        out += got
        if st != END:
            return st, out
        first = False


def accept(wrap, data, cap, status, got, ref=None):
    """None if (status, got) meet the acceptance for this stream, else a string saying why not.  ref: reference(wrap, data, cap) where
    the caller has it already."""
    want_st, want = ref or reference(wrap, data, cap)
    if status != want_st:
        return "status %d, reference %d" % (status, want_st)
    if status == END and got != want:
        return "bytes differ (%d vs %d)" % (len(got), len(want))
    k = min(len(got), len(want))
    if got[:k] != want[:k]:
        return "partial output differs in the first %d bytes" % k
    return None
