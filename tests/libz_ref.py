"""libz itself as the reference for inflate (ctypes on libz.so.1, the library Python's zlib module already maps).  Test
infrastructure only.

reference_inflate  what decompress_chunk() (decompression.cpp:11-37) gets from libz: inflateInit, Z_NO_FLUSH into a 65 535-byte
                   buffer, again while the buffer came back full, every return code ignored.
expected_status    the inflate status (inflate_core.h: InflateStatus) the product must report for a payload: the zlib header check
                   inflate_begin makes, then libz in raw mode on the rest -- Z_STREAM_END -> END, Z_DATA_ERROR -> DATA_ERROR,
                   anything else -> NEED_INPUT -- and OVERFLOW when the output passes 65 535 bytes.
raw_inflate        the same for a raw DEFLATE body (a BGZF member's): (bytes, status).
"""
import ctypes
import ctypes.util
import zlib

CHUNK = 65535
END, NEED_INPUT, DATA_ERROR, OVERFLOW = 0, 1, 2, 3
Z_OK, Z_STREAM_END, Z_NEED_DICT, Z_DATA_ERROR, Z_BUF_ERROR = 0, 1, 2, -3, -5
_LIMIT = 1 << 24      # the corpus never decodes to this much; a stream that would is a generator bug


class ZStream(ctypes.Structure):
    """struct z_stream_s, LP64."""
    _fields_ = [("next_in", ctypes.c_void_p), ("avail_in", ctypes.c_uint), ("total_in", ctypes.c_ulong),
                ("next_out", ctypes.c_void_p), ("avail_out", ctypes.c_uint), ("total_out", ctypes.c_ulong),
                ("msg", ctypes.c_char_p), ("state", ctypes.c_void_p),
                ("zalloc", ctypes.c_void_p), ("zfree", ctypes.c_void_p), ("opaque", ctypes.c_void_p),
                ("data_type", ctypes.c_int), ("adler", ctypes.c_ulong), ("reserved", ctypes.c_ulong)]


assert ctypes.sizeof(ctypes.c_void_p) == 8 and ctypes.sizeof(ZStream) == 112, "z_stream is declared for LP64"

_z = None


def lib():
    global _z
    if _z is None:
        name = "libz.so.1"
        try:
            z = ctypes.CDLL(name)
        except OSError:
            z = ctypes.CDLL(ctypes.util.find_library("z"))
        z.zlibVersion.restype = ctypes.c_char_p
        z.inflateInit_.argtypes = [ctypes.POINTER(ZStream), ctypes.c_char_p, ctypes.c_int]
        z.inflateInit2_.argtypes = [ctypes.POINTER(ZStream), ctypes.c_int, ctypes.c_char_p, ctypes.c_int]
        z.inflate.argtypes = [ctypes.POINTER(ZStream), ctypes.c_int]
        z.inflateEnd.argtypes = [ctypes.POINTER(ZStream)]
        _z = z
    return _z


def version():
    return lib().zlibVersion().decode()


def _run(data: bytes, window_bits):
    """Feed `data` in one piece; Z_NO_FLUSH into a 65 535-byte buffer while it comes back full.  -> (output, last return code)."""
    z = lib()
    s = ZStream()
    src = ctypes.create_string_buffer(data, len(data))
    if window_bits is None:
        rc = z.inflateInit_(ctypes.byref(s), z.zlibVersion(), ctypes.sizeof(ZStream))
    else:
        rc = z.inflateInit2_(ctypes.byref(s), window_bits, z.zlibVersion(), ctypes.sizeof(ZStream))
    assert rc == Z_OK, rc
    s.next_in = ctypes.cast(src, ctypes.c_void_p)
    s.avail_in = len(data)
    out = ctypes.create_string_buffer(CHUNK)
    parts, total = [], 0
    try:
        while True:
            s.next_out = ctypes.cast(out, ctypes.c_void_p)
            s.avail_out = CHUNK
            rc = z.inflate(ctypes.byref(s), 0)
            k = CHUNK - s.avail_out
            parts.append(out.raw[:k])
            total += k
            assert total < _LIMIT, "stream decodes to more than the corpus allows"
            if s.avail_out != 0:
                break
    finally:
        z.inflateEnd(ctypes.byref(s))
    return b"".join(parts), rc


def reference_inflate(payload: bytes) -> bytes:
    """decompress_chunk(): an empty record yields nothing; otherwise everything libz emits before it stops."""
    if not payload:
        return b""
    return _run(payload, None)[0]


def _status(out, rc):
    if len(out) > CHUNK:
        return OVERFLOW
    return END if rc == Z_STREAM_END else DATA_ERROR if rc == Z_DATA_ERROR else NEED_INPUT


def raw_inflate(body: bytes):
    """A raw DEFLATE body -> (libz's output, status)."""
    out, rc = _run(body, -15)
    return out, _status(out, rc)


def expected_status(payload: bytes) -> int:
    if len(payload) < 2:
        return NEED_INPUT
    cmf, flg = payload[0], payload[1]
    if ((cmf << 8) | flg) % 31 or (cmf & 15) != 8 or (cmf >> 4) > 7 or flg & 0x20:
        return DATA_ERROR
    return raw_inflate(payload[2:])[1]


def describe():
    return "libz %s (zlib module built against %s)" % (version(), zlib.ZLIB_VERSION)
