"""What zwz_deflate_streams_dev must write, from libz itself (Python's zlib is libz 1.2.11 here, as tests/libz_ref.py checks): level 6,
every 65 280 bytes of input followed by Z_FULL_FLUSH, the last by Z_FINISH.  A full flush with all input consumed clears libz's hash
and window, so every piece is compressed as if alone -- which is what lets the GPU compress them independently."""
import zlib

PIECE = 65280
WBITS = {"raw": -15, "zlib": 15, "gzip": 31, 0: -15, 1: 15, 2: 31}
WRAPS = ("raw", "zlib", "gzip")


def deflate_stream(data: bytes, wrap) -> bytes:
    c = zlib.compressobj(6, zlib.DEFLATED, WBITS[wrap])
    out = b"".join(c.compress(data[i:i + PIECE]) + c.flush(zlib.Z_FULL_FLUSH) for i in range(0, len(data), PIECE))
    return out + c.flush()
