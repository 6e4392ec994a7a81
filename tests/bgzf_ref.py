"""Python BGZF writers for the tests: the exact stream the product must produce (from the CPU oracle's level-6 deflate) and
the looser forms other writers emit (other levels, more extra subfields, no EOF member).  Test infrastructure only."""
import struct
import zlib

BLOCK = 65280
EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def member(block: bytes, body: bytes, extra_before: bytes = b"", extra_after: bytes = b"") -> bytes:
    xlen = len(extra_before) + 6 + len(extra_after)
    bsize = 12 + xlen + len(body) + 8
    assert bsize <= 65536
    return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff" + struct.pack("<H", xlen) + extra_before + b"BC\x02\x00" +
            struct.pack("<H", bsize - 1) + extra_after + body + struct.pack("<II", zlib.crc32(block), len(block)))


def reference(oracle, data: bytes) -> bytes:
    """What zwz_bgzf_compress_dev must write: each block's body is the oracle's zlib-1.2.11 level-6 stream without its
    2-byte header and 4-byte Adler-32."""
    out = [member(data[i:i + BLOCK], oracle.deflate6(data[i:i + BLOCK])[2:-4]) for i in range(0, len(data), BLOCK)]
    return b"".join(out) + EOF


def other_writer(data: bytes, level: int, block: int = BLOCK, extra: bool = False, eof: bool = True) -> bytes:
    """BGZF as another tool might write it: host zlib at `level`, optional extra subfields around BC."""
    out = []
    for i in range(0, len(data), block):
        blk = data[i:i + block]
        co = zlib.compressobj(level, zlib.DEFLATED, -15)
        body = co.compress(blk) + co.flush()
        if extra:
            out.append(member(blk, body, extra_before=b"XY\x03\x00abc", extra_after=b"ZZ\x00\x00"))
        else:
            out.append(member(blk, body))
    return b"".join(out) + (EOF if eof else b"")
