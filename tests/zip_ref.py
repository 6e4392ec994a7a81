"""What zwz_zip_dev and zwz_zip_dir must write, byte for byte: a reference ZIP writer over libz (tests/deflate_stream_ref.py) with the
header fields include/zwz.h fixes.  Every entry is method 8, its data the level-6 raw stream with a full flush every 65 280 bytes.

    local header    PK\\3\\4 | needed | flags | 8 | time | date | CRC | csize | usize | name length | extra length | name | extra
    needed          20; 45 in a record that carries a ZIP64 extra field
    flags           0x0800 iff a name byte is >= 0x80
    big entry       csize or usize >= 0xFFFFFFFF: both sizes 0xFFFFFFFF, local extra 01 00 10 00 | usize u64 | csize u64
    central record  PK\\1\\2 | made-by 0x032D | needed | ... | comment 0 | disk 0 | internal 0 | external | header offset (saturated with its
                    own ZIP64 field when >= 0xFFFFFFFF); the extra holds only the saturated fields: usize, csize, offset
    end records     ZIP64 end record + locator when n >= 0xFFFF or the directory's size or offset >= 0xFFFFFFFF; the classic one's
                    fields saturated with min
force64: every entry big, every offset saturated, the ZIP64 end records present.
"""
import struct
import zlib

import deflate_stream_ref

SAT32, SAT16 = 0xFFFFFFFF, 0xFFFF
MADE_BY = 0x032D
DEFAULT_META = (0, 0x0021, 0o100644 << 16)      # time, date, external attribute


def name_flags(name: bytes) -> int:
    return 0x0800 if any(b >= 0x80 for b in name) else 0


def local_header(name, crc, csize, usize, meta=DEFAULT_META, force64=False) -> bytes:
    big = force64 or csize >= SAT32 or usize >= SAT32
    extra = struct.pack("<HHQQ", 1, 16, usize, csize) if big else b""
    return struct.pack("<IHHHHHIIIHH", 0x04034B50, 45 if big else 20, name_flags(name), 8, meta[0], meta[1], crc,
                       SAT32 if big else csize, SAT32 if big else usize, len(name), len(extra)) + name + extra


def central_record(name, crc, csize, usize, offset, meta=DEFAULT_META, force64=False) -> bytes:
    big = force64 or csize >= SAT32 or usize >= SAT32
    sat = force64 or offset >= SAT32
    fields = (struct.pack("<QQ", usize, csize) if big else b"") + (struct.pack("<Q", offset) if sat else b"")
    extra = struct.pack("<HH", 1, len(fields)) + fields if fields else b""
    return struct.pack("<IHHHHHHIIIHHHHHII", 0x02014B50, MADE_BY, 45 if extra else 20, name_flags(name), 8, meta[0], meta[1], crc,
                       SAT32 if big else csize, SAT32 if big else usize, len(name), len(extra), 0, 0, 0, meta[2],
                       SAT32 if sat else offset) + name + extra


def end_records(n, cd_size, cd_off, force64=False) -> bytes:
    out = b""
    if force64 or n >= SAT16 or cd_size >= SAT32 or cd_off >= SAT32:
        out += struct.pack("<IQHHIIQQQQ", 0x06064B50, 44, MADE_BY, 45, 0, 0, n, n, cd_size, cd_off)
        out += struct.pack("<IIQI", 0x07064B50, 0, cd_off + cd_size, 1)
    return out + struct.pack("<IHHHHIIH", 0x06054B50, 0, 0, min(n, SAT16), min(n, SAT16), min(cd_size, SAT32), min(cd_off, SAT32), 0)


def write(entries, metas=None, force64=False, deflate=None) -> bytes:
    """entries: [(name bytes or str, data bytes)] -> the archive.  metas: [(time, date, attr)] or None.  deflate: data -> raw stream
    (a cache of the caller's), default deflate_stream_ref's."""
    deflate = deflate or (lambda d: deflate_stream_ref.deflate_stream(d, "raw"))
    parts, central, off = [], [], 0
    for i, (name, data) in enumerate(entries):
        name = name.encode("utf-8") if isinstance(name, str) else bytes(name)
        meta = metas[i] if metas else DEFAULT_META
        raw, crc = deflate(data), zlib.crc32(data)
        head = local_header(name, crc, len(raw), len(data), meta, force64)
        parts.append(head)
        parts.append(raw)
        central.append(central_record(name, crc, len(raw), len(data), off, meta, force64))
        off += len(head) + len(raw)
    cd = b"".join(central)
    return b"".join(parts) + cd + end_records(len(entries), len(cd), off, force64)


def dos_time(t):
    """time.struct_time (local) -> (time, date) as zipfile and Info-ZIP store it."""
    y, mo, d, h, mi, s = t[:6]
    if y < 1980:
        y, mo, d, h, mi, s = 1980, 1, 1, 0, 0, 0
    if y > 2107:
        y, mo, d, h, mi, s = 2107, 12, 31, 23, 59, 59
    return h << 11 | mi << 5 | s // 2, (y - 1980) << 9 | mo << 5 | d
