"""Python .gzi writer and reader for the tests (include/zwz.h: the layout of htslib's bgzf_index_dump, and this project's rule for
empty members), plus a BGZF writer with chosen member sizes.  Test infrastructure only; builds on bgzf_ref."""
import struct
import zlib

import bgzf_ref


def members(gz: bytes):
    """[(compressed offset, ISIZE)] of every member of a BGZF stream (a plain walk by the BC subfield; the streams here are well formed)."""
    out, o = [], 0
    while o < len(gz):
        (xlen,) = struct.unpack_from("<H", gz, o + 10)
        x, bsize = o + 12, None
        while x < o + 12 + xlen:
            slen = struct.unpack_from("<H", gz, x + 2)[0]
            if gz[x:x + 2] == b"BC":
                bsize = struct.unpack_from("<H", gz, x + 4)[0] + 1
            x += 4 + slen
        out.append((o, struct.unpack_from("<I", gz, o + bsize - 4)[0]))
        o += bsize
    return out


def entries(gz: bytes, empty_entries: bool = True, eof_entry: bool = False):
    """(compressed, decoded) offsets of every member after the first.  The writer's rule is the default: every member but a last one
    that decodes to nothing.  empty_entries=False leaves out every empty member; eof_entry=True keeps a trailing empty one."""
    ms, out, raw = members(gz), [], 0
    for i, (o, isize) in enumerate(ms):
        last = i == len(ms) - 1
        if i and (isize or (empty_entries and (not last or eof_entry))):
            out.append((o, raw))
        raw += isize
    return out


def write(ents) -> bytes:
    return struct.pack("<Q", len(ents)) + b"".join(struct.pack("<QQ", c, u) for c, u in ents)


def gzi(gz: bytes, **kw) -> bytes:
    return write(entries(gz, **kw))


def read(g: bytes):
    """[(compressed, decoded)] with the implied (0, 0) first; ValueError for what the library rejects as ZWZ_E_FORMAT."""
    if len(g) < 8:
        raise ValueError("short")
    (n,) = struct.unpack_from("<Q", g)
    if len(g) != 8 + 16 * n:
        raise ValueError("length")
    out = [(0, 0)]
    for i in range(n):
        c, u = struct.unpack_from("<QQ", g, 8 + 16 * i)
        if c <= out[-1][0] or u < out[-1][1]:
            raise ValueError("order")
        out.append((c, u))
    return out


def sized_writer(data: bytes, sizes, level: int = 6, eof: bool = True) -> bytes:
    """BGZF with member i holding sizes[i] bytes (0 allowed: an empty member), cycling through sizes until data is used up."""
    out, o, i = [], 0, 0
    while o < len(data) or (i < len(sizes) and sizes[i] == 0):
        n = sizes[i % len(sizes)]
        blk = data[o:o + n]
        co = zlib.compressobj(level, zlib.DEFLATED, -15)
        out.append(bgzf_ref.member(blk, co.compress(blk) + co.flush()))
        o += len(blk)
        i += 1
    return b"".join(out) + (bgzf_ref.EOF if eof else b"")
