"""The files of the tests of zwz_inflate_legs_file (tests/test_legs_file_cpu.py on the CPU restatement, tests/test_gpu_legs_file.py on the
GPU), with what they decode to -- from how they were put together and from libz, never from the product -- and the shape each must
reach in the call's counters.  Test infrastructure."""
import random
import zlib
from dataclasses import dataclass, field

import legs_ref
from index_ref import GZIP, RAW, ZLIB
from legs_ref import LETTERS, deflate

SPAN = 16384
LEG_OUT = 65536
LEG_INS = (4096, 16384)


@dataclass
class Case:
    name: str
    wrap: int
    stream: bytes
    data: bytes                       # what the file decodes to
    index: bool = True                # whether an index is made (a gzip file of several members: none)
    shape: dict = field(default_factory=dict)      # stats word -> the least it must reach at LEG_INS[0]


def good_cases():
    grainy = legs_ref.grainy()
    rng = random.Random(31)
    out = []
    for wrap, w in ((RAW, "raw"), (ZLIB, "zlib"), (GZIP, "gzip")):
        for level, data in ((1, grainy[:150_000]), (6, grainy), (9, grainy[100_000:300_000])):
            out.append(Case("%s level %d" % (w, level), wrap, deflate(data, wrap, level), data, shape={"legs": 3, "rewound": 2, "commits": 2}))
        out.append(Case("%s sync flushes" % w, wrap, deflate(grainy[:200_000], wrap, 6, 30_000), grainy[:200_000], shape={"legs": 3, "rewound": 2, "commits": 2}))
        out.append(Case("%s empty" % w, wrap, deflate(b"", wrap), b"", shape={"legs": 1}))
    # every match reaches 32 768 back, across every restart point
    block = bytes(rng.getrandbits(8) for _ in range(32768))
    out.append(Case("32 KiB repeated", GZIP, deflate(block * 40, GZIP, 9), block * 40, shape={"legs": 4, "rewound": 3, "commits": 3}))
    # a block longer than the input window: letters at level 9 come in blocks of about 24 KiB compressed
    letters = bytes(rng.choices(LETTERS, k=200_000))
    out.append(Case("a block longer than the input window", GZIP, deflate(letters, GZIP, 9), letters, shape={"grown": 2, "max_in_window": 16384}))
    # a run of zeros larger than the output window: one block, no restart point inside it
    out.append(Case("zeros larger than the output window", ZLIB, deflate(bytes(1 << 20), ZLIB), bytes(1 << 20), shape={"grown": 4, "max_out_window": 1 << 20}))
    # gzip members with zero padding across window ends: decoded, never indexed
    streams, caps, expect = legs_ref.member_streams()
    whole = expect[0][1]
    first = len(expect[2][1])
    parts = [whole[:first], whole[first:first + 80_000], whole[first + 80_000:]]
    m = [deflate(p, GZIP, 6) for p in parts]
    out.append(Case("three members", GZIP, streams[0], whole, index=False, shape={"legs": 3, "rewound": 2}))
    out.append(Case("three members, zero padding across window ends", GZIP, streams[1], whole, index=False, shape={"legs": 3, "rewound": 2}))
    out.append(Case("two members, zero padding", GZIP, m[0] + bytes(4096 - len(m[0]) % 4096 + 40) + m[1] + bytes(7), parts[0] + parts[1], index=False, shape={"legs": 3, "rewound": 2}))
    out.append(Case("one member, padding to the end", GZIP, streams[2], parts[0], shape={"legs": 3, "rewound": 2}))
    return out


def damaged_cases():
    """-> (name, wrap, file, the cut or None): cuts at every 997th byte and flipped bytes of a zlib and a gzip file, garbage behind the
    padding, a bad CRC in member 1 with a data error in member 3."""
    grainy = legs_ref.grainy()
    out = []
    for wrap, w in ((ZLIB, "zlib"), (GZIP, "gzip")):
        s = deflate(grainy[:120_000], wrap)
        for cut in range(0, len(s), 997):
            out.append(("%s cut at %d" % (w, cut), wrap, s[:cut], cut))
        rng = random.Random(3 + wrap)
        for _ in range(12):
            b = bytearray(s)
            at = rng.randrange(len(s))
            b[at] ^= 1 << rng.randrange(8)
            out.append(("%s flipped at %d" % (w, at), wrap, bytes(b), None))
    streams, caps, expect = legs_ref.member_streams()
    out.append(("garbage behind the padding", GZIP, streams[3], None))
    out.append(("a bad CRC in member 1, a data error in member 3", GZIP, streams[4], None))
    out.append(("a data error in member 3", GZIP, streams[5], None))
    return out


def rc_of_status(status):
    """The return code the file calls give for a stream status (include/zwz.h): 0 ZWZ_OK, 33 / 34 ZWZ_E_CHECKSUM (-7), else ZWZ_E_FORMAT (-6)."""
    return 0 if status == 0 else -7 if status in (33, 34) else -6


def libz_decodes(wrap, stream):
    """What libz makes of a whole file: its decoded bytes, or None if it raises or the file ends early."""
    try:
        if wrap == GZIP:
            out, rest = [], stream                         # (zeros may follow a member, not precede the first)
            while rest:
                d = zlib.decompressobj(31)
                out.append(d.decompress(rest))
                if not d.eof:
                    return None
                rest = d.unused_data.lstrip(b"\x00")
            return b"".join(out) if out else None
        d = zlib.decompressobj(15 if wrap == ZLIB else -15)
        data = d.decompress(stream)
        return data if d.eof else None
    except zlib.error:
        return None
