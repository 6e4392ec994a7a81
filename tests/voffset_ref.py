"""Decoded offsets -> BGZF virtual offsets by a .gzi, in Python (include/zwz.h: zwz_bgzf_voffsets).  Test infrastructure only."""
import bisect

import gzi_ref


def voffsets(gzi: bytes, offsets):
    """The member of an offset is the LAST index entry whose decoded offset is at or below it; ValueError where the library refuses."""
    ents = gzi_ref.read(gzi)                # [(compressed, decoded)] with the implied (0, 0)
    us = [u for _, u in ents]
    out = []
    for a in offsets:
        c, u = ents[bisect.bisect_right(us, a) - 1]
        if c >= 1 << 48 or a - u >= 65536:
            raise ValueError("offset %d" % a)
        out.append(c << 16 | (a - u))
    return out
