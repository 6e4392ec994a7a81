"""BGZF streams for the tests of the member walk and of chunk reads, built once: well-formed ones from the Python writers of bgzf_ref
and gzi_ref, and damaged variants of one of them.  Test infrastructure only."""
import struct
import zlib

import bgzf_ref
import corpus
import gzi_ref

B = bgzf_ref.BLOCK


def _full_member():
    """One member of exactly 65 536 bytes: 65 505 random bytes in one stored block (5 + 65 505 body bytes, 18 + 8 of framing)."""
    blk = corpus.random_bytes(31, 65505)
    body = b"\x01" + struct.pack("<HH", len(blk), len(blk) ^ 0xffff) + blk
    assert zlib.decompress(body, -15) == blk
    m = bgzf_ref.member(blk, body)
    assert len(m) == 65536
    return m, blk


def _good():
    text = corpus.text_like(21, 3 * B + 77)
    out = {}
    out["empty"] = (b"", b"")
    out["eof_only"] = (bgzf_ref.EOF, b"")
    out["one_member"] = (bgzf_ref.other_writer(text[:1000], 6, eof=False), text[:1000])
    out["plain"] = (bgzf_ref.other_writer(text, 6), text)
    out["extra"] = (bgzf_ref.other_writer(text[:100000], 6, block=20000, extra=True), text[:100000])
    out["joined"] = (bgzf_ref.other_writer(text[:70000], 6) + bgzf_ref.EOF + bgzf_ref.other_writer(text[70000:90000], 1, block=7000), text[:90000])
    out["no_eof"] = (bgzf_ref.other_writer(text[:150000], 6, block=30000, eof=False), text[:150000])
    full, blk = _full_member()
    out["full_member"] = (bgzf_ref.other_writer(text[:500], 6, eof=False) + full + bgzf_ref.other_writer(text[500:1300], 6, block=200),
                          text[:500] + blk + text[500:1300])
    tiny = corpus.text_like(22, 5000)
    out["tiny_members"] = (gzi_ref.sized_writer(tiny, [1]), tiny)
    # a BGZF file of random bytes, stored (level 0) inside another: whole valid headers at offsets that are no members
    inner = bgzf_ref.other_writer(corpus.random_bytes(23, 150000), 6, block=9000)
    out["nested"] = (bgzf_ref.other_writer(inner, 0, block=40000), inner)
    return out


GOOD = _good()


def _damaged():
    """name -> damaged stream, from GOOD["plain"] (members 0..3 and the EOF member)"""
    gz = GOOD["plain"][0]
    ms = gzi_ref.members(gz)
    o2 = ms[2][0]
    out = {}
    b = bytearray(gz); b[o2 + 1] ^= 0x40
    out["bad_magic_member2"] = bytes(b)
    b = bytearray(gz); b[0] = 0x1e
    out["bad_magic_member0"] = bytes(b)
    b = bytearray(gz); b[o2 + 12] = ord("X")
    out["no_bc"] = bytes(b)
    b = bytearray(gz); struct.pack_into("<H", b, ms[-1][0] + 16, 999)
    out["bsize_past_end"] = bytes(b)
    out["cut_last_member"] = gz[:-5]
    out["cut_in_header"] = gz[:ms[-1][0] + 7]
    out["trailing_garbage"] = gz + b"\x00garbage"
    out["trailing_two_bytes"] = gz + b"\x1f\x8b"
    b = bytearray(gz); struct.pack_into("<I", b, ms[3][0] - 4, 65536)
    out["isize_above_65535"] = bytes(b)
    b = bytearray(gz); b[o2 + 3] = 0x0c
    out["flags"] = bytes(b)
    b = bytearray(gz); b[o2 + 3] = 0x00
    out["no_extra"] = bytes(b)
    b = bytearray(gz); struct.pack_into("<H", b, o2 + 16, 20)
    out["bsize_small"] = bytes(b)
    return out


DAMAGED = _damaged()


def decoded_offsets(gz):
    """{compressed offset of a member: (decoded offset of its first byte, ISIZE)}, and the decoded size"""
    table, raw = {}, 0
    for o, isize in gzi_ref.members(gz):
        table[o] = (raw, isize)
        raw += isize
    return table, raw


def chunk_slice(gz, data, vbeg, vend):
    """The chunk (vbeg, vend) of a well-formed stream by the definition of include/zwz.h: data[P(vbeg):P(vend)]"""
    table, raw = decoded_offsets(gz)

    def pos(v):
        c, w = v >> 16, v & 0xffff
        if c == len(gz):
            assert w == 0
            return raw
        u, isize = table[c]
        assert w <= isize
        return u + w
    return data[pos(vbeg):pos(vend)]
