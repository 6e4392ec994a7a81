"""tests/piece_ref.py against libz on whole inputs, at a size where the whole input is cheap: the composed stream, checksums, offsets
and BGZF file of a sequence must be what libz writes for the bytes the sequence spells.  No GPU.  tests/test_gpu_beyond_4gib.py takes its
expectations from piece_ref "by construction"; this is what that construction rests on."""
import gzip
import struct
import zlib

import pytest

import bgzf_ref
import deflate_stream_ref
import gzi_ref
import piece_ref
from piece_ref import PIECE


class _Libz:
    """bgzf_ref.reference wants an oracle's deflate6: here libz at level 6, which tests/test_oracle.py holds the oracle to"""
    @staticmethod
    def deflate6(data):
        return zlib.compress(data, 6)


def _sequences():
    w = piece_ref.word(piece_ref.MIX_ALL, 1)[0]
    out = []
    for tail in (12345, 0):
        s = piece_ref.Sequence([], w[:40], piece_ref.corpus.text_like(77, tail))
        out.append(pytest.param(s, id="40 pieces, tail %d" % tail))
    # a whole word, two pieces and a tail: the word-level sums and bytes
    s = piece_ref.Sequence([piece_ref.word(piece_ref.MIX_MOSTLY_ZEROS, 2)], [piece_ref.LZ, piece_ref.RANDOM_B], piece_ref.corpus.skewed(5, 999))
    out.append(pytest.param(s, id="a word, 2 pieces, tail 999"))
    return out


def test_alphabet_body_lengths():
    """the six pieces and the lengths of their full-flush bodies under libz 1.2.11 at level 6 (random pieces are stored: 65 280 bytes,
    a 5-byte block header and the flush's empty stored block, twice over the 32 KiB mark)"""
    a = piece_ref.alphabet()
    assert [len(u.data) for u in a] == [PIECE] * 6
    assert [len(u.body) for u in a] == [65305, 65305, 25301, 84, 4466, 25545]
    assert a[0].data != a[1].data
    for u in a:
        assert u.body[-4:] == b"\x00\x00\xff\xff" and zlib.decompressobj(-15).decompress(u.body) == u.data


def test_words_mix_and_differ():
    idx, unit = piece_ref.word(piece_ref.MIX_MOSTLY_RANDOM, 0)
    assert len(idx) == piece_ref.WORD and len(unit.data) == piece_ref.WORD * PIECE
    assert 16 <= int((idx >= 2).sum()) <= 64                        # about one piece in eight compressible
    assert int((idx[1:] != idx[:-1]).sum()) >= piece_ref.WORD // 3  # neighbours differ often: a misplaced piece changes the bytes
    assert (piece_ref.word(piece_ref.MIX_MOSTLY_RANDOM, 1)[0] != idx).any()
    z = piece_ref.word(piece_ref.MIX_ZEROS_LZ, 0)[0]
    assert set(z.tolist()) == {piece_ref.ZEROS, piece_ref.LZ}


@pytest.mark.parametrize("seq", _sequences())
def test_composed_equals_libz(seq):
    data = seq.host_input()
    assert len(data) == seq.in_len == seq.n_full * PIECE + len(seq.tail.data)
    before = piece_ref.Sums.calls
    assert seq.crc32() == zlib.crc32(data)
    assert seq.adler32() == zlib.adler32(data)
    assert piece_ref.Sums.calls - before <= len(seq.units)
    for wrap in deflate_stream_ref.WRAPS:
        want = deflate_stream_ref.deflate_stream(data, wrap)
        got = seq.host_stream(wrap)
        assert got == want, wrap
        assert len(got) == seq.stream_len(wrap)
        assert got.startswith(seq.header(wrap)) and got.endswith(piece_ref.FINAL + seq.trailer(wrap))
    assert seq.header("gzip") == bytes.fromhex("1f8b0800000000000003")
    assert seq.trailer("gzip") == struct.pack("<II", zlib.crc32(data), len(data))
    assert gzip.decompress(seq.host_stream("gzip")) == data
    # offsets: piece i's input and body stand where the arrays say
    ino, outo = seq.in_offsets(), seq.out_offsets("zlib")
    z = seq.host_stream("zlib")
    assert len(ino) == len(outo) == seq.n_pieces + 1 and ino[-1] == seq.in_len and outo[-1] == len(z) - 6
    for i in (0, 1, seq.n_pieces // 2, seq.n_pieces - 1):
        assert piece_ref.full_flush_body(data[ino[i]:ino[i + 1]]) == z[outo[i]:outo[i + 1]], i
    # BGZF
    bg = seq.host_bgzf()
    assert bg == bgzf_ref.reference(_Libz, data)
    assert len(bg) == seq.bgzf_len
    assert [o for o, _ in gzi_ref.members(bg)] == [int(x) for x in seq.bgzf_offsets()]
    assert seq.gzi_entries() == gzi_ref.entries(bg)


def test_of_length_is_exact_and_cheap():
    n = 3 * piece_ref.WORD * PIECE + 17 * PIECE + 4321
    before = piece_ref.Sums.calls
    seq = piece_ref.Sequence.of_length(n, [piece_ref.MIX_MOSTLY_ZEROS, piece_ref.MIX_ZEROS_LZ], 3)
    assert (seq.in_len, len(seq.words), len(seq.extra), len(seq.tail.data)) == (n, 3, 17, 4321)
    seq.crc32()
    assert piece_ref.Sums.calls - before <= 2000
    data = seq.host_input()
    assert (seq.crc32(), seq.adler32()) == (zlib.crc32(data), zlib.adler32(data))
    assert seq.host_stream("gzip") == deflate_stream_ref.deflate_stream(data, "gzip")


def test_wrapped_isize():
    """the trailer of an input longer than 2^32 bytes carries its length mod 2^32 (no bytes are made for it)"""
    seq = piece_ref.Sequence([piece_ref.word(piece_ref.MIX_ZEROS_LZ, 0)] * 258, [], b"abc")
    assert seq.in_len == 258 * 256 * PIECE + 3 > 1 << 32
    assert seq.trailer("gzip")[4:] == struct.pack("<I", seq.in_len - (1 << 32))


def test_tune_tail():
    for want in (13048, 13049):
        t = piece_ref.tune_tail("text", 4, want)
        assert len(piece_ref.full_flush_body(t)) == want


def test_stream_ref_skips_zeros_as_lstrip_does():
    """stream_ref finds the next gzip member with numpy, not bytes.lstrip: the two agree, also across its 16 MiB steps"""
    import stream_ref
    step = 1 << 24
    cases = [b"", bytes(5), b"a", bytes(3) + b"x" + bytes(2), bytes(step) + b"q", bytes(step - 1) + b"q" + bytes(7), bytes(2 * step + 5)]
    for data in cases:
        for start in (0, 1, 3, step - 1, step, step + 1):
            if start <= len(data):
                assert stream_ref._first_nonzero(data, start) == len(data) - len(data[start:].lstrip(b"\x00")), (len(data), start)
    two = gzip.compress(b"x") + bytes(9) + gzip.compress(b"y") + bytes(4)
    assert stream_ref.reference(stream_ref.GZIP, two, 10) == (0, b"xy")
    assert stream_ref.reference(stream_ref.GZIP, two + b"q", 10) == (stream_ref.TRAILING, b"xy")
    assert stream_ref.reference(stream_ref.GZIP, bytes(9), 10) == (stream_ref.NEED_INPUT, b"")
