"""The two composing references' streams and seek indexes against the whole-input references, at 3 to 6 MiB where the whole input is
cheap: tests/dep_piece_ref.py against deflate_dep_ref.deflate_dep_stream / dep_index, and piece_ref.Sequence.index against
flush_index_ref.writer_index.  No GPU.  tests/test_gpu_index_beyond_4gib.py takes its expectations from the composers "by
construction"; this is what that construction rests on."""
import zlib

import pytest

import corpus
import deflate_dep_ref
import dep_piece_ref as dpr
import flush_index_ref
import piece_ref
from deflate_dep_ref import D, P

SPANS = (32768, 65536, 1 << 20)


def test_alphabet():
    """five units of 32 768 bytes; 5 first and 25 pair bodies, every one closed by a sync flush and decoding to its unit behind the
    window it was primed with; a compressible unit behind itself has a shorter body than at a stream's start (a body chosen by the
    wrong pair changes the bytes and the lengths behind it), and random units stay stored"""
    a = dpr.alphabet()
    assert [len(u) for u in a.units] == [P] * 5 and len(set(a.units)) == 5
    assert a.lens.shape == (6, 5)
    for u in range(5):
        bodies = [a.first[u]] + [a.pair[p][u] for p in range(5)]
        assert all(b.endswith(deflate_dep_ref.MARKER) for b in bodies)
        assert zlib.decompressobj(-15).decompress(a.first[u]) == a.units[u]
        for p in range(5):
            assert zlib.decompressobj(-15, zdict=a.units[p][P - D:]).decompress(a.pair[p][u]) == a.units[u]
        if u in (dpr.TEXT, dpr.LZ, dpr.SKEWED):
            assert len(a.pair[u][u]) < len(a.first[u]), dpr.NAMES[u]                # (behind itself a unit finds itself in the window)
    assert all(P < n <= P + 15 for n in a.lens[:, dpr.RANDOM])


def _spans_of(i, wrap):
    """Sequence i meets wrapper number w at span (i + w) % 3: the three sequences cover the nine (wrapper, span) pairs once each
    (the whole-input references check every entry with libz, which is what takes the time)"""
    return (SPANS[(i + deflate_dep_ref.WRAPS.index(wrap)) % 3],)


def _dep_sequences():
    idx = dpr.word(dpr.MIX_ALL, 1).idx
    return [pytest.param(0, dpr.Sequence([], idx[:100], corpus.text_like(77, 12345)), id="100 units, tail 12345"),
            pytest.param(1, dpr.Sequence([], idx[40:150], b""), id="110 units, no tail"),
            pytest.param(2, dpr.Sequence([], idx[70:190], corpus.random_bytes(78, P - 1)), id="120 units, tail 32767")]


@pytest.mark.parametrize("i,seq", _dep_sequences())
def test_dependent_composed_equals_the_whole_input_reference(i, seq):
    data = seq.host_input()
    assert 3 << 20 <= len(data) == seq.in_len <= 6 << 20
    assert (seq.crc32(), seq.adler32()) == (zlib.crc32(data), zlib.adler32(data))
    for wrap in deflate_dep_ref.WRAPS:
        want = deflate_dep_ref.deflate_dep_stream(data, wrap)
        assert seq.host_stream(wrap) == want, wrap
        assert seq.stream_len(wrap) == len(want)
        for span in SPANS:
            assert seq.entries(wrap, span) == deflate_dep_ref.entries_of(data, wrap, 6, span)
        for span in _spans_of(i, wrap):
            _, index = deflate_dep_ref.dep_index(data, wrap, 6, span)
            assert seq.index(wrap, span) == index, (wrap, span)


def test_dependent_words_take_their_first_body_from_the_word_in_front():
    """two different words, three units and a tail: 16 MiB through the word-level bytes, sums and lengths (gzip, one span)"""
    words = [dpr.word(dpr.MIX_HALF, 0), dpr.word(dpr.MIX_ALL, 2)]
    assert (words[0].idx != words[1].idx).any()
    seq = dpr.Sequence(words, [dpr.LZ, dpr.TEXT, dpr.ZEROS], corpus.skewed(5, 999))
    data = seq.host_input()
    assert len(data) == (2 * dpr.WORD + 3) * P + 999
    before = piece_ref.Sums.calls
    assert (seq.crc32(), seq.adler32()) == (zlib.crc32(data), zlib.adler32(data))
    assert piece_ref.Sums.calls - before <= 8
    stream, index = deflate_dep_ref.dep_index(data, "gzip", 6, 1 << 20)
    assert seq.host_stream("gzip") == stream and seq.index("gzip", 1 << 20) == index
    assert zlib.decompress(stream, 31) == data


def test_the_gpu_sequence_contains_every_ordered_pair():
    """the condition tests/test_gpu_index_beyond_4gib.py rests on: each of the 25 pair bodies, and so each libz call of the alphabet,
    is part of the stream the GPU has to reproduce; the stream stays near half of the input"""
    seq = dpr.gpu_sequence()
    assert seq.in_len == dpr.GPU_LEN == (1 << 32) + (1 << 28) + 5 * P + 12345
    assert seq.n_pieces > 139000 and len(seq.tail) == 12345
    assert seq.pairs() == {(p, u) for p in range(5) for u in range(5)}
    assert 0.4 * seq.in_len < seq.stream_len("gzip") < 0.6 * seq.in_len
    entries = seq.entries("gzip", 1 << 20)
    assert 4300 < len(entries) < 4400 and sum(1 for e in entries if e[1] >> 32) > 200
    assert len({seq.window(e[1] // P) for e in entries[1:]}) == 5
    assert seq.trailer("gzip")[4:] == (seq.in_len - (1 << 32)).to_bytes(4, "little")


def _flush_sequences():
    w = piece_ref.word(piece_ref.MIX_ALL, 1)[0]
    return [pytest.param(0, piece_ref.Sequence([], w[:50], corpus.text_like(77, 12345)), id="50 pieces, tail 12345"),
            pytest.param(1, piece_ref.Sequence([], w[100:155], b""), id="55 pieces, no tail"),
            pytest.param(2, piece_ref.Sequence([], w[3:63], corpus.lz_heavy(79, 65279)), id="60 pieces, tail 65279")]


@pytest.mark.parametrize("i,seq", _flush_sequences())
def test_independent_composed_index_equals_the_writer_index(i, seq):
    data = seq.host_input()
    assert 3 << 20 <= len(data) <= 6 << 20
    for wrap in deflate_dep_ref.WRAPS:
        for span in _spans_of(i, wrap):
            stream, index = flush_index_ref.writer_index(data, deflate_dep_ref.WRAP_ID[wrap], span)
            assert seq.host_stream(wrap) == stream
            assert seq.index(wrap, span) == index, (wrap, span)
