"""The seek index at full-flush points on the CPU: the reference (tests/flush_index_ref.py, libz and the rule in plain Python, every
entry put through index_ref.check_index) against a host build of csrc/index_core.h's index_flush_due and sealing helper inside the
loops the kernels run (tests/emu_flush_index).  No GPU."""
import zlib

import pytest

import corpus as kinds
import flush_index_emu_binding as emu
import flush_index_ref as ref
import index_ref
import split_corpus
from index_ref import GZIP, RAW, ZLIB

SPANS = (16384, 131072, 262144)
WRAPS = (RAW, ZLIB, GZIP)
TEXT_LEN = 785000
IRREGULAR = [100, 5000, 16384, 16385, 40000, 131072, 131079, 300000, TEXT_LEN]


@pytest.fixture(scope="module")
def lib():
    return emu.load()


@pytest.fixture(scope="module")
def text():
    return kinds.text_like(2031, TEXT_LEN)


def _check_of(wrap, data):
    return zlib.crc32(data) if wrap == GZIP else zlib.adler32(data) if wrap == ZLIB else 0


def _both(lib, stream, data, wrap, span, points, end_bit):
    """The reference and the emulation's compaction of the same points; the emulation's own parse accepts the result"""
    want = ref.compose(stream, data, wrap, span, points, end_bit)
    got = emu.index(lib, wrap, span, len(stream), len(data), end_bit, _check_of(wrap, data), points)
    assert got == want
    fault, f = emu.parse(lib, got)
    assert fault == "ok" and f["count"] == len(ref.entries_of(points, len(data), span)) and f["win_off"] + (-f["win_off"]) % 16 == len(got)
    assert len(got) <= lib.emu_flush_bound(len(data), span)
    return want


@pytest.mark.parametrize("wrap", WRAPS)
def test_the_writers_cuts_give_the_counted_entries(lib, text, wrap):
    stream, points, end_bit = ref.flush_stream(text, ref.writer_cuts(TEXT_LEN), wrap)
    assert len(points) == 14                                   # 12 pieces and a tail, and the empty final block
    for span, count in zip(SPANS, (13, 6, 3)):
        idx = _both(lib, stream, text, wrap, span, points, end_bit)
        assert len(index_ref.parse(idx).entries) == count


@pytest.mark.parametrize("wrap", WRAPS)
def test_irregular_cuts(lib, text, wrap):
    stream, points, end_bit = ref.flush_stream(text, IRREGULAR, wrap)
    idx = _both(lib, stream, text, wrap, 16384, points, end_bit)
    assert [o for _, o, _ in index_ref.parse(idx).entries] == [0, 16384, 40000, 131072, 300000]
    # a non-empty last piece: the end bit comes from the search
    stream, points, end_bit = ref.flush_stream(text, IRREGULAR[:-1], wrap)
    _both(lib, stream, text, wrap, 16384, points, end_bit)


@pytest.mark.parametrize("wrap", WRAPS)
def test_edge_streams(lib, text, wrap):
    for n in (0, 1, 65280, 65281):
        stream, points, end_bit = ref.flush_stream(text[:n], ref.writer_cuts(n), wrap)
        for span in SPANS:
            _both(lib, stream, text[:n], wrap, span, points, end_bit)
    small = text[:300000]
    for how in (dict(doubled=(1, 3)), dict(first_flush=True), dict(level=1), dict(level=9)):
        stream, points, end_bit = ref.flush_stream(small, list(range(50000, 300000, 50000)), wrap, **how)
        _both(lib, stream, small, wrap, 16384, points, end_bit)
    # a cut exactly on a bucket boundary, and an empty last piece behind it
    stream, points, end_bit = ref.flush_stream(small, [131072, 262144, 300000], wrap)
    idx = _both(lib, stream, small, wrap, 131072, points, end_bit)
    assert [o for _, o, _ in index_ref.parse(idx).entries] == [0, 131072, 262144]


@pytest.mark.parametrize("wrap", WRAPS)
@pytest.mark.parametrize("m,lead", [(1 << 20, 0), (4, 0), (4, 3), (1, 0), (5, 7)])
def test_the_writers_loops_in_slices(lib, text, wrap, m, lead):
    """The index does not depend on how the pieces fall into slices, nor on what stands in front of the stream in the call"""
    for n in (0, 1, 65280, 65281, TEXT_LEN):
        data = text[:n]
        for span in SPANS:
            stream, want = ref.writer_index(data, wrap, span)
            points = ref.points_of(stream, wrap)
            slen = [b - a for (a, _), (b, _) in zip(points, points[1:])]
            assert len(slen) == -(-n // ref.PIECE)
            assert emu.writer(lib, wrap, span, n, slen, _check_of(wrap, data), m, lead) == want
            short = emu.writer(lib, wrap, span, n, slen, _check_of(wrap, data), m, lead, cap=len(want) - 16)
            assert short == b""


def test_bound_is_reached_and_never_exceeded(lib):
    for span in SPANS + (1 << 20,):
        assert lib.emu_flush_bound(0, span) == 96
        for n in (1, span - 1, span, span + 1, 5 * span + 1, TEXT_LEN, 7 * ref.PIECE, 7 * ref.PIECE + 1, (1 << 24) + 12345):
            pieces = [(10 + k, k * ref.PIECE) for k in range(-(-n // ref.PIECE))] or [(10, 0)]
            count = len(ref.entries_of(pieces, n, span))
            bound = lib.emu_flush_bound(n, span)
            assert bound == (64 + 24 * (n // span + 1) + 15) // 16 * 16
            assert (64 + 24 * count + 15) // 16 * 16 <= bound
    # reached: every bucket of a span above a piece holds a piece start when the last bucket does
    assert len(ref.entries_of([(10 + k, k * ref.PIECE) for k in range(13)], TEXT_LEN, 131072)) == TEXT_LEN // 131072 + 1
    assert len(ref.entries_of([(10 + k, k * ref.PIECE) for k in range(13)], TEXT_LEN, 262144)) == TEXT_LEN // 262144 + 1
    for bad in (0, 8192, 16385, 3 << 14, 1 << 31):
        assert lib.emu_flush_bound(TEXT_LEN, bad) == 0


def test_split_corpus_group_a(lib):
    n = 0
    for it in split_corpus.corpus(2027, big=False):
        if it.group != "a":
            continue
        data = zlib.decompress(it.data, index_ref.WBITS[it.wrap])
        points = ref.points_of(it.data, it.wrap)
        assert len(points) in (it.chain, it.chain + 1) or len(data) == 0      # (the empty final block behind the last marker is a point too)
        # the end bit: behind an empty last piece the writer's rule; else the search, from the last point
        last, tail = points[-1][0], ref.TRAILER[it.wrap]
        if it.data[last:len(it.data) - tail] == b"\x03\x00":
            end_bit = 8 * last + 10
        else:
            end_bit = ref._end_bit(it.data, data, last, points[-1][1], tail)
        span = SPANS[n % 3]
        _both(lib, it.data, data, it.wrap, span, points, end_bit)
        n += 1
    assert n > 100
