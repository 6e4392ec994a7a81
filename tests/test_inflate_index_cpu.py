"""The seek index of ordinary streams without a GPU: index_core.h's parse and plan, and the CPU emulation of inflate_kernel's marking
and indexed-segment forms (tests/emu/index_emu.cpp) against libz (tests/index_ref.py)."""
import random
import zlib

import pytest

import deflate_gen
import index_emu_binding as emu
import index_ref
import stream_corpus
from index_ref import GZIP, RAW, ZLIB

WB = index_ref.WBITS


@pytest.fixture(scope="module")
def lib():
    return emu.load()


@pytest.fixture(scope="module")
def text():
    return deflate_gen.text(random.Random(7), 1_400_000)


@pytest.fixture(scope="module")
def flushed(text):
    """The issue's 1.4 MB text stream with 14 sync-flush points and its Python-composed index."""
    cuts = [100_000 * i for i in range(1, 15)]
    stream, idx = index_ref.sync_flush_stream(text, cuts, GZIP)
    return stream, idx, cuts


def test_reference_index_passes_the_libz_check(flushed, text, lib):
    stream, idx, cuts = flushed
    ix = index_ref.check_index(idx, stream, text, GZIP)
    assert [e[1] for e in ix.entries] == [0] + cuts
    fault, f = emu.parse(lib, idx)
    assert fault == "ok" and f["count"] == 15 and f["decoded_len"] == len(text) and f["end_bit"] == ix.end_bit


# ---- index_parse: one assertion per rule --------------------------------------------------------------------------------------

def _small(text):
    data = text[:200_000]
    stream, idx = index_ref.sync_flush_stream(data, [20_000, 70_000, 140_000], ZLIB)
    return data, stream, index_ref.parse(idx), idx


def test_parse_refuses_malformed_indexes(lib, text):
    data, stream, ix, idx = _small(text)
    assert emu.parse(lib, idx)[0] == "ok"
    assert emu.parse(lib, b"ZWZIDX\x00\x02" + idx[8:])[0] == "magic"
    assert emu.parse(lib, idx[:48])[0] == "length"                                  # shorter than a header
    assert emu.parse(lib, idx + bytes(8))[0] == "length"                            # not a multiple of 16
    assert emu.parse(lib, idx + bytes(16))[0] in ("crc", "window_sum")              # longer than its windows
    assert emu.parse(lib, index_ref.compose(ix, crc=zlib.crc32(idx[64:]) ^ 1))[0] == "crc"
    flipped = bytearray(idx)
    flipped[-20] ^= 1                                                               # a window byte, CRC not redone
    assert emu.parse(lib, bytes(flipped))[0] == "crc"
    # the windows' sum against the length (CRC right): a window one byte short of its hist
    cut = index_ref.Index(**{**ix.__dict__, "windows": ix.windows[:-1] + [ix.windows[-1][:-17]]})
    assert emu.parse(lib, index_ref.compose(cut))[0] == "window_sum"
    e = ix.entries
    swapped = index_ref.Index(**{**ix.__dict__, "entries": [e[0], e[2], e[1], e[3]], "windows": [ix.windows[i] for i in (0, 2, 1, 3)]})
    assert emu.parse(lib, index_ref.compose(swapped))[0] == "order"
    same_bit = index_ref.Index(**{**ix.__dict__, "entries": [e[0], e[1], (e[1][0], e[2][1], e[2][2]), e[3]]})
    assert emu.parse(lib, index_ref.compose(same_bit))[0] == "order"
    falling = index_ref.Index(**{**ix.__dict__, "entries": [e[0], e[1], (e[2][0], e[1][1] - 1, e[2][2]), e[3]]})
    assert emu.parse(lib, index_ref.compose(falling))[0] == "order"
    first = index_ref.Index(**{**ix.__dict__, "entries": [(e[0][0], 1, 0)] + e[1:]})
    assert emu.parse(lib, index_ref.compose(first))[0] == "order"                   # entry 0 is decoded offset 0
    over = index_ref.Index(**{**ix.__dict__, "entries": [e[0], (e[1][0], e[1][1], e[1][1] + 1)] + e[2:], "windows": [b"", data[:20_001]] + ix.windows[2:]})
    assert emu.parse(lib, index_ref.compose(over))[0] == "hist"                     # 20 001 > min(32768, 20 000)
    over32 = index_ref.Index(**{**ix.__dict__, "entries": e[:3] + [(e[3][0], e[3][1], 32769)], "windows": ix.windows[:3] + [data[140_000 - 32769:140_000]]})
    assert emu.parse(lib, index_ref.compose(over32))[0] == "hist"
    beyond = index_ref.Index(**{**ix.__dict__, "end_bit": 8 * len(stream) + 1})
    assert emu.parse(lib, index_ref.compose(beyond))[0] == "end_bit"
    before = index_ref.Index(**{**ix.__dict__, "end_bit": e[3][0]})
    assert emu.parse(lib, index_ref.compose(before))[0] == "end_bit"
    assert emu.parse(lib, index_ref.compose(index_ref.Index(**{**ix.__dict__, "span": 3 << 14})))[0] == "field"
    assert emu.parse(lib, index_ref.compose(index_ref.Index(**{**ix.__dict__, "wrap": 3})))[0] == "field"
    assert emu.parse(lib, index_ref.compose(index_ref.Index(**{**ix.__dict__, "decoded_len": 1032 * len(stream) + 1032})))[0] == "field"
    assert emu.parse(lib, index_ref.compose(index_ref.Index(**{**ix.__dict__, "decoded_len": 1032 * len(stream)})))[0] == "ok"


# ---- index_plan against a brute-force plan ---------------------------------------------------------------------------------

def brute_plan(ix, ranges):
    """Byte by byte: which segment holds every requested byte (the LAST entry at or below it), runs joined per range."""
    offs = [e[1] for e in ix.entries]
    rows, dst = {}, 0
    for a, n in ranges:
        run = None
        for x in range(a, a + n):
            s = max(k for k, o in enumerate(offs) if o <= x)
            if run and run[0] == s:
                run[3] += 1
            else:
                run = [s, dst, x - offs[s], 1]
                rows.setdefault(s, []).append(run)
            dst += 1
    segs = sorted(rows)
    return segs, [[(r[1], r[2], r[3]) for r in rows[s]] for s in segs]


def test_plan_matches_brute_force(lib, text):
    data, stream, ix, idx = _small(text)
    n = len(data)
    cases = [
        [(5, 0), (70_000, 0), (n, 0)],                                   # zero-length ranges, one at the very end
        [(19_990, 120_100)],                                             # across three boundaries: four segments
        [(69_999, 2), (139_950, 100)],
        [(n - 1, 1), (n - 4096, 4096), (0, 1)],                          # ending at the last byte
        [(0, 300), (20_000, 1), (19_999, 1), (150_000, 50), (30, 40_000), (150_000, 50)],   # any order, overlapping, repeated
    ]
    rng = random.Random(3)
    cases.append([(rng.randrange(n - 600), rng.randrange(600)) for _ in range(40)])
    for ranges in cases:
        bad, segs, row, pieces = emu.plan(lib, idx, ranges)
        assert bad == -1
        want_segs, want_rows = brute_plan(ix, ranges)
        assert segs == want_segs
        assert [pieces[row[i]:row[i + 1]] for i in range(len(segs))] == want_rows
    assert emu.plan(lib, idx, [(0, 10), (n, 1)])[0] == 1                 # one past the end
    assert emu.plan(lib, idx, [(n + 1, 0)])[0] == 0
    assert emu.plan(lib, idx, [(1, 2 ** 64 - 1)])[0] == 0                # offset + length overflows


# ---- the marking form against libz -------------------------------------------------------------------------------------

def _check_built(lib, wrap, stream, data, span, seen_bits, hists):
    st, out, idx = emu.build(lib, wrap, stream, len(data) + 5, span)
    assert st == 0 and out == data
    ix = index_ref.check_index(idx, stream, data, wrap)
    assert ix.span == span
    offs = [e[1] for e in ix.entries]
    assert all(b - a >= span for a, b in zip(offs, offs[1:]))
    assert all(e[2] == min(32768, e[1]) for e in ix.entries)
    for bit, off, hist in ix.entries:
        seen_bits.add(bit & 7)
        if off:
            hists.add(hist == 32768)
    return ix, idx


def test_marking_form_on_libz_levels(lib, text):
    seen_bits, hists, counts = set(), set(), []
    rng = random.Random(11)
    # letters with little to match, a slice of text every 4 KiB: blocks of 16 383 symbols end every 20 to 30 KB
    mixed = b"".join(bytes(rng.choices(b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789+/", k=4096)) + text[4096 * i:4096 * i + 1500]
                     for i in range(180))
    for level in (1, 6, 9):
        for wrap in (RAW, ZLIB, GZIP):
            for span in (16384, 65536):
                data = text[:900_000] if (level + wrap) % 2 else mixed
                c = zlib.compressobj(level, zlib.DEFLATED, WB[wrap])
                stream = c.compress(data) + c.flush()
                ix, _ = _check_built(lib, wrap, stream, data, span, seen_bits, hists)
                counts.append(len(ix.entries))
    assert max(counts) >= 24                                 # dozens of segments in one stream
    assert seen_bits == set(range(8)), seen_bits             # a checkpoint at every bit offset of a byte
    assert hists == {True, False}                            # a window below 32768 and a full one


def test_marking_form_on_the_stream_corpus(lib):
    """Every stream of the inflate corpus: statuses and bytes as the stream decode's (libz's), an index exactly for the good one-member
    streams, every entry through the libz check."""
    import stream_ref
    made = none = 0
    for wrap, streams in stream_corpus.corpus(big=False, n_conformance=60).items():
        for s in streams:
            st, out, idx = emu.build(lib, wrap, s.data, s.cap, 16384)
            assert stream_ref.accept(wrap, s.data, s.cap, st, out) is None, s.name
            if st != 0:
                assert idx == b"", s.name
                continue
            if idx:
                index_ref.check_index(idx, s.data, out, wrap)
                made += 1
            else:
                none += 1
                assert wrap == GZIP and s.data.count(b"\x1f\x8b") >= 2, s.name     # only a second member leaves a good stream without one
    assert made > 100 and none >= 1


def test_no_index_for_two_members_but_for_zero_padding(lib, text):
    a, b = text[:50_000], text[50_000:90_000]
    two = stream_corpus.gz_member(a) + stream_corpus.gz_member(b)
    st, out, idx = emu.build(lib, GZIP, two, 100_000, 16384)
    assert st == 0 and out == a + b and idx == b""
    padded = stream_corpus.gz_member(a) + bytes(300)
    st, out, idx = emu.build(lib, GZIP, padded, 100_000, 16384)
    assert st == 0 and out == a
    index_ref.check_index(idx, padded, a, GZIP)
    # a capacity too small for the index: the decode is whole, no index
    st, out, idx = emu.build(lib, GZIP, padded, 100_000, 16384, idx_cap=64 + 24 + 8)        # (entry 0 and the padding need 64 + 24 + 15)
    assert st == 0 and out == a and idx == b""
    assert emu.build(lib, GZIP, padded, 100_000, 16384, idx_cap=lib.emu_index_bound(len(a), 16384))[2] != b""


# ---- the indexed-segment form: lanes in random order ---------------------------------------------------------------------

def test_segment_form_equals_libz_slices(lib, text, flushed):
    stream, ref_idx, _ = flushed
    c = zlib.compressobj(9, zlib.DEFLATED, -15)
    raw = c.compress(text[:700_000]) + c.flush()
    _, _, own_idx = emu.build(lib, RAW, raw, 700_000, 16384)
    rng = random.Random(5)
    for s, idx, data in ((stream, ref_idx, text), (raw, own_idx, text[:700_000])):
        ix = index_ref.parse(idx)
        offs = [e[1] for e in ix.entries] + [ix.decoded_len]
        for k, (bit, off, hist) in enumerate(ix.entries):
            good, got = emu.segment(lib, s, idx, k, hist, offs[k + 1] - off, shift=rng.randrange(16), seed=rng.getrandbits(60))
            assert good == 1, k
            assert got == data[off:offs[k + 1]], k


def test_segment_form_refuses_a_lying_index(lib, text):
    data, stream, ix, idx = _small(text)
    e = ix.entries
    offs = [x[1] for x in e] + [ix.decoded_len]

    def run(ix2, k):
        lied = index_ref.compose(ix2)
        assert emu.parse(lib, lied)[0] == "ok"
        o = [x[1] for x in ix2.entries] + [ix2.decoded_len]
        return emu.segment(lib, stream, lied, k, ix2.entries[k][2], o[k + 1] - o[k])[0]

    assert run(ix, 2) == 1
    bit_off = index_ref.Index(**{**ix.__dict__, "entries": [e[0], e[1], (e[2][0] + 1, e[2][1], e[2][2]), e[3]]})
    assert run(bit_off, 2) == 0 and run(bit_off, 1) == 0                  # the segment that starts there, and the one that ends there
    dec_off = index_ref.Index(**{**ix.__dict__, "entries": [e[0], e[1], (e[2][0], e[2][1] + 1, e[2][2]), e[3]],
                                 "windows": ix.windows[:2] + [data[e[2][1] + 1 - e[2][2]:e[2][1] + 1], ix.windows[3]]})
    assert run(dec_off, 1) == 0 and run(dec_off, 2) == 0                  # one byte more than the blocks give; one byte less
    inside = index_ref.Index(**{**ix.__dict__, "end_bit": ix.end_bit - 9})
    assert run(inside, 3) == 0                                            # an end bit inside the final block
