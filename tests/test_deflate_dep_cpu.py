"""zwz_deflate_dep_streams_dev's format without a GPU: the host build of the portable cores with a start offset (tests/emu_dep) must
write, byte for byte, what libz writes for pieces of 32 768 bytes primed with the 32 512 bytes in front of them
(tests/deflate_dep_ref.py), at levels 4, 5 and 6; the bounds hold; the index with windows equals a reference written from the rule."""
import random
import zlib

import pytest

import corpus
import deflate_dep_emu_binding as emu_binding
import deflate_dep_ref as ref
import deflate_stream_ref
import dep_cases
import flush_index_emu_binding
import index_ref

P, D = ref.P, ref.D
LENGTHS = (0, 1, 2, 3, 259, 32767, 32768, 32769, 65535, 65536, 65537, 98309)
KINDS = ("text", "lz", "periodic", "lowent", "random", "gradient")      # text_like, lz_heavy, periodic, low_entropy, random_bytes, gradient
K_SLIDE, K_WSIZE, K_MAXDIST, K_SYMS = 65274, 32768, 32506, 16383


@pytest.fixture(scope="module")
def emu():
    return emu_binding.load()


def test_reference_is_what_the_issue_states():
    assert ref.deflate_dep_stream(b"", "raw") == b"\x03\x00"
    assert ref.deflate_dep_stream(b"", "zlib") == b"\x78\x9c\x03\x00\x00\x00\x00\x01"
    assert ref.deflate_dep_stream(b"", "gzip") == bytes.fromhex("1f8b0800000000000003") + b"\x03\x00" + bytes(8)
    data = corpus.text_like(3, 3 * P + 100)
    for wrap in ref.WRAPS:
        for level in (4, 5, 6):
            out = ref.deflate_dep_stream(data, wrap, level)
            assert zlib.decompress(out, deflate_stream_ref.WBITS[wrap]) == data
            assert out.count(ref.MARKER) >= 4
            if wrap == "zlib":
                assert out[1] & 0x20 == 0          # no FDICT
    # a dependent piece refers back: the second piece alone does not decode without its dictionary
    shares = ref.pieces(data)
    with pytest.raises(zlib.error):
        zlib.decompressobj(-15).decompress(shares[1])
    assert zlib.decompressobj(-15, zdict=data[P - D:P]).decompress(shares[1]) == data[P:2 * P]


@pytest.mark.parametrize("level", (4, 5, 6))
@pytest.mark.parametrize("kind", KINDS)
def test_emu_writes_libz_dependent_streams(emu, kind, level):
    for i, n in enumerate(LENGTHS):
        data = corpus.make(kind, 11 + n % 7, n)
        wrap = ref.WRAPS[(i + level) % 3]
        got, want = emu_binding.stream(emu, data, wrap, level, 2), ref.deflate_dep_stream(data, wrap, level)
        assert got == want, (kind, level, n, wrap, len(got), len(want))


def test_every_wrapper_at_every_length(emu):
    for n in LENGTHS:
        data = corpus.text_like(5, n)
        for wrap in ref.WRAPS:
            assert emu_binding.stream(emu, data, wrap, 6, 1) == ref.deflate_dep_stream(data, wrap, 6), (n, wrap)


def both(emu, data, level=6):
    got, want = emu_binding.stream(emu, data, "zlib", level), ref.deflate_dep_stream(data, "zlib", level)
    assert got == want
    return got


def test_match_at_the_window_edge_from_a_piece_s_first_byte(emu):
    # piece 1 starts at chunk position D; a match from there reaches distance MAX_DIST = 32 506 and not 32 507
    rng = random.Random(1)
    pat = rng.randbytes(40)
    for dist, hit in ((K_MAXDIST, True), (K_MAXDIST + 1, False), (K_MAXDIST - 1, True)):
        data = bytearray(rng.randbytes(2 * P))
        data[P - dist:P - dist + 40] = pat
        data[P:P + 40] = pat
        data = bytes(data)
        tok, rec = emu_binding.piece(emu, data[P - D:2 * P], D)
        assert rec[0]["start"] == D
        assert (tok[0] == (40, dist)) == hit, (dist, tok[:3])
        if not hit:
            assert tok[0] == (0, pat[0])
        both(emu, data)


def test_slid_window_hides_dictionary_bytes_from_the_last_positions(emu):
    # a full piece: at chunk positions >= 65 274 libz's window has slid and a chain entry at chunk position <= 32 768 reads as NIL
    rng = random.Random(2)
    q = K_SLIDE                                 # the first position behind the slide; K_WSIZE lies MAX_DIST in front of it
    for at, hit in ((K_WSIZE, False), (K_WSIZE + 1, True)):
        chunk = dep_cases.slid_window_chunk(rng, at)      # `at` is the chain's first entry for q
        tok, rec = emu_binding.piece(emu, chunk, D)
        if hit:
            assert tok[-3] == (4, q - at) and tok[-2][0] == 0 and tok[-1][0] == 0, tok[-3:]
        else:
            assert q - at == K_MAXDIST and [t[0] for t in tok[-6:]] == [0] * 6, tok[-6:]
        data = rng.randbytes(P - D) + chunk      # the chunk is piece 1 and its dictionary
        assert len(data) == 2 * P
        both(emu, data)


def test_full_piece_of_one_block_is_not_stored(emu):
    # a full piece behind a dictionary that is one block: it starts at 32 512 < 32 768 and is flushed at 65 280 >= 65 274
    rng = random.Random(3)
    seen = 0
    for lit in (1, 2, 3, 8):
        for data in dep_cases.one_block_bodies(rng, lit):
            tok, rec = emu_binding.piece(emu, data[P - D:], D)
            assert len(rec) == 1 and len(tok) <= K_SYMS and rec[0]["start"] == D < K_WSIZE and rec[0]["flush_pos"] == D + P >= K_SLIDE
            assert rec[0]["type"] != emu_binding.STORED
            seen += 1
            out = both(emu, data)
            assert len(out) <= emu.emu_dep_stream_bound(len(data), 1)
    assert seen == 12


def test_pieces_of_several_blocks_and_stored_pieces(emu):
    rng = random.Random(4)
    data = dep_cases.stored_pieces_input(rng)
    # piece 1, full and incompressible: several blocks, all stored (the first is flushed before the window slides)
    tok, rec = emu_binding.piece(emu, data[P - D:2 * P], D)
    assert len(rec) >= 2 and rec[0]["n_sym"] == K_SYMS and sum(r["n_sym"] for r in rec) == len(tok)
    assert [r["type"] for r in rec] == [emu_binding.STORED] * len(rec) and sum(r["bytes"] for r in rec) == P
    assert rec[0]["start"] == D and rec[0]["flush_pos"] < K_SLIDE and rec[1]["start"] >= K_WSIZE
    # piece 2, short: one stored block
    tok, rec = emu_binding.piece(emu, data[2 * P - D:], D)
    assert len(rec) == 1 and rec[0]["type"] == emu_binding.STORED and rec[0]["bytes"] == 10000
    both(emu, data)
    # several coded blocks: literals of a small alphabet
    data = corpus.low_entropy(9, 2 * P, 200)
    tok, rec = emu_binding.piece(emu, data[P - D:], D)
    assert len(rec) >= 2 and all(r["type"] == emu_binding.DYNAMIC for r in rec[:2])
    both(emu, data)


def test_bound_holds(emu):
    rng = random.Random(5)
    for n in LENGTHS:
        for data in (rng.randbytes(n), corpus.text_like(1, n)):
            for w, wrap in enumerate(ref.WRAPS):
                for level in (4, 6):
                    assert emu.emu_dep_stream_bound(n, w) >= len(ref.deflate_dep_stream(data, wrap, level)), (n, wrap)
    for w in range(3):
        assert emu.emu_dep_stream_bound(0, w) == (2, 8, 20)[w]
        assert emu.emu_dep_stream_bound(1 << 30, w) < 1.002 * (1 << 30)
        for n in list(range(0, 70)) + [16382, 16383, 16384, P - 1, P, P + 1, 3 * P + 5]:
            assert emu.emu_dep_stream_bound(n, w) >= n + (2, 8, 20)[w] + 5 * -(-n // P)
    # the term of the block that may not be stored: every full piece behind a dictionary, and the shorter ones that reach the slide
    assert emu.emu_dep_piece_bound(P, D) - emu.emu_dep_piece_bound(P, 0) == 28
    assert emu.emu_dep_piece_bound(K_SLIDE - D, D) - emu.emu_dep_piece_bound(K_SLIDE - D - 1, D) == 30


@pytest.mark.parametrize("span", (16384, 32768, 65536, 1 << 20))
def test_index_equals_the_reference(emu, span):
    fl = flush_index_emu_binding.load()
    for n, wrap, level in ((0, "gzip", 6), (1, "raw", 6), (P, "zlib", 6), (P + 1, "gzip", 5), (5 * P - 7, "gzip", 6), (9 * P, "zlib", 4), (9 * P + 1, "raw", 6)):
        data = corpus.text_like(n % 11, n)
        stream, want = ref.dep_index(data, wrap, level, span)
        got = emu_binding.index(emu, data, wrap, level, span)
        assert got == want, (n, wrap, span, len(got), len(want))
        assert len(got) == emu.emu_dep_index_bound(n, span)          # the bound is exact: reached, never exceeded
        fault, f = flush_index_emu_binding.parse(fl, got)             # index_parse accepts it
        assert fault == "ok" and f["count"] == len(index_ref.parse(got).entries) and f["decoded_len"] == n
        ix = index_ref.parse(got)
        assert [h for _, _, h in ix.entries] == [0] + [D] * (len(ix.entries) - 1)
    assert emu.emu_dep_index_bound(100, 12345) == 0


def test_dependent_streams_are_smaller():
    # the reason for the feature, as a condition: on 4 MiB of these kinds the reference dependent stream is smaller than the stream
    # of independent pieces
    for kind in ("text", "gradient", "lz"):
        data = corpus.make(kind, 1, 4 << 20)
        dep, ind = len(ref.deflate_dep_stream(data, "raw")), len(deflate_stream_ref.deflate_stream(data, "raw"))
        assert dep < ind, (kind, dep, ind)
