"""Z_HUFFMAN_ONLY and Z_RLE on the CPU: csrc/rle_core.h, built on the host (tests/emu_strategy), gives libz's tokens, symbol count
and block count for every chunk of tests/strategy_ref.py's corpus -- with the positions evaluated in random order, since none may
depend on another -- and tests/strategy_ref.py itself says about libz what the GPU tests rely on: the header bytes, that the level
changes no byte, that a piece behind a full flush is compressed as if alone."""
import zlib

import numpy as np
import pytest

import corpus
import level_ref
import libz_ref
import strategy_ref as sr

CHUNKS = sr.chunks()
PIECE = sr.PIECE


def _libz_tokens(data, strategy):
    """[(position, length, distance-or-byte)] of libz's raw stream, the literals of its stored blocks included; the stored ranges."""
    tok, stored, n = level_ref.tokenise(sr.raw_stream(data, strategy))
    assert n == len(data)
    for a, b in stored:
        tok += [(p, 0, data[p]) for p in range(a, b)]
    return sorted(tok), stored


def test_libz_is_1_2_11():
    assert libz_ref.version().startswith("1.2.11") and zlib.ZLIB_RUNTIME_VERSION.startswith("1.2.11"), libz_ref.describe()


def test_corpus_names_are_unique_and_sizes_fit():
    names = [n for n, _ in CHUNKS]
    assert len(set(names)) == len(names)
    assert all(len(d) <= sr.CHUNK for _, d in CHUNKS)


@pytest.mark.parametrize("strategy", sr.STRATEGIES, ids=lambda s: sr.NAMES[s])
def test_tokens_match_libz_in_any_order(strategy):
    rs = np.random.RandomState(5)
    for name, data in CHUNKS:
        want, _ = _libz_tokens(data, strategy)
        order = rs.permutation(len(data)).astype(np.uint32)
        tok, n_sym, n_blocks = sr.emu_tokens(strategy, data, order)
        got, end = level_ref.positioned(tok)
        assert end == len(data), name
        assert got == want, "%s under %s: the tokens differ from libz's (first at %s)" % (
            name, sr.NAMES[strategy], next((g, w) for g, w in zip(got + [None], want + [None]) if g != w))
        assert n_sym == len(want) and n_blocks == n_sym // sr.SYMS_PER_BLOCK + 1, name
        if strategy == sr.HUFFMAN:
            assert n_sym == len(data)
        # the quiet-word shortcut changes nothing, and neither does the order
        tok2, n2, b2 = sr.emu_tokens(strategy, data, None, quiet=False)
        assert np.array_equal(tok, tok2) and (n2, b2) == (n_sym, n_blocks), name


def test_symbol_counts_of_the_block_edge_chunks():
    """The corpus holds chunks of exactly 16 382, 16 383, 16 384 and 32 766 symbols: an empty last block at 16 383 and 32 766."""
    by_name = dict(CHUNKS)
    for n in (16382, 16383, 16384, 32766):
        for strategy in sr.STRATEGIES:
            _, n_sym, n_blocks = sr.emu_tokens(strategy, by_name["symbols-%d-literals" % n])
            assert (n_sym, n_blocks) == (n, n // 16383 + 1)
        tok, n_sym, n_blocks = sr.emu_tokens(sr.RLE, by_name["symbols-%d-with-matches" % n])
        assert (n_sym, n_blocks) == (n, n // 16383 + 1) and (tok[:, 0] > 0).sum() == 2
    # libz writes that empty block: its stream of 16 383 symbols ends in two blocks
    for strategy in sr.STRATEGIES:
        raw = sr.raw_stream(by_name["symbols-16383-literals"], strategy)
        assert raw != sr.raw_stream(by_name["symbols-16383-literals"][:-1], strategy)
        blocks = sr.emu_blocks(strategy, by_name["symbols-16383-literals"])
        assert len(blocks) == 2 and blocks[1][:2] == (16383, 16383)


@pytest.mark.parametrize("strategy", sr.STRATEGIES, ids=lambda s: sr.NAMES[s])
def test_blocks_libz_stores_are_blocks_that_may_be_stored(strategy):
    """Every range libz puts into a stored block is one of the cut blocks, and the flush_pos rule lets the plan store it: random
    bytes on both sides of the window slide (65 273 / 65 274 bytes), blocks that start below 32 768 among them.
    (The rule cannot forbid a block that libz would want to store: a block it forbids covers more than 32 506 bytes in at most
    16 383 symbols, and with matches at distance 1 -- at most 18 bits for three bytes or more -- that is always far shorter coded.)"""
    seen = 0
    for name, data in CHUNKS:
        _, stored = _libz_tokens(data, strategy)
        blocks = sr.emu_blocks(strategy, data)
        assert len(blocks) == sr.emu_tokens(strategy, data)[2]
        assert blocks[0][0] == 0 and blocks[-1][1] == len(data) and all(a[1] == b[0] for a, b in zip(blocks, blocks[1:])), name
        for rng in stored:
            hit = [b for b in blocks if b[:2] == rng]
            assert len(hit) == 1 and hit[0][3] == 1, (name, rng, blocks)
            seen += 1
        for start, end, flush_pos, ok in blocks:
            if not ok:
                assert end - start > 32506, (name, start, end)
    assert seen >= 20
    rnd = dict(CHUNKS)["random-65535"]
    assert [b[:2] for b in sr.emu_blocks(strategy, rnd)] == [(0, 16383), (16383, 32766), (32766, 49149), (49149, 65532), (65532, 65535)]
    # what the issue's figure comes from: level 6 finds a few matches in random bytes and needs four blocks, the strategies five
    assert len(sr.raw_stream(rnd, strategy)) == 65557 and len(level_ref.raw_stream(rnd, 6)) == 65555


def test_header_bytes():
    data = corpus.text_like(3, 1000)
    for strategy in sr.STRATEGIES:
        for level in (1, 4, 6, 9):
            assert sr.deflate_stream(data, "zlib", strategy, level)[:2] == sr.ZLIB_HEADER
            # (XFL is 2 at level 9 whatever the strategy -- a level no writer here has; everything behind the header is the same)
            want = sr.GZIP_HEADER if level != 9 else sr.GZIP_HEADER[:8] + b"\x02" + sr.GZIP_HEADER[9:]
            assert sr.deflate_stream(data, "gzip", strategy, level)[:10] == want
            assert sr.deflate_stream(data, "gzip", strategy, level)[10:] == sr.deflate_stream(data, "gzip", strategy, 6)[10:]
        for level in (4, 5, 6):
            assert sr.emu_headers(level, strategy) == (0x01, 4)
        assert sr.chunk_stream(data, strategy)[:2] == sr.ZLIB_HEADER
    assert [sr.emu_headers(n, sr.DEFAULT) for n in (4, 5, 6)] == [(0x5e, 0), (0x5e, 0), (0x9c, 0)]
    assert [bool(sr.emu().emu_strategy_exists(s)) for s in (-1, 0, 1, 2, 3, 4, 5)] == [False, True, False, True, True, False, False]


def test_level_changes_no_byte():
    for name, data in CHUNKS[::7] + [c for c in CHUNKS if c[0].startswith(("lowent", "skewed", "seams"))]:
        for strategy in sr.STRATEGIES:
            ref = sr.chunk_stream(data, strategy, 6)
            assert all(sr.chunk_stream(data, strategy, level) == ref for level in (1, 4, 5, 9)), name


def test_pieces_are_independent():
    """Behind a full flush with the input consumed libz starts over: the second piece of 70 000 equal bytes is that piece alone."""
    for data in (b"\x07" * 70000, corpus.low_entropy(9, PIECE + 3000), dict(CHUNKS)["seams"] + dict(CHUNKS)["runs-in-a-row"]):
        for strategy in sr.STRATEGIES:
            c = zlib.compressobj(6, zlib.DEFLATED, -15, 8, strategy)
            first = c.compress(data[:PIECE]) + c.flush(zlib.Z_FULL_FLUSH)
            second = c.compress(data[PIECE:]) + c.flush(zlib.Z_FULL_FLUSH)
            alone = zlib.compressobj(6, zlib.DEFLATED, -15, 8, strategy)
            assert second == alone.compress(data[PIECE:]) + alone.flush(zlib.Z_FULL_FLUSH)
            assert sr.deflate_stream(data, "raw", strategy) == first + second + b"\x03\x00"


def test_strategies_differ():
    sr.check_strategies_differ()
    text = corpus.text_like(7, sr.CHUNK)
    assert sr.chunk_stream(text, sr.HUFFMAN) == sr.chunk_stream(text, sr.RLE)      # text has no runs: why it is not among the first kinds


def test_bgzf_reference_reads_back():
    import gzip
    data = corpus.low_entropy(23, PIECE + 5000)
    for strategy in sr.STRATEGIES:
        assert gzip.decompress(sr.bgzf(data, strategy)) == data
