"""Compression levels 4, 5 and 6 on the CPU: the portable LZ cores (csrc/lz_core.h, lz_band.h, lz_lazy.h), templated on the level
(csrc/zwz_common.h: LzLevel<N>) and built on the host (tests/emu_level), against libz itself at that level.

(a) the chain walk, the band (band_generic; the first pass's keys + band_deep and band_deep_batched<4>) and lz_lazy's on-demand
    search give the same (long, short) records at every position;
(b) the sequential lz_parse, fresh_step's orbit and lazy_chain's give one token sequence, and it is the one libz's level-N raw
    stream decodes to.
Block boundaries, Huffman construction and bit packing do not depend on the level, so token equality plus the header byte is
stream equality.  No GPU."""
import zlib

import pytest

import level_ref
import libz_ref

CHUNKS = level_ref.chunks()
IDS = [name for name, _ in CHUNKS]


def test_libz_is_1_2_11():
    assert libz_ref.version() == "1.2.11" and zlib.ZLIB_RUNTIME_VERSION == "1.2.11", libz_ref.describe()


@pytest.mark.parametrize("level", level_ref.LEVELS)
def test_level_numbers_are_libz_configuration_table(level):
    good, lazy, nice, chain, short, flg = level_ref.emu_numbers(level)
    assert (good, lazy, nice, chain) == level_ref.LIBZ_CONFIG[level]
    assert short == chain >> 2                                       # longest_match: chain_length >>= 2 once prev_length >= good_match
    assert bytes([0x78, flg]) == level_ref.ZLIB_HEADER[level] == zlib.compress(b"x", level)[:2]


def test_first_kinds_differ_between_levels():
    level_ref.check_levels_differ()


def test_tokeniser_reproduces_the_input():
    """The tokeniser itself: replaying its tokens (and copying its stored ranges) gives the input back."""
    for name, data in CHUNKS[:5] + CHUNKS[8:9]:
        tokens, stored, total = level_ref.tokenise(level_ref.raw_stream(data, 5))
        assert total == len(data)
        out = bytearray(len(data))
        for a, b in stored:
            out[a:b] = data[a:b]
        for p, ln, v in tokens:
            if ln == 0:
                out[p] = v
            else:
                for i in range(ln):
                    out[p + i] = out[p + i - v]
        assert bytes(out) == data, name


@pytest.mark.parametrize("level", level_ref.LEVELS)
@pytest.mark.parametrize("chunk", range(len(CHUNKS)), ids=IDS)
def test_three_searches_same_records(level, chunk):
    name, data = CHUNKS[chunk]
    for tile in (6016, 320):                     # the kernel's tile; a small one: every halo path, tiles of either word format
        code, _, _ = level_ref.emu_records(level, data, tile)
        assert code == 0, "%s level %d tile %d: search %d (1 band_generic, 2 band_deep, 3 band_deep_batched<4>, 4 lazy_search) differs from lz_search at position %d" % (
            name, level, tile, code >> 24, (code & 0xffffff) - 1)


@pytest.mark.parametrize("level", level_ref.LEVELS)
@pytest.mark.parametrize("chunk", range(len(CHUNKS)), ids=IDS)
def test_tokens_are_libz(level, chunk):
    name, data = CHUNKS[chunk]
    ours, end = level_ref.positioned(level_ref.emu_tokens(level, data))      # (asserts lz_parse == fresh_step's orbit == lazy_chain's)
    assert end == len(data)
    theirs, stored, total = level_ref.tokenise(level_ref.raw_stream(data, level))
    assert total == len(data)
    # a stored block keeps no tokens: there, ours must tile the block's byte range exactly (a block ends between two symbols)
    def outside(p):
        return not any(a <= p < b for a, b in stored)
    assert [t for t in ours if outside(t[0])] == theirs, "%s level %d: the token sequence differs from libz's" % (name, level)
    starts = {t[0] for t in ours} | {len(data)}
    for a, b in stored:
        assert a in starts and b in starts, "%s level %d: a stored block of libz does not begin and end between two of our symbols" % (name, level)
