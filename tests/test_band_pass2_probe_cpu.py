"""lz_match_band's second pass behind the probe at the best length (csrc/lz_band.h: band_deep_probed, the specification of the kernel's
compare and run-ahead steps) without a GPU: the host build of the pass (tests/emu_band/band_pass2_probe_emu.cpp, assertions on: the
probe's address is checked to lie inside the data at every visit) against band_deep and against lz_search, record by record, and the
sharers looked at against the plain walk's -- on every corpus kind, on the chunks built for the batched pass's corners
(tests/band_pass2_chunks.py) and on those built for the probe's (tests/band_pass2_probe_chunks.py), at levels 4, 5 and 6."""
import numpy as np
import pytest

import band_pass2_chunks as bp
import band_pass2_probe_chunks as pp
import corpus


@pytest.fixture(scope="module")
def emu():
    return pp.load()


@pytest.fixture(scope="module")
def emu_batched():
    return bp.load()


def _check(emu, data, tiles, what, levels=(6,), emu_batched=None):
    for level in levels:
        want128, want32 = pp.search_records(emu, data, level)
        for tile, fmt in tiles:
            plain = pp.Walks(emu, data, tile, fmt, level, 0)
            assert np.array_equal(plain.e128, want128) and np.array_equal(plain.e32, want32), (what, level, tile, fmt, "band_deep against lz_search")
            got = pp.Walks(emu, data, tile, fmt, level, 1)
            assert np.array_equal(got.e128, plain.e128), (what, level, tile, fmt, "e128")
            assert np.array_equal(got.e32, plain.e32), (what, level, tile, fmt, "e32")
            assert np.array_equal(got.visited, got.visited_ref), (what, level, tile, fmt, "sharers looked at")
            assert np.all(got.compared <= got.visited) and np.all((got.compared > 0) == (got.visited > 0)), (what, level, tile, fmt, "sharers compared")
            if emu_batched is not None and level == 6:                 # the batched walk's own host build counts the same sharers
                old = bp.Walks(emu_batched, data, tile, fmt, 4)
                assert np.array_equal(got.visited, old.visited) and np.array_equal(got.e128, old.e128) and np.array_equal(got.e32, old.e32), (what, tile, fmt)


@pytest.mark.parametrize("kind", list(corpus.KINDS))
def test_probed_walk_gives_band_deep_and_lz_search_records(emu, emu_batched, kind):
    """Both word formats; tiles small enough that chains cross halos (and, at 192 and 64 entries, halos of the other format)."""
    for i, n in enumerate([0, 3, 4, 11, 12, 13, 300, 4097, 20000, 65535]):
        if kind == "lz" and 20000 < n:
            continue
        data = corpus.make(kind, 5200 + i, n)
        tiles = ((6016, -1), (6016, 0)) if n > 20000 else ((6016, -1), (6016, 0), (192, -1), (64, 0))
        _check(emu, data, tiles, (kind, n), pp.LEVELS if n <= 20000 else (6,), emu_batched)


def test_probed_walk_on_the_batched_pass_chunks(emu, emu_batched):
    for name, data in bp.checked_chunks(emu_batched).items():
        _check(emu, data, ((6016, -1), (6016, 0), (1024, -1), (192, -1)), name, pp.LEVELS, emu_batched)


def test_probed_walk_on_the_probe_chunks(emu, emu_batched):
    """A false probe hit, a later sharer of the best length, an improving sharer on either side of the short chain's end at every level, a
    best that reaches the chunk's end, a best beyond the sixteen compared bytes, a long run of rejected sharers through a halo, the nice
    stop -- each checked to hold its feature (band_pass2_probe_chunks.checked_chunks), at the kernel's tile and at small ones."""
    for name, data in pp.checked_chunks(emu).items():
        _check(emu, data, ((6016, -1), (6016, 0), (1024, -1), (192, -1)), name, pp.LEVELS, emu_batched)


def test_probed_walk_on_runs_and_short_periods(emu):
    """Every sharer of `nice` length: the walk ends at its first sharer."""
    for i, per in enumerate((1, 2, 3, 5, 7, 64, 300)):
        data = (corpus.random_bytes(600 + i, per) * (9000 // per + 1))[:9000 - i]
        _check(emu, data, ((6016, -1), (6016, 0), (192, -1)), ("period", per), pp.LEVELS)
