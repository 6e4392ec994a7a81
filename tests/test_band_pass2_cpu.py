"""lz_match_band's second pass in batches (csrc/lz_band.h: band_deep_batched<H>, the specification of the kernel's chase / compare /
fold) without a GPU: the host build of the pass (tests/emu_band) against band_deep (H = 0) and against lz_search, record by record,
for H = 1, 3, 8 and 16, on every corpus kind and on the chunks built for the pass's corners (tests/band_pass2_chunks.py)."""
import numpy as np
import pytest

import band_pass2_chunks as bp
import corpus

BATCHES = (1, 3, 8, 16)


@pytest.fixture(scope="module")
def emu():
    return bp.load()


def _check(emu, data, tiles, what):
    want128, want32 = bp.search_records(emu, data)
    for tile, fmt in tiles:
        plain = bp.Walks(emu, data, tile, fmt, 0)
        assert np.array_equal(plain.e128, want128) and np.array_equal(plain.e32, want32), (what, tile, fmt, "band_deep against lz_search")
        for h in BATCHES:
            got = bp.Walks(emu, data, tile, fmt, h)
            assert np.array_equal(got.e128, plain.e128), (what, tile, fmt, h, "e128")
            assert np.array_equal(got.e32, plain.e32), (what, tile, fmt, h, "e32")
            assert np.array_equal(got.visited, plain.visited), (what, tile, fmt, h, "sharers looked at")


@pytest.mark.parametrize("kind", list(corpus.KINDS))
def test_batched_walk_gives_band_deep_and_lz_search_records(emu, kind):
    """Both word formats; tiles small enough that chains cross halos (and, at 192 and 64 entries, halos of the other format)."""
    for i, n in enumerate([0, 3, 4, 11, 12, 13, 300, 4097, 20000, 65535]):
        if kind == "lz" and 20000 < n:
            continue
        data = corpus.make(kind, 5200 + i, n)
        tiles = ((6016, -1), (6016, 0)) if n > 20000 else ((6016, -1), (6016, 0), (192, -1), (64, 0))
        _check(emu, data, tiles, (kind, n))


def test_batched_walk_on_the_constructed_chunks(emu):
    """The chunks tests/test_gpu_band_pass2.py sends to the GPU -- long chains through a halo, walks of H - 1, H, H + 1 and 2 H sharers,
    lengths that end at the edges of the sixteen compared bytes, the nice stop inside a batch, the short chain's snapshot, the chunk's
    last positions, a halo of another format -- each checked to hold its feature, at the kernel's tile and at small ones."""
    for name, data in bp.checked_chunks(emu).items():
        _check(emu, data, ((6016, -1), (6016, 0), (1024, -1), (192, -1)), name)


def test_batched_walk_on_runs_and_short_periods(emu):
    """Every sharer of `nice` length: the walk ends at its first sharer, whatever was chased behind it."""
    for i, per in enumerate((1, 2, 3, 5, 7, 64, 300)):
        data = (corpus.random_bytes(600 + i, per) * (9000 // per + 1))[:9000 - i]
        _check(emu, data, ((6016, -1), (6016, 0), (192, -1)), ("period", per))
