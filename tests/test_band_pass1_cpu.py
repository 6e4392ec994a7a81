"""lz_match_band's first pass without a GPU (csrc/lz_band.h: band_key_pair, band_trip_mask, band_pair_mask, band_first_pass -- the
specification of the kernel's loop: two candidates' keys in the halves of a word, trips of eight, and beyond the wave's smallest count
a mask per trip that turns a candidate the position does not have into a key of length 0, which is let into the maximum because it
cannot win).  The host build (tests/emu_band/band_pass1_emu.cpp) against band_key / band_key_masked and the plain maximum over the
candidates a position has: every pair of 8-byte words that differ first in byte 0 .. 7 or not at all, every k in 1 .. 128, every count in
0 .. 128, the pure and the impure start value, every level; and the constructed chunks of tests/test_gpu_band_pass1.py, each checked to
hold its corner and, record by record, against lz_search."""
import numpy as np
import pytest

import band_pass1_chunks as b1
import band_pass2_chunks as bp
import level_ref


@pytest.fixture(scope="module")
def emu():
    return b1.load()


def test_pair_keys_are_band_keys_half_by_half(emu):
    assert emu.emu_pass1_pairs(1) == 0
    assert emu.emu_pass1_pairs(0xfeed) == 0


def test_trip_masks_say_which_candidates_a_position_has(emu):
    assert emu.emu_pass1_masks() == 0


@pytest.mark.parametrize("fill", [0, 1, 2, 3])
@pytest.mark.parametrize("impure", [False, True])
@pytest.mark.parametrize("level", [4, 5, 6])
def test_first_pass_is_the_maximum_over_the_candidates_a_position_has(emu, level, impure, fill):
    """fill: what the other candidates hold -- 0: a differing first byte, 1: the position's own word (beyond the count that would be the
    longest key there is), 2: a first difference anywhere, 3: a differing first byte within the count and the own word beyond it (only
    the masks keep the position's best at length 0)."""
    numbers = b1.numbers(emu, level)
    none = numbers["none_impure"] if impure else numbers["none_pure"]
    bad, first = b1.sweep(emu, level, none, fill, 77 + fill)
    assert bad == 0, "first difference: byte %d, k %d, count %d, kmin %d, kmax %d: best %#x (want %#x), short %#x (want %#x)" % tuple(first)


def test_the_constructed_chunks_hold_their_corners_and_give_lz_search_records(emu):
    """What goes to the GPU: b1.checked_chunks asserts each chunk's corner; here the band's records of every chunk (the host build of the
    whole search, tests/emu_band and tests/emu_level) against lz_search's at every level."""
    chunks = b1.checked_chunks(emu)
    assert 20 <= len(chunks) <= 48 and all(len(d) <= 65535 for d in chunks.values())
    walks = bp.load()
    for name, data in chunks.items():
        want128, want32 = bp.search_records(walks, data)
        got = bp.Walks(walks, data, b1.TILE, -1, 4)
        assert np.array_equal(got.e128, want128) and np.array_equal(got.e32, want32), name
        for level in (4, 5):
            code, _, _ = level_ref.emu_records(level, data)
            assert code == 0, (name, level)
