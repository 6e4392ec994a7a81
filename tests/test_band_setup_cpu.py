"""lz_match_band's tile set-up without a GPU (csrc/lz_band.h: band_lo and band_in_reach -- band_valid as a range test, what the count
phase and band_count ask).  The host build is tests/emu_band/band_setup_emu.cpp."""
import collections

import pytest

import band_setup_chunks as bs
import corpus

MAX_DIST = bs.MAX_DIST
HALO = 0xffff0000


@pytest.fixture(scope="module")
def emu():
    return bs.load()


def _words():
    """own x candidate words around every edge of band_valid."""
    pos = sorted({0, 1, 2, MAX_DIST - 1, MAX_DIST, MAX_DIST + 1, 40000, 65532})
    buckets = (0, 1, 0x1234, 0x7ffe, 0x7fff)
    owns = [h << 16 | p for h in buckets for p in pos] + [HALO]
    out = []
    for own in owns:
        h, p = own >> 16, own & 0xffff
        qs = {0, 1, 2, 65532, 65535} | {q for d in (1, 2, MAX_DIST - 1, MAX_DIST, MAX_DIST + 1) for q in (p - d, p + d) if 0 <= q <= 65535}
        cands = {h << 16 | q for q in qs}
        cands |= {(h2 & 0xffff) << 16 | q for h2 in (h - 1, h + 1, 0, 0x7fff) if 0 <= h2 for q in (0, 1, 65535, p, max(p - 1, 0))}
        cands |= {HALO, (h << 16) - 1 & 0xffffffff, own + 1 & 0xffffffff}      # the halo word; the word in front of the bucket's first possible one
        cands.discard(own)
        out += [(own, c) for c in sorted(cands)]
    return out


def test_the_range_test_is_band_valid(emu):
    """Own position 0, 1, kMaxDist - 1, kMaxDist, kMaxDist + 1, 65 532; candidate position 0 and 1; distance kMaxDist - 1, kMaxDist,
    kMaxDist + 1; bucket 0 and the highest; the word in front of a bucket's first; the halo word as candidate and as own.  (c == own is
    left out: no entry is its own predecessor -- csrc/lz_band.h.)"""
    pairs = _words()
    assert len(pairs) > 800
    seen = collections.Counter()
    for own, c in pairs:
        r = emu.emu_setup_reach(own, c)
        assert r in (0, 3), (hex(own), hex(c), r)
        seen[r] += 1
    assert seen[0] >= 50 and seen[3] >= 50                                     # (both answers are well represented in the set)
    # the named corners, by what they must say
    say = lambda own, c: emu.emu_setup_reach(own, c)
    h = 0x1234 << 16
    assert say(h | 40000, h | 40000 - (MAX_DIST - 1)) == 3 and say(h | 40000, h | 40000 - MAX_DIST) == 0
    assert say(h | 5, h | 0) == 0 and say(h | 5, h | 1) == 3 and say(h | 0, h | 0 | 1) == 0
    assert say(h | 1, h | 0) == 0 and say(h | MAX_DIST, h | 1) == 3 and say(h | MAX_DIST + 1, h | 1) == 0 and say(h | MAX_DIST + 1, h | 2) == 3
    assert say(0 | 7, 0 | 3) == 3 and say(0x7fff << 16 | 7, 0x7fff << 16 | 3) == 3 and say(0x7fff << 16 | 7, HALO) == 0
    assert say(HALO, HALO - 1) == 0 and say(HALO, 0x7fff << 16 | 65535) == 0 and say(h | 7, h - 1) == 0
    assert emu.emu_setup_lo(HALO) == HALO and emu.emu_setup_lo(h | 0) == h and emu.emu_setup_lo(h | 9) == h | 1
    assert emu.emu_setup_lo(h | MAX_DIST + 7) == h | 8


@pytest.mark.parametrize("level", [4, 5, 6])
def test_band_count_is_the_search_over_band_valid_on_every_corpus_kind(emu, level):
    for i, kind in enumerate(sorted(corpus.KINDS)):
        for n in (65535, 6500 + 37 * i, 3, 2, 0):
            data = corpus.make(kind, 50 + i, n)
            bad, cnt, _ = bs.counts(emu, data, level)
            assert bad == 0, (kind, n)
    # (the counts are not all zero)
    assert int(bs.counts(emu, corpus.text_like(1, 20000), level)[1].max()) == {4: 16, 5: 32, 6: 128}[level]


def test_the_constructed_chunks_hold_their_corners(emu):
    """What goes to the GPU (tests/test_gpu_band_setup.py): bs.checked_chunks asserts every corner; here also every chunk's counts
    against the search over band_valid, at every level."""
    chunks = bs.checked_chunks(emu)
    assert 36 <= len(chunks) <= 48
    for name, data in chunks.items():
        for level in (4, 5, 6):
            assert bs.counts(emu, data, level)[0] == 0, (name, level)
