"""lz_match_band's tile set-up on the GPU (csrc/zwz_band.hip: the scan of a tile's entries, eight a thread, the count by
csrc/lz_band.h's band_in_reach on running addresses, the compaction of the flagged entries with one add a wave) on chunks built for its
corners: every chunk through the band (context option match=band), payloads against the oracle byte for byte at level 6 and against
libz at levels 4 and 5, and every chunk inflated back.

The chunks come from tests/band_setup_chunks.py, where the host build first says that each holds what it was built for: (a) tiles
whose entry count runs through all residues mod 8, as a chunk's only tile and as its second; (b) one pair of differing trigrams in one
bucket at each of the eight places of a thread's eight entries, the seam between two threads among them, each deciding its tile's
word format alone; (c) candidates at distance kMaxDist - 1, kMaxDist and kMaxDist + 1, a candidate at position 0 and at 1, and the
pair at kMaxDist in front of and at the place where zlib's window has slid (33 KB chunks and two full ones); (d) tiles with 0, 1, 63,
64, 65 and more than 1 024 flagged entries.  All inputs are plain valid data."""
import importlib

import pytest

import band_setup_chunks as bs
import level_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def chunks():
    return bs.checked_chunks(bs.load())          # the CPU's word first: the corners are there


@pytest.fixture(scope="module")
def codec():
    """torch brings its own HIP runtime: it must have opened the GPU before a Codec does."""
    import torch
    torch.zeros(1, device="cuda")
    zwz = importlib.import_module("parallel-data-compression-and-decompression_amd")
    c = zwz.Codec(0, 1024)
    c.set_option("match", "band")
    yield c
    c.close()


@pytest.mark.parametrize("level", [4, 5, 6])
def test_set_up_corners_give_the_oracle_payloads(chunks, codec, oracle, level):
    names = list(chunks)
    data = [chunks[n] for n in names]
    assert 36 <= len(data) <= 48
    codec.set_level(level)
    try:
        got = codec.deflate_chunks(data)
        back, _ = codec.inflate_chunks(got)
    finally:
        codec.set_level(0)
    want = [oracle.payload(c) if level == 6 else level_ref.chunk_stream(c, level) for c in data]
    bad = [n for n, g, w in zip(names, got, want) if g != w]
    assert not bad, (level, bad)
    assert all(b == c for b, c in zip(back, data))
