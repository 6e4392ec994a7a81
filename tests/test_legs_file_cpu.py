"""The file loop of the decode in legs without a GPU: csrc/legfile_core.h's loop -- the one zwz_inflate_legs_file runs -- over windows in
host memory (tests/emu_legfile/legfile_emu.cpp), around the restated leg of tests/emu_legs.  What it is compared with shares no code with
the loop: the decoded bytes are libz's, the index is the one tests/emu_legs/legs_emu.cpp's whole-stream call seals for the same stream
(index_seal over the whole output), the verdicts are the one-launch restatement's (tests/emu/index_emu.cpp).  Windows of 4096 / 16 384
input bytes and 65 536 output bytes, span 16 KiB; every case asserts from the counters that it reached its shape."""
import zlib

import pytest

import index_emu_binding
import index_ref
import legfile_emu_binding as emu
import legs_emu_binding
import legs_file_cases as cases
from index_ref import GZIP, RAW, ZLIB
from legs_file_cases import LEG_INS, LEG_OUT, SPAN

WBITS = {RAW: -15, ZLIB: 15, GZIP: 31}


@pytest.fixture(scope="module")
def lib():
    return emu.load()


@pytest.fixture(scope="module")
def legs():
    return legs_emu_binding.load()


@pytest.fixture(scope="module")
def one():
    return index_emu_binding.load()


@pytest.fixture(scope="module")
def good():
    return cases.good_cases()


def whole_stream_index(legs, one, c):
    """The index legs_emu.cpp's whole-stream call makes of the stream, in one leg: the reference for the loop's."""
    cap = len(c.data) + 16
    st, out, idx, counts = legs_emu_binding.legs(legs, c.wrap, c.stream, cap, SPAN, 1 << 28, (1 << 32) - 65536, one.emu_index_bound(cap, SPAN))
    assert st == 0 and out == c.data and counts == (1, 0, 0)
    return idx


@pytest.mark.parametrize("leg_in", LEG_INS)
def test_dst_is_libz_and_the_index_is_the_whole_stream_calls(lib, legs, one, good, leg_in):
    for c in good:
        assert cases.libz_decodes(c.wrap, c.stream) == c.data, c.name
        want_idx = whole_stream_index(legs, one, c)
        assert (len(want_idx) > 0) == c.index, c.name
        both = emu.run(lib, c.wrap, c.stream, SPAN, leg_in, LEG_OUT)
        only_dst = emu.run(lib, c.wrap, c.stream, SPAN, leg_in, LEG_OUT, idx=False)
        assert only_dst["rc"] == 0 and only_dst["dst"] == c.data, c.name
        if c.index:
            only_idx = emu.run(lib, c.wrap, c.stream, SPAN, leg_in, LEG_OUT, dst=False)
            assert both["rc"] == 0 and both["dst"] == c.data and both["idx"] == want_idx == only_idx["idx"], c.name
            index_ref.check_index(both["idx"], c.stream, c.data, c.wrap)
            assert both["stats"] == only_idx["stats"], c.name
            assert both["stats"]["index_entries"] == len(index_ref.parse(want_idx).entries), c.name
        else:
            assert both["rc"] == emu.E_FORMAT and both["dst"] is None and both["idx"] is None, c.name
        # the same legs whether or not an index is made (restart points are taken by the same rule)
        for k in ("legs", "rewound", "grown", "commits", "max_in_window", "max_out_window"):
            assert both["stats"][k] == only_dst["stats"][k], (c.name, k)
        if leg_in == LEG_INS[0]:
            for k, least in c.shape.items():
                assert both["stats"][k] >= least, (c.name, k, both["stats"])
        assert both["stats"]["legs"] == both["stats"]["rewound"] + 1 and both["stats"]["commits"] <= both["stats"]["legs"], c.name


def test_one_leg_at_the_default_windows(lib, legs, one, good):
    c = good[1]
    r = emu.run(lib, c.wrap, c.stream, SPAN, 67108864, 268435456)
    assert r["rc"] == 0 and r["dst"] == c.data and r["idx"] == whole_stream_index(legs, one, c)
    assert (r["stats"]["legs"], r["stats"]["rewound"], r["stats"]["grown"], r["stats"]["commits"]) == (1, 0, 0, 1)


def test_the_carry_brings_a_full_window_and_a_short_one(lib, good):
    c = next(c for c in good if c.name == "32 KiB repeated")
    r = emu.run(lib, c.wrap, c.stream, SPAN, LEG_INS[0], LEG_OUT)
    assert r["rc"] == 0 and r["dst"] == c.data
    block_starts = [t for t in r["trace"] if t[0] == legs_emu_binding.BLOCK]
    assert any(hist == 32768 for _, _, _, _, hist, _ in block_starts), "a leg started with a full window in front of it"
    assert any(hist < 32768 for _, _, _, _, hist, _ in block_starts), "a leg started at a block header with hist below 32 768"
    for kind, bit, out, origin, hist, carried in r["trace"]:
        assert hist <= carried < hist + 16 and (out - carried) % 16 == 0       # hist bytes and the 0..15 down to the 16-byte boundary


def test_members_start_legs_with_an_empty_window(lib, good):
    c = next(c for c in good if c.name == "three members, zero padding across window ends")
    r = emu.run(lib, c.wrap, c.stream, SPAN, LEG_INS[0], LEG_OUT, idx=False)
    assert r["rc"] == 0 and r["dst"] == c.data
    assert any(t[0] == legs_emu_binding.MEMBER and t[4] == 0 for t in r["trace"])
    assert any(t[0] == legs_emu_binding.BLOCK and t[3] > 0 for t in r["trace"]), "a restart inside a later member"


def test_growth_stops_at_the_limits(lib, good):
    c = next(c for c in good if c.name == "a block longer than the input window")
    r = emu.run(lib, c.wrap, c.stream, SPAN, 4096, LEG_OUT, max_in=10_000)
    assert (r["rc"], r["status"], r["dst"], r["idx"]) == (emu.E_FORMAT, 36, None, None) and r["stats"]["grown"] == 2
    c = next(c for c in good if c.name == "zeros larger than the output window")
    r = emu.run(lib, c.wrap, c.stream, SPAN, 4096, LEG_OUT, max_out=200_000)
    assert (r["rc"], r["status"], r["dst"], r["idx"]) == (emu.E_FORMAT, 36, None, None) and r["stats"]["grown"] == 2


def test_cut_and_damaged_files_get_the_one_launch_verdict_and_leave_nothing(lib, one):
    seen = set()
    for name, wrap, s, cut in cases.damaged_cases():
        want = index_emu_binding.build(one, wrap, s, 400_000, SPAN)
        for leg_in in LEG_INS:
            r = emu.run(lib, wrap, s, SPAN, leg_in, LEG_OUT)
            assert r["status"] == want[0], (name, leg_in, r["status"], want[0])
            assert r["rc"] == cases.rc_of_status(want[0]) or (want[0] == 0 and len(want[2]) == 0 and r["rc"] == emu.E_FORMAT), (name, r["rc"])
            if r["rc"] == 0:                                   # (a flipped bit libz does not mind: a header's MTIME or OS byte)
                assert r["dst"] == want[1] == cases.libz_decodes(wrap, s) and r["idx"] == want[2], name
            else:
                assert r["dst"] is None and r["idx"] is None, name
                assert cases.libz_decodes(wrap, s) is None or want[0] == 0, name
            if r["rc"] == emu.E_FORMAT and want[0] != 0:
                assert r["stop"] <= len(s), (name, r["stop"])
                if cut is not None:
                    assert r["stop"] <= cut and r["status"] == 1, (name, r["stop"])
            seen.add(r["rc"])
    assert seen >= {emu.E_FORMAT, emu.E_CHECKSUM}


def test_a_bad_crc_beats_a_later_data_error(lib):
    name, wrap, s, cut = next(d for d in cases.damaged_cases() if d[0].startswith("a bad CRC in member 1"))
    r = emu.run(lib, wrap, s, SPAN, 4096, LEG_OUT, idx=False)
    assert (r["rc"], r["status"]) == (emu.E_CHECKSUM, 33)
    assert r["stats"]["legs"] >= 3, "the bad CRC and the data error lie in different legs"
