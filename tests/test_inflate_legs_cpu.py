"""The decode in legs without a GPU: leg_core.h's planner, snapshot rule and 64-bit entry, and the CPU restatement of inflate_kernel's
leg form with the host loop around it (tests/emu_legs/legs_emu.cpp), against libz and against the one-launch marking form's restatement
(tests/emu/index_emu.cpp, itself checked against libz by tests/index_ref.py).  As for that emu, this checks the method and the helpers
the kernel shares, not the kernel's control flow."""
import ctypes
import random
import struct
import zlib

import pytest

import index_emu_binding
import index_ref
import legs_emu_binding as emu
import legs_ref
from index_ref import GZIP, RAW, ZLIB
from legs_ref import LETTERS, deflate

SPAN = 16384
LEG_OUT = 65536


@pytest.fixture(scope="module")
def lib():
    return emu.load()


@pytest.fixture(scope="module")
def one():
    return index_emu_binding.load()


@pytest.fixture(scope="module")
def grainy():
    return legs_ref.grainy()


def same_as_one_launch(lib, one, wrap, stream, cap, leg_bytes, leg_out=LEG_OUT, span=SPAN):
    want = index_emu_binding.build(one, wrap, stream, cap, span)
    bound = one.emu_index_bound(cap, span)
    st, out, idx, counts = emu.legs(lib, wrap, stream, cap, span, leg_bytes, leg_out, bound)
    assert (st, len(out), len(idx)) == (want[0], len(want[1]), len(want[2])), (st, want[0], len(out), len(want[1]), len(idx), len(want[2]), counts)
    assert out == want[1] and idx == want[2]
    return st, out, idx, counts


# ---- the whole call ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("wrap", [RAW, ZLIB, GZIP])
@pytest.mark.parametrize("leg_bytes", [4096, 16384])
def test_legs_give_the_one_launch_results_and_libz_checkpoints(lib, one, grainy, wrap, leg_bytes):
    for data, level, every in ((grainy, 6, None), (grainy[:150_000], 1, None), (grainy[100_000:300_000], 9, None), (grainy[:200_000], 6, 30_000), (b"", 6, None)):
        s = deflate(data, wrap, level, every)
        st, out, idx, counts = same_as_one_launch(lib, one, wrap, s, len(data) + 3, leg_bytes)
        assert st == 0 and out == data
        index_ref.check_index(idx, s, data, wrap)
        assert (counts[0] > 1 and counts[1] >= 1) or not data, counts


def test_one_leg_at_the_default_sizes(lib, one, grainy):
    s = deflate(grainy, GZIP)
    st, out, idx, counts = same_as_one_launch(lib, one, GZIP, s, len(grainy), 268435456, (1 << 32) - 65536, span=1 << 16)
    assert st == 0 and counts == (1, 0, 0)


def test_restart_at_every_bit_offset_and_input_alignment(lib, one):
    rng = random.Random(5)
    bits, starts = set(), set()
    for _ in range(4):
        s, data = legs_ref.z_block_stream(rng)
        st, out, idx, counts = same_as_one_launch(lib, one, RAW, s, len(data), 16384)
        assert st == 0 and out == data and counts[0] > 8 and counts[1] >= 8, counts
        for bit, off, hist in index_ref.parse(idx).entries[1:]:
            bits.add(bit & 7); starts.add((bit >> 3) & 15)
    assert bits == set(range(8)) and starts == set(range(16))


def test_rewind_at_the_input_edge(lib, one):
    names, streams, datas = legs_ref.edge_streams(edge=4096)
    for name, s, data in zip(names, streams, datas):
        st, out, idx, counts = same_as_one_launch(lib, one, GZIP, s, len(data), 4096)
        assert st == 0 and out == data, name
        assert counts[0] > 1 and counts[1] >= 1, (name, counts)
    assert counts[2] >= 1, "a header longer than the window makes it grow"


def test_several_members(lib, one):
    streams, caps, expect = legs_ref.member_streams()
    for i, (s, cap, (want_st, want)) in enumerate(zip(streams, caps, expect)):
        st, out, idx, counts = same_as_one_launch(lib, one, GZIP, s, cap, 4096)
        assert want_st is None or st == want_st, (i, st)
        if want is not None:
            assert out[:len(want)] == want and (want_st != 0 or out == want), i
        assert counts[0] > 1 and counts[1] >= 1, (i, counts)
        assert (len(idx) > 0) == (i == 2), i


@pytest.mark.parametrize("wrap", [ZLIB, GZIP])
def test_cut_and_damaged_streams(lib, one, grainy, wrap):
    data = grainy[:120_000]
    s = deflate(data, wrap)
    for cut in range(0, len(s), 997):
        st, out, idx, counts = same_as_one_launch(lib, one, wrap, s[:cut], len(data), 4096)
        assert st == 1 and idx == b"" and out == data[:len(out)], cut
    rng = random.Random(3)
    for _ in range(12):
        b = bytearray(s)
        b[rng.randrange(len(s))] ^= 1 << rng.randrange(8)
        same_as_one_launch(lib, one, wrap, bytes(b), len(data), 4096)
    st, out, idx, counts = same_as_one_launch(lib, one, wrap, s, len(data) - 1, 4096)
    assert st == 3 and idx == b""


def test_an_index_capacity_too_small(lib, one, grainy):
    data = grainy[:200_000]
    s = deflate(data, GZIP)
    for icap in (64, 4096, 64 + 3 * 24 + 40_000):
        want = index_emu_binding.build(one, GZIP, s, len(data), SPAN, idx_cap=icap)
        got = emu.legs(lib, GZIP, s, len(data), SPAN, 4096, LEG_OUT, icap)
        assert got[:3] == want and got[:3] == (0, data, b"") and got[3][0] > 4, (icap, got[3])


def test_decode_only_takes_the_same_legs(lib, one, grainy):
    s = deflate(grainy, GZIP)
    bound = one.emu_index_bound(len(grainy), SPAN)
    a = emu.legs(lib, GZIP, s, len(grainy), SPAN, 4096, LEG_OUT, bound)
    b = emu.legs(lib, GZIP, s, len(grainy), SPAN, 4096, LEG_OUT, bound, index=False)
    assert a[0] == b[0] == 0 and a[1] == b[1] == grainy and b[2] == b"" and a[3] == b[3]


# ---- the planner ------------------------------------------------------------------------------------------------------------------

def test_planner_windows_and_growth(lib):
    s, w = emu.fresh(lib), emu.LegPlan()
    v, grew = emu.next_leg(lib, s, w, 100_000, 1_000_000, 4096, 65536)
    assert (v, grew) == (emu.GO, False)
    assert (w.in_base, w.in_len, w.in_final, w.out_base, w.out_len, w.out_final) == (0, 4096, 0, 0, 65536, 0)
    # rewound to where it started, input ran out: the input window doubles, the output window stays
    s.status = 1
    v, grew = emu.next_leg(lib, s, w, 100_000, 1_000_000, 4096, 65536)
    assert (v, grew, w.in_len, w.out_len) == (emu.GO, True, 8192, 65536)
    s.status = 3
    v, grew = emu.next_leg(lib, s, w, 100_000, 1_000_000, 4096, 65536)
    assert (v, grew, w.in_len, w.out_len) == (emu.GO, True, 8192, 131072)
    # a restart point further on: base windows again, the input from the restart bit's byte rounded down to 16, the output from
    # first - hist rounded down to 16
    s.start, s.bit, s.out, s.origin, s.status = emu.BLOCK, 8 * 70_007 + 3, 200_005, 0, 1
    v, grew = emu.next_leg(lib, s, w, 100_000, 1_000_000, 4096, 65536)
    assert (v, grew) == (emu.GO, False)
    assert (w.in_base, w.in_len, w.out_base, w.out_len) == (70_000, 4096, (200_005 - 32768) & ~15, 65536)
    # hist = min(32768, decoded offset - the member's first byte)
    s.origin = 190_000
    emu.next_leg(lib, s, w, 100_000, 1_000_000, 4096, 65536)
    assert w.out_base == 190_000 & ~15
    # a member start: an empty window
    s.start, s.bit = emu.MEMBER, 8 * 99_000
    emu.next_leg(lib, s, w, 100_000, 200_100, 4096, 65536)
    assert (w.in_base, w.in_len, w.in_final, w.out_base, w.out_len, w.out_final) == (99_000 & ~15, 100_000 - (99_000 & ~15), 1, 200_005 & ~15, 200_100 - (200_005 & ~15), 1)
    s.done = 1
    assert emu.next_leg(lib, s, w, 100_000, 200_100, 4096, 65536)[0] == emu.DONE


def test_planner_growth_stops_at_the_limits(lib):
    for status, field in ((1, "in_len"), (3, "out_len")):
        s, w = emu.fresh(lib), emu.LegPlan()
        sizes = []
        for _ in range(12):
            v, grew = emu.next_leg(lib, s, w, 1 << 30, 1 << 30, 4096, 65536, max_in=30_000, max_out=500_000)
            if v != emu.GO:
                break
            sizes.append(getattr(w, field))
            s.status = status
        assert v == emu.TOO_LARGE
        assert sizes == ([4096, 8192, 16384, 30_000] if status == 1 else [65536, 131072, 262144, 500_000])


def test_too_large_names_the_last_restart_point(lib, one):
    rng = random.Random(4)
    data = bytes(rng.choices(LETTERS, k=200_000))
    s = deflate(data, GZIP, 9)                         # blocks of about 24 KiB compressed: none fits 10 000 bytes
    bound = one.emu_index_bound(len(data), SPAN)
    st, out, idx, counts = emu.legs(lib, GZIP, s, len(data), SPAN, 4096, LEG_OUT, bound, max_in=10_000)
    assert st == 36 and out == b"" and idx == b"" and counts[2] == 2
    st, out, idx, counts = emu.legs(lib, ZLIB, deflate(bytes(1 << 20), ZLIB), 1 << 20, SPAN, 4096, LEG_OUT, bound, max_out=200_000)
    assert st == 36 and counts[2] == 2
    st, out, idx, counts = emu.legs(lib, GZIP, s, len(data), SPAN, 4096, LEG_OUT, bound, max_in=40_000)
    assert st == 0 and out == data and counts[2] >= 2


# ---- offsets beyond 2^32 ----------------------------------------------------------------------------------------------------------

def test_entries_carry_into_the_high_words(lib):
    """One leg from a start state whose bases lie just under 2^32 bits and 2^32 bytes: the entries it writes carry into the high words,
    and so do the end bit and the decoded length.  Nothing of that size is decoded: the leg sees its windows only."""
    rng = random.Random(2)
    data = bytes(rng.choices(LETTERS, k=120_000))
    body = deflate(data, RAW, 6, flush_every=15_000)                  # one block a flush: headers at every 15 000 decoded bytes
    window = bytes(rng.choices(LETTERS, k=32768))
    in_base, out_base = (1 << 29) - 4096, (1 << 32) - 40_000 & ~15
    first_bit, first_out = 8 * (in_base + 5), out_base + 7 + 32768
    buf_in = ctypes.create_string_buffer(bytes(5) + body + bytes(32))
    buf_out = ctypes.create_string_buffer(bytes(7) + window + bytes(len(data) + 64))
    idx = ctypes.create_string_buffer(1 << 20)
    s, w = emu.fresh(lib), emu.LegPlan()
    s.start, s.bit, s.out, s.origin = emu.BLOCK, first_bit, first_out, 12345
    s.mk_seen, s.mk_count, s.mk_last, s.mk_bytes = 5, 5, first_out - 1000, 64 + 5 * (24 + 32768)
    v, grew = emu.next_leg(lib, s, w, in_base + 5 + len(body), first_out + len(data), 1 << 20, 1 << 20)
    assert v == emu.GO and (w.in_base, w.out_base, w.in_final, w.out_final) == (in_base, out_base, 1, 1)
    lib.emu_leg_run(RAW, ctypes.addressof(buf_in), ctypes.addressof(buf_out), SPAN, ctypes.addressof(idx), 1 << 20, ctypes.addressof(s), ctypes.addressof(w))
    assert (s.done, s.status) == (1, 0)
    assert s.end_out == first_out + len(data) and s.end_out >> 32 == 1
    assert buf_out.raw[7 + 32768:7 + 32768 + len(data)] == data
    assert s.mk_end > first_bit and s.mk_end >> 32 == 1
    got = [struct.unpack_from("<QQII", idx.raw, 64 + 24 * k) for k in range(5, s.mk_count)]
    assert len(got) >= 4 and s.mk_seen == s.mk_count
    # checkpoints are due by the running offset, which the state brought along: 1000 bytes in front of the leg's first byte
    offs = [o - first_out for b, o, h, z in got]
    want, last = [], -1000
    for at in range(0, len(data) + 1, 15_000):
        if at - last >= SPAN:
            want.append(at); last = at
    assert offs == want, (offs, want)
    assert all(h == 32768 and z == 0 for b, o, h, z in got)
    assert any(b >> 32 == 1 for b, o, h, z in got) and any(o >> 32 == 1 for b, o, h, z in got)
    assert first_bit >> 32 == 0 and first_out >> 32 == 0, "the leg starts under 2^32: the carry happens inside it"
    # every entry's bit is a block header of the body: libz decodes from there with the window in front
    whole = window + data
    for b, o, h, z in got:
        index_ref.check_checkpoint(body, data, b - first_bit, o - first_out, whole[32768 + (o - first_out) - h:32768 + (o - first_out)])
