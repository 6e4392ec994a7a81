"""The directory pipeline's portable parts (csrc/pipeline_core.h), on the CPU through tests/emu_pipeline/pipeline_emu.cpp: the slice size
against md5_routes.cap_for, the digest text against bytes.hex(), and the pwritev loop of the shard writer and the decode's file writers against a fake writer
that takes at most q bytes and p pieces a call and answers every third call with EINTR -- short writes that a file system rarely produces on demand."""
import bisect
import itertools

import pytest

import corpus
import md5_routes
import pipeline_emu_binding as emu


@pytest.fixture(scope="module")
def lib():
    return emu.load()


@pytest.mark.parametrize("k", [1, 2, 3, 64, 2048, 51200])
def test_slice_cap_is_cap_for(lib, k):
    for total in (0, 1, 2, 3, 4, 5, 127, 4095, 4096, 4097, 2 ** 31, 2 ** 32 - 1):      # the last one wrapped in 32 bits: slice size 1
        assert lib.emu_slice_cap(k, total) == md5_routes.cap_for(total, k), (k, total)


def test_digest_hex(lib):
    for d in (bytes(16), b"\xff" * 16, corpus.random_bytes(77, 16)):
        assert emu.digest_hex(lib, d) == d.hex()


# empty pieces at the front, in the middle and at the end; runs of small pieces (7 bytes end on a boundary after 3 + 4, a write of 7
# spans 2 + 2 + 2 + 1 of 5); 972 + 3096 bytes behind those 28 (a boundary at 4096), pieces larger than q = 4096, q itself, and three of 2000
SIZES = [0, 0, 3, 4, 0, 10, 2, 2, 2, 5, 0, 972, 3096, 5000, 1, 0, 0, 4096, 4095, 1, 9000, 2000, 2000, 2000, 300, 0, 0]
PIECES = [corpus.random_bytes(500 + i, n) for i, n in enumerate(SIZES)]
WHOLE = b"".join(PIECES)
OFF0 = 2 ** 32 + 5
CELLS = list(itertools.product((1, 7, 4096), (1, 3, 1024)))


def check_calls(calls, p):
    """The rules every call keeps; -> the kinds of short write seen: ends on a piece boundary / inside a piece / covers several pieces."""
    ends = list(itertools.accumulate(len(x) for x in PIECES))
    kinds = set()
    pos = 0                                   # bytes accepted so far
    for off, cnt, first_len, took in calls:
        assert off == OFF0 + pos, "a call's offset is the previous one plus what that call accepted"
        first = bisect.bisect_right(ends, pos)                  # the piece the next byte lies in (empty pieces skipped)
        assert 1 <= cnt <= p and first_len == ends[first] - pos, "the first piece passed is what is left of that piece, never empty"
        if took > 0:
            passed_end = ends[min(first + cnt, len(ends)) - 1]
            assert took <= passed_end - pos
            pos += took
            if pos < passed_end:                                 # a short write
                kinds.add("boundary" if pos in ends else "inside")
                if bisect.bisect_right(ends, pos - 1) - first >= 2:
                    kinds.add("several")
    return kinds


@pytest.mark.parametrize("q,p", CELLS, ids=["q%d-p%d" % c for c in CELLS])
def test_write_loop_short_writes_and_eintr(lib, q, p):
    ok, got, calls = emu.write_pieces(lib, PIECES, OFF0, q, p)
    assert ok and got == WHOLE
    assert any(c[3] < 0 for c in calls), "an EINTR answer was retried"
    kinds = check_calls(calls, p)
    assert "inside" in kinds
    if p > 1:                                 # (one piece a call: a short write can only end inside it)
        assert "boundary" in kinds
        assert q == 1 or "several" in kinds


@pytest.mark.parametrize("fail_at", [1, 2, 5, 40])
@pytest.mark.parametrize("q,p", [(7, 3), (4096, 1024)])
def test_write_loop_hard_failure(lib, q, p, fail_at):
    ok, got, calls = emu.write_pieces(lib, PIECES, OFF0, q, p, fail_at=fail_at)
    if fail_at > len(emu.write_pieces(lib, PIECES, OFF0, q, p)[2]):
        assert ok and got == WHOLE                     # (the loop was done before the failing call)
        return
    assert not ok and len(calls) == fail_at, "the loop stops at the failure"
    assert len(got) < len(WHOLE) and got == WHOLE[:len(got)]
    check_calls(calls, p)


def test_write_loop_nothing_to_write(lib):
    for pieces in ([], [b""], [b"", b"", b""]):
        ok, got, calls = emu.write_pieces(lib, pieces, OFF0, 7, 3)
        assert ok and got == b"" and calls == []
