"""Inflate against libz itself, on the CPU: the DEFLATE writer checks itself against libz, then the CPU oracle (oracle/zo_inflate.c) and
the host build of the product's decoder (csrc/inflate_core.h through tests/emu/zwz_emu.cpp) must give libz's bytes -- and the
product its status -- on the whole conformance corpus (tests/deflate_gen.py): zlib streams of every strategy, level, memLevel,
windowBits and flush mode, hand-built valid and invalid streams, size edges and damage."""
import collections

import pytest

import deflate_gen
import emu_binding
import libz_ref

CHUNK = 65535


@pytest.fixture(scope="module")
def corpus():
    cases = deflate_gen.conformance_corpus()
    counts = collections.Counter(c.group for c in cases)
    print("\ninflate conformance corpus (%s): %s" % (libz_ref.describe(), ", ".join("%s %d" % kv for kv in sorted(counts.items()))))
    assert set(counts) == set("abcde") and all(counts.values())
    return cases


@pytest.fixture(scope="module")
def reference(corpus):
    """(libz's output, expected status) per case."""
    return [(libz_ref.reference_inflate(c.payload), libz_ref.expected_status(c.payload)) for c in corpus]


@pytest.fixture(scope="module")
def emu():
    return emu_binding.load()


def _why(c):
    return "%s/%s (%d bytes, %s)" % (c.group, c.name, len(c.payload), libz_ref.describe())


def test_corpus_groups_are_all_there(corpus, reference):
    counts = collections.Counter(c.group for c in corpus)
    assert counts["a"] >= 1000 and counts["b"] >= 100 and counts["c"] >= 40 and counts["d"] >= 15 and counts["e"] >= 1000, counts
    status = collections.Counter(st for _, st in reference)
    assert all(status[s] for s in (0, 1, 2, 3)), status


def test_generator_against_libz(corpus):
    """Every stream the writer calls valid ends with Z_STREAM_END in libz and gives the bytes it recorded; every stream it built
    invalid on purpose does not end."""
    for c in corpus:
        if c.valid is None:
            continue
        if c.valid:
            out, rc = libz_ref._run(c.payload, None)
            assert rc == libz_ref.Z_STREAM_END and out == c.data, _why(c)
            raw, st = libz_ref.raw_inflate(c.body)
            assert raw == c.data and st in (0, 3), _why(c)
        else:
            assert libz_ref.expected_status(c.payload) != libz_ref.END, _why(c)


def test_oracle_matches_libz(corpus, reference, oracle):
    for c, (want, _) in zip(corpus, reference):
        got, total, _ = oracle.inflate(c.payload, 1 << 20)
        assert total == len(want) and got == want, _why(c)


def _check_product(c, got, st, want, want_st):
    if want_st == libz_ref.OVERFLOW:
        # the slot holds 65 535 bytes: decoding stops at the symbol that would cross it (a stored block is cut at it)
        assert st == libz_ref.OVERFLOW and want.startswith(got) and len(got) >= CHUNK - 257, (_why(c), len(got), st)
    else:
        assert st == want_st and got == want, (_why(c), len(got), len(want), st, want_st)


def test_emu_inflate_matches_libz(corpus, reference, emu):
    for c, (want, want_st) in zip(corpus, reference):
        got, st = emu_binding.inflate(emu, c.payload)
        _check_product(c, got, st, want, want_st)


def test_emu_bytewise_copy_matches_libz(corpus, reference, emu):
    """The kernel's batch copy (one byte per lane, owners by binary search), at the kernel's batch and at a short one."""
    for c, (want, want_st) in zip(corpus, reference):
        a = emu_binding.inflate(emu, c.payload)
        for batch in (64, 5):
            assert emu_binding.inflate_bytewise(emu, c.payload, CHUNK, batch) == a, (_why(c), batch)


def test_emu_packed_window_decode(corpus, emu):
    """The device's window decode on packed fast tables, slot by slot beside the classic decoder."""
    import ctypes
    ns, nslow = ctypes.c_uint64(), ctypes.c_uint64()
    total = 0
    for c in corpus:
        assert emu.emu_packed_window_check(c.payload, len(c.payload), ctypes.byref(ns), ctypes.byref(nslow)) == 0, _why(c)
        total += ns.value
    assert total > 1_000_000


def test_overflow_cases_stop_at_the_slot(corpus, reference, emu):
    over = [(c, w) for c, (w, s) in zip(corpus, reference) if s == libz_ref.OVERFLOW]
    assert len(over) >= 5
    for c, want in over:
        got, st = emu_binding.inflate(emu, c.payload)
        assert st == libz_ref.OVERFLOW and want.startswith(got) and len(got) >= CHUNK - 257, _why(c)
