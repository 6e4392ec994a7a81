"""The geometry corpus of the inflate kernel's batch copy (tests/copy_corpus.py) on the CPU: its own preconditions (every shape it is
there for is reached, from the token lists alone), then the CPU oracle and the host build of the product's decoder -- plain, and with the
kernel's byte-wise copy in both owner forms (per-byte map up to 1024 bytes, binary search) at batches of 64 and 5 symbols -- against
libz on every case of at most 65 535 bytes; and the emu's own counters over the corpus, which say that the byte-wise copy did go
through a 63-deep chase, mapped and searched batches, self-overlap inside a batch and the one-symbol path."""
import pytest

import copy_corpus
import emu_binding
import libz_ref

CHUNK = 65535


@pytest.fixture(scope="module")
def cases():
    cs = copy_corpus.corpus()                      # (runs copy_corpus.check)
    print("\ncopy corpus (%s): %s" % (libz_ref.describe(), ", ".join("%s %d cases %d bytes" % (f, n, b) for f, (n, b) in sorted(copy_corpus.summary(cs).items()))))
    return cs


@pytest.fixture(scope="module")
def small(cases):
    """(case, zlib payload, libz's bytes, expected status) for every case that fits the chunk form"""
    out = []
    for c in cases:
        if len(c.data) > CHUNK:
            continue
        p = copy_corpus.wrapped(1, c.body, c.data)
        out.append((c, p, libz_ref.reference_inflate(p), libz_ref.expected_status(p)))
    return out


@pytest.fixture(scope="module")
def emu():
    return emu_binding.load()


def test_preconditions(cases, small):
    copy_corpus.check(cases)
    fams = copy_corpus.summary(cases)
    assert all(fams[f][0] >= 10 for f in "abcdefgh"), fams
    assert len(small) > 700
    for c, p, want, st in small:
        assert want == c.data and st == (libz_ref.END if c.valid else libz_ref.DATA_ERROR), c.name


def test_a_broken_geometry_is_noticed(cases):
    """check() is a condition, not a measurement: a corpus that stops reaching a shape fails it."""
    with pytest.raises(AssertionError):
        copy_corpus.check([c for c in cases if "d37 " not in c.name])
    with pytest.raises(AssertionError):
        copy_corpus.check([c for c in cases if "edge 1024 " not in c.name])
    with pytest.raises(AssertionError):
        copy_corpus.check([c for c in cases if not (c.family == "b" and " deep " in c.name and " long " in c.name)])
    with pytest.raises(AssertionError):
        copy_corpus.check([c for c in cases if "long length code" not in c.name and "long distance code" not in c.name and "valid slow" not in c.name])


def test_oracle_matches_libz(small, oracle):
    for c, p, want, _ in small:
        got, total, _ = oracle.inflate(p, 1 << 17)
        assert total == len(want) and got == want, c.name


def test_emu_inflate_matches_libz(small, emu):
    for c, p, want, want_st in small:
        assert emu_binding.inflate(emu, p) == (want, want_st), c.name


@pytest.mark.parametrize("own_cap", [1024, 0])
def test_emu_bytewise_copy_matches_libz(small, emu, own_cap):
    emu_binding.copy_counters(emu)
    for c, p, want, want_st in small:
        for batch in (64, 5):
            assert emu_binding.inflate_bytewise_mapped(emu, p, CHUNK, batch, own_cap) == (want, want_st), (c.name, batch)
        if own_cap == 0:
            assert emu_binding.inflate_bytewise(emu, p, CHUNK, 64) == (want, want_st), c.name
    n = emu_binding.copy_counters(emu)
    print("\nbyte-wise copy, owner map up to %d bytes: %s" % (own_cap, n))
    assert n["deepest_chase"] >= 63, n
    assert n["batches_above_cap"] > 0 and n["self_overlap_in_batch"] > 0 and n["slow_matches"] > 0, n
    assert (n["batches_mapped"] > 0) == (own_cap > 0), n


def test_capacity_twins_stop_at_the_symbol(cases, emu):
    """The three streams around 65 535 bytes in the chunk form's decoder: the end, and the stop in front of the symbol that would cross."""
    twins = {c.name: c for c in cases if c.family == "cap"}
    for name, st, n in (("65535 by a 258 match", libz_ref.END, CHUNK), ("65536 by a 258 match", libz_ref.OVERFLOW, CHUNK - 257),
                        ("a literal at 65535", libz_ref.OVERFLOW, CHUNK)):
        c = twins[name]
        assert c.stop_length(CHUNK) == n
        p = copy_corpus.wrapped(1, c.body, c.data)
        assert libz_ref.expected_status(p) == st and libz_ref.reference_inflate(p) == c.data
        assert emu_binding.inflate(emu, p) == (c.data[:n], st), name

