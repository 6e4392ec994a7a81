"""tests/dep_cases.py without a GPU: every case reaches the shape it claims on the host build of the portable cores (tests/emu_dep), a
case list that stops reaching one is refused, and the emu writes libz's bytes for every case at levels 4, 5 and 6 and for long
streams whose checksums go through the combine schedule with more than 64 full pieces in a slice."""
import dataclasses
import random

import pytest

import deflate_dep_emu_binding as emu_binding
import deflate_dep_ref as ref
import dep_cases

P = ref.P


@pytest.fixture(scope="module")
def emu():
    return emu_binding.load()


@pytest.fixture(scope="module")
def cases():
    return dep_cases.cases()


def test_every_claim_holds(cases, emu):
    dep_cases.check(cases, emu)
    s = dep_cases.summary(cases)
    print({f: s[f] for f in sorted(s)}, "in all:", len(cases), "cases,", sum(b for _, b in s.values()), "bytes")
    assert sum(n for n, _ in s.values()) == len(cases) and set(s) == {"a", "b", "d", "e"}


def test_every_family_stands_on_both_backgrounds(cases):
    for fam in "abde":
        assert {"sparse", "dense"} <= {c.background for c in cases if c.family == fam}, fam
    # every shape of a, b and d that a background can change has both; a and b stand at pieces 1 and 3
    for fam in "abd":
        for shape in {c.shape for c in cases if c.family == fam} - {"slid window source 32768", "slid window source 32769"}:
            assert {c.background for c in cases if c.shape == shape} == {"sparse", "dense"}, shape
    for fam in "ab":
        for shape in {c.shape for c in cases if c.family == fam}:
            assert {c.piece for c in cases if c.shape == shape} == {1, 3}, shape


def test_a_broken_geometry_is_noticed(cases, emu):
    """check() is a condition, not a measurement: a case list that stops reaching a shape fails it."""
    def without(f):
        with pytest.raises(AssertionError):
            dep_cases.check([c for c in cases if not f(c)], emu)
    without(lambda c: c.shape == "edge 32506 at 0" and c.background == "dense" and c.piece == 3)
    without(lambda c: c.shape == "nothing pending")
    without(lambda c: c.shape == "query at 256" and c.background == "sparse")
    without(lambda c: c.shape.startswith("slid window"))
    without(lambda c: c.shape == "short 3 near")
    without(lambda c: c.shape == "match as symbol 16384")
    without(lambda c: c.family == "e" and c.piece == 2)
    # ... and a case whose bytes stop producing the claimed tokens
    k = next(i for i, c in enumerate(cases) if c.shape == "edge 32506 at 0")
    c = cases[k]
    moved = dep_cases.Case(c.family, c.shape, c.background, c.data[1:P - 100] + b"\x00" + c.data[P - 100:], c.piece, c.claim, c.levels)
    with pytest.raises(AssertionError):
        dep_cases.check(cases[:k] + [moved] + cases[k + 1:], emu)
    # ... and a candidate that cannot run past the piece's end: the next piece gone, or beginning with what padding would hold.  The
    # tokens stay what they were, the bytes behind the piece decide
    k = next(i for i, c in enumerate(cases) if c.shape == "candidate runs past the end" and c.background == "dense" and c.piece == 3)
    c, end = cases[k], 4 * P
    assert len(c.data) > end + c.behind
    for data, behind in ((c.data[:end], 0), (c.data[:end], c.behind), (c.data[:end] + bytes(c.behind) + c.data[end + c.behind:], c.behind),
                         (c.data[:end + 3] + b"\x00" + c.data[end + 4:], c.behind)):
        with pytest.raises(AssertionError):
            dep_cases.check([dataclasses.replace(c, data=data, behind=behind)] + cases[:k] + cases[k + 1:], emu)


def test_the_gpu_batches_are_ordered_as_their_comments_say():
    """What tests/test_gpu_deflate_dep_cases.py asserts of its own batches, where no GPU is needed to see an order go wrong"""
    names = [s[0] for s in dep_cases.LONG_STREAMS]
    dep_cases.check_long_stream_order(names, dep_cases.long_stream_lengths())
    dep_cases.check_wrappers_rotate()
    lens = dep_cases.long_stream_lengths()
    with pytest.raises(AssertionError):                                  # without the stream of 7 pieces in front the counts are others
        dep_cases.check_long_stream_order(names, [0] + lens[1:])


@pytest.mark.parametrize("level", (4, 5, 6))
def test_emu_writes_libz_bytes_for_every_case(cases, emu, level):
    for i, c in enumerate(cases):
        wrap = ref.WRAPS[(i + level) % 3]
        want = ref.deflate_dep_stream(c.data, wrap, level)
        for pieces in (2, 8192) if len(c.data) > 2 * P else (2,):       # (two pieces are one slice either way: the same call)
            got = emu_binding.stream(emu, c.data, wrap, level, pieces)
            assert got == want, (c.name, level, wrap, pieces, len(got), len(want))


@pytest.mark.parametrize("pieces,last,slice_pieces", ((65, 1, 8192), (66, P, 8192), (130, 5, 100), (130, P, 64)))
def test_long_streams_through_the_combine_schedule(emu, pieces, last, slice_pieces):
    """More than 64 full pieces of a stream in a slice: the rows of K >= 2 values, the padding in front, sum_ptimes(p1, K)"""
    n = (pieces - 1) * P + last
    for data in (b"\xff" * n, random.Random(pieces).randbytes(n)):
        for wrap in ("zlib", "gzip"):
            assert emu_binding.stream(emu, data, wrap, 6, slice_pieces) == ref.deflate_dep_stream(data, wrap, 6), (pieces, last, slice_pieces, wrap, data[:1])
