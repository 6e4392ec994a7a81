"""zwz_deflate_dep_streams_dev on the GPU where tests/test_gpu_deflate_dep.py's corpus kinds do not reach: the hand-built pieces of
tests/dep_cases.py (the entry at `skip` of lz_match, lz_parse, lz_lazy and blockify; blocks counted from there) under every value of
the match option at every level, streams of 64 to 1 030 pieces whose checksums go through dstream_combine_kernel's rows of two and
more values, 0xff bytes through dstream_adler_kernel, and twenty thousand streams through the layout's search.  Every output is
compared with libz's (tests/deflate_dep_ref.py), byte for byte."""
import random

import numpy as np
import pytest

import corpus
import deflate_dep_ref as ref
import dep_cases
import test_gpu_deflate_dep as base
from test_gpu_deflate_dep import bounds, check_equal, run_batch

pytestmark = pytest.mark.gpu

P, D = ref.P, ref.D
MATCHES, LEVELS = dep_cases.MATCHES, dep_cases.LEVELS

z, torch_first, codec, small_codec = base.z, base.torch_first, base.codec, base.small_codec


def assemble(body, data, wrap, level=6):
    """deflate_dep_ref.deflate_dep_stream from its parts: the pieces' shares are the same under every wrapper"""
    return ref.header(wrap, level) + body + b"\x03\x00" + ref.trailer(wrap, data)


class Reference:
    """libz's streams of a list of buffers per (wrapper, level); the pieces are compressed once a level"""

    def __init__(self, bufs):
        self.bufs, self.bodies = bufs, {}

    def __call__(self, wrap, level=6):
        if level not in self.bodies:
            self.bodies[level] = [b"".join(ref.pieces(b, level)) for b in self.bufs]
        return [assemble(body, b, wrap, level) for body, b in zip(self.bodies[level], self.bufs)]


def check_named(names, bufs, want, st, olen, out, what):
    bad = [names[i] for i in range(len(bufs)) if st[i] != 0 or olen[i] != len(want[i]) or out[i] != want[i]]
    try:
        check_equal(bufs, want, st, olen, out)
    except AssertionError as e:
        raise AssertionError("%s: %d differ: %s\n%s" % (what, len(bad), "; ".join(bad[:30]), e)) from None
    assert not bad


# ---- the hand-built cases ---------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def case_batch():
    """Every case in a fixed shuffled order, an empty or a one-byte stream behind every third"""
    cases = dep_cases.cases()
    random.Random(31).shuffle(cases)
    names, bufs = [], []
    for i, c in enumerate(cases):
        names.append(c.name)                     # family: shape, background, piece
        bufs.append(c.data)
        if i % 3 == 0:
            names.append("(filler behind %s)" % c.name)
            bufs.append(b"" if i % 2 else bytes([i & 255]))
    assert ref.deflate_dep_stream(bufs[0][:P + 1], "zlib", 4) == assemble(b"".join(ref.pieces(bufs[0][:P + 1], 4)), bufs[0][:P + 1], "zlib", 4)
    return names, bufs, Reference(bufs)


@pytest.mark.parametrize("slices", ("default", "five"))
@pytest.mark.parametrize("match", MATCHES)
def test_every_case_under_every_route(z, codec, small_codec, torch_first, case_batch, match, slices):
    names, bufs, want = case_batch
    c = codec if slices == "default" else small_codec
    seen = 0
    c.set_option("match", match)
    try:
        for li, level in enumerate(LEVELS):
            wrap = dep_cases.wrapper_of(match, li, slices == "five")                     # all three at every level, over the six values
            c.set_level(level)
            st, olen, out = run_batch(c, torch_first, wrap, bufs, bounds(z, bufs, wrap))
            check_named(names, bufs, want(wrap, level), st, olen, out, "match %s, level %d, %s, %s slices" % (match, level, wrap, slices))
            seen += len(out)
    finally:
        c.set_level(0)
        c.set_option("match", "auto")
    assert seen == 3 * len(bufs)


def test_the_wrappers_rotate():
    dep_cases.check_wrappers_rotate()


# ---- long streams -----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def long_streams():
    """dep_cases.LONG_STREAMS, which says what the order is for"""
    make = {"text": corpus.text_like, "random": corpus.random_bytes, "lz_heavy": corpus.lz_heavy, "ff": lambda seed, n: b"\xff" * n}
    names = [s[0] for s in dep_cases.LONG_STREAMS]
    bufs = [make[kind](seed, n) for (_, kind, seed, _, _), n in zip(dep_cases.LONG_STREAMS, dep_cases.long_stream_lengths())]
    return names, bufs, Reference(bufs)


def test_the_long_streams_fill_the_combine_s_rows(long_streams):
    """The arithmetic of the order, on the buffers that go in: full pieces of 63, 64, 65 and 128 and more in a slice"""
    names, bufs, _ = long_streams
    dep_cases.check_long_stream_order(names, [len(b) for b in bufs])


@pytest.fixture(scope="module", params=(0, 64, 65, 100))
def sliced_codec(request, z, torch_first):
    assert (request.param or dep_cases.DEFAULT_SLICE) in dep_cases.LONG_SLICES       # the slices check_long_stream_order counts in
    c = z.Codec(0, max_batch_chunks=request.param)
    yield c
    c.close()


def test_long_streams(z, sliced_codec, torch_first, long_streams):
    names, bufs, want = long_streams
    for wrap in ("zlib", "gzip"):
        st, olen, out = run_batch(sliced_codec, torch_first, wrap, bufs, bounds(z, bufs, wrap))
        check_named(names, bufs, want(wrap), st, olen, out, wrap)


def test_long_streams_raw(z, codec, torch_first, long_streams):
    names, bufs, want = long_streams
    st, olen, out = run_batch(codec, torch_first, "raw", bufs, bounds(z, bufs, "raw"))
    check_named(names, bufs, want("raw"), st, olen, out, "raw")


@pytest.fixture(scope="module")
def hundred_codec(z, torch_first):
    c = z.Codec(0, max_batch_chunks=100)
    yield c
    c.close()


@pytest.fixture(scope="module")
def indexed():
    data = corpus.text_like(62, 130 * P)
    cache = {}

    def want(span):
        if span not in cache:
            cache[span] = ref.dep_index(data, "gzip", 6, span or 1 << 20)
        return cache[span]
    return data, want


@pytest.mark.parametrize("span", (32768, 65536, None))
def test_long_stream_with_its_index(z, codec, hundred_codec, indexed, span):
    data, want = indexed
    for c in (codec, hundred_codec):
        (stream, index), = c.deflate_dep_streams_index([data], "gzip", span)
        assert (stream, index) == want(span), (span, len(stream), len(index), len(want(span)[0]), len(want(span)[1]))
        assert len(index) == z.deflate_dep_stream_index_bound(len(data), span)
        assert c.inflate_indexed(stream, index) == data


def test_long_file_with_its_index_in_slices(z, hundred_codec, indexed, tmp_path):
    """The partial form with a dictionary in front of a slice's first piece, 100 pieces of one stream in a slice"""
    data = indexed[0] + b"tail."
    (tmp_path / "in").write_bytes(data)
    for wrap, span in (("gzip", 65536), ("zlib", 32768)):
        hundred_codec.deflate_dep_stream_file_index(tmp_path / "in", tmp_path / "out", tmp_path / "idx", wrap, span=span)
        stream, index = ref.dep_index(data, wrap, 6, span)
        assert (tmp_path / "out").read_bytes() == stream and (tmp_path / "idx").read_bytes() == index, (wrap, span)


# ---- many streams -----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def many():
    rng = np.random.default_rng(20001)
    pool = corpus.text_like(70, 8 << 20) + corpus.random_bytes(71, 4 << 20) + b"\xff" * (1 << 20) + corpus.text_like(72, 4 << 20)
    sizes = rng.integers(0, 301, 20000)
    sizes[::50] = rng.integers(1, 3 * P + 1, 400)                  # 1 to 3 pieces: steps between long flat stretches of pfirst
    sizes[100:150:50] = P
    sizes[::997] = 0
    starts = rng.integers(0, len(pool) - 3 * P, 20000)
    bufs = [pool[s:s + k] for s, k in zip(starts.tolist(), sizes.tolist())]
    assert 20 << 20 < sum(sizes) < 30 << 20 and {-(-len(b) // P) for b in bufs} == {0, 1, 2, 3}
    return bufs, [ref.deflate_dep_stream(b, "zlib") for b in bufs]


@pytest.mark.parametrize("slices", ("default", "hundred"))
def test_twenty_thousand_zlib_streams(z, codec, hundred_codec, torch_first, many, slices):
    bufs, want = many
    st, olen, out = run_batch(codec if slices == "default" else hundred_codec, torch_first, "zlib", bufs, bounds(z, bufs, "zlib"))
    check_equal(bufs, want, st, olen, out)
