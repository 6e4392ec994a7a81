"""What the batched seek-index calls add to index_core.h, without a GPU (tests/emu/index_batch_emu.cpp): the table-driven index CRC against
zlib.crc32, index_parse on top of it against the rules one by one, the plan of a batch of (stream, offset, length) triples against a
plan computed in Python, and the layout of a stream's checksum pieces."""
import random
import zlib

import pytest

import index_batch_cases as cases
import index_batch_emu_binding as emu
import index_ref
from index_ref import GZIP, RAW, ZLIB


@pytest.fixture(scope="module")
def lib():
    return emu.load()


@pytest.fixture(scope="module")
def batch():
    return cases.batch()


def test_table_crc_equals_zlib(lib):
    """Every length 0 .. 100 at every alignment of the start (the code steps 16 bytes at a time and has no other boundary: its length is
    64 bits, there is no 2^30 chunk on the host any more), a 1 MiB random buffer, and the register carried across calls."""
    rng = random.Random(1)
    buf = bytes(rng.getrandbits(8) for _ in range(300)) + random.Random(2).randbytes(1 << 20)
    for n in range(101):
        for a in range(16):
            assert lib.emu_crc_tables(buf[a:a + n], n) == zlib.crc32(buf[a:a + n]), (n, a)
    for n in (127, 128, 129, 255, 256, 257, 4095, 4096, 4097, 65535, 65536, 65537):
        assert lib.emu_crc_tables(buf[3:3 + n], n) == zlib.crc32(buf[3:3 + n]), n
    big = buf[300:]
    assert len(big) == 1 << 20
    assert lib.emu_crc_tables(big, len(big)) == zlib.crc32(big)
    assert lib.emu_crc_bits(big[:70_001], 70_001) == zlib.crc32(big[:70_001])          # (the old form, for the record)
    c = 0xffffffff
    for lo, hi in ((0, 7), (7, 7), (7, 40), (40, 100_003), (100_003, len(big))):       # slices of any length, an empty one too
        c = lib.emu_crc_tables_from(c, big[lo:hi], hi - lo)
    assert c ^ 0xffffffff == zlib.crc32(big)


def test_parse_gives_the_same_answers(lib, batch):
    """The malformed indexes of test_inflate_index_cpu.py's kind, one per rule, through index_parse with the faster CRC."""
    datas, streams, indexes = batch
    data, stream, idx = datas[1], streams[1], indexes[1]
    ix = index_ref.parse(idx)
    fault, f = emu.parse(lib, idx)
    assert fault == "ok" and f["count"] == 4 and f["wrap"] == ZLIB and f["decoded_len"] == len(data) and f["stream_len"] == len(stream)
    assert f["end_bit"] == ix.end_bit and f["check"] == zlib.adler32(data) and f["win_off"] == 64 + 4 * 24
    assert emu.parse(lib, b"ZWZIDX\x00\x02" + idx[8:])[0] == "magic"
    assert emu.parse(lib, idx[:48])[0] == "length"
    assert emu.parse(lib, idx + bytes(8))[0] == "length"
    assert emu.parse(lib, idx + bytes(16))[0] in ("crc", "window_sum")
    assert emu.parse(lib, index_ref.compose(ix, crc=zlib.crc32(idx[64:]) ^ 1))[0] == "crc"
    for at in (64, 65, 64 + 4 * 24 + 5, len(idx) - 20, len(idx) - 17):                 # an entry byte and window bytes, CRC not redone
        flipped = bytearray(idx)
        flipped[at] ^= 0x40
        assert emu.parse(lib, bytes(flipped))[0] == "crc", at
    mk = lambda **kw: index_ref.compose(index_ref.Index(**{**ix.__dict__, **kw}))
    e, w = ix.entries, ix.windows
    assert emu.parse(lib, mk(windows=w[:-1] + [w[-1][:-17]]))[0] == "window_sum"
    assert emu.parse(lib, mk(entries=[e[0], e[2], e[1], e[3]], windows=[w[i] for i in (0, 2, 1, 3)]))[0] == "order"
    assert emu.parse(lib, mk(entries=[e[0], e[1], (e[1][0], e[2][1], e[2][2]), e[3]]))[0] == "order"
    assert emu.parse(lib, mk(entries=[(e[0][0], 1, 0)] + e[1:]))[0] == "order"
    assert emu.parse(lib, mk(entries=[e[0], (e[1][0], e[1][1], e[1][1] + 1)] + e[2:], windows=[b"", data[:20_001]] + w[2:]))[0] == "hist"
    assert emu.parse(lib, mk(end_bit=8 * len(stream) + 1))[0] == "end_bit"
    assert emu.parse(lib, mk(end_bit=e[3][0]))[0] == "end_bit"
    assert emu.parse(lib, mk(span=3 << 14))[0] == "field"
    assert emu.parse(lib, mk(wrap=3))[0] == "field"
    assert emu.parse(lib, mk(decoded_len=1032 * len(stream) + 1032))[0] == "field"
    assert emu.parse(lib, mk(decoded_len=1032 * len(stream)))[0] == "ok"


def test_batch_plan_equals_python(lib, batch):
    """The triples of the GPU range test: the same touched (stream, segment) list and the same pieces as a plan computed in Python;
    unnamed streams' indexes are not read; the bad ranges are named."""
    _, _, indexes = batch
    trip = cases.triples()
    want_total, want_rows = cases.python_plan(indexes, trip)
    code, total, rows = emu.plan(lib, indexes, trip)
    assert code == -1 and total == want_total == sum(t[2] for t in trip)
    assert rows == want_rows
    assert {s for s, _, _ in rows} == {0, 1, 2, 3, 4, 7}
    assert (2, 0) in [(s, g) for s, g, _ in rows] and (2, 1) in [(s, g) for s, g, _ in rows] and (2, 2) in [(s, g) for s, g, _ in rows]
    # an index no range names may be rubbish; one that a range names may not
    broken = list(indexes)
    broken[5] = b"rubbish" + bytes(89)
    broken[6] = b""
    assert emu.plan(lib, broken, trip)[0] == -1
    broken[3] = broken[5]
    assert emu.plan(lib, broken, trip)[0] == -2 - 3
    n = len(indexes)
    assert emu.plan(lib, indexes, trip[:4] + [(n, 0, 0)] + trip[4:])[0] == 4                # a stream number past the batch
    assert emu.plan(lib, indexes, trip[:7] + [(2, cases.N, 1)])[0] == 7                     # one byte past the end
    assert emu.plan(lib, indexes, [(1, 0, 1), (1, 1, 2 ** 64 - 1)])[0] == 1                 # offset + length overflows
    assert emu.plan(lib, indexes, []) == (-1, 0, [])
    # random triples
    rng = random.Random(9)
    rnd = [(rng.randrange(5), a, rng.randrange(min(3000, cases.N - a) + 1)) for a in (rng.randrange(cases.N + 1) for _ in range(300))]
    want_total, want_rows = cases.python_plan(indexes, rnd)
    assert emu.plan(lib, indexes, rnd) == (-1, want_total, want_rows)


def test_piece_layout(lib):
    """Per stream: a head up to the next 16-byte boundary, then pieces of 65 280 bytes; none for a raw stream."""
    P = 65280
    for low4 in range(16):
        head_room = -low4 % 16
        for total in (0, 1, 14, 15, 16, 17, P - 1, P, P + 1, P + 15, P + 16, 3 * P + 7, 200_000):
            head = min(head_room, total)
            want = [(0, head)] + [(head + j * P, min(P, total - head - j * P)) for j in range((total - head + P - 1) // P)]
            for wrap in (ZLIB, GZIP):
                assert emu.piece_layout(lib, wrap, low4, total) == (len(want), want), (low4, total)
            assert emu.piece_layout(lib, RAW, low4, total) == (0, [])
    assert emu.piece_layout(lib, GZIP, 5, (1 << 40) + 3, cap=2)[0] == 1 + ((1 << 40) + 3 - 11 + P - 1) // P
