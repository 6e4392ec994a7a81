"""The batch of indexed streams and the (stream, offset, length) triples that the range tests of the batched seek-index calls share:
tests/test_gpu_inflate_index_batch.py reads them on the GPU, tests/test_inflate_index_batch_cpu.py plans them on the host.  Streams and
indexes come from libz and index_ref, the expected plan from plain Python.  Test infrastructure only."""
import bisect
import random

import deflate_gen
import index_ref
from index_ref import GZIP, RAW, ZLIB

N = 200_000
CUTS = [20_000, 70_000, 140_000]
WRAPS = [GZIP, ZLIB, RAW, GZIP, ZLIB, GZIP, RAW, ZLIB]


def batch():
    """Eight streams of N text bytes with sync flushes at CUTS, their Python-composed indexes of four segments -> (datas, streams, indexes)."""
    text = deflate_gen.text(random.Random(23), N + 7 * 30_000)
    datas = [text[30_000 * i:30_000 * i + N] for i in range(len(WRAPS))]
    pairs = [index_ref.sync_flush_stream(d, CUTS, w) for d, w in zip(datas, WRAPS)]
    return datas, [p[0] for p in pairs], [p[1] for p in pairs]


def triples():
    """Over streams 0 .. 4 and 7, scrambled: repeats and overlaps, empty ranges (one at a stream's very end), ranges across one and two
    segment boundaries, a whole stream.  Streams 5 and 6 are named by no range; of stream 7 only segment 0 is touched."""
    t = [(0, 5, 300), (0, 5, 300), (0, 100, 400), (0, 150_000, 5_000),
         (1, 0, 0), (1, N, 0), (1, 70_000, 0), (1, 69_990, 9),
         (2, 19_990, 20), (2, 19_000, 60_000), (2, 139_999, 2),
         (3, 0, N),
         (4, N - 1, 1), (4, N - 4096, 4096), (4, 20_000, 1), (4, 19_999, 1),
         (7, 10, 100), (7, 19_999, 1)]
    random.Random(4).shuffle(t)
    return t


def python_plan(indexes, trip):
    """The plan of zwz_inflate_read_ranges_batch_dev in plain Python -> (total, [(stream, segment, [(dst, off, len), ...]), ...]):
    the touched segments ascending by (stream, segment), each with its pieces in range order.  A byte belongs to the LAST entry at or
    below its offset."""
    rows, dst = {}, 0
    for s, a, n in trip:
        ix = index_ref.parse(indexes[s])
        offs = [e[1] for e in ix.entries]
        assert a + n <= ix.decoded_len
        at = a
        while at < a + n:
            g = bisect.bisect_right(offs, at) - 1
            end = offs[g + 1] if g + 1 < len(offs) else ix.decoded_len
            take = min(a + n, end) - at
            rows.setdefault((s, g), []).append((dst, at - offs[g], take))
            at += take
            dst += take
    return dst, [(s, g, rows[(s, g)]) for s, g in sorted(rows)]
