"""Chunks built for lz_match_band's second pass (csrc/zwz_band.hip; csrc/lz_band.h: band_deep_batched), and the host build of that
pass (tests/emu_band) that says what their walks look like.  Shared by tests/test_band_pass2_cpu.py and tests/test_gpu_band_pass2.py.

A chunk is 6.1 - 12.2 KB of random letters '@'..'_' -- 32 values whose trigrams zlib's hash keeps apart, so every bucket holds one trigram
and the tiles are "pure" -- with copies of a base string planted in it.  A copy of `n` bytes is followed by a byte that differs from the
base string's next one: its common length with a longer copy is exactly n.  The position that is looked at (the "target") is the last
copy, of 300 bytes; the copies in front of it are its sharers, the nearest first."""
import ctypes
import os
import subprocess

import numpy as np

import corpus

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "parallel-data-compression-and-decompression_amd", "csrc")
TILE = 6016                 # kBandTile: sorted entries a tile
BAND = 128                  # kBand
FLAGGED, HALO, SLOW, PURE, NICE = 1, 2, 4, 8, 16
BATCHES = (4, 8, 16)        # the batch sizes that were swept (ZWZ_BAND_P2_BATCH): edges are built for all of them


def load():
    so = os.path.join(HERE, "emu_band", "libband_pass2_emu.so")
    src = os.path.join(HERE, "emu_band", "band_pass2_emu.cpp")
    deps = [src] + [os.path.join(CSRC, h) for h in ("lz_band.h", "lz_core.h", "zwz_common.h")]
    if not os.path.exists(so) or max(os.path.getmtime(d) for d in deps) > os.path.getmtime(so):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, src])
    lib = ctypes.CDLL(so)
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    lib.emu_search_records.restype = None
    lib.emu_search_records.argtypes = [ctypes.c_char_p, u32, vp, vp]
    lib.emu_band_pass2.restype = u32
    lib.emu_band_pass2.argtypes = [ctypes.c_char_p, u32, u32, ctypes.c_int, u32, vp, vp, vp, vp, vp, vp]
    return lib


def search_records(lib, data):
    n = len(data)
    a, b = np.zeros(n + 1, dtype=np.uint32), np.zeros(n + 1, dtype=np.uint32)
    lib.emu_search_records(data, n, a.ctypes.data, b.ctypes.data)
    return a[:n], b[:n]


class Walks:
    """What the emulator says about a chunk: records, and per position the second pass's chain."""
    def __init__(self, lib, data, tile=TILE, fmt=-1, batch=0):
        n = len(data)
        self.e128, self.e32 = np.zeros(n + 1, dtype=np.uint32), np.zeros(n + 1, dtype=np.uint32)
        self.chain, self.visited, self.k1 = (np.zeros(n + 1, dtype=np.uint16) for _ in range(3))
        self.flags = np.zeros(n + 1, dtype=np.uint8)
        self.pure_tiles = lib.emu_band_pass2(data, n, tile, fmt, batch, self.e128.ctypes.data, self.e32.ctypes.data, self.chain.ctypes.data,
                                             self.visited.ctypes.data, self.k1.ctypes.data, self.flags.ctypes.data)
        assert self.pure_tiles != 0xffffffff, "batch size %d is not built into the emulator" % batch
        self.e128, self.e32 = self.e128[:n], self.e32[:n]


# ------------------------------------------------------------------------------------------------ building
def _letters(seed, n):
    return (0x40 | (np.frombuffer(corpus.random_bytes(seed, n), dtype=np.uint8) & 31)).astype(np.uint8)


def _other(x):
    return 0x40 | ((int(x) + 1) & 31)


def hash3(a, b, c):
    return ((int(a) << 10) ^ (int(b) << 5) ^ int(c)) & 0x7fff


def trigram_of(h):
    """A trigram of letters with hash h (the letters' constant upper bits cost bits 6 and 11)."""
    h ^= (0x40 << 5) & 0x7fff ^ 0x40
    t = (0x40 | (h >> 10) & 31, 0x40 | (h >> 5) & 31, 0x40 | h & 31)
    return t


def common(data, q, p, cap=258):
    n = 0
    while n < cap and p + n < len(data) and data[q + n] == data[p + n]:
        n += 1
    return n


def sorted_index(data):
    """Position -> index in the (bucket, position) order lz_sort produces."""
    d = np.frombuffer(data, dtype=np.uint8).astype(np.int64)
    h = ((d[:-2] << 10) ^ (d[1:-1] << 5) ^ d[2:]) & 0x7fff
    order = np.lexsort((np.arange(len(h)), h))
    inv = np.empty(len(h), dtype=np.int64)
    inv[order] = np.arange(len(h))
    return inv


class Plan:
    """Letters of `size` bytes; base(h) makes a 300-byte base string whose trigram has hash h; put() plants copies."""
    def __init__(self, seed, size):
        self.seed, self.buf, self.at = seed, _letters(seed, size), 64

    def base(self, h, salt=0):
        b = _letters(self.seed * 1000 + salt, 300)
        b[:3] = trigram_of(h)
        return b

    def put(self, base, n, gap=3):
        """A copy of base[:n] at the next free place, a differing byte behind it.  Returns its position."""
        p = self.at
        assert p + n + 1 + gap <= len(self.buf), "the chunk is full"
        self.buf[p:p + n] = base[:n]
        if n < len(base):
            self.buf[p + n] = _other(base[n])
        self.at = p + n + 1 + gap
        return p

    def bytes(self):
        return self.buf.tobytes()


def _straddling(make, want=TILE, lo=40, hi=100):
    """make(h) -> (data, positions of the planted copies).  The h for which the copies' bucket lies across sorted index `want`, with at
    least `lo` copies in front of it and `hi` behind.  The bucket's place follows its hash -- but for the base string's second and
    third trigram, which move with it: bisection gets near, a walk over the neighbouring hashes does the rest."""
    def fits(h):
        data, pos = make(h)
        front = int((sorted_index(data)[pos] < want).sum())
        return data, pos, front
    a, b = 0, 0x7fff
    while a <= b:
        h = (a + b) // 2
        data, pos, front = fits(h)
        if front >= lo and len(pos) - front >= hi:
            return data, pos
        if front < lo:
            b = h - 1           # the bucket lies too far back in the order: a smaller hash moves it forward
        else:
            a = h + 1
    for step in range(1, 400):
        for h2 in (h - step, h + step):
            if 0 < h2 < 0x7fff:
                data, pos, front = fits(h2)
                if front >= lo and len(pos) - front >= hi:
                    return data, pos
    raise AssertionError("no hash puts the bucket across the tile's end")


def long_chain(seed=1):
    """(a) one 11-byte context 230 times: walks of 128 sharers, the cap, through the second tile's halo."""
    def make(h):
        pl = Plan(seed, 11800)
        base = pl.base(h)
        pos = [pl.put(base, 11 + (i * 7) % 5, gap=30 + (i * 11) % 9) for i in range(230)]
        return pl.bytes(), np.array(pos)
    return _straddling(make, lo=60, hi=110)


def batch_edges(seed=2):
    """(b) a context 41 times, every copy a little longer than the one before: the i-th copy walks exactly i - 1 sharers and improves on
    none but the nearest -- walks of H - 1, H, H + 1 and 2 H sharers for every H that was swept."""
    pl = Plan(seed, 9000)
    base = pl.base(0x2345)
    pos = [pl.put(base, 12 + i, gap=60) for i in range(41)]
    return pl.bytes(), np.array(pos)


def _mix(pl):
    """Two trigrams of one bucket near the chunk's end: '___' and '\x7f__' differ in a bit the hash drops.  Their bucket and those of
    the trigrams around them ('_' in front) are among the last in the order: the tile they fall into is impure, the one before is not."""
    for at, first in ((len(pl.buf) - 400, 0x5f), (len(pl.buf) - 200, 0x7f)):
        assert pl.at < at
        pl.buf[at - 2:at + 3] = (0x5f, 0x5f, first, 0x5f, 0x5f)


def length_edges(seed=3, deep=11):
    """(c) sharers whose common length with the target ends at deep + 7, + 8, + 15, + 16, + 17, and at 258 (the farthest: a length of
    `nice` or more ends the walk).  deep = 8: the context's bucket in the second tile, which is made impure."""
    pl = Plan(seed, 9000)
    base = pl.base(0x3456 if deep == 11 else 0x7800)
    if deep == 8:
        _mix(pl)
    lens = [300] + [deep + d for d in (17, 16, 15, 8, 7)]            # farthest first
    pos = [pl.put(base, n, gap=40) for n in lens]
    target = pl.put(base, 300, gap=200)
    return pl.bytes(), np.array(pos), target, lens


def nice_stop(seed=4):
    """(d) nearest first: 12 bytes, 130 (>= nice: zlib stops here), then longer ones in the same batch (200 at the third place) and in
    later ones (258 at the 6th, 10th and 18th place)."""
    pl = Plan(seed, 10500)
    base = pl.base(0x4567)
    lens = [12] * 20                                               # place k (1 = nearest)
    lens[1], lens[2], lens[5], lens[9], lens[17] = 130, 200, 300, 300, 300
    pos = [pl.put(base, n, gap=25) for n in reversed(lens)]         # planted farthest first
    target = pl.put(base, 300, gap=200)
    return pl.bytes(), np.array(pos[::-1]), target, lens


def snapshot(seed=5, near=True):
    """(e) the short chain's snapshot.  near: the nearest sharer is the first candidate, 44 sharers of 12 bytes, a sharer of 40 bytes
    as the 45th -- e32 is the best of the first 32, e128 the 40 bytes.  not near: 35 candidates with the trigram and other bytes behind
    it, then sharers of 30 bytes: the nearest sharer is the 36th candidate, e32 stays the first pass's."""
    pl = Plan(seed, 9000)
    base = pl.base(0x5678)
    if near:
        pos = [pl.put(base, 40, gap=30)] + [pl.put(base, 12, gap=30) for _ in range(44)]
    else:
        pos = [pl.put(base, 30, gap=30) for _ in range(4)]
        for i in range(35):
            other = pl.base(0x5678, salt=1 + i)
            other[3] = _other(base[3] + i % 7)                      # the trigram, then something else
            pl.put(other, 11, gap=30)
    target = pl.put(base, 300, gap=200)
    return pl.bytes(), np.array(pos), target


def tail(seed=6):
    """(f) the chunk ends in the first 27 bytes of a context seen before: flagged positions with 12 .. 27 bytes of lookahead."""
    pl = Plan(seed, 7000)
    base = pl.base(0x6789)
    for _ in range(5):
        pl.put(base, 60, gap=50)
    data = bytearray(pl.bytes())
    data[len(data) - 27:] = base[:27].tobytes()
    return bytes(data)


def mixed_bucket(seed=7):
    """(g) the long chain across the first tile's end, and far behind it in the order two trigrams of one bucket ('_' and 0x7f differ in a bit
    the hash drops): the second tile is impure behind a pure one, and walks that reach its halo go the slow way."""
    def make(h):
        pl = Plan(seed, 11800)
        base = pl.base(h)
        pos = [pl.put(base, 11 + (i * 5) % 4, gap=28 + (i * 13) % 11) for i in range(230)]
        _mix(pl)
        return pl.bytes(), np.array(pos)
    return _straddling(make, lo=60, hi=110)


def _len(e):
    return int(e) & 0xffff


def _dist(e):
    return int(e) >> 16


def checked_chunks(lib):
    """Every constructed chunk, by name -- each after the emulator has said that the feature it was built for is there."""
    out = {}

    def take(name, data):
        assert 6100 <= len(data) <= 12200, (name, len(data))
        out[name] = data
        return Walks(lib, data)

    data, pos = long_chain()                                        # (a)
    w = take("long_chain", data)
    assert len(pos) >= 200 and w.pure_tiles == 2
    assert int((w.chain[pos] >= BAND - 2).sum()) >= 90, "walks to the band's end: 128 candidates, of which the letters around may own one or two"
    through = [p for p in pos if w.flags[p] & HALO]
    assert len(through) >= 100 and all(w.chain[p] == w.visited[p] for p in through) and not any(w.flags[p] & SLOW for p in through)

    data, pos = batch_edges()                                       # (b)
    w = take("batch_edges", data)
    for i, p in enumerate(pos):
        assert w.chain[p] == i and w.visited[p] == i, (i, w.chain[p], w.visited[p])
    assert {h + d for h in BATCHES for d in (-1, 0, 1)} | {2 * h for h in BATCHES} <= set(range(len(pos)))

    for deep in (11, 8):                                            # (c)
        data, pos, target, lens = length_edges(deep=deep)
        w = take("length_edges_deep%d" % deep, data)
        assert bool(w.flags[target] & PURE) == (deep == 11) and w.flags[target] & FLAGGED
        assert [common(data, q, target) for q in pos] == [min(n, 258) for n in lens]
        assert sorted(n - deep for n in lens[1:]) == [7, 8, 15, 16, 17]
        assert w.visited[target] == len(pos) and _len(w.e128[target]) == 258 and _dist(w.e128[target]) == target - pos[0]

    data, pos, target, lens = nice_stop()                           # (d)
    w = take("nice_stop", data)
    assert [common(data, q, target) for q in pos] == [min(n, 258) for n in lens]
    assert w.chain[target] == len(pos) and w.visited[target] == 2 and w.flags[target] & NICE
    assert _len(w.e128[target]) == 130 and _dist(w.e128[target]) == target - pos[1]
    for h in BATCHES:                                               # a longer sharer behind the stop, inside its batch and in the next one
        assert any(lens[k] > 130 for k in range(2, h)) and any(lens[k] > 130 for k in range(h, 2 * h))

    data, pos, target = snapshot(near=True)                         # (e)
    w = take("snapshot_near", data)
    assert w.k1[target] == 1 and w.chain[target] == 45 and w.visited[target] == 45
    assert _len(w.e32[target]) == 12 and _len(w.e128[target]) == 40 and _dist(w.e128[target]) == target - pos[0]
    data, pos, target = snapshot(near=False)
    w = take("snapshot_far", data)
    assert w.k1[target] == 36 and _len(w.e128[target]) == 30 and w.e32[target] != w.e128[target]

    data = tail()                                                   # (f)
    w = take("tail", data)
    last = [p for p in range(len(data) - 27, len(data)) if w.flags[p] & FLAGGED]
    assert len(last) >= 12 and all(_len(w.e128[p]) == len(data) - p for p in last)

    data, pos = mixed_bucket()                                      # (g)
    w = take("mixed_bucket", data)
    assert w.pure_tiles == 1 and w.flags[pos[0]] & PURE
    assert sum(1 for p in pos if w.flags[p] & SLOW) >= 100, "walks into a halo of another format"
    return out
