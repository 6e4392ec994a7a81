"""Chunks built for the corners of lz_match_band's first pass (csrc/zwz_band.hip: two candidates' keys a word, trips of eight, masks a
trip beyond the wave's smallest count), and the host build of that pass (tests/emu_band/band_pass1_emu.cpp).  Shared by
tests/test_band_pass1_cpu.py and tests/test_gpu_band_pass1.py.

The chunks are tests/band_pass2_chunks.py's kind: 6.2 - 9 KB of random letters '@'..'_', whose trigrams zlib's hash keeps apart, with
copies of a base string planted in them; a copy of n bytes is followed by a byte that differs from the base string's next one, so
its common length with a longer copy is exactly n.  Every builder looks for a trigram the random letters around do not hold (a bucket's
counts are then the planted copies' alone) and asserts, from the emulator's view of the tiles, that the corner it is named for is
there."""
import ctypes
import os
import subprocess

import numpy as np

import band_pass2_chunks as bp

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = bp.CSRC
TILE = bp.TILE
BAND = bp.BAND
TOO_FAR = 4096
TRIPS = (7, 8, 9, 15, 16, 17, 31, 32, 33)          # candidates around every trip's end the levels' chains know (16 / 32: caps and snapshots)


def load():
    so = os.path.join(HERE, "emu_band", "libband_pass1_emu.so")
    src = os.path.join(HERE, "emu_band", "band_pass1_emu.cpp")
    deps = [src] + [os.path.join(CSRC, h) for h in ("lz_band.h", "lz_core.h", "zwz_common.h")]
    if not os.path.exists(so) or max(os.path.getmtime(d) for d in deps) > os.path.getmtime(so):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, src])
    lib = ctypes.CDLL(so)
    vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    lib.emu_pass1_pairs.restype = u32
    lib.emu_pass1_pairs.argtypes = [u64]
    lib.emu_pass1_masks.restype = u32
    lib.emu_pass1_masks.argtypes = []
    lib.emu_pass1_sweep.restype = u32
    lib.emu_pass1_sweep.argtypes = [ctypes.c_int, u32, u32, u64, vp]
    lib.emu_pass1_numbers.restype = None
    lib.emu_pass1_numbers.argtypes = [ctypes.c_int, vp]
    lib.emu_band_layout.restype = u32
    lib.emu_band_layout.argtypes = [ctypes.c_char_p, u32, u32, vp, vp, vp]
    return lib


def numbers(lib, level):
    out = (ctypes.c_uint32 * 6)()
    lib.emu_pass1_numbers(level, out)
    return dict(zip(("max_chain", "snap_chain", "none_pure", "none_impure", "too_far", "max_dist"), out))


def sweep(lib, level, none, fill, seed):
    first = (ctypes.c_uint32 * 9)()
    bad = lib.emu_pass1_sweep(level, none, fill, seed, first)
    return bad, list(first)


class Layout:
    """The tiles as the kernel sees them: per position its sorted index, its candidates (level 6: the cap is 128), its tile's format."""
    def __init__(self, lib, data, tile=TILE):
        n = len(data)
        self.sidx, self.cnt, self.pure = np.zeros(n + 1, dtype=np.uint32), np.zeros(n + 1, dtype=np.uint16), np.zeros(n + 1, dtype=np.uint8)
        self.tiles = lib.emu_band_layout(data, n, tile, self.sidx.ctypes.data, self.cnt.ctypes.data, self.pure.ctypes.data)
        self.tile = tile

    def run_of(self, p):
        """(tile, run of eight inside it) of position p: entries of one run sit in one wave whatever the order phase does."""
        u = int(self.sidx[p])
        return u // self.tile, (u % self.tile) // 8


def _occurs(data, tri):
    return bytes(tri) in data


def _free_hashes(seed, size, start, step=37):
    """Hashes whose letter trigram the plan's random letters do not hold, from `start` on."""
    pl = bp.Plan(seed, size)
    back = pl.bytes()
    h = start
    while True:
        h = (h + step) & 0x7fff
        if not _occurs(back, bp.trigram_of(h)):
            yield h


def _ladder(seed, h, copies, size, mix=False):
    pl = bp.Plan(seed, size)
    base = pl.base(h)
    if mix:
        bp._mix(pl)
    pos = [pl.put(base, 4 + (i * 5) % 6, gap=14 + (i * 7) % 9) for i in range(copies)]       # common lengths 4 .. 9: the first pass's own
    return pl.bytes(), np.array(pos)


def count_ladder(lib, seed=11, mix=False):
    """One bucket whose entries have 0, 1, 2, ... 128, 128, ... candidates: every trip's end falls inside some wave, beside lanes at the
    cap.  mix: the bucket lies in a tile of mixed buckets (two trigrams of one bucket near the chunk's end)."""
    for h in _free_hashes(seed, 9000, 0x7a00 if mix else 0x1000, step=-61 if mix else 37):
        data, pos = _ladder(seed, h, 150, 9000, mix)
        lay = Layout(lib, data)
        c = lay.cnt[pos]
        if not np.array_equal(c, np.minimum(np.arange(len(pos)), BAND)):
            continue                                                                         # (the base string's own letters repeat the trigram)
        if lay.pure[pos].any() if mix else not lay.pure[pos].all():
            continue                                                                         # (the bucket is not in the tile it was meant for)
        assert set(TRIPS) | {1, 2, 127, 128} <= set(c.tolist()) and int((c == BAND).sum()) >= 20
        return data, pos


def one_beside_full(lib, seed=12):
    """A run of eight entries that holds lanes at the cap and a lane with ONE candidate: the end of a bucket of 140 and, right behind it in
    the order, the next hash's bucket of three."""
    for h in _free_hashes(seed, 7000, 0x2000):
        t2 = bp.trigram_of(h + 1)
        pl = bp.Plan(seed, 7000)
        if _occurs(pl.bytes(), t2):
            continue
        base, base2 = pl.base(h), pl.base(h + 1, salt=9)
        pos = [pl.put(base, 5 + i % 4, gap=12 + i % 5) for i in range(140)]
        pos2 = [pl.put(base2, 6, gap=40) for _ in range(3)]
        data = pl.bytes()
        lay = Layout(lib, data)
        if lay.cnt[pos[-1]] != BAND or list(lay.cnt[pos2]) != [0, 1, 2]:
            continue
        if lay.run_of(pos[-1]) != lay.run_of(pos2[1]):
            continue                                                                         # the run's end fell between them: another hash
        run = [p for p in pos + pos2 if lay.run_of(p) == lay.run_of(pos2[1])]
        assert {int(lay.cnt[p]) for p in run} >= {1, BAND}
        return data, np.array(pos + pos2)


def fourth_byte(lib, seed=13, mix=False):
    """Entries whose only candidate shares the trigram and nothing more: records of length 3 -- kept at distance 1 000, dropped at 5 000
    (beyond kTooFar).  Returns (data, near target, far target)."""
    gen = _free_hashes(seed, 9000, 0x7a00 if mix else 0x3000, step=-53 if mix else 41)
    for h in gen:
        h2 = next(gen)
        pl = bp.Plan(seed, 9000)
        if mix:
            bp._mix(pl)
        a, b = pl.base(h), pl.base(h2, salt=3)
        buf = pl.buf
        spots = {"a0": 200, "a1": 1200, "b0": 1500, "b1": 6500}
        for name, at in spots.items():
            base = a if name[0] == "a" else b
            buf[at:at + 3] = base[:3]
            buf[at + 3] = base[3] if name[1] == "0" else bp._other(base[3])
        data = pl.bytes()
        lay = Layout(lib, data)
        if [int(lay.cnt[spots[k]]) for k in ("a0", "a1", "b0", "b1")] != [0, 1, 0, 1]:
            continue
        if any(bool(lay.pure[spots[k]]) == mix for k in ("a1", "b1")):
            continue
        assert bp.common(data, spots["a0"], spots["a1"]) == 3 and bp.common(data, spots["b0"], spots["b1"]) == 3
        assert spots["a1"] - spots["a0"] <= TOO_FAR < spots["b1"] - spots["b0"]
        return data, spots["a1"], spots["b1"]


def best_at_place(lib, place, short, long_, seed=14, total=40):
    """A position of `total` candidates that all share `short` bytes with it but the one at `place` (1 = the nearest), which shares
    `long_`: the best candidate at, just in front of and just behind the place where a level's short chain ends (8, 16 or 32 candidates)
    and a trip ends.  Returns (data, target, positions of the candidates nearest first)."""
    for h in _free_hashes(seed + place, 6200, 0x3800 + 97 * place):
        pl = bp.Plan(seed + place, 6200)
        base = pl.base(h)
        lens = [long_ if k == place else short for k in range(total, 0, -1)]                  # planted farthest first
        pos = [pl.put(base, n, gap=6 + (i * 3) % 5) for i, n in enumerate(lens)]
        target = pl.put(base, 14, gap=100)
        data = pl.bytes()
        lay = Layout(lib, data)
        if int(lay.cnt[target]) != total or not lay.pure[target]:
            continue
        near = pos[::-1]
        assert [bp.common(data, q, target) for q in near] == [long_ if k == place else short for k in range(1, total + 1)]
        assert [int(lay.sidx[target]) - int(lay.sidx[q]) for q in near] == list(range(1, total + 1)), "the k-th nearest is the k-th in front in the order"
        return data, target, near


def tail(lib, seed=15, mix=False):
    """The chunk ends in the first 13 bytes of a context seen five times before: positions with 3 .. 10 bytes of lookahead that have
    candidates -- their comparison words reach past the data (the plain loop, masked to the bytes that exist)."""
    for h in _free_hashes(seed, 7000, 0x7a00 if mix else 0x4000, step=-59 if mix else 43):
        pl = bp.Plan(seed, 7000)
        if mix:
            bp._mix(pl)
        base = pl.base(h)
        for _ in range(5):
            pl.put(base, 40, gap=50)
        data = bytearray(pl.bytes())
        data[len(data) - 13:] = base[:13].tobytes()
        data = bytes(data)
        lay = Layout(lib, data)
        last = [len(data) - la for la in range(3, 11)]
        if not all(lay.cnt[p] >= 1 for p in last) or lay.cnt[len(data) - 13] < 5:
            continue
        if bool(lay.pure[len(data) - 13]) == mix:
            continue
        return data


def straddle(lib, seed=16):
    """A bucket of 100 entries across the first tile's end: the entries behind the seam find their candidates in the halo."""
    def make(h):
        pl = bp.Plan(seed, 9000)
        base = pl.base(h)
        pos = [pl.put(base, 4 + (i * 3) % 7, gap=20 + i % 7) for i in range(100)]
        return pl.bytes(), np.array(pos)
    data, pos = bp._straddling(make, want=TILE, lo=25, hi=25)
    lay = Layout(lib, data)
    front = int((lay.sidx[pos] < TILE).sum())
    assert 25 <= front <= 75 and len(pos) < BAND
    bucket = np.sort(lay.sidx[pos])
    assert int(bucket[-1]) - int(bucket[0]) < BAND, "fewer than 128 entries from the bucket's first to its last"
    behind = [p for p in pos if lay.sidx[p] >= TILE]
    assert all(lay.cnt[p] >= front for p in behind), "every entry behind the seam has the ones in front of it as candidates"
    return data, pos


def checked_chunks(lib):
    """Every constructed chunk, by name, each after the emulator has said that its corner is there."""
    out = {}
    walks = bp.load()                                               # lz_search's records (level 6): what the corner must come out as

    def take(name, data):
        assert 6100 <= len(data) <= 65535, (name, len(data))
        out[name] = data
        return bp.search_records(walks, data)

    take("count_ladder", count_ladder(lib)[0])
    take("count_ladder_mixed", count_ladder(lib, mix=True)[0])
    take("one_beside_full", one_beside_full(lib)[0])
    for mix in (False, True):
        data, near, far = fourth_byte(lib, mix=mix)
        e128, _ = take("fourth_byte_mixed" if mix else "fourth_byte", data)
        assert (bp._len(e128[near]), bp._dist(e128[near])) == (3, 1000) and e128[far] == 0
    for place in TRIPS:
        for short, long_, seed in ((5, 9, 14), (3, 4, 40)):
            data, target, near = best_at_place(lib, place, short, long_, seed=seed)
            e128, e32 = take("best_at_%d_of_lengths_%d_%d" % (place, short, long_), data)
            assert (bp._len(e128[target]), bp._dist(e128[target])) == (long_, target - near[place - 1])
            if place <= 32:                                         # level 6's short chain sees it
                assert e32[target] == e128[target]
            else:
                assert (bp._len(e32[target]), bp._dist(e32[target])) == (short, target - near[0])
    take("tail", tail(lib))
    take("tail_mixed", tail(lib, mix=True))
    take("straddle", straddle(lib)[0])
    return out
