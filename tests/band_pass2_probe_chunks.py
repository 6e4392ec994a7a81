"""Chunks built for the probe of lz_match_band's second pass (csrc/zwz_band.hip; csrc/lz_band.h: band_deep_probed), and the host build
of that pass at a compression level (tests/emu_band/band_pass2_probe_emu.cpp).  Shared by tests/test_band_pass2_probe_cpu.py and
tests/test_gpu_band_pass2_probe.py; the building blocks are tests/band_pass2_chunks.py's (random letters, copies of a base string of
which the last, 300 bytes long, is the "target", the copies in front of it its sharers, the nearest first)."""
import ctypes
import os
import subprocess

import numpy as np

import band_pass2_chunks as bp

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = bp.CSRC
LEVELS = (4, 5, 6)
SNAP_CHAIN = {4: 16, 5: 8, 6: 32}           # zwz_common.h: LzLevel<N>::snap_chain
MAX_CHAIN = {4: 16, 5: 32, 6: 128}
NICE = {4: 16, 5: 32, 6: 128}
RUN_MAX = 16                                # the greatest bounded ZWZ_BAND_P2_RUN that was swept
FLAGGED, HALO, SLOW, PURE, NICE_STOP = bp.FLAGGED, bp.HALO, bp.SLOW, bp.PURE, bp.NICE


def load():
    so = os.path.join(HERE, "emu_band", "libband_pass2_probe_emu.so")
    src = os.path.join(HERE, "emu_band", "band_pass2_probe_emu.cpp")
    deps = [src] + [os.path.join(CSRC, h) for h in ("lz_band.h", "lz_core.h", "zwz_common.h")]
    if not os.path.exists(so) or max(os.path.getmtime(d) for d in deps) > os.path.getmtime(so):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, src])
    lib = ctypes.CDLL(so)
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    lib.emu_probe_search_records.restype = ctypes.c_int
    lib.emu_probe_search_records.argtypes = [ctypes.c_char_p, u32, ctypes.c_int, vp, vp]
    lib.emu_band_pass2_probe.restype = u32
    lib.emu_band_pass2_probe.argtypes = [ctypes.c_char_p, u32, u32, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, vp, vp, vp, vp, vp, vp, vp]
    return lib


def search_records(lib, data, level=6):
    n = len(data)
    a, b = np.zeros(n + 1, dtype=np.uint32), np.zeros(n + 1, dtype=np.uint32)
    assert lib.emu_probe_search_records(data, n, level, a.ctypes.data, b.ctypes.data) == 0
    return a[:n], b[:n]


class Walks:
    """What the emulator says about a chunk at a level: records (mode 0: band_deep's, 1: band_deep_probed's), and per position the second pass's chain,
    the sharers band_deep_probed looked at and compared, and the sharers the plain walk looks at."""
    def __init__(self, lib, data, tile=bp.TILE, fmt=-1, level=6, mode=1):
        n = len(data)
        self.e128, self.e32 = np.zeros(n + 1, dtype=np.uint32), np.zeros(n + 1, dtype=np.uint32)
        self.chain, self.visited, self.visited_ref, self.compared, self.k1 = (np.zeros(n + 1, dtype=np.uint16) for _ in range(5))
        self.flags = np.zeros(n + 1, dtype=np.uint8)
        self.pure_tiles = lib.emu_band_pass2_probe(data, n, tile, fmt, level, mode, self.e128.ctypes.data, self.e32.ctypes.data, self.chain.ctypes.data,
                                                   self.visited.ctypes.data, self.visited_ref.ctypes.data, self.compared.ctypes.data, self.k1.ctypes.data,
                                                   self.flags.ctypes.data)
        assert self.pure_tiles != 0xffffffff, "level %d does not exist" % level
        self.e128, self.e32 = self.e128[:n], self.e32[:n]


# ------------------------------------------------------------------------------------------------ building
def _put_all(pl, base, lens, gap=25):
    """Copies of the given common lengths, lens[0] the nearest to the target that follows them.  Returns (positions nearest first, target)."""
    pos = [pl.put(base, n, gap=gap) for n in reversed(lens)]
    target = pl.put(base, 300, gap=200)
    return np.array(pos[::-1]), target


def false_hit(seed=21):
    """(a) nearest first: 20 bytes; then a copy that differs from the target at offset 14 and agrees again from 15 to 29 -- the probe at offset 20
    hits, the compare says 14; then 40 bytes."""
    pl = bp.Plan(seed, 7000)
    base = pl.base(0x2468)
    far = pl.put(base, 40, gap=25)
    mid = pl.put(base, 30, gap=25)
    pl.buf[mid + 14] = bp._other(base[14])
    near = pl.put(base, 20, gap=25)
    target = pl.put(base, 300, gap=200)
    return pl.bytes(), np.array([near, mid, far]), target


def equal_length(seed=22):
    """(b) two sharers of 20 bytes, then one of 12: the probe misses at both later ones, the nearest of the greatest length is kept."""
    pl = bp.Plan(seed, 7000)
    base = pl.base(0x2469)
    pos, target = _put_all(pl, base, [20, 20, 12])
    return pl.bytes(), pos, target


def snapshot_edge(level, past, seed=23):
    """(c) sharers of 12 bytes and one of 40 bytes as candidate snap_chain (past = 0) or snap_chain + 1 (past = 1) of `level`."""
    k = SNAP_CHAIN[level] + past
    pl = bp.Plan(seed + 2 * level + past, 7000)
    base = pl.base(0x2470 + 2 * level + past)
    pos, target = _put_all(pl, base, [12] * (k - 1) + [40, 12, 12])
    return pl.bytes(), pos, target, k


def chunk_end(seed=24):
    """(d) the chunk ends 60 bytes into the target; nearest first: 12 bytes, 80 bytes (the whole lookahead: the walk ends), 100 bytes."""
    pl = bp.Plan(seed, 7000)
    base = pl.base(0x2480)
    pos = [pl.put(base, n, gap=25) for n in (100, 80, 12)][::-1]
    data = bytearray(pl.bytes())
    data[len(data) - 60:] = base[:60].tobytes()
    return bytes(data), np.array(pos), len(data) - 60


def serial_tail(seed=25, deep=11):
    """(e) nearest first: deep + 16 + 13 bytes, then 90: the second compare finds all sixteen bytes equal and goes on byte by byte."""
    pl = bp.Plan(seed, 7000)
    base = pl.base(0x2490)
    pos, target = _put_all(pl, base, [deep + 29, 90])
    return pl.bytes(), pos, target


def long_rejection(seed=26, rejected=2 * RUN_MAX + 8):
    """(f) nearest first: 30 bytes, `rejected` sharers of 12 bytes that differ from the target at offset 30, then 50 bytes; the bucket lies across
    the first tile's end, the target behind it.  Beside it thirty pairs of other strings: their second copies have one sharer each."""
    def make(h):
        pl = bp.Plan(seed, 11800)
        base = pl.base(h)
        for i in range(30):
            other = pl.base((h + 0x1111 + 37 * i) & 0x7fff, salt=1 + i)
            pl.put(other, 40, gap=20)
            pl.put(other, 40, gap=20)
        pos = [pl.put(base, 50, gap=25)]
        for _ in range(rejected):
            q = pl.put(base, 12, gap=25)
            if pl.buf[q + 30] == base[30]:
                pl.buf[q + 30] = bp._other(base[30])
            pos.append(q)
        pos.append(pl.put(base, 30, gap=25))
        pos.append(pl.put(base, 300, gap=200))
        return pl.bytes(), np.array(pos)
    data, pos = bp._straddling(make, lo=12, hi=12)
    return data, pos[:-1][::-1], int(pos[-1])


def nice_then_longer(seed=27):
    """(g) nearest first: 12 bytes, 130 (nice at every level), then 200 and 300 bytes."""
    pl = bp.Plan(seed, 7000)
    base = pl.base(0x24a0)
    pos, target = _put_all(pl, base, [12, 130, 200, 300])
    return pl.bytes(), pos, target


def _len(e):
    return int(e) & 0xffff


def _dist(e):
    return int(e) >> 16


def checked_chunks(lib):
    """Every constructed chunk, by name -- each after the emulator has said that the feature it was built for is there."""
    out = {}

    def take(name, data, level=6):
        assert len(data) <= 65535, (name, len(data))
        out[name] = data
        return Walks(lib, data, level=level)

    data, pos, t = false_hit()                                      # (a)
    w = take("false_hit", data)
    assert [bp.common(data, q, t) for q in pos] == [20, 14, 40] and data[pos[1] + 20] == data[t + 20]
    assert w.visited[t] == 3 and w.compared[t] == 3 and _len(w.e128[t]) == 40 and _dist(w.e128[t]) == t - pos[2]
    out["false_hit_cut"] = data[:t + 100]                           # once more, the chunk's end 100 bytes into the target: lookahead < nice at level 6

    data, pos, t = equal_length()                                   # (b)
    w = take("equal_length", data)
    assert [bp.common(data, q, t) for q in pos] == [20, 20, 12]
    assert w.visited[t] == 3 and w.compared[t] == 1 and _len(w.e128[t]) == 20 and _dist(w.e128[t]) == t - pos[0]

    for level in LEVELS:                                            # (c)
        for past in (0, 1):
            data, pos, t, k = snapshot_edge(level, past)
            w = take("snapshot_edge_l%d_%d" % (level, k), data, level)
            assert w.k1[t] == 1 and bp.common(data, pos[k - 1], t) == 40
            if k <= MAX_CHAIN[level]:
                assert _len(w.e128[t]) == 40 and _dist(w.e128[t]) == t - pos[k - 1] and w.compared[t] >= 2
                assert _len(w.e32[t]) == (12 if past else 40), "the short chain's record holds the best from before candidate snap_chain + 1"
            else:                                                   # level 4: the chain ends at snap_chain candidates
                assert _len(w.e128[t]) == 12 and w.e32[t] == w.e128[t] and w.visited[t] == MAX_CHAIN[level]
            if past:
                assert _dist(w.e32[t]) == t - pos[0]

    data, pos, t = chunk_end()                                      # (d)
    for level in LEVELS:
        w = take("chunk_end", data, level)
        assert w.flags[t] & FLAGGED and w.chain[t] == 3 and w.visited[t] == 2 and w.flags[t] & NICE_STOP
        assert _len(w.e128[t]) == min(60, 258) == len(data) - t and _dist(w.e128[t]) == t - pos[1]

    data, pos, t = serial_tail()                                    # (e)
    w = take("serial_tail", data)
    assert w.flags[t] & PURE and [bp.common(data, q, t) for q in pos] == [40, 90] and 40 >= 11 + 16
    assert w.compared[t] == 2 and _len(w.e128[t]) == 90
    out["serial_tail_cut"] = data[:t + 100]

    data, pos, t = long_rejection()                                 # (f)
    w = take("long_rejection", data)
    assert len(pos) > 2 * RUN_MAX + 2 and all(data[q + 30] != data[t + 30] for q in pos[1:-1])
    assert w.visited[t] == len(pos) and w.compared[t] == 2 and _len(w.e128[t]) == 50 and _dist(w.e128[t]) == t - pos[-1]
    assert w.flags[t] & HALO and not w.flags[t] & SLOW, "the chain crosses a halo of the same word format"
    assert int(((w.flags & FLAGGED) != 0)[w.chain == 1].sum()) >= 30, "lanes with one sharer beside the long walk"

    data, pos, t = nice_then_longer()                               # (g)
    for level in LEVELS:
        w = take("nice_then_longer", data, level)
        assert w.chain[t] == 4 and w.visited[t] == 2 and w.compared[t] == 2 and w.flags[t] & NICE_STOP
        assert _len(w.e128[t]) == 130 and _dist(w.e128[t]) == t - pos[1]
    out["nice_then_longer_cut"] = data[:t + 100]
    return out
