"""Chunks built for the corners of lz_match_band's tile set-up (csrc/zwz_band.hip: the scan of a tile's entries, eight a thread, the count
by band_in_reach, the compaction of the flagged entries), and the host build of what the set-up takes from lz_band.h
(tests/emu_band/band_setup_emu.cpp).  Shared by tests/test_band_setup_cpu.py and tests/test_gpu_band_setup.py.

The chunks are tests/band_pass2_chunks.py's kind where they can be: random letters '@'..'_', whose trigrams zlib's hash keeps apart.
Every builder asserts, from the host build's view of the tiles, that the corner it is named for is there."""
import ctypes
import os
import subprocess

import numpy as np

import band_pass1_chunks as b1
import band_pass2_chunks as bp
import corpus

HERE = os.path.dirname(os.path.abspath(__file__))
TILE, BAND = bp.TILE, bp.BAND
MAX_DIST, SLIDE_POS, W_SIZE = 32506, 65274, 32768


def load():
    so = os.path.join(HERE, "emu_band", "libband_setup_emu.so")
    src = os.path.join(HERE, "emu_band", "band_setup_emu.cpp")
    deps = [src] + [os.path.join(bp.CSRC, h) for h in ("lz_band.h", "lz_core.h", "zwz_common.h")]
    if not os.path.exists(so) or max(os.path.getmtime(d) for d in deps) > os.path.getmtime(so):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, src])
    lib = ctypes.CDLL(so)
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    lib.emu_setup_lo.restype = u32
    lib.emu_setup_lo.argtypes = [u32]
    lib.emu_setup_reach.restype = u32
    lib.emu_setup_reach.argtypes = [u32, u32]
    lib.emu_setup_counts.restype = u32
    lib.emu_setup_counts.argtypes = [ctypes.c_char_p, u32, u32, ctypes.c_int, vp, vp]
    lib.emu_setup_numbers.restype = None
    lib.emu_setup_numbers.argtypes = [vp]
    out = (ctypes.c_uint32 * 5)()
    lib.emu_setup_numbers(out)
    assert list(out) == [MAX_DIST, BAND, 0xffff0000, SLIDE_POS, W_SIZE]
    return lib


def counts(lib, data, level=6, tile=TILE):
    """(differences from the search over band_valid, candidates per position, sorted index per position)"""
    n = len(data)
    cnt, sidx = np.zeros(n + 1, dtype=np.uint16), np.zeros(n + 1, dtype=np.uint32)
    bad = lib.emu_setup_counts(data, n, tile, level, cnt.ctypes.data, sidx.ctypes.data)
    return bad, cnt[:n], sidx[:n]


# ------------------------------------------------------------------------------------------------ (a) ragged tile ends
def ragged_ends():
    """Eight chunk lengths whose only tile holds 0 .. 7 entries mod 8, and eight whose second tile does: the last thread's eight
    entries lie partly beyond the tile's end.  Text: candidates everywhere, the entries at the end among them."""
    out = {}
    for first in (True, False):
        res = set()
        for i in range(8):
            L = (6001 if first else 6301) + i
            own = L - 2 if first else L - 2 - TILE                  # the ragged tile's own entries
            assert 0 < own < TILE and (first or L - 2 > TILE)
            res.add(own % 8)
            out["ragged_%s_%d" % ("first" if first else "second", own % 8)] = corpus.text_like(900 + i, L)
        assert res == set(range(8))
    return out


# ------------------------------------------------------------------------------------------------ (b) one mixed pair a tile
def _mixed_pairs(data):
    """The array indices (tile, index in the tile's array) whose entry and the entry in front of it share a bucket and differ in their
    trigrams -- what makes a tile impure."""
    d = np.frombuffer(data, dtype=np.uint8).astype(np.int64)
    h = ((d[:-2] << 10) ^ (d[1:-1] << 5) ^ d[2:]) & 0x7fff
    tri = d[:-2] | d[1:-1] << 8 | d[2:] << 16
    order = np.lexsort((np.arange(len(h)), h))
    hs, ts = h[order], tri[order]
    u = np.nonzero((hs[1:] == hs[:-1]) & (ts[1:] != ts[:-1]))[0] + 1
    return [(int(x) // TILE, int(x) % TILE + BAND) for x in u]


def mixed_places():
    """Chunks with ONE pair of differing neighbours in one bucket (band_pass2_chunks._mix's two trigrams that differ in a bit the hash
    drops), in the second tile, the pair's second entry at each place e = 0 .. 7 of a thread's eight: e = 0 is the compare across the
    seam between two threads, the others are a thread's own seven.  Missed, the tile would be taken for pure and the second trigram's
    entry would get a match with the first's."""
    out = {}
    lib1 = b1.load()
    for L in range(6400, 7400):
        pl = bp.Plan(21, L)
        bp._mix(pl)
        data = pl.bytes()
        pairs = _mixed_pairs(data)
        if len(pairs) != 1 or pairs[0][0] != 1:
            continue
        e = pairs[0][1] % 8
        if e in out:
            continue
        lay = b1.Layout(lib1, data)
        in_tile = lay.sidx[:len(data) - 2] >= TILE
        assert not lay.pure[:len(data) - 2][in_tile].any() and lay.pure[:len(data) - 2][~in_tile].all()
        out[e] = data
        if len(out) == 8:
            break
    assert set(out) == set(range(8)), sorted(out)
    return {"mixed_at_%d" % e: d for e, d in sorted(out.items())}


# ------------------------------------------------------------------------------------------------ (c) the reach's ends
def _sparse_letters(seed, n):
    """Letters '@'..'O': 4 096 trigrams, one a bucket, and no byte with bit 4 set -- a trigram that ends in such a byte has a bucket
    (the hash's bit 4 is the last byte's) of its own."""
    return (0x40 | (np.frombuffer(corpus.random_bytes(seed, n), dtype=np.uint8) & 15)).astype(np.uint8)


def _plant(buf, at, last):
    buf[at:at + 8] = (0x41, 0x42, last, 0x43, 0x44, 0x45, 0x46, 0x47)


def reach_ends(lib, walks):
    """Two occurrences of a trigram nothing else shares a bucket with, at distance kMaxDist - 1 (a candidate), kMaxDist (the first
    candidate alone may sit there) and kMaxDist + 1 (none); the first occurrence at position 0 (zlib's NIL: none) and at 1; and, in
    a full chunk, the pair at distance kMaxDist in front of and at the place where zlib's window has slid (band_first_at_max_dist)."""
    out = {}

    def check(name, data, p, cnt_want, dist_want):
        bad, cnt, _ = counts(lib, data)
        e128, _ = bp.search_records(walks, data)
        assert bad == 0 and int(cnt[p]) == cnt_want, (name, bad, int(cnt[p]))
        assert (bp._dist(e128[p]) if e128[p] else 0) == dist_want, (name, int(e128[p]))
        out[name] = data

    for d, cnt_want in ((MAX_DIST - 1, 1), (MAX_DIST, 1), (MAX_DIST + 1, 0)):
        buf = _sparse_letters(31, 33200)
        _plant(buf, 300, 0x51)
        _plant(buf, 300 + d, 0x51)
        check("distance_%d" % d, buf.tobytes(), 300 + d, cnt_want, d if cnt_want else 0)
    for q, cnt_want in ((0, 0), (1, 1)):
        buf = _sparse_letters(32, 6500)
        _plant(buf, q, 0x51)
        _plant(buf, 5000, 0x51)
        check("candidate_at_%d" % q, buf.tobytes(), 5000, cnt_want, 5000 - q if cnt_want else 0)
    for q, cnt_want in ((W_SIZE - 1, 1), (W_SIZE, 0)):                       # p = 65 273: in reach; p = 65 274 = kSlidePos, q = 32 768: slid
        buf = _sparse_letters(33, 65535)
        _plant(buf, q, 0x51)
        _plant(buf, q + MAX_DIST, 0x51)
        check("slid_window" if not cnt_want else "last_before_the_slide", buf.tobytes(), q + MAX_DIST, cnt_want, MAX_DIST if cnt_want else 0)
    # own positions at and around kMaxDist and at the chunk's end have entries in this chunk too: every count is the old search's (bad == 0)
    return out


# ------------------------------------------------------------------------------------------------ (d) flagged entries a tile
def flagged_counts(walks):
    """One-tile chunks with 0, 1, 63, 64, 65 and more than 1 024 flagged entries (positions whose best candidate shares all eight
    comparison bytes: the second pass's work list, which the compaction writes): an empty list, a wave's ballot with one bit, a
    list that ends one short of, at and one behind a wave of 64, and threads that hold several flagged entries."""
    out = {}
    for want in (0, 1, 63, 64, 65, 1100):
        for n in range(want + 10 if want else 0, want + 40):
            buf = bp._letters(41, 6010)
            if n:
                buf[3000:3000 + n] = buf[200:200 + n]
                buf[3000 + n] = bp._other(buf[200 + n])
            data = buf.tobytes()
            w = bp.Walks(walks, data)
            got = int(((w.flags[:len(data)] & bp.FLAGGED) != 0).sum())
            if got == want or (want > 1024 and got > 1024):
                out["flagged_%d" % want] = data
                break
        else:
            raise AssertionError("no copy length gives %d flagged entries" % want)
    return out


def checked_chunks(lib):
    """Every constructed chunk, by name, each after the host build has said that its corner is there."""
    walks = bp.load()
    out = {}
    out.update(ragged_ends())
    out.update(mixed_places())
    out.update(reach_ends(lib, walks))
    out.update(flagged_counts(walks))
    assert len(out) <= 48 and all(len(d) <= 65535 for d in out.values())
    return out
