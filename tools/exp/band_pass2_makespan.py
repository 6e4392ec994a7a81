#!/usr/bin/env python3
"""Offline study of lz_match_band's second pass (csrc/zwz_band.hip), per TILE: band_pass2_skew.py looked at a chunk's flagged entries as one
list; the kernel takes them a tile of 6 016 sorted entries at a time, sixteen waves taking groups of 64 off a counter, and a tile's pass
lasts until its last group is done.  The walks come from the host build of the pass (tests/emu_band: sharers a walk looks at, tile by
tile as the kernel sees them).  Counted in HOPS (a hop = one sharer visited by a wave's slowest lane):

  wave-trips   sum over the groups of their longest walk: what the sixteen waves do between them
  work / 64    sharers visited / 64: the same with every lane busy
  longest      the tile's longest walk, summed over the tiles: what the pass lasts with waves to spare (7 - 28 groups for 16 waves)
  makespan     groups handed to 16 waves in order, a tile's time = its busiest wave's

What it prints for three text chunks of bench.py's workload, 11 tiles each (the walks do not depend on how the kernel takes them):

  text chunk | flagged | sharers visited | wave-trips | work / 64 | makespan (the longest walk per tile, summed: 237 / 416 / 187)
  seed +0    |   8 222 |          34 891 |      1 649 |       545 | 237 hops
  seed +1    |  13 245 |          89 546 |      3 725 |     1 399 | 446 hops
  seed +2    |   6 815 |          23 154 |      1 163 |       361 | 192 hops

A tile has 5 - 28 groups for 16 waves, so its pass lasts as long as its longest walk (18 - 40 hops), eleven times a chunk: 188 k cycles over
~240 hops is ~790 cycles a hop.  `batched H` counts a tile's longest walk in batches of H on the assumption that the hop's price is its
dependent chain (a hop of chase at CHASE of a full hop, the batch's compares as one more): 115 / 86 / 88 for H = 4 / 8 / 16 against 237.
The GPU said otherwise: with sixteen waves on a CU the hop's price is its instruction count, four waves
sharing a SIMD's issue slots, and the batched walk gained 11 %, not 50 %.

Ruled out here, before anything was built: the STRIDED walk -- a flagged entry's walk shared by s = 2, 4, 8 lanes, lane r taking the sharers
r, r + s, ... .  The links lead to the NEXT sharer only, so lane r first hops r times to its start and every later sharer costs it s hops
of chase (nothing compared on the way); an entry takes s lanes, so a tile has s times the groups.  Under the same assumption: 220 / 220 /
331 hops for seed +0 against 237 (the issue that asked for this study had 176 / 219 / 453 from a variant of the model that charged the
pre-hops differently): the pre-hops and the extra groups eat what the shorter compare chain gives, and it issues MORE instructions.
Run: python tools/exp/band_pass2_makespan.py [chunks]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "tests"))
import band_pass2_chunks as bp
import corpus
import workloads

TILE, WAVES = bp.TILE, 16
CHASE = 0.2          # a hop that only follows the link, against one that also compares (8 instructions against 45: the issue's estimate)


def makespan(durations, waves=WAVES):
    """Groups handed out in order to whichever wave is free first."""
    free = [0.0] * waves
    for d in durations:
        i = free.index(min(free))
        free[i] += d
    return max(free)


def groups(walks, lanes_per_entry=1):
    per = 64 // lanes_per_entry
    return [walks[i:i + per] for i in range(0, len(walks), per)]


def study(lib, data):
    w = bp.Walks(lib, data)
    idx = bp.sorted_index(data)
    flagged = np.nonzero(w.flags[:len(idx)] & bp.FLAGGED)[0]
    flagged = flagged[np.argsort(idx[flagged])]                       # array order: the order the kernel compacts them in
    tiles = idx[flagged] // TILE
    out = {"flagged": len(flagged), "visited": int(w.visited[flagged].sum()), "tiles": int(tiles.max()) + 1 if len(flagged) else 0,
           "wave_trips": 0, "longest": 0, "makespan": 0.0, "groups_per_tile": []}
    for h in (4, 8, 16):
        out["batched_%d" % h] = 0.0
    for s in (2, 4, 8):
        out["strided_%d" % s] = 0.0
    for t in range(out["tiles"]):
        v = w.visited[flagged[tiles == t]].astype(np.int64)
        if not len(v):
            continue
        g = groups(v)
        out["groups_per_tile"].append(len(g))
        out["wave_trips"] += sum(int(x.max()) for x in g)
        out["longest"] += int(v.max())
        out["makespan"] += makespan([int(x.max()) for x in g])
        for h in (4, 8, 16):          # a batch: H hops of chase on the chain, the compares beside one another (counted as one hop's worth a batch)
            out["batched_%d" % h] += makespan([-(-int(x.max()) // h) * (h * CHASE + 1.0) for x in g])
        for s in (2, 4, 8):           # lane r: r pre-hops, then every s-th sharer at s hops of chase + one compare each
            dur = []
            for x in groups(v, s):
                longest = int(x.max())
                dur.append(max(r * CHASE + -(-(longest - r) // s) * (s * CHASE + 1.0) for r in range(min(s, longest))))
            out["strided_%d" % s] += makespan(dur)
    out["work_per_64"] = out["visited"] // 64
    return out


if __name__ == "__main__":
    lib = bp.load()
    for i in range(int(sys.argv[1]) if len(sys.argv) > 1 else 3):
        data = corpus.text_like(workloads.TEXT_SEED0 + i, 262144)[:65535]
        r = study(lib, data)
        g = r.pop("groups_per_tile")
        print("text chunk seed +%d" % i, {k: (round(v, 1) if isinstance(v, float) else v) for k, v in r.items()}, "groups a tile %d - %d" % (min(g), max(g)))
