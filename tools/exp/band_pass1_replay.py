#!/usr/bin/env python3
"""Offline replay of lz_match_band's group formation on the bench corpus: what the first pass's loop spends on
lanes that have nothing left to compare.  Counts exactly as band_count (same bucket, nearer than MAX_DIST, not position 0, the first
candidate alone at MAX_DIST, capped at 128), tiles of 6 016 entries, runs of R consecutive entries sorted by their greatest count
(longest first, runs without candidates dropped), 64 / R runs a wave, trips of eight candidates: unmasked up to the smallest count among
the wave's lanes that have candidates, masked from there to the greatest.  Prints, per chunk and run length: trips, masked trips,
lanes busy (candidates compared that a lane has / 64 x 8 x trips) and the pass's vector instructions at `--unmasked` and `--masked`
instructions a candidate (8.5 and 10.5: the 32-bit keys with compare + select + max; 6.9 and 8.25: the packed keys with a mask a
trip, as disassembled).   Run: python tools/exp/band_pass1_replay.py [--unmasked 6.9 --masked 8.25]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "tests"))
import numpy as np

import corpus
import workloads

TILE, BAND, MAX_DIST, WSIZE, SLIDE = 6016, 128, 32506, 32768, 65274


def counts_of(data):
    """(sorted positions, candidates per sorted entry) -- csrc/lz_band.h band_valid / band_first_at_max_dist / band_count at level 6."""
    d = np.frombuffer(data, dtype=np.uint8).astype(np.int64)
    n = len(d) - 2
    h = ((d[:-2] << 10) ^ (d[1:-1] << 5) ^ d[2:]) & 0x7fff
    order = np.lexsort((np.arange(n), h))
    pos, hs = order, h[order]
    cnt = np.zeros(n, dtype=np.int64)
    start = 0
    for u in range(n):
        if u and hs[u] != hs[u - 1]:
            start = u
        c = 0
        for v in range(u - 1, max(start, u - BAND) - 1, -1):
            if pos[u] - pos[v] >= MAX_DIST or pos[v] == 0:
                break
            c += 1
        if c == 0 and u > start and pos[u - 1] != 0 and pos[u] - pos[u - 1] == MAX_DIST and not (pos[u] >= SLIDE and pos[u - 1] <= WSIZE):
            c = 1
        cnt[u] = c
    return pos, cnt


def replay(cnt, run):
    trips = masked = busy = 0
    for a in range(0, len(cnt), TILE):
        c = cnt[a:a + TILE]
        pad = (-len(c)) % run
        runs = np.concatenate([c, np.zeros(pad, dtype=np.int64)]).reshape(-1, run)
        key = runs.max(axis=1)
        live = runs[key > 0][np.argsort(-key[key > 0], kind="stable")]
        per = 64 // run
        for g in range(0, len(live), per):
            lanes = live[g:g + per].ravel()
            kmax, kmin = int(lanes.max()), int(lanes[lanes > 0].min())
            t_un = kmin // 8
            t_all = (kmax + 7) // 8
            trips += t_all
            masked += t_all - t_un
            busy += int(lanes.sum())
    return trips, masked, busy


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--unmasked", type=float, default=8.5, help="vector instructions a candidate in an unmasked trip")
    ap.add_argument("--masked", type=float, default=10.5, help="... in a masked trip")
    ap.add_argument("--seeds", type=int, default=2)
    args = ap.parse_args()
    for seed in range(args.seeds):
        data = corpus.text_like(workloads.TEXT_SEED0 + seed, 262144)[:65535]
        _, cnt = counts_of(data)
        for run in (8, 4, 2, 1):
            trips, masked, busy = replay(cnt, run)
            instr = 8 * ((trips - masked) * args.unmasked + masked * args.masked)
            print("seed %d, runs of %d: %5d trips, %5d masked (%.2f), lanes busy %.3f, %.0f k wave-instructions a chunk"
                  % (seed, run, trips, masked, masked / trips, busy / (512.0 * trips), instr / 1e3))


if __name__ == "__main__":
    main()
