#!/usr/bin/env python3
"""Offline replay of lz_match_band's second pass behind its probe (csrc/zwz_band.hip; csrc/lz_band.h: band_deep_probed) on bench.py's text
workload: what the probe at the best length rejects, and what the kernel's two alternating steps -- a compare for the lanes that stand on a
candidate, a run-ahead of up to R hops through rejected sharers -- then cost a wave, with the kernel's own tiles (6 016 sorted entries) and
its flagged entries in array order, 64 a wave.

Per flagged entry the sharers are the candidates that agree on the entry's eight bytes (what the links chain together), nearest first; the
walk is band_deep_probed's: the first sharer compared, a later one only if its byte at offset `best` is the entry's, the nice stop.  `best`
evolves the same whatever sound probe is used, so the one-byte and the two-byte probe (offsets best - 1 and best) are counted on one walk.
The host build of the pass (tests/emu_band/band_pass2_probe_emu.cpp) says which entries are flagged and which word format their tile has,
and its visited / compared counts are checked against the replay's.

Per wave:  compare rounds (the wave meets once per round: as many as its busiest lane compares, plus the rounds that a run-ahead bound
cuts short), run-ahead hops (a round's hops last for its longest lane, at most R), the longest run-ahead; and a price in vector
instructions -- 60 a compare round, 14 a hop (estimates from before the kernel was written; the built hop is 11 vector, 2 LDS and 6 scalar
instructions, and the GPU's answer is in DESIGN.md section 4 round 8) against the
batched walk's 56 a sharer in batches of four that last for the wave's longest lane.

Run: python tools/exp/band_pass2_probe.py [chunks]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "tests"))
import band_pass2_chunks as bp
import band_pass2_probe_chunks as pp
import corpus
import workloads

TILE, BAND, MAX_DIST, NICE, MAX_MATCH = bp.TILE, bp.BAND, 32506, 128, 258
COMPARE, HOP, BATCHED = 60, 14, 56
RUNS = (4, 6, 8, 16, 0)          # ZWZ_BAND_P2_RUN as swept, 0 = unbounded


def common(d, q, p, cap):
    x = np.nonzero(d[q:q + cap] != d[p:p + cap])[0]
    return int(x[0]) if len(x) else cap


def walks(lib, data):
    """Per flagged entry, in array order: (tile, outcomes) -- outcomes a string over the sharers looked at, 'C' compared, 'c' compared with the
    one-byte probe only (the two-byte probe rejects it), 'r' rejected."""
    w = pp.Walks(lib, data)
    d = np.frombuffer(data, dtype=np.uint8)
    L = len(data)
    idx = bp.sorted_index(data)
    h = ((d[:-2].astype(np.int64) << 10) ^ (d[1:-1].astype(np.int64) << 5) ^ d[2:]) & 0x7fff
    order = np.argsort(idx)                                           # position of sorted index u
    flagged = np.nonzero(w.flags[:len(idx)] & bp.FLAGGED)[0]
    flagged = flagged[np.argsort(idx[flagged])]
    out, bad = [], 0
    for p in flagged.tolist():
        u, off = int(idx[p]), 3 if w.flags[p] & bp.PURE else 0
        own = data[p + off:p + off + 8]
        sharers = []
        for k in range(1, BAND + 1):
            if u - k < 0:
                break
            c = int(order[u - k])
            if h[c] != h[p] or c == 0 or p - c >= MAX_DIST:
                break
            if k >= w.k1[p] and data[c + off:c + off + 8] == own:
                sharers.append(c)
        max_len = min(MAX_MATCH, L - p)
        nice = min(NICE, L - p)
        best, res = 0, []
        for n, c in enumerate(sharers):
            one = n == 0 or d[c + best] == d[p + best]
            two = n == 0 or (one and d[c + best - 1] == d[p + best - 1])
            res.append("C" if two else "c" if one else "r")
            if one:
                ln = common(d, c, p, max_len)
                if ln > best:
                    best = ln
                    if best >= nice:
                        break
        s = "".join(res)
        bad += len(s) != w.visited[p] or sum(x != "r" for x in s) != w.compared[p]
        out.append((u // TILE, s))
    return out, bad


def wave_cost(lanes, run):
    """lanes: outcome strings of a wave's entries.  Returns (compare rounds, hops, longest run-ahead) of the two alternating steps."""
    at = [0] * len(lanes)                                             # the sharer a lane stands on; every lane starts on a candidate
    rounds = hops = longest = 0
    cand = [True] * len(lanes)
    while True:
        if any(cand):
            rounds += 1
            for i, s in enumerate(lanes):
                if cand[i]:
                    at[i] += 1
                    cand[i] = False
        hopping = [not cand[i] and at[i] < len(s) for i, s in enumerate(lanes)]   # lanes with sharers left that stand on no candidate yet
        r = 0
        while any(hopping) and (run == 0 or r < run):
            r += 1
            for i, s in enumerate(lanes):
                if hopping[i]:
                    if s[at[i]] != "r":
                        cand[i], hopping[i] = True, False
                    else:
                        at[i] += 1
                        hopping[i] = at[i] < len(s)
        hops += r
        longest = max(longest, r)
        if not any(cand) and not any(at[i] < len(s) for i, s in enumerate(lanes)):
            return rounds, hops, longest


if __name__ == "__main__":
    lib = pp.load()
    n_chunks = int(sys.argv[1]) if len(sys.argv) > 1 else 4
    tot = {"flagged": 0, "visited": 0, "one": 0, "two": 0, "waves": 0, "batched": 0}
    per_run = {r: {"rounds": 0, "hops": 0, "longest": 0, "price": 0} for r in RUNS}
    for i in range(n_chunks):
        text = corpus.text_like(workloads.TEXT_SEED0 + i // 2, 262144)
        data = text[65535 * (i % 2):65535 * (i % 2 + 1)]              # chunks 0 and 1 of each file
        ws, bad = walks(lib, data)
        assert bad == 0, "%d walks differ from the host build's counts" % bad
        tot["flagged"] += len(ws)
        tot["visited"] += sum(len(s) for _, s in ws)
        tot["one"] += sum(sum(x != "r" for x in s) for _, s in ws)
        tot["two"] += sum(s.count("C") for _, s in ws)
        for t in sorted({t for t, _ in ws}):
            lanes_all = [s for tt, s in ws if tt == t]
            for g in range(0, len(lanes_all), 64):
                lanes = lanes_all[g:g + 64]
                tot["waves"] += 1
                tot["batched"] += -(-max(len(s) for s in lanes) // 4) * 4 * BATCHED
                for r in RUNS:
                    rounds, hops, longest = wave_cost(lanes, r)
                    pr = per_run[r]
                    pr["rounds"] += rounds; pr["hops"] += hops; pr["longest"] = max(pr["longest"], longest); pr["price"] += rounds * COMPARE + hops * HOP
    print("chunks %d  flagged %d  sharers visited %d  compared: one-byte probe %d (%.1f %%), two-byte %d (%.1f %%)  waves %d" % (
        n_chunks, tot["flagged"], tot["visited"], tot["one"], 100.0 * tot["one"] / tot["visited"], tot["two"], 100.0 * tot["two"] / tot["visited"], tot["waves"]))
    print("batched walk: %d wave-instructions (%d a wave)" % (tot["batched"], tot["batched"] // max(tot["waves"], 1)))
    for r in RUNS:
        pr = per_run[r]
        print("run-ahead %-9s compare rounds a wave %.2f  hops a wave %.2f  longest run-ahead %d  wave-instructions %d = %.2f of the batched walk's" % (
            "unbounded" if r == 0 else "<= %d" % r, pr["rounds"] / tot["waves"], pr["hops"] / tot["waves"], pr["longest"], pr["price"], pr["price"] / tot["batched"]))
