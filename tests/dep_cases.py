"""Hand-built inputs for zwz_deflate_dep_streams_dev: streams whose piece `piece` puts one stated shape in front of the start-offset forms
of lz_match, lz_parse, lz_lazy and blockify and of the dependent stream kernels.  Test infrastructure only.

Coordinates: P = 32 768 is the piece length, D = 32 512 the dictionary length.  A *chunk position* counts from the start of
[dictionary | piece], so the piece starts at chunk position D; a *piece position* counts from the piece's first byte.

cases() -> [Case].  A case is a stream's input bytes, the index of the piece it is about and a claim about that piece's tokens
[(0, byte) | (length, distance)] and block records (tests/deflate_dep_emu_binding.py: piece).  The claims say what libz does with the
bytes; check(cases, emu) asserts every one on the host build of the portable cores (tests/emu_dep) at the levels the case names (at
level 6 alone where the levels' limits have nothing to choose between: Case.one_level), every chunk parsed once a level, and
that every shape listed in REQUIRED is there, on both backgrounds and at both places where that applies.  What the bytes must
compress to is never taken from a claim: it is libz's output (tests/deflate_dep_ref.py).

Backgrounds: "sparse" is random bytes (under match = auto lz_match's screening pass), "dense" is corpus.text_like (the sorted work
order under walk, the band or lz_lazy otherwise).  Patterns are random bytes behind a guard byte of their own, so that the background
supplies no competing match.  Every case is piece 1 of a stream of two pieces (of three where the next piece's bytes matter); the
cases of families a and b stand a second time as piece 3 of a stream whose first two pieces are text: the same chunk, at another
place of a slice of five pieces and with another chunk index.

Families (Case.family):
  a  the border, a piece's first symbols: runs of one value and of periods 2 and 3 across it, with 1, 2, 3, 4 and 300 bytes (one
     period) of the run in the dictionary; a 40-byte pattern at piece positions 0 and 1 whose only source is 32 505, 32 506 (hits) or
     32 507 (a literal) bytes back; a match that a walk coming in from D - 1 would have pending, and its mirror, a short match at piece
     position 0 that the lazy rule drops for a longer one at position 1 (levels 5 and 6); a source that begins in the dictionary's
     last two positions
  b  tiles, trips and the piece's end: a 50-byte match from the dictionary whose query stands at piece positions 254 .. 257 and
     16 638 .. 16 641, either side of chunk positions 32 768 and 49 152, and a 258-byte match across each; a 258-byte match that ends
     on the piece's last byte, a match found in its last three bytes, a candidate that would run on behind the piece's end (here
     the stream has a third piece of 40 bytes, which begins as the source goes on; check() asserts that it does); the slid window
     at chunk position 65 274 (a source at 32 768 is a miss, one at 32 769 a hit)
  d  short last pieces behind a dictionary: 1, 2, 3, 4, 5, 258, 259 and 260 bytes that stand in the dictionary, far back (three bytes
     further back than 4 096 are literals) and, for three bytes, near
  e  blocks counted from the piece's first byte: a filler without a repeated byte triple -- literals only -- cut to 16 382 .. 16 385
     and 32 766 .. 32 768 bytes; the filler with one 100-byte match as symbol 16 382 .. 16 385 of the piece; full pieces of one block
     that may not be stored; stored pieces
"""
import random
from dataclasses import dataclass, replace
from typing import Callable, Optional

import numpy as np

import corpus
import deflate_dep_emu_binding as emu_binding
import deflate_dep_ref as ref

P, D = ref.P, ref.D
LEAD = P - D                     # a chunk position c of piece 1 is input position c + LEAD
K_SLIDE, K_WSIZE, K_MAXDIST, K_SYMS = 65274, 32768, 32506, 16383
LEVELS = (4, 5, 6)
FILLER_LENGTHS = (16382, 16383, 16384, 16385, 32766, 32767, 32768)
PLANTED_SYMBOLS = (16382, 16383, 16384, 16385)
SHORT_LENGTHS = (1, 2, 3, 4, 5, 258, 259, 260)
BORDER_QUERIES = (254, 255, 256, 257, 16638, 16639, 16640, 16641)
PAST_END, PAST_END_TAIL = 16, 40   # "candidate runs past the end": the next piece's bytes that go on as the source does; its length
STATED_RECORDS = {16382: ((16382, D),), 16384: ((16383, D), (1, 48895)), 32768: ((16383, D), (16383, 48895), (2, 65278))}


@dataclass
class Case:
    family: str
    shape: str                     # the entry of REQUIRED it fills
    background: Optional[str]      # "sparse" | "dense" | None where there is no choice
    data: bytes                    # the stream's input
    piece: int                     # the piece the claim is about
    claim: Callable                # (tokens, records) -> None, asserting
    levels: tuple = LEVELS         # the levels at which the claim holds (the bytes equal libz's at every level)
    behind: int = 0                # so many bytes of the next piece go on as the source of this piece's last match does
    one_level: bool = False        # no position of the piece has two candidates, and none a match a lazy rule could drop: the
                                   # levels' limits choose nothing, and check() asks the claim at level 6 alone

    @property
    def name(self):
        return "%s: %s, %s, piece %d" % (self.family, self.shape, self.background or "-", self.piece)

    def chunk(self):
        return self.data[self.piece * P - D:(self.piece + 1) * P] if self.piece else self.data[:P]

    def tail(self):
        """the bytes that stand behind the chunk in the stream and that the case is about"""
        return self.data[(self.piece + 1) * P:(self.piece + 1) * P + self.behind]


# ---- claims -----------------------------------------------------------------------------------------------------------------

def first(*want):
    def claim(tok, rec):
        assert tuple(tok[:len(want)]) == want, (tok[:len(want) + 2], want)
    return claim


def last(*want):
    def claim(tok, rec):
        assert tuple(tok[-len(want):]) == want, (tok[-len(want) - 2:], want)
    return claim


def at(pos, want):
    def claim(tok, rec):
        p = i = 0
        while p < pos and i < len(tok):
            p += tok[i][0] or 1
            i += 1
        assert p == pos and i < len(tok), ("no token starts at piece position", pos)
        assert tok[i] == want, (pos, tok[i], want)
    return claim


def tokens(*want):
    def claim(tok, rec):
        assert tuple(tok) == want, (tok[:6], want[:6])
    return claim


def records(*want):
    """(n_sym, start) of every block"""
    def claim(tok, rec):
        assert tuple((r["n_sym"], r["start"]) for r in rec) == want, ([(r["n_sym"], r["start"]) for r in rec], want)
    return claim


def matches(n):
    def claim(tok, rec):
        assert sum(t[0] != 0 for t in tok) == n, [t for t in tok if t[0]][:5]
    return claim


def every(*claims):
    def claim(tok, rec):
        for c in claims:
            c(tok, rec)
    return claim


def blocks_of(lengths, last_is_match=False):
    """libz's blocks of a piece whose tokens cover `lengths` bytes each: a block is flushed when it holds 16 383 symbols and another
    symbol is certain (deflate_slow keeps a last literal back) -> ((n_sym, start chunk position), ...)"""
    s = len(lengths)
    s_in = s - 1 if s and not last_is_match else s
    nb = s_in // K_SYMS + 1
    where = np.concatenate([[0], np.cumsum(lengths)])
    return tuple((min(K_SYMS, s - b * K_SYMS) if b + 1 < nb else s - b * K_SYMS, D + int(where[b * K_SYMS])) for b in range(nb))


# ---- builders ---------------------------------------------------------------------------------------------------------------

class Canvas:
    """The input of a stream of two pieces, written to in chunk positions of piece 1"""

    def __init__(self, background, seed, rng, n=2 * P):
        self.background, self.rng = background, rng
        self.b = bytearray(corpus.text_like(seed, n) if background == "dense" else rng.randbytes(n))

    def __getitem__(self, c):
        return self.b[c + LEAD]

    def put(self, c, data):
        assert 0 <= c + LEAD and c + LEAD + len(data) <= len(self.b)
        self.b[c + LEAD:c + LEAD + len(data)] = data

    def guard(self, c, avoid=()):
        """a byte at chunk position c that no text has and that is none of `avoid`"""
        while True:
            g = self.rng.randrange(0x80, 0x100)
            if g not in avoid:
                self.put(c, bytes([g]))
                return g

    def plant(self, c, pat, avoid=()):
        """pat at chunk position c behind a guard byte -> the guard"""
        self.put(c, pat)
        return self.guard(c - 1, avoid)

    def differ(self, c, other):
        """the byte at chunk position c made unequal to the one at `other`"""
        self.guard(c, (self[other],))

    def pair(self, src, q, pat):
        """pat at src and at q, nothing equal in front of or behind the two"""
        g = self.plant(src, pat)
        self.plant(q, pat, (g,))
        if q + len(pat) + LEAD < len(self.b):
            self.differ(q + len(pat), src + len(pat))

    def bytes(self):
        return bytes(self.b)


def slid_window_chunk(rng, at_):
    """A chunk of a full piece whose position 65 274, the first behind the slide, repeats the four bytes at `at_`, the first entry of
    its chain (at distance MAX_DIST only the first is looked at).  at_ = 32 768 reads as NIL behind the slide, 32 769 is found."""
    q = K_SLIDE

    def bucket(c, p):
        return ((c[p] << 10) ^ (c[p + 1] << 5) ^ c[p + 2]) & 0x7fff

    while True:
        chunk = bytearray(rng.randbytes(D + P))
        chunk[q:q + 4] = chunk[at_:at_ + 4]   # four bytes: the three that still match one position on are too far for a match of three
        chunk[q + 4] = chunk[at_ + 4] ^ 0x55
        if all(bucket(chunk, p) != bucket(chunk, q) for p in range(at_ + 1, q)):
            return bytes(chunk)


def one_block_bodies(rng, lit):
    """Three inputs of two pieces whose piece 1 is one block that starts at D < 32 768 and is flushed at D + P >= 65 274: runs of 258
    zeros `lit` random bytes apart, the same behind random bytes, and text"""
    run = bytes(258)
    body = b"".join(rng.randbytes(lit) + run for _ in range(2 * P // (258 + lit) + 1))[:2 * P]
    return body, rng.randbytes(P + 4000) + body[P + 4000:], corpus.text_like(lit, 2 * P)


def stored_pieces_input(rng):
    """Two pieces and 10 000 bytes of random bytes: piece 1 is several stored blocks, piece 2 one"""
    return rng.randbytes(2 * P + 10000)


def literal_filler(rng, n=2 * P):
    """Random bytes in which no three bytes stand twice, so no parser finds a match in them: a byte that ends a repeated triple is
    drawn again until none is left"""
    b = bytearray(rng.randbytes(n))
    while True:
        seen, bad = set(), []
        for p in range(n - 2):
            k = b[p] << 16 | b[p + 1] << 8 | b[p + 2]
            if k in seen:
                bad.append(p + 2)
            seen.add(k)
        if not bad:
            return bytes(b)
        for p in bad:
            b[p] = rng.randrange(256)


def family_a(rng):
    out = []
    for bg in ("sparse", "dense"):
        def canvas(seed):
            return Canvas(bg, seed, rng)

        def add(shape, cv, claim, levels=LEVELS):
            out.append(Case("a", shape, bg, cv.bytes(), 1, claim, levels))
        for r in (1, 2, 3, 4, 300):
            cv = canvas(100 + r)
            v = cv.guard(D - r)
            cv.put(D - r, bytes([v]) * (r + 300))
            cv.guard(D - r - 1, (v,))
            cv.guard(D + 300, (v,))
            add("run r=%d" % r, cv, first((258, 1), (42, 1)))
        for per in (2, 3):
            cv = canvas(110 + per)
            unit = bytes(rng.sample(range(0x80, 0x100), per))
            cv.put(D - per, (unit * 200)[:per + 300])
            cv.guard(D - per - 1, (unit[-1],))
            cv.guard(D + 300, ((unit * 200)[per + 300],))
            add("run period %d" % per, cv, first((258, per), (42, per)))
        for pos in (0, 1):
            for dist in (K_MAXDIST - 1, K_MAXDIST, K_MAXDIST + 1):
                cv = canvas(120 + pos)
                pat = rng.randbytes(40)
                cv.pair(D + pos - dist, D + pos, pat)
                add("edge %d at %d" % (dist, pos), cv, at(pos, (40, dist) if dist <= K_MAXDIST else (0, pat[0])))
        # a match that stands in the dictionary's parse at D - 1 and covers the piece's first 59 bytes: the piece searches for itself
        cv = canvas(130)
        pat = rng.randbytes(60)
        g = cv.plant(5000, pat)
        cv.plant(D - 1, pat, (g,))
        cv.differ(D + 59, 5060)
        cv.plant(20000, pat[1:11], (g,))
        cv.guard(20010, (pat[11],))
        add("nothing pending", cv, first((59, D - 5001)))
        # the mirror: five bytes match at piece position 0, thirty at position 1
        cv = canvas(131)
        a5 = rng.randbytes(5)
        b30 = a5[1:] + rng.randbytes(26)
        g = cv.plant(6000, a5)
        cv.guard(6005, (b30[4],))
        cv.plant(9000, b30, (a5[0], g))
        cv.put(D, a5[:1] + b30)
        cv.differ(D + 31, 9030)
        add("lazy at the first byte", cv, first((0, a5[0]), (30, D + 1 - 9000)), (5, 6))
        for back in (2, 1):
            cv = canvas(140 + back)
            cv.pair(D - back, D + 1000, rng.randbytes(40))
            add("source at D-%d" % back, cv, at(1000, (40, 1000 + back)))
    return out


def family_b(rng):
    out = []
    for bg in ("sparse", "dense"):
        def add(shape, cv, claim, behind=0):
            out.append(Case("b", shape, bg, cv.bytes(), 1, claim, LEVELS, behind))
        for q in BORDER_QUERIES:
            cv = Canvas(bg, 200 + q % 7, rng)
            cv.pair(20000, D + q, rng.randbytes(50))
            add("query at %d" % q, cv, at(q, (50, D + q - 20000)))
        for border in (K_WSIZE, 49152):
            q = border - D - 129
            cv = Canvas(bg, 210, rng)
            cv.pair(20000, D + q, rng.randbytes(258))
            add("258 across %d" % border, cv, at(q, (258, D + q - 20000)))
        cv = Canvas(bg, 220, rng)
        cv.pair(D + 3000, D + P - 258, rng.randbytes(258))
        add("258 to the last byte", cv, last((258, P - 258 - 3000)))
        cv = Canvas(bg, 221, rng)
        cv.pair(D + P - 3 - 1000, D + P - 3, rng.randbytes(3))
        add("match in the last three bytes", cv, last((3, 1000)))
        # a full piece that is not the stream's last: the source goes on with sixteen bytes, none of them zero, and so does the
        # next piece, so a length that the lookahead did not end at ten would run on into it
        cv = Canvas(bg, 222, rng, 2 * P + PAST_END_TAIL)
        pat, cont = rng.randbytes(10), bytes(rng.randrange(1, 256) for _ in range(PAST_END))
        g = cv.plant(D + P - 10 - 3000, pat + cont)
        cv.plant(D + P - 10, pat, (g,))
        cv.put(D + P, cont)
        cv.differ(D + P + PAST_END, D + P - 3000 + PAST_END)
        add("candidate runs past the end", cv, last((10, 3000)), PAST_END)
    for at_, hit in ((K_WSIZE, False), (K_WSIZE + 1, True)):
        chunk = slid_window_chunk(rng, at_)
        claim = last((4, K_SLIDE - at_), (0, chunk[-2]), (0, chunk[-1])) if hit else last(*((0, x) for x in chunk[K_SLIDE:]))
        out.append(Case("b", "slid window source %d" % at_, "sparse", rng.randbytes(LEAD) + chunk, 1, claim))
    return out


def family_d(rng):
    out = []
    for bg in ("sparse", "dense"):
        for n in SHORT_LENGTHS + (-3,):
            cv = Canvas(bg, 300 + n, rng, P + 300)
            pat = rng.randbytes(260)
            src = 10000 if n > 0 else D - 2000             # (-3: three bytes within 4 096)
            cv.plant(src, pat)
            m = abs(n)
            cv.put(D, pat[:m])
            lits = tuple((0, x) for x in pat[:m])
            want = (lits if n in (1, 2, 3) else ((min(m, 258), D - src),) + lits[258:])
            out.append(Case("d", "short %d %s" % (m, "near" if n < 0 else "far"), bg, cv.bytes()[:P + m], 1, tokens(*want)))
    return out


def family_e(rng):
    out = []
    filler = literal_filler(rng)
    for n in FILLER_LENGTHS:
        out.append(Case("e", "filler %d" % n, "sparse", filler[:P + n], 1, every(matches(0), records(*blocks_of([1] * n))), one_level=True))
    for k in PLANTED_SYMBOLS:                               # the match is symbol k of the piece: k - 1 literals in front of it
        b = bytearray(filler[:P + k - 1 + 100 + 50])
        q = P + k - 1
        b[q:q + 100] = b[q - 5000:q - 4900]
        while b[q + 100] == b[q - 4900]:
            b[q + 100] = rng.randrange(256)
        lengths = [1] * (k - 1) + [100] + [1] * 50
        out.append(Case("e", "match as symbol %d" % k, "sparse", bytes(b), 1,
                        every(matches(1), at(k - 1, (100, 5000)), records(*blocks_of(lengths))), one_level=True))

    def one_block(tok, rec):
        assert len(rec) == 1 and len(tok) <= K_SYMS and rec[0]["start"] == D < K_WSIZE and rec[0]["flush_pos"] == D + P >= K_SLIDE
        assert rec[0]["type"] != emu_binding.STORED
    for name, bg, data in zip(("zero runs", "zero runs behind random bytes", "text"), (None, None, "dense"), one_block_bodies(rng, 2)):
        out.append(Case("e", "one block not stored: " + name, bg, data, 1, one_block))
    data = stored_pieces_input(rng)

    def stored_full(tok, rec):
        assert len(rec) >= 2 and rec[0]["n_sym"] == K_SYMS and sum(r["n_sym"] for r in rec) == len(tok)
        assert [r["type"] for r in rec] == [emu_binding.STORED] * len(rec) and sum(r["bytes"] for r in rec) == P
        assert rec[0]["start"] == D and rec[0]["flush_pos"] < K_SLIDE and rec[1]["start"] >= K_WSIZE

    def stored_short(tok, rec):
        assert len(rec) == 1 and rec[0]["type"] == emu_binding.STORED and rec[0]["bytes"] == 10000
    out.append(Case("e", "stored full piece", "sparse", data, 1, stored_full))
    out.append(Case("e", "stored short piece", "sparse", data, 2, stored_short))
    return out


def cases(seed=2029):
    """Every case, in the order of the families; no emu is needed to build them"""
    rng = random.Random(seed)
    out = family_a(rng) + family_b(rng)
    head = corpus.text_like(7, 2 * P)
    out += [replace(c, data=head + c.data, piece=c.piece + 2) for c in out]
    return out + family_d(rng) + family_e(rng)


# ---- preconditions ----------------------------------------------------------------------------------------------------------

BOTH, SPARSE = ("sparse", "dense"), ("sparse",)
REQUIRED = {                       # family -> {shape: (backgrounds, pieces)}
    "a": {s: (BOTH, (1, 3)) for s in ["run r=%d" % r for r in (1, 2, 3, 4, 300)] + ["run period 2", "run period 3"] +
          ["edge %d at %d" % (d, p) for d in (32505, 32506, 32507) for p in (0, 1)] +
          ["nothing pending", "lazy at the first byte", "source at D-2", "source at D-1"]},
    "b": {**{s: (BOTH, (1, 3)) for s in ["query at %d" % q for q in BORDER_QUERIES] + ["258 across 32768", "258 across 49152", "258 to the last byte",
                                           "match in the last three bytes", "candidate runs past the end"]},
          **{s: (SPARSE, (1, 3)) for s in ("slid window source 32768", "slid window source 32769")}},
    "d": {s: (BOTH, (1,)) for s in ["short %d far" % n for n in SHORT_LENGTHS] + ["short 3 near"]},
    "e": {**{s: (SPARSE, (1,)) for s in ["filler %d" % n for n in FILLER_LENGTHS] + ["match as symbol %d" % k for k in PLANTED_SYMBOLS] + ["stored full piece"]},
          "stored short piece": (SPARSE, (2,)), "one block not stored: text": (("dense",), (1,)),
          "one block not stored: zero runs": ((None,), (1,)), "one block not stored: zero runs behind random bytes": ((None,), (1,))},
}


def check(cases_, emu):
    """Every claim holds on the emu, and every shape of REQUIRED is there.  A condition, not a measurement: nothing is skipped."""
    assert len({c.name for c in cases_}) == len(cases_)
    have = {(c.family, c.shape, c.background, c.piece) for c in cases_}
    assert {c.family for c in cases_} == set(REQUIRED), sorted({c.family for c in cases_})
    for fam, shapes in REQUIRED.items():
        for shape, (bgs, pieces) in shapes.items():
            for bg in bgs:
                for k in pieces:
                    assert (fam, shape, bg, k) in have, ("missing", fam, shape, bg, k)
    groups = {}                    # a case of a or b and its copy at piece 3 are one chunk: it is parsed once
    for c in cases_:
        assert c.piece >= 1 and len(c.data) > c.piece * P and (c.levels == LEVELS or c.levels == (5, 6)), c.name
        assert len(c.tail()) == c.behind and (c.behind >= PAST_END) == (c.shape == "candidate runs past the end"), c.name
        groups.setdefault((c.chunk(), c.tail()), []).append(c)
    e_level6 = {}                  # family e at level 6: shape -> (index of the first match token, records)
    for (chunk, tail), group in groups.items():
        for level in sorted({lv for c in group for lv in ((6,) if c.one_level else c.levels)}):
            tok, rec = emu_binding.piece(emu, chunk, D, level, tail)
            assert rec and rec[0]["start"] == D and sum(r["n_sym"] for r in rec) == len(tok), group[0].name
            assert sum(t[0] or 1 for t in tok) == len(chunk) - D, group[0].name
            for c in group:
                if level not in ((6,) if c.one_level else c.levels):
                    continue
                try:
                    c.claim(tok, rec)
                    if c.behind:   # the next piece begins as the source of the last match goes on: only the lookahead ends it
                        n, dist = tok[-1]
                        assert len(chunk) == D + P and n and dist >= c.behind and tail == chunk[len(chunk) - dist:len(chunk) - dist + c.behind] and 0 not in tail, (tok[-1], tail)
                except AssertionError as e:
                    raise AssertionError("%s at level %d: %s" % (c.name, level, e)) from None
                if c.family == "e" and level == 6:
                    e_level6[c.shape] = (next((i for i, t in enumerate(tok) if t[0]), None), rec)
    # e, on the emu's records: the blocks the issue states, the second block of a full piece flushed behind the slide position, and
    # the planted match as the last two symbols of the first block and the first two of the second
    for n, want in STATED_RECORDS.items():
        records(*want)(None, e_level6["filler %d" % n][1])
    rec = e_level6["filler %d" % P][1]
    assert rec[1]["flush_pos"] == rec[2]["start"] >= K_SLIDE, rec
    planted = []
    for k in PLANTED_SYMBOLS:
        i, rec = e_level6["match as symbol %d" % k]
        b = next(b for b in range(len(rec)) if i < sum(r["n_sym"] for r in rec[:b + 1]))
        planted.append((b, i - sum(r["n_sym"] for r in rec[:b])))
    assert planted == [(0, K_SYMS - 2), (0, K_SYMS - 1), (1, 0), (1, 1)], planted


# ---- the order of the GPU file's batches: host arithmetic, asserted with and without a GPU -------------------------------------------

MATCHES = ("auto", "walk", "band", "lazy", "autoband", "autolazy")
SUM_ROW = 64                       # dstream_core.h: kSumRow, the values a wave joins in one step
DEFAULT_SLICE = 8192               # zwz_ctx_create: max_batch_chunks = 0
LONG_SLICES = (DEFAULT_SLICE, 64, 65, 100)
# (name, data, seed, pieces, bytes of the last piece).  A stream of 7 pieces and one of 27 in front, so that the text stream of 130
# pieces starts at piece 34: a slice of 100 pieces holds its first 66 and the next its last 64; slices of 65 hold 31, 65 and 34 of
# them, slices of 64 hold 30, 64 and 36.
LONG_STREAMS = (("text 7", "text", 60, 7, 100), ("random 27", "random", 61, 27, 1), ("text 130", "text", 62, 130, P), ("ff 64", "ff", 0, 64, P),
                ("random 65", "random", 63, 65, 1), ("text 66", "text", 64, 66, P - 1), ("ff 67", "ff", 0, 67, 1), ("random 128", "random", 65, 128, P),
                ("text 129", "text", 66, 129, P - 1), ("ff 130", "ff", 0, 130, P), ("empty", "ff", 0, 0, 0), ("random 129", "random", 67, 129, 1),
                ("lz_heavy 1030", "lz_heavy", 68, 1030, P), ("ff 1030", "ff", 0, 1030, P - 1))


def long_stream_lengths():
    return [(pieces - 1) * P + last if pieces else 0 for _, _, _, pieces, last in LONG_STREAMS]


def wrapper_of(match, level_index, slices_index):
    """The wrapper of one call of the case batch: all three occur at every level over the six values of the match option"""
    return ref.WRAPS[(MATCHES.index(match) + level_index + slices_index) % 3]


def check_wrappers_rotate():
    for slices_index in (0, 1):
        for li in range(len(LEVELS)):
            assert {wrapper_of(m, li, slices_index) for m in MATCHES} == set(ref.WRAPS)


def slice_counts(lens, m):
    """[[pieces of stream i in every slice of m pieces it has a piece in]], as dstream_launch cuts the list: slices begin at
    multiples of m in the pieces counted over the batch, and an empty stream has none"""
    pfirst = np.concatenate([[0], np.cumsum([-(-n // P) for n in lens])])
    out = []
    for i in range(len(lens)):
        lo, hi = int(pfirst[i]), int(pfirst[i + 1])
        out.append([min(hi, (s + 1) * m) - max(lo, s * m) for s in range(lo // m, -(-hi // m))] if hi > lo else [])
    return out


def check_long_stream_order(names, lens):
    """What dstream_combine_kernel sees of the long streams: it joins the full pieces of a stream in a slice (all but the last
    one there) in rows of K = ceil(full / 64) values -- full = 63, 64, 65 and 128 and more, and the checksum carried between slices"""
    assert list(names) == [s[0] for s in LONG_STREAMS] and len(lens) == len(names)
    full = {m: [[c - 1 for c in s] for s in slice_counts(lens, m)] for m in LONG_SLICES}
    k = list(names).index("text 130")
    assert full[DEFAULT_SLICE][k] == [129] and full[100][k] == [65, 63] and full[65][k] == [30, 64, 33] and full[64][k] == [29, 63, 35]
    one = [f[0] for f in full[DEFAULT_SLICE] if f]
    assert len(one) == len(lens) - 1 and {63, 64, 65, 66, 127, 128, 129, 1029} <= set(one)            # K = 1, 1, 2, ..., 3, 17
    assert all(len(f) >= 2 for m in (64, 65, 100) for f, n in zip(full[m], lens) if n > 100 * P)     # the checksum goes from slice to slice
    for m in (64, 65, 100):
        assert max(max(f) for f in full[m] if f) == m - 1
        assert sum(m - 1 in f for f in full[m]) >= 3
    # rows of K values with and without padding in front: full = 128 fills 64 rows of 2, full = 65 leaves 63 places empty
    rows = lambda f: (-(-f // SUM_ROW), -(-f // SUM_ROW) * SUM_ROW - f)
    have = {rows(f) for m in LONG_SLICES for s in full[m] for f in s}
    assert {(1, 0), (2, 63), (2, 29), (2, 0), (3, 63), (17, 59)} <= have, sorted(have)


def summary(cases_):
    """{family: (cases, input bytes)}"""
    out = {}
    for c in cases_:
        n, b = out.get(c.family, (0, 0))
        out[c.family] = (n + 1, b + len(c.data))
    return out
