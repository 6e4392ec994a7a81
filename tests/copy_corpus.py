"""Hand-built match geometries for the inflate kernel's batch copy (csrc/zwz_kernels.hip, inflate_kernel: "The wave moves the bytes of
this batch" down to the sequential-decoder branch), written with deflate_gen.Stream.  Test infrastructure only.

corpus(seed) -> [Case].  A case is a list of blocks -- ("stored", bytes) | ("fixed", tokens) | ("dyn", tokens, llens, dlens) -- with
the raw DEFLATE body they encode (last block final), the bytes a decoder must produce (for an invalid case: everything before the
refused symbol) and whether it is valid.  No reference of a case reaches in front of its own first byte, so a case can be wrapped
(wrapped()), put behind another gzip member (gzip_second()) or chained as a full-flush piece (Case.piece(), chain()).

What the kernel does decides only WHICH streams are here: a round of it ends at a stopping symbol, at 64 symbols (BATCH) or where
its 512-bit window ends (WINDOW); a batch of up to 1024 bytes (OWN_CAP) looks its owners up in a per-byte map, a larger one searches;
length symbols on codes above 10 bits and distance symbols on codes above 8 go through the one-symbol sequential path.  The expected
bytes come from the token lists and are checked against libz, never from any of that.

Two code sets: "fixed", where a round ends at the window's end with fewer than 64 symbols, and "dense" -- a dynamic code with
Huffman lengths for the block's own few symbols, literals at about 3 bits -- where a round does fill 64 symbols.  A *phase* is a
number of literals in front of a pattern: a block's first round starts at its first symbol, so the phase moves the pattern through
every place of a round.

Families (Case.family):
  a    self-overlap: every distance 1..70, 127..129, 255..259 behind d fresh literals, lengths 3, d-1, d, d+1, 2d+1, 257, 258; the
       period in the same round as the match, in an earlier block (older output), and written by a match of the same round
  b    reference chains of 200 and more matches in a row, each reaching into the symbol before it (deep: the first byte of the symbol
       before, so a chase runs through every symbol of the batch down to the literal in front), into the two before it (straddle), or
       anywhere up to two bytes beyond it (random); short lengths 3..12 (a batch stays under 1024 bytes: mapped) and long ones
       100..258 (far above: searched); sources of one batch in ascending, descending and shuffled order
  c    the 1024-byte edge: one-round blocks (at most 60 symbols and 400 bits, ending in end-of-block) that decode to every size
       1000..1050 and to multiples of 16 +- 1 around them, with sources in front of the block, inside it and across its start
  d    batch-start straddle: a match with distance < length whose source begins in older output and ends in its own round, moved by
       the phase to every symbol index of a dense run (0, 1, 62 and 63 among them)
  e    just-written sources: the first symbol of a round copying the last 1..64 bytes of the round before it; a Huffman block whose
       first symbol is a match into the stored block right before it (1, 15, 16, 17, 64, 1000 bytes; distance 1, the stored length,
       and one that starts in front of the stored block; output at 0 and 5 mod 16)
  f    one-symbol sequential path: length symbols on 11- to 13-bit codes and distance symbols on 9- to 11-bit codes, reading what the
       batch wrote right before them, what the path itself wrote last, and far-back output (with and without a fence since); lengths
       below and above the distance; always followed by a fast-path match into what the path wrote
  g    window and position edges: distances 32 768 and 32 767, lengths 258 and 3, behind stored random bytes, at output positions
       32 768, 65 013 (the last match ends at 65 535), 65 535, 65 536, 65 537 and 131 071
  h    invalid twins of a, b, e, f and g: the same shapes with one distance exactly one more than the output so far, on the batch
       path and on the sequential path; libz says data error, the output is everything before that symbol
  cap  capacity twins: streams that end in a 258 match or in a literal (the stream form gets capacities of the size, one less and one
       more), and three that reach 65 535 bytes exactly, by a 258 match that ends one past it, and by a literal at it

check(cases) asserts, from the token lists alone, that the shapes above are really reached; corpus() runs it.
"""
import random
import struct
import zlib
from dataclasses import dataclass

import deflate_gen as dg
import stream_ref

BATCH, WINDOW, OWN_CAP = 64, 512, 1024
CHUNK = 65535
SELF_OVERLAP_DISTANCES = list(range(1, 71)) + [127, 128, 129] + list(range(255, 260))
EDGE_SIZES = sorted(set(range(1000, 1051)) | {975, 977, 991, 993, 1055, 1057, 1071, 1073})
STORED_LENGTHS = (1, 15, 16, 17, 64, 1000)
POSITIONS = (32768, 65013, 65535, 65536, 65537, 131071)
SLOW_LEN_BITS, SLOW_DIST_BITS = 11, 9


# ---- blocks -----------------------------------------------------------------------------------------------------------------

def fixed(tokens):
    return ("fixed", list(tokens))


def dense(tokens):
    """A dynamic block whose code lengths are Huffman's for the block's own symbols (literal/length <= 9 bits, distance <= 8)."""
    tokens = list(tokens)
    lf, df = [0] * 286, [0] * 30
    lf[256] = 1
    for t in tokens:
        if isinstance(t, int):
            lf[t] += 1
        else:
            lf[dg.length_code(t[1])[0]] += 1
            df[dg.dist_code(t[2])[0]] += 1
    return ("dyn", tokens, dg.huffman_lengths(lf, 9), dg.huffman_lengths(df, 8))


def block(code, tokens):
    return fixed(tokens) if code == "fixed" else dense(tokens)


def stored(data):
    return [("stored", bytes(data[i:i + CHUNK])) for i in range(0, max(len(data), 1), CHUNK)]


def code_lengths(b):
    """(literal/length lengths, distance lengths) of a Huffman block"""
    return (dg.FIXED_LIT, dg.FIXED_DIST) if b[0] == "fixed" else (b[2], b[3])


def token_bits(t, llens, dlens):
    if isinstance(t, int):
        return llens[t]
    lc, lx, _ = dg.length_code(t[1])
    dc, dx, _ = dg.dist_code(t[2])
    return llens[lc] + lx + dlens[dc] + dx


def is_slow(t, llens, dlens):
    """a match the kernel hands to its one-symbol sequential path: a code longer than its fast tables"""
    return not isinstance(t, int) and (llens[dg.length_code(t[1])[0]] >= SLOW_LEN_BITS or dlens[dg.dist_code(t[2])[0]] >= SLOW_DIST_BITS)


def complete(want, n, fillers):
    """Code lengths over n symbols: `want` {symbol: length} plus as many of `fillers` (unused symbols) as make the code complete."""
    lens = [0] * n
    for s, l in want.items():
        lens[s] = l
    left = dg.kraft(lens)
    assert left >= 0
    fillers = [s for s in fillers if s not in want]
    for bit in range(14, -1, -1):
        if left >> bit & 1:
            lens[fillers.pop()] = 15 - bit
    assert dg.kraft(lens) == 0
    return lens


def encode(blocks, final=True, marker=False):
    """-> (raw DEFLATE bytes, Stream.data, Stream.valid, bit index of the last block's BFINAL, bits in all).  marker: every block
    non-final, an empty stored block (00 00 ff ff on a byte boundary) behind them.  Leading stored blocks are written byte-wise (the
    bit writer is quadratic in the stream's length)."""
    head, seen, i = bytearray(), bytearray(), 0
    while i < len(blocks) - 1 and blocks[i][0] == "stored":
        d = blocks[i][1]
        head += b"\x00" + struct.pack("<HH", len(d), len(d) ^ 0xffff) + d
        seen += d
        i += 1
    s = dg.Stream(header=None)
    s.data = seen
    for j in range(i, len(blocks)):
        b, last = blocks[j], final and not marker and j == len(blocks) - 1
        if j == len(blocks) - 1:
            bfinal = 8 * len(head) + s.w.n
        if b[0] == "stored":
            s.stored(b[1], final=last)
        elif b[0] == "fixed":
            s.fixed(b[1], final=last)
        else:
            s.dynamic(b[1], b[2], b[3], final=last)
    if marker:
        s.stored(b"")
    return bytes(head) + s.w.bytes(), bytes(s.data), s.valid, bfinal, 8 * len(head) + s.w.n


def symbols(blocks):
    """The token lists decoded in plain Python -> (data, [(block, index in block, token | None, position, bytes)], position of the
    first symbol whose distance reaches in front of the data, its block and index | None).  A stored block is one entry with token None."""
    data, syms, bad = bytearray(), [], None
    for bi, b in enumerate(blocks):
        if b[0] == "stored":
            syms.append((bi, 0, None, len(data), len(b[1])))
            data += b[1]
            continue
        for ti, t in enumerate(b[1]):
            if isinstance(t, int):
                syms.append((bi, ti, t, len(data), 1))
                data.append(t)
                continue
            _, n, d = t
            if d > len(data):
                return bytes(data), syms, (len(data), bi, ti)
            syms.append((bi, ti, t, len(data), n))
            data += (bytes(data[-d:]) * (n // d + 1))[:n]
    return bytes(data), syms, bad


@dataclass
class Case:
    family: str
    name: str
    blocks: list
    data: bytes
    valid: bool
    body: bytes
    bfinal: int = 0                # bit index of the last block's BFINAL in body
    nbits: int = 0                 # bits of body in use

    def piece(self):
        """the same blocks, none final, with an empty stored block behind them: a full-flush piece.  (encode(blocks, marker=True)
        without encoding again: BFINAL cleared, the three header bits 000 in the zero padding where they fit.)"""
        b = bytearray(self.body)
        b[self.bfinal >> 3] &= ~(1 << (self.bfinal & 7)) & 255
        return bytes(b) + (b"" if len(b) * 8 - self.nbits >= 3 else b"\x00") + b"\x00\x00\xff\xff"

    def stop_length(self, cap):
        """Output of a decoder that stops at the first symbol that would pass `cap` bytes (a stored block is cut there)."""
        for _, _, t, pos, n in symbols(self.blocks)[1]:
            if pos + n > cap:
                return cap if t is None else pos
        return len(self.data)


def make(family, name, blocks):
    blocks = [b for x in blocks for b in (x if isinstance(x, list) else [x])]
    body, sdata, valid, bfinal, nbits = encode(blocks)
    data, _, bad = symbols(blocks)
    assert valid == (bad is None), name
    if valid:
        assert data == sdata, name
    return Case(family, name, blocks, data, valid, body, bfinal, nbits)


def wrapped(wrap, body, data):
    """wrap: 0 raw, 1 zlib, 2 gzip (stream_ref's numbers)"""
    if wrap == 0:
        return body
    if wrap == 1:
        return b"\x78\x9c" + body + struct.pack(">I", zlib.adler32(data))
    return b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\x03" + body + struct.pack("<II", zlib.crc32(data), len(data) & 0xffffffff)


def gzip_second(case, first):
    """A gzip stream of two members: `first` in stored blocks, then the case -- the case's bytes start at len(first), not at 0."""
    body = b"".join(bytes([i + CHUNK >= len(first)]) + struct.pack("<HH", len(first[i:i + CHUNK]), len(first[i:i + CHUNK]) ^ 0xffff) +
                    first[i:i + CHUNK] for i in range(0, max(len(first), 1), CHUNK))
    return wrapped(2, body, first) + wrapped(2, case.body, case.data)


def chain(wrap, cases):
    """One stream of the cases as full-flush pieces, ended by a final empty stored block -> (stream, bytes, pieces)"""
    data = b"".join(c.data for c in cases)
    return wrapped(wrap, b"".join(c.piece() for c in cases) + b"\x01\x00\x00\xff\xff", data), data, len(cases)


# ---- families ---------------------------------------------------------------------------------------------------------------

def _alphabet(rng, code):
    return rng.sample(range(256), 6) if code == "dense" else list(range(256))


def _lits(rng, n, alpha):
    return [rng.choice(alpha) for _ in range(n)]


def family_a(rng):
    out = []
    for d in SELF_OVERLAP_DISTANCES:
        lens = sorted({min(258, max(3, x)) for x in (3, d - 1, d, d + 1, 2 * d + 1, 257, 258)})
        for code in ("fixed", "dense"):
            alpha = _alphabet(rng, code)
            blocks = []
            for n in lens:
                blocks.append(block(code, _lits(rng, d, alpha) + [("m", n, d)] + _lits(rng, 2, alpha)))            # period and match in one block
                blocks.append(block(code, _lits(rng, d, alpha)))                                                   # the period is older output:
                blocks.append(block(code, [("m", n, d)] + _lits(rng, 1, alpha)))                                   # the match starts its block
                blocks.append(block(code, _lits(rng, d, alpha) + [("m", min(258, max(3, d)), d), ("m", n, d)]))              # the period written by a match
            out.append(make("a", "self-overlap d%d %s" % (d, code), blocks))
    return out


def _chain_tokens(rng, kind, lo, hi, count, produced, prev):
    """`count` matches in a row behind `produced` bytes whose last symbol was `prev` bytes long"""
    toks = []
    for i in range(count):
        n = rng.randint(lo, hi)
        if kind == "deep":
            d = prev
        elif kind == "straddle":
            d = min(produced, prev + rng.randint(1, 2))
        else:
            d = prev if rng.random() < 0.5 else rng.randint(1, min(produced, prev + 2))
        toks.append(("m", n, d))
        produced += n
        prev = n
    return toks


def family_b(rng):
    out = []
    plan = [("short", 3, 12, "deep", "dense", range(64)), ("short", 3, 12, "random", "dense", range(0, 64, 4)),
            ("short", 3, 12, "straddle", "dense", (0, 1, 2, 31, 32, 33, 62, 63)), ("short", 3, 12, "deep", "fixed", (0, 1, 13, 63)),
            ("short", 3, 12, "random", "fixed", (0, 1, 13, 63)), ("short", 3, 3, "deep", "dense", (1, 2, 3, 31, 62, 63)),
            ("long", 100, 258, "deep", "dense", (0, 1, 2, 33, 62, 63)), ("long", 100, 258, "random", "dense", (0, 1, 2, 33, 62, 63)),
            ("long", 100, 258, "straddle", "dense", (0, 1, 33, 63)), ("long", 258, 258, "deep", "dense", (1, 17)),
            ("long", 100, 258, "deep", "fixed", (1, 40)), ("long", 100, 258, "random", "fixed", (0, 5))]
    for size, lo, hi, kind, code, phases in plan:
        for phase in phases:
            alpha = _alphabet(rng, code)
            seed = rng.randbytes(16)
            toks = _lits(rng, phase, alpha)
            toks += _chain_tokens(rng, kind, lo, hi, 220, 16 + phase, 1)
            out.append(make("b", "chain %s %d-%d %s %s phase %d" % (size, lo, hi, kind, code, phase), [stored(seed), block(code, toks)]))
    # the sources of one batch in ascending, descending and shuffled order: 16 literals, then 40 matches of 4 bytes into them
    for order in ("ascending", "descending", "shuffled"):
        for code in ("fixed", "dense"):
            alpha = list(range(256))
            toks = rng.sample(alpha, 16)
            targets = [rng.randrange(0, 13) for _ in range(40)]
            targets = sorted(targets) if order == "ascending" else sorted(targets, reverse=True) if order == "descending" else targets
            pos = 16
            for tg in targets:
                toks.append(("m", 4, pos - tg))
                pos += 4
            out.append(make("b", "order %s %s" % (order, code), [block(code, toks)]))
    return out


def family_c(rng):
    out = []
    for n in EDGE_SIZES:
        for code in ("fixed", "dense"):
            alpha = _alphabet(rng, code)
            r = n - 720
            toks = _lits(rng, 4, alpha) + [("m", 258, 304),            # wholly in front of the block
                                           ("m", 200, 100),            # inside it, overlapping itself
                                           ("m", 258, 150),            # inside it
                                           ("m", r - 100, 850),        # begins in front of the block, ends inside it
                                           ("m", 94, 5)] + _lits(rng, 6, alpha)
            out.append(make("c", "edge %d %s" % (n, code), [stored(rng.randbytes(300)), block(code, toks)]))
    return out


D_RUN = 70


def family_d(rng):
    out = []
    for phase in range(64):
        for code in ("dense", "fixed"):
            alpha = _alphabet(rng, code)
            toks = _lits(rng, phase, alpha)
            for n, d in ((100, 70), (50, 2), (258, 65), (9, 8)):
                toks += _lits(rng, D_RUN, alpha) + [("m", n, d)]
            toks += _lits(rng, 3, alpha)
            out.append(make("d", "straddle %s phase %d" % (code, phase), [stored(rng.randbytes(80)), block(code, toks)]))
    return out


def family_e(rng):
    out = []
    for d in range(1, 65):
        for code in ("dense", "fixed"):
            alpha = _alphabet(rng, code)
            blocks = [stored(rng.randbytes(70))]
            for phase in (0, 1, 2, 31, 32, 33, 62, 63):
                blocks.append(block(code, _lits(rng, phase + BATCH, alpha) + [("m", 3, d), ("m", min(258, d + 5), d)] + _lits(rng, 2, alpha)))
            out.append(make("e", "round before d%d %s" % (d, code), blocks))
    for n in STORED_LENGTHS:
        for pre in (16, 21):
            for which, d in (("1", 1), ("stored length", n), ("before the stored block", n + 3)):
                for code in ("fixed", "dense"):
                    alpha = _alphabet(rng, code)
                    out.append(make("e", "stored %d at %d distance %s %s" % (n, pre, which, code),
                                    [fixed(_lits(rng, pre, range(256))), stored(rng.randbytes(n)),
                                     block(code, [("m", 7, d), ("m", 40, d)] + _lits(rng, 3, alpha))]))
    return out


def slow_codes(alpha):
    """A dynamic code with length symbols 258, 262, 266, 284 on 11- to 13-bit codes and distance symbols 1, 4, 8, 13, 20 on 9- to
    11-bit codes beside short codes for 257, 259, 264, 285 and distance symbols 0, 3, 5, 7, 10, 14, 21."""
    want = {s: 3 for s in alpha}
    want.update({256: 5, 257: 5, 259: 5, 264: 6, 285: 6, 258: 11, 262: 11, 266: 12, 284: 13})
    llens = complete(want, 286, [s for s in range(255, -1, -1) if s not in alpha][:20])
    dlens = complete({0: 2, 3: 3, 5: 3, 7: 3, 10: 4, 14: 4, 21: 5, 1: 9, 4: 9, 8: 10, 13: 10, 20: 11}, 30, list(range(29, 21, -1)) + [2, 6, 9, 11, 12])
    return llens, dlens


def family_f(rng):
    out = []
    alpha = rng.sample(range(256), 6)
    llens, dlens = slow_codes(alpha)
    L = lambda n: _lits(rng, n, alpha)
    tail = [("m", 5, 4), ("m", 3, 1)]                       # fast-path matches into what the sequential path just wrote
    scenes = {
        # reads what the batch of the same round wrote right before it; length above the distance
        "after the batch": L(10) + [("m", 5, 4), ("m", 10, 7), ("m", 4, 4), ("m", 8, 7)] + tail,
        # reads its own previous output; the second wraps (13 over 8)
        "own output": L(9) + [("m", 8, 16), ("m", 13, 8), ("m", 14, 13)] + tail + L(2),
        # far back with nothing fenced yet, then far back again right after a fence
        "far back": [("m", 4, 1100), ("m", 8, 1536), ("m", 227, 1030)] + tail + L(3),
        # a fence by the first, then far-back sources well below it
        "far back after a fence": L(5) + [("m", 4, 4), ("m", 8, 1100), ("m", 257, 1200), ("m", 258, 2)] + tail,
        # length below the distance (no wrap) and far above it
        "below and above": L(20) + [("m", 4, 7), ("m", 4, 16), ("m", 240, 4), ("m", 8, 1), ("m", 13, 40)] + tail,
        # the distance symbol alone is the long code
        "long distance codes": L(30) + [("m", 5, 2), ("m", 10, 5), ("m", 10, 6), ("m", 3, 20), ("m", 258, 24), ("m", 5, 100)] + tail,
        # in a row, each reading the one before
        "in a row": L(4) + [("m", 4, 4)] * 5 + [("m", 8, 4), ("m", 13, 8), ("m", 5, 2), ("m", 5, 2)] + tail,
        # between fast matches that read it
        "between fast matches": L(8) + [("m", 3, 8), ("m", 4, 1), ("m", 10, 4), ("m", 8, 13), ("m", 258, 8), ("m", 258, 130), ("m", 4, 140)] + tail,
    }
    for name, toks in scenes.items():
        assert any(is_slow(t, llens, dlens) for t in toks), name
        for phase in (0, 1, 31, 62, 63):
            out.append(make("f", "slow: %s phase %d" % (name, phase), [stored(rng.randbytes(1600)), ("dyn", L(phase) + toks + L(1), llens, dlens)]))
    # the long code as a block's first symbol, reading the stored block right before it
    for n in (1, 16, 17):
        out.append(make("f", "slow: first symbol behind stored %d" % n, [stored(rng.randbytes(40)), ("dyn", L(3), llens, dlens), stored(rng.randbytes(n)),
                                                                            ("dyn", [("m", 8, 1) if n == 1 else ("m", 4, 16), ("m", 5, 4)] + L(2), llens, dlens)]))
    return out


G_ORDERS = {"A": [("m", 258, 32768), ("m", 3, 32767), ("m", 3, 32768), ("m", 258, 32767)],
            "B": [("m", 3, 32767), ("m", 258, 32768), ("m", 258, 32767), ("m", 3, 32768)]}


def family_g(rng):
    out = []
    for p in POSITIONS:
        for order, code in (("A", "fixed"), ("B", "fixed"), ("A", "dense")):
            out.append(make("g", "window edge at %d %s %s" % (p, order, code), [stored(rng.randbytes(p)), block(code, G_ORDERS[order])]))
    return out


def family_h(rng):
    out = []
    alpha = rng.sample(range(256), 6)
    llens, dlens = slow_codes(alpha)
    L = lambda n, a=alpha: _lits(rng, n, a)
    for code in ("fixed", "dense"):
        a = _alphabet(rng, code)
        out.append(make("h", "twin of a: self-overlap d8 %s" % code, [block(code, L(7, a) + [("m", 20, 8)] + L(3, a))]))
        toks = L(1, a) + _chain_tokens(rng, "deep", 3, 12, 100, 17, 1)
        n = 17 + sum(t[1] for t in toks[1:])
        out.append(make("h", "twin of b: chain %s" % code, [stored(rng.randbytes(16)), block(code, toks + [("m", 5, n + 1)] + L(3, a))]))
        out.append(make("h", "twin of e: behind stored 17 %s" % code, [fixed(L(16, range(256))), stored(rng.randbytes(17)),
                                                                         block(code, [("m", 5, 34)] + L(3, a))]))
        out.append(make("h", "twin of e: round before %s" % code, [block(code, L(BATCH, a) + [("m", 3, 65)] + L(2, a))]))
    # on the sequential path: a long length code with a short distance code, and long distance codes
    out.append(make("h", "twin of f: long length code", [("dyn", L(3) + [("m", 4, 4)] + L(2), llens, dlens)]))
    out.append(make("h", "twin of f: long distance code 2", [("dyn", L(1) + [("m", 5, 2)] + L(2), llens, dlens)]))
    out.append(make("h", "twin of f: long distance code 17", [("dyn", L(12) + [("m", 4, 4), ("m", 10, 17)] + L(2), llens, dlens)]))
    out.append(make("h", "twin of f: behind valid slow symbols", [stored(rng.randbytes(5)), ("dyn", L(3) + [("m", 4, 4), ("m", 8, 7), ("m", 13, 21)] + L(2), llens, dlens)]))
    out.append(make("h", "twin of g: distance 32768 at 32767", [stored(rng.randbytes(32767)), fixed(G_ORDERS["A"])]))
    out.append(make("h", "twin of g: distance 32767 at 32766", [stored(rng.randbytes(32766)), fixed(G_ORDERS["B"])]))
    out.append(make("h", "twin of g: distance 32768 at 32767 dense", [stored(rng.randbytes(32767)), dense([("m", 258, 32768), 65])]))
    return out


def family_cap(rng):
    out = []
    for code in ("fixed", "dense"):
        a = _alphabet(rng, code)
        for n in (300, 1500):
            out.append(make("cap", "ends in a 258 match %d %s" % (n, code), [stored(rng.randbytes(n)), block(code, _lits(rng, 40, a) + [("m", 258, 100)])]))
            out.append(make("cap", "ends in a literal %d %s" % (n, code), [stored(rng.randbytes(n)), block(code, [("m", 258, 100)] + _lits(rng, 40, a))]))
    lits = lambda n: _lits(rng, n, range(256))

    def fill(n):        # n bytes that compress (the chunk form takes payloads of at most 65 535 bytes)
        return [stored(rng.randbytes(300)), fixed([("m", 258, 300)] * ((n - 300) // 258) + lits((n - 300) % 258))]
    out.append(make("cap", "65535 by a 258 match", fill(CHUNK - 268) + [fixed(lits(10) + [("m", 258, 500)])]))
    out.append(make("cap", "65536 by a 258 match", fill(CHUNK - 267) + [fixed(lits(10) + [("m", 258, 500)])]))
    out.append(make("cap", "a literal at 65535", fill(CHUNK - 5) + [fixed(lits(6))]))
    return out


# ---- preconditions ----------------------------------------------------------------------------------------------------------

def chase_depth(case, bi, first):
    """Owner lookups a byte-wise copy makes below the deepest byte of the batch of BATCH symbols that starts at token `first` of block
    bi, counting only chases that end on a literal of the batch; and the batch's bytes."""
    syms = [s for s in symbols(case.blocks)[1] if s[0] == bi and first <= s[1] < first + BATCH]
    start, end = syms[0][3], syms[-1][3] + syms[-1][4]
    owner = {}
    for s in syms:
        for p in range(s[3], s[3] + s[4]):
            owner[p] = s
    hops = {}                                   # position -> lookups behind it down to a literal, or None (leaves the batch)
    for p in range(start, end):
        _, _, t, pos, n = owner[p]
        if isinstance(t, int):
            hops[p] = 0
            continue
        src = pos - t[2] + (p - pos) % t[2]
        hops[p] = None if src < start or hops[src] is None else hops[src] + 1
    return max((h for h in hops.values() if h is not None), default=0), end - start


def check(cases):
    by = {}
    for c in cases:
        by.setdefault(c.family, []).append(c)
    assert set(by) == {"a", "b", "c", "d", "e", "f", "g", "h", "cap"}, sorted(by)
    assert len({c.name for c in cases}) == len(cases)
    for i, c in enumerate(cases):
        if i % 16 == 0:
            assert c.piece() == encode(c.blocks, marker=True)[0], c.name
        if c.valid:
            d = zlib.decompressobj(-15)
            assert d.decompress(c.body) == c.data and d.eof and not d.unused_data, c.name
            d = zlib.decompressobj(-15)                                       # the piece form: the same bytes, not the end of a stream
            assert d.decompress(c.piece()) == c.data and not d.eof and c.piece().endswith(b"\x00\x00\xff\xff"), c.name
        else:
            # zlib.decompressobj refuses the stream; it drops what it decoded in the call that fails, so the bytes in front of the
            # refused symbol are counted on the z_stream of the same libz (stream_ref)
            assert c.family == "h", c.name
            try:
                zlib.decompressobj(-15).decompress(c.body)
                raise AssertionError("libz accepts " + c.name)
            except zlib.error as e:
                assert "too far back" in str(e), (c.name, str(e))
            st, got = stream_ref.reference(stream_ref.RAW, c.body, 1 << 20)
            assert st == stream_ref.DATA_ERROR and got == c.data, (c.name, st, len(got), len(c.data))
    # a: every listed distance overlaps itself (distance < length; at 258 and 259 the longest match there is)
    for d in SELF_OVERLAP_DISTANCES:
        assert any(not isinstance(t, int) and t[2] == d and t[1] >= min(d + 1, 258) for c in by["a"] for b in c.blocks if b[0] != "stored" for t in b[1]), d
    # b: a batch whose chase runs through all its symbols down to a literal; 64-symbol runs under and over OWN_CAP bytes
    deep, small, large = 0, False, False
    for c in by["b"]:
        if " deep " not in c.name:
            continue
        phase = int(c.name.rsplit(" ", 1)[1])
        if phase == 0:
            continue
        hops, nbytes = chase_depth(c, 1, phase - 1)
        deep = max(deep, hops)
        if " short " in c.name:
            assert nbytes < OWN_CAP, (c.name, nbytes)
            small = True
        else:
            assert nbytes > OWN_CAP, (c.name, nbytes)
            large = True
    assert deep >= BATCH - 1 and small and large, (deep, small, large)
    # b, sources in order: in the dense code all 56 symbols start inside one window, so they are one batch
    orders = [c for c in by["b"] if c.name.startswith("order ") and c.name.endswith(" dense")]
    assert len(orders) == 3
    for c in orders:
        b = c.blocks[0]
        ll, dl = code_lengths(b)
        assert len(b[1]) < BATCH and sum(token_bits(t, ll, dl) for t in b[1][:-1]) < WINDOW, c.name
    # b, all matches 3 bytes: 64 symbols do fit a window (every symbol starts within it), so a round ends at a full batch
    for c in by["b"]:
        if " short 3-3 deep dense " in c.name:
            ll, dl = code_lengths(c.blocks[1])
            assert max(token_bits(t, ll, dl) for t in c.blocks[1][1]) * (BATCH - 1) < WINDOW, c.name
    # c: every size, each block one round
    sizes = set()
    for c in by["c"]:
        b = c.blocks[-1]
        ll, dl = code_lengths(b)
        assert len(b[1]) <= 60 and sum(token_bits(t, ll, dl) for t in b[1]) + ll[256] <= 400, c.name
        sizes.add(len(c.data) - 300)
    assert sizes >= set(range(1000, 1051)) and min(sizes) < 1000 - 16 and max(sizes) > 1050 + 16, sorted(sizes)
    # d: the first pattern's match stands at every index of a dense run of full batches
    idx = set()
    for c in by["d"]:
        if " dense " in c.name:
            b = c.blocks[-1]
            ll, dl = code_lengths(b)
            k = next(i for i, t in enumerate(b[1]) if not isinstance(t, int))
            assert max(token_bits(t, ll, dl) for t in b[1][:k]) * (BATCH - 1) < WINDOW and b[1][k][2] < b[1][k][1], c.name
            idx.add(k % BATCH)
    assert idx == set(range(BATCH)), sorted(idx)
    # e: a match as symbol 64 of a dense block, for every distance 1..64
    firsts = set()
    for c in by["e"]:
        if c.name.startswith("round before") and c.name.endswith("dense"):
            b = c.blocks[1]
            ll, dl = code_lengths(b)
            assert max(token_bits(t, ll, dl) for t in b[1][:BATCH]) * (BATCH - 1) < WINDOW and not isinstance(b[1][BATCH], int), c.name
            firsts.add(b[1][BATCH][2])
    assert firsts == set(range(1, 65)), sorted(firsts)
    # f: long-code matches with the length below and above the distance, each case with a fast match behind one
    below = above = 0
    for c in by["f"]:
        b = c.blocks[-1]
        slow = [i for i, t in enumerate(b[1]) if is_slow(t, b[2], b[3])]
        assert slow and any(not isinstance(t, int) and not is_slow(t, b[2], b[3]) for t in b[1][slow[-1] + 1:]), c.name
        below += sum(b[1][i][1] < b[1][i][2] for i in slow)
        above += sum(b[1][i][1] > b[1][i][2] for i in slow)
    assert below and above
    # g: every position
    assert {len(c.blocks[-2][1]) + CHUNK * (len(c.blocks) - 2) for c in by["g"]} == set(POSITIONS)
    # h: twins of five families, on both paths
    assert {c.name.split(":")[0] for c in by["h"]} == {"twin of " + f for f in "abefg"}
    refused = []
    for c in by["h"]:
        pos, bi, ti = symbols(c.blocks)[2]
        t = c.blocks[bi][1][ti]
        assert t[2] == pos + 1 == len(c.data) + 1, c.name
        refused.append(is_slow(t, *code_lengths(c.blocks[bi])))
    assert any(refused) and not all(refused)


def corpus(seed=2028):
    rng = random.Random(seed)
    cases = []
    for fam in (family_a, family_b, family_c, family_d, family_e, family_f, family_g, family_h, family_cap):
        cases += fam(rng)
    check(cases)
    return cases


def summary(cases):
    """{family: (cases, decoded bytes)}"""
    out = {}
    for c in cases:
        n, b = out.get(c.family, (0, 0))
        out[c.family] = (n + 1, b + len(c.data))
    return out
