"""A seeded DEFLATE / zlib bit writer and the inflate conformance corpus built with it.  Test infrastructure only.

The writer puts stored, fixed and dynamic blocks together from explicit symbol lists, with explicit code lengths and an explicit
run-length encoding of those lengths, so that streams no zlib deflate writes -- 15-bit literal codes, a lone or missing distance code,
a 16 that repeats a zero or crosses from the literal into the distance lengths, minimal HCLEN, 7-bit code-length codes, invalid
symbols, bad headers -- can be built on purpose.  Every stream records whether it is valid and, if so, the bytes it encodes.

conformance_corpus(seed) -> [Case]: payloads of at most 65 535 bytes in five groups:
  a  zlib itself: every strategy, level, memLevel, windowBits and flush mode; whole, cut, one bit flipped
  b  hand-built valid streams
  c  hand-built invalid streams: one per verdict of inflate_dyn_begin / inflate_dyn_lengths / inflate_table_ok, per invalid symbol
  d  size edges: exactly 65 535 bytes ending in a 258 match, 65 536 and more, distance 32 768, distance = output so far (+1)
  e  damage: every cut of small multi-block streams, single-bit flips across headers and bodies
"""
import heapq
import random
import zlib
from dataclasses import dataclass
from typing import Optional

CHUNK = 65535

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [i // 2 for i in range(2, 28)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 30


def length_code(n):
    """258 -> code 285 (not 284 + 31)."""
    assert 3 <= n <= 258
    if n == 258:
        return 285, 0, 0
    c = max(i for i in range(28) if LEN_BASE[i] <= n)
    return 257 + c, LEN_EXTRA[c], n - LEN_BASE[c]


def dist_code(d):
    assert 1 <= d <= 32768
    c = max(i for i in range(30) if DIST_BASE[i] <= d)
    return c, DIST_EXTRA[c], d - DIST_BASE[c]


def canonical(lens):
    """RFC 1951 3.2.2: the code of every symbol with a length (None for the others); over-subscribed lengths still get codes."""
    mx = max(lens) if lens else 0
    count = [0] * (max(mx, 15) + 1)
    for l in lens:
        count[l] += 1
    count[0] = 0
    code, nxt = 0, [0] * (len(count) + 1)
    for b in range(1, len(count)):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = []
    for l in lens:
        if l:
            out.append(nxt[l])
            nxt[l] += 1
        else:
            out.append(None)
    return out


def kraft(lens):
    """0 complete, > 0 incomplete, < 0 over-subscribed (in units of 2^-15)."""
    return (1 << 15) - sum(1 << (15 - l) for l in lens if l)


class BitWriter:
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, v, k):
        assert 0 <= v < (1 << k) or k == 0
        self.acc |= v << self.n
        self.n += k

    def put_code(self, code, k):            # Huffman codes go most significant bit first
        self.put(int(format(code, "0%db" % k)[::-1], 2) if k else 0, k)

    def align(self):
        self.n = (self.n + 7) & ~7

    def bytes(self):
        return self.acc.to_bytes((self.n + 7) // 8, "little")


# ---- Huffman code lengths -----------------------------------------------------------------------------------------------

def split_tree(rng, nleaves, maxbits, deep=False):
    """Depths of a complete prefix code with `nleaves` leaves, none deeper than maxbits: split random leaves of a tree (deep: always
    split the deepest leaf that may be split, which makes the longest codes)."""
    assert 2 <= nleaves <= 1 << maxbits
    leaves = [1, 1]
    while len(leaves) < nleaves:
        idx = [i for i, d in enumerate(leaves) if d < maxbits]
        if deep:
            m = max(leaves[i] for i in idx)
            i = rng.choice([i for i in idx if leaves[i] == m])
        else:
            i = rng.choice(idx)
        d = leaves.pop(i)
        leaves += [d + 1, d + 1]
    return leaves


def huffman_lengths(freq, maxbits):
    """Length-limited code lengths for the symbols with freq > 0 (plain Huffman; too deep -> a balanced split tree).  A single used
    symbol gets length 1 and a partner so that the code is complete."""
    used = [s for s, f in enumerate(freq) if f]
    lens = [0] * len(freq)
    if not used:
        return lens
    if len(used) == 1:
        used.append(0 if used[0] else 1)
    heap = [(freq[s] or 1, i, [s]) for i, s in enumerate(used)]
    heapq.heapify(heap)
    k = len(heap)
    while len(heap) > 1:
        f1, _, a = heapq.heappop(heap)
        f2, _, b = heapq.heappop(heap)
        for s in a + b:
            lens[s] += 1
        heapq.heappush(heap, (f1 + f2, k, a + b))
        k += 1
    if max(lens) > maxbits:
        depths = sorted(split_tree(random.Random(len(used)), len(used), maxbits))
        order = sorted(used, key=lambda s: -freq[s])
        for s, d in zip(order, depths):
            lens[s] = d
    return lens


def assign(rng, symbols, depths, n):
    lens = [0] * n
    symbols = list(symbols)
    rng.shuffle(symbols)
    for s, d in zip(symbols, depths):
        lens[s] = d
    return lens


def random_code(rng, n, nsyms, maxbits, must=(), deep=False):
    """A random complete code over nsyms of the n symbols (those in `must` included)."""
    pool = [s for s in range(n) if s not in must]
    syms = list(must) + rng.sample(pool, nsyms - len(must))
    return assign(rng, syms, split_tree(rng, nsyms, maxbits, deep), n)


# ---- run-length encoding of the code lengths (symbols 16 / 17 / 18) -----------------------------------------------------

def rle_plain(lens):
    """Literal lengths only."""
    return [(l, 0) for l in lens]


def rle_random(rng, lens, p=0.7):
    """A random valid encoding: at every place a repeat is taken with probability p when one fits.  16 repeats whatever length
    was written last -- a zero written by a 17 / 18 too, and across the literal / distance boundary."""
    out, i, n = [], 0, len(lens)
    while i < n:
        same = 0
        if i:
            while i + same < n and lens[i + same] == lens[i - 1] and same < 6:
                same += 1
        zeros = 0
        while i + zeros < n and lens[i + zeros] == 0 and zeros < 138:
            zeros += 1
        opts = []
        if same >= 3:
            opts.append(16)
        if zeros >= 3:
            opts.append(17)
        if zeros >= 11:
            opts.append(18)
        if opts and rng.random() < p:
            s = rng.choice(opts)
            if s == 16:
                r = rng.randint(3, same)
                out.append((16, r - 3))
            elif s == 17:
                r = rng.randint(3, min(zeros, 10))
                out.append((17, r - 3))
            else:
                r = rng.randint(11, zeros)
                out.append((18, r - 11))
            i += r
        else:
            out.append((lens[i], 0))
            i += 1
    return out


def rle_expand(rle):
    out = []
    for s, x in rle:
        if s < 16:
            out.append(s)
        elif s == 16:
            out += [out[-1] if out else None] * (3 + x)
        else:
            out += [0] * ((3 if s == 17 else 11) + x)
    return out


# ---- blocks and streams --------------------------------------------------------------------------------------------------

class Stream:
    """A zlib stream (or a raw DEFLATE body: header=None) written block by block.  .data follows what a decoder must produce;
    .valid drops to False whenever something invalid is written on purpose."""

    def __init__(self, header=(0x78, 0x9C)):
        self.w = BitWriter()
        self.data = bytearray()
        self.valid = True
        self.header = header
        if header is not None:
            self.w.put(header[0], 8)
            self.w.put(header[1], 8)

    def _tokens(self, tokens, lcodes, llens, dcodes, dlens, eob):
        w = self.w

        def lit(sym):
            assert llens[sym], "symbol %d has no code" % sym
            w.put_code(lcodes[sym], llens[sym])

        def dist(sym):
            assert dlens[sym], "distance code %d has no code" % sym
            w.put_code(dcodes[sym], dlens[sym])

        for t in tokens:
            if isinstance(t, int):
                lit(t)
                self.data.append(t)
            elif t[0] == "m":                      # ("m", length, distance)
                _, n, d = t
                c, xb, xv = length_code(n)
                lit(c)
                w.put(xv, xb)
                c, xb, xv = dist_code(d)
                dist(c)
                w.put(xv, xb)
                if d > len(self.data):
                    self.valid = False
                for _ in range(n):
                    self.data.append(self.data[-d] if d <= len(self.data) else 0)
            elif t[0] == "L":                      # ("L", symbol, extra value, extra bits): a raw literal/length symbol
                lit(t[1])
                w.put(t[2], t[3])
            elif t[0] == "D":                      # ("D", symbol, extra value, extra bits): a raw distance symbol
                dist(t[1])
                w.put(t[2], t[3])
            elif t[0] == "bits":                   # ("bits", value, count): anything at all
                w.put(t[1], t[2])
            else:
                raise ValueError(t)
        if eob:
            lit(256)

    def stored(self, data, final=False, len_=None, nlen=None):
        w = self.w
        w.put(int(final), 1)
        w.put(0, 2)
        w.align()
        n = len(data) if len_ is None else len_
        w.put(n, 16)
        w.put((n ^ 0xFFFF) if nlen is None else nlen, 16)
        for b in data:
            w.put(b, 8)
        self.data += data
        if n != len(data) or (nlen is not None and nlen != n ^ 0xFFFF):
            self.valid = False
        return self

    def fixed(self, tokens, final=False, eob=True):
        self.w.put(int(final), 1)
        self.w.put(1, 2)
        self._tokens(tokens, canonical(FIXED_LIT), FIXED_LIT, canonical(FIXED_DIST + [5, 5]), FIXED_DIST + [5, 5], eob)
        return self

    def dynamic(self, tokens, llens, dlens, final=False, rle=None, cl=None, hlit=None, hdist=None, hclen=None, eob=True):
        """llens / dlens: the literal/length and distance code lengths (trailing zeros are dropped unless hlit / hdist say
        otherwise); rle: the (symbol, extra) sequence of the code-length symbols, default literal lengths; cl: the code-length
        code's 19 lengths, default Huffman (<= 7 bits) on the symbols used; hclen: lengths of cl sent, default the fewest."""
        w = self.w
        llens = list(llens) + [0] * (286 - len(llens))
        dlens = list(dlens) + [0] * (30 - len(dlens))
        nl = hlit + 257 if hlit is not None else max(257, max((i + 1 for i, l in enumerate(llens) if l), default=0))
        nd = hdist + 1 if hdist is not None else max(1, max((i + 1 for i, l in enumerate(dlens) if l), default=0))
        both = (llens + [0] * 2)[:nl] + (dlens + [0] * 2)[:nd]
        if rle is None:
            rle = rle_plain(both)
        freq = [0] * 19
        for s, _ in rle:
            freq[s] += 1
        if cl is None:
            cl = huffman_lengths(freq, 7)
        nc = hclen + 4 if hclen is not None else max(4, max(i + 1 for i, s in enumerate(CL_ORDER) if cl[s]))
        w.put(1 if final else 0, 1)
        w.put(2, 2)
        w.put(nl - 257, 5)
        w.put(nd - 1, 5)
        w.put(nc - 4, 4)
        for i in range(nc):
            w.put(cl[CL_ORDER[i]], 3)
        ccodes = canonical(cl)
        for s, x in rle:
            w.put_code(ccodes[s], cl[s])
            if s >= 16:
                w.put(x, {16: 2, 17: 3, 18: 7}[s])
        if any(cl[CL_ORDER[i]] for i in range(nc, 19)) or rle_expand(rle) != both:
            self.valid = False
        self._tokens(tokens, canonical(llens[:nl] + [0] * (288 - nl)), llens[:nl] + [0] * (288 - nl),
                     canonical(dlens[:nd] + [0] * (32 - nd)), dlens[:nd] + [0] * (32 - nd), eob)
        return self

    def payload(self, trailer=True, junk=b""):
        b = self.w.bytes()
        if trailer and self.header is not None:
            b += zlib.adler32(bytes(self.data)).to_bytes(4, "big")
        return b + junk

    def body(self):
        b = self.w.bytes()
        return b[2:] if self.header is not None else b


def zlib_header(cinfo=7, fdict=False, level=2, fix=True):
    cmf = cinfo << 4 | 8
    flg = level << 6 | (0x20 if fdict else 0)
    if fix:
        flg += (31 - ((cmf << 8) + flg) % 31) % 31
    return cmf, flg


@dataclass
class Case:
    group: str
    name: str
    payload: bytes
    valid: Optional[bool] = None         # hand-built streams: what the writer says
    data: Optional[bytes] = None         # valid streams: the bytes they encode
    body: Optional[bytes] = None         # the raw DEFLATE body (payload without header / trailer), for BGZF


# ---- data and symbol helpers ----------------------------------------------------------------------------------------------

def text(rng, n):
    words = [bytes(rng.choice(b"abcdefghijklmnopqrstuvwxyz") for _ in range(rng.randint(2, 8))) for _ in range(300)]
    out = bytearray()
    while len(out) < n:
        out += words[min(int(rng.paretovariate(1.0)) - 1, 299)] + b" "
    return bytes(out[:n])


def mixed(rng, n):
    """Text with runs and random stretches: matches of every length and distance."""
    out = bytearray()
    while len(out) < n:
        k = rng.random()
        if k < 0.6:
            out += text(rng, rng.randint(10, 3000))
        elif k < 0.8:
            out += bytes([rng.randrange(256)]) * rng.randint(1, 700)
        else:
            out += rng.randbytes(rng.randint(1, 2000))
    return bytes(out[:n])


def tokens_for(rng, n, lit_syms, len_syms, dist_syms, start=0):
    """About n output bytes of random tokens that use only the given literals, length codes and distance codes."""
    toks, produced = [], start
    lit_syms, len_syms, dist_syms = list(lit_syms), list(len_syms), list(dist_syms)
    while produced < start + n:
        if len_syms and dist_syms and produced > 0 and rng.random() < 0.4:
            lc = rng.choice(len_syms) - 257
            ln = 258 if lc == 28 else LEN_BASE[lc] + rng.randrange((1 << LEN_EXTRA[lc]) - (lc == 27))   # (284 + 31 is 258: code 285)
            fits = [d for d in dist_syms if DIST_BASE[d] <= produced]
            if fits:
                dc = rng.choice(fits)
                d = min(produced, DIST_BASE[dc] + rng.randrange(1 << DIST_EXTRA[dc]))
                if dist_code(d)[0] == dc:
                    toks.append(("m", ln, d))
                    produced += ln
                    continue
        toks.append(rng.choice(lit_syms))
        produced += 1
    return toks


def random_dynamic(rng, s, n, maxbits=15, deep=False, p=0.7, final=False):
    """A dynamic block with random complete codes, random symbols of those codes and a random run-length encoding."""
    nl = rng.randint(2, 286)
    llens = random_code(rng, 286, nl, maxbits, must=(256,), deep=deep)
    nd = rng.randint(1, 30)
    dlens = random_code(rng, 30, nd, maxbits, deep=deep) if nd > 1 else [0] * 30
    if nd == 1:
        dlens[rng.randrange(30)] = 1
    lit = [i for i in range(256) if llens[i]] or [None]
    lens_ = [i for i in range(257, 286) if llens[i]]
    dists = [i for i in range(30) if dlens[i]]
    if lit == [None]:
        lit = []
    if not lit:                                             # no literals: the block can only start where output exists
        toks = tokens_for(rng, n, [], lens_, dists, len(s.data)) if s.data and lens_ else []
    else:
        toks = tokens_for(rng, n, lit, lens_, dists, len(s.data))
    nlt = max(257, max(i + 1 for i in range(286) if llens[i]))
    ndt = max(1, max((i + 1 for i in range(30) if dlens[i]), default=0))
    both = llens[:nlt] + dlens[:ndt]
    s.dynamic(toks, llens, dlens, final=final, rle=rle_random(rng, both, p))
    return s


# ---- the corpus ------------------------------------------------------------------------------------------------------------

STRATEGIES = [zlib.Z_DEFAULT_STRATEGY, zlib.Z_FILTERED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE, zlib.Z_FIXED]
FLUSHES = [None, zlib.Z_SYNC_FLUSH, zlib.Z_FULL_FLUSH, zlib.Z_PARTIAL_FLUSH, zlib.Z_BLOCK]


def zlib_stream(rng, data, level, mem, wbits, strategy, flush):
    co = zlib.compressobj(level, zlib.DEFLATED, wbits, mem, strategy)
    out = bytearray()
    if flush is None:
        out += co.compress(data)
    else:
        cuts = sorted(rng.sample(range(len(data) + 1), min(len(data) + 1, rng.randint(1, 40))))
        prev = 0
        for c in cuts:
            out += co.compress(data[prev:c])
            out += co.flush(flush)
            if rng.random() < 0.2:
                out += co.flush(flush)             # a second flush in a row: an empty stored block / an empty block
            prev = c
        out += co.compress(data[prev:])
    out += co.flush(zlib.Z_FINISH)
    return bytes(out)


def group_a(seed, count=1500):
    rng = random.Random(seed)
    cases = []
    for i in range(count):
        strategy = STRATEGIES[i % 5]
        flush = FLUSHES[(i // 5) % 5]
        level = rng.choice([0, 1, 2, 3, 4, 5, 6, 7, 8, 9]) if strategy == zlib.Z_DEFAULT_STRATEGY else rng.randint(1, 9)
        mem = rng.choice([1, 8, 9])
        wbits = rng.choice([9, 12, 15])
        n = rng.choice([0, 1, 2, 3, 100, rng.randint(1, 4000), rng.randint(1, 65535), rng.randint(30000, 65535), 65535])
        kind = rng.random()
        data = text(rng, n) if kind < 0.5 else mixed(rng, n) if kind < 0.85 else rng.randbytes(n)
        z = zlib_stream(rng, data, level, mem, wbits, strategy, flush)
        tag = "zlib s%d l%d m%d w%d f%s n%d" % (strategy, level, mem, wbits, flush, n)
        if len(z) <= CHUNK:
            cases.append(Case("a", tag, z, True, data, z[2:-4]))
        v = rng.randrange(3)
        if v == 0 and len(z) > 2:
            k = rng.randrange(2, min(len(z), CHUNK + 1))
            cases.append(Case("a", tag + " cut %d" % k, z[:k]))
        elif v == 1:
            b = bytearray(z[:CHUNK])
            bit = rng.randrange(16, max(17, 8 * len(b)))
            if bit >> 3 < len(b):
                b[bit >> 3] ^= 1 << (bit & 7)
                cases.append(Case("a", tag + " flip %d" % bit, bytes(b)))
    return cases


def _valid(name, s, group="b", junk=b""):
    return Case(group, name, s.payload(junk=junk), s.valid, bytes(s.data), s.body())


def _invalid(name, s, group="c", trailer=True):
    assert not s.valid or name
    return Case(group, name, s.payload(trailer=trailer), False, None, s.body())


def group_b(seed):
    rng = random.Random(seed + 1)
    out = []
    # random complete codes up to 15 bits with random run-length encodings, one to several blocks a stream
    for i in range(120):
        s = Stream()
        for b in range(1 + i % 4):
            random_dynamic(rng, s, rng.choice([0, 1, 50, 700, 5000]), deep=i % 3 == 0, p=[0.3, 0.7, 1.0][i % 3], final=b == i % 4)
        out.append(_valid("random dynamic %d" % i, s))
    # literal codes exactly 10 bits (the literal fast table's width) and 11 bits; distance codes exactly 8 and 9 bits
    for lb, db in ((10, 8), (11, 9), (15, 15), (9, 7)):
        llens = [0] * 286
        syms = list(range(0, 256, 3)) + [256, 257, 265, 284, 285]
        depths = sorted(split_tree(rng, len(syms), lb, deep=True))
        for sm, d in zip(syms[::-1], depths[::-1]):
            llens[sm] = d
        llens[256] = lb                              # end-of-block has a longest code
        if kraft(llens) != 0:
            llens = assign(rng, syms, split_tree(rng, len(syms), lb, deep=True), 286)
        dsyms = list(range(30))
        dlens = assign(rng, dsyms, split_tree(rng, 30, db, deep=True), 30)
        s = Stream()
        s.dynamic(tokens_for(rng, 20000, [i for i in range(256) if llens[i]], [i for i in range(257, 286) if llens[i]],
                             [i for i in range(30) if dlens[i]]), llens, dlens, final=True, rle=rle_random(rng, llens + dlens))
        out.append(_valid("max code %d / %d bits" % (lb, db), s))
    # 15-bit literal codes on a skewed alphabet: every long code used many times
    llens = random_code(rng, 286, 200, 15, must=(256, 257, 285), deep=True)
    s = Stream()
    lits = [i for i in range(256) if llens[i]]
    s.dynamic(tokens_for(rng, 30000, lits, [257, 285], []), llens, [0] * 30, final=True)
    out.append(_valid("15-bit literal codes, no distance codes", s))
    # a single distance code of length 1 (incomplete, legal), used
    for code in (0, 5, 29):
        llens = random_code(rng, 286, 60, 12, must=(256, 258, 97, 98))
        dlens = [0] * 30
        dlens[code] = 1
        s = Stream()
        toks = [97, 98] * (DIST_BASE[code] + 2)
        d = DIST_BASE[code]
        toks += [("m", 4, d), ("m", 4, d)]
        s.dynamic(toks, llens, dlens, final=True, rle=rle_random(rng, llens[:257 + 2] + dlens))
        out.append(_valid("single 1-bit distance code %d" % code, s))
    # no distance codes at all: HDIST = 0 with a zero length, literals only
    llens = random_code(rng, 286, 100, 9, must=(256,))
    s = Stream()
    s.dynamic(tokens_for(rng, 3000, [i for i in range(256) if llens[i]], [], []), llens, [0], final=True)
    out.append(_valid("empty distance tree", s))
    # a single literal/length code of length 1: only end-of-block
    llens = [0] * 286
    llens[256] = 1
    s = Stream().stored(b"abc")
    s.dynamic([], llens, [0], final=True)
    out.append(_valid("only end-of-block, one 1-bit code", s))
    # length code 284 with extra 31: zlib accepts it as 258
    for x in (30, 31):
        s = Stream().fixed([65, 66, 67, ("L", 284, x, 5), ("D", 0, 0, 0)], final=True)
        s.data += s.data[-1:] * (258 if x == 31 else 257)
        out.append(_valid("284+%d" % x, s))
    llens = random_code(rng, 286, 30, 8, must=(256, 284, 65))
    s = Stream().dynamic([65] * 4 + [("L", 284, 31, 5), ("D", 3, 0, 0)] * 3, llens, [0, 0, 0, 1], final=True)
    s.data = bytearray(b"A" * (4 + 3 * 258))
    out.append(_valid("284+31 dynamic", s))
    # code-length encodings: 16 after 17 and after 18 (repeating a zero), 16 across the literal/distance boundary, an 18 run of 138
    llens = [0] * 286
    for i in list(range(64, 77)) + [256, 257, 258]:
        llens[i] = 4
    dlens = [4] * 16
    rle = [(18, 53), (4, 0), (16, 3), (16, 3),                  # 0..63 zero, 64..76 four
           (17, 7), (16, 3),                                    # 77..86 by a 17, 87..92 by a 16 repeating its zero
           (18, 127), (16, 3), (18, 8),                         # 93..230 by an 18 of 138, 231..236 by a 16, 237..255
           (4, 0), (16, 3), (16, 3), (16, 3)]                   # 256 .. 258 and on through the 16 distance lengths
    assert rle_expand(rle) == llens[:259] + dlens
    s = Stream().dynamic(tokens_for(rng, 4000, range(64, 77), [257, 258], range(16)), llens, dlens, final=True, rle=rle)
    out.append(_valid("16 after 17 and 18, 16 across the boundary, 18 run of 138", s))
    # an 18 run that crosses from the literal into the distance lengths
    llens = [0] * 286
    for i in (0, 1, 2, 256):
        llens[i] = 2
    dlens = [1] + [0] * 28 + [1]
    rle = [(2, 0)] * 3 + [(18, 127), (18, 253 - 138 - 11), (2, 0), (1, 0), (18, 28 - 11), (1, 0)]
    assert rle_expand(rle) == llens[:257] + dlens
    s = Stream().dynamic([0, 1, 2, 2, 1, 0] * 50, llens, dlens, final=True, rle=rle)
    out.append(_valid("18 runs of 138 and into the distance lengths", s))
    rle = [(2, 0)] * 3 + [(18, 127), (18, 253 - 138 - 11), (2, 0), (1, 0), (18, 30 - 11)]
    assert rle_expand(rle)[:257] == llens[:257]
    s = Stream().dynamic([0, 1, 2], llens, [1], final=True, rle=rle, hdist=29)
    s.valid = False
    out.append(_invalid("18 run past HLIT + HDIST by one", s))
    # the fewest code-length codes a valid block can send: HCLEN = 1 (16, 17, 18, 0 and 8)
    llens = [8] * 255 + [0, 8] + [0] * 29
    assert kraft(llens) == 0
    s = Stream().dynamic(tokens_for(rng, 2000, range(255), [], []), llens, [0], final=True, rle=rle_random(rng, llens[:257] + [0], 1.0))
    out.append(_valid("HCLEN 5 codes", s))
    # 7-bit code-length codes (a deep code-length code)
    for i in range(6):
        llens = random_code(rng, 286, rng.randint(30, 286), 15, must=(256,))
        dlens = random_code(rng, 30, rng.randint(2, 30), 15)
        nlt = max(257, max(k + 1 for k in range(286) if llens[k]))
        ndt = max(k + 1 for k in range(30) if dlens[k])
        rle = rle_random(rng, llens[:nlt] + dlens[:ndt])
        used = sorted({sm for sm, _ in rle})
        cl = [0] * 19
        for sm, d in zip(used, sorted(split_tree(rng, len(used), 7, deep=True), reverse=True)):
            cl[sm] = d
        s = Stream().dynamic(tokens_for(rng, 1500, [k for k in range(256) if llens[k]], [k for k in range(257, 286) if llens[k]],
                                        [k for k in range(30) if dlens[k]]), llens, dlens, final=True, rle=rle, cl=cl, hclen=15)
        out.append(_valid("7-bit code-length code %d" % i, s))
    # stored blocks: LEN = 0 between Huffman blocks, many short ones, one ending at the payload's last byte
    s = Stream().stored(b"").fixed([72, 105]).stored(b"").stored(b"").fixed([("m", 3, 1)]).stored(bytes(range(40)), final=True)
    out.append(_valid("stored LEN = 0 between fixed blocks", s))
    s = Stream()
    for i in range(400):
        k = rng.choice([0, 0, 1, 3, 17, 200])
        s.stored(rng.randbytes(k))
        if i % 5 == 0:
            s.fixed(tokens_for(rng, rng.randint(0, 40), range(256), range(257, 286), range(30), len(s.data)))
        if i % 9 == 0:
            random_dynamic(rng, s, rng.randint(0, 300), maxbits=12)
    s.stored(b"", final=True)
    out.append(_valid("400 stored blocks between Huffman blocks", s))
    s = Stream()
    for i in range(700):                         # hundreds of tiny fixed blocks
        s.fixed(tokens_for(rng, rng.randint(0, 30), range(256), range(257, 286), range(30), len(s.data)))
    s.fixed([], final=True)
    out.append(_valid("700 fixed blocks", s))
    # block headers at every bit offset around the kernel's 1 KiB ring refills: thousands of short fixed and dynamic blocks
    for kind in ("fixed", "dynamic"):
        s = Stream()
        while s.w.n < 8 * 9000:
            if kind == "fixed":
                s.fixed([rng.randrange(256) for _ in range(rng.randint(0, 2))])
            else:
                random_dynamic(rng, s, rng.randint(0, 30), maxbits=10)
        s.fixed([], final=True)
        out.append(_valid("block headers across 1 KiB boundaries (%s)" % kind, s))
    # BFINAL in the middle: bytes after the trailer are junk
    s = Stream().fixed([1, 2, 3, ("m", 20, 3)], final=True)
    out.append(_valid("final block then junk", s, junk=b"\x00\xff" + rng.randbytes(30)))
    s = Stream().stored(b"hello", final=True)
    out.append(_valid("final stored block then junk", s, junk=bytes([2, 0xff]) + rng.randbytes(30)))
    # header forms: every window size, every level, a header with FDICT clear and FCHECK right
    for cinfo in range(8):
        h = zlib_header(cinfo=cinfo, level=cinfo % 4)
        s = Stream(header=h).fixed([7, 8, 9, ("m", 50, 2)], final=True)
        out.append(_valid("header cinfo %d" % cinfo, s))
    # the distance one short of and equal to the output so far
    s = Stream().fixed([1, 2, 3, 4, ("m", 10, 4), ("m", 258, 14)], final=True)
    out.append(_valid("distance = output so far", s))
    return out


def group_c(seed):
    """One stream per verdict of the block-header functions and per invalid symbol."""
    rng = random.Random(seed + 2)
    out = []
    good_l = random_code(rng, 286, 40, 9, must=(256, 97, 260))
    good_d = [0] * 30
    good_d[0] = good_d[1] = 1
    pre = [97] * 5

    def dyn(name, **kw):
        s = Stream().fixed(pre)
        args = dict(tokens=[97, ("m", 6, 1), 97], llens=good_l, dlens=good_d, final=True)
        args.update(kw)
        s.dynamic(**args)
        s.valid = False
        out.append(_invalid(name, s))

    # inflate_dyn_begin: HLIT 287 / 288, HDIST 31 / 32, a stream that ends inside the code-length code's lengths
    for hl in (30, 31):
        dyn("HLIT %d" % (hl + 257), hlit=hl, llens=good_l + [0] * 2, tokens=[])
    for hd in (30, 31):
        dyn("HDIST %d" % (hd + 1), hdist=hd, dlens=good_d + [0] * 2, tokens=[])
    s = Stream().fixed(pre).dynamic([97], good_l, good_d, final=True)
    p = s.payload(trailer=False)
    out.append(Case("c", "ends inside HCLEN lengths", p[:len(Stream().fixed(pre).payload(trailer=False)) + 3], False))
    # the code-length code: over-subscribed, incomplete, all zero (invalid in every case)
    cl_over = [0] * 19
    for k in (0, 8, 9, 16, 17, 18):
        cl_over[k] = 2
    dyn("code-length code over-subscribed", cl=cl_over)
    cl_inc = [0] * 19
    for k in range(19):
        cl_inc[k] = 5
    dyn("code-length code incomplete", cl=cl_inc)
    dyn("code-length code all zero", cl=[0] * 19, hclen=0)
    # inflate_dyn_lengths: 16 first, a run past HLIT + HDIST, end-of-block without a length, a code that ends the input
    both = good_l[:261] + good_d[:2]
    dyn("16 with nothing before it", rle=[(16, 0)] + rle_plain(both))
    dyn("18 past HLIT + HDIST", rle=rle_plain(both[:-3]) + [(18, 0)])
    dyn("16 past HLIT + HDIST", rle=rle_plain(both[:-1]) + [(16, 2)])
    l_no_eob = list(good_l)
    l_no_eob[256] = 0
    s = Stream().fixed(pre)
    s.dynamic([97], l_no_eob, good_d, final=True, eob=False)
    s.valid = False
    out.append(_invalid("no code for end-of-block", s))
    # inflate_table_ok: literal/length over-subscribed, incomplete (not a single 1-bit code), distance over / incomplete
    l_over = list(good_l)
    l_over[98] = 1
    dyn("literal/length over-subscribed", llens=l_over, tokens=[])
    l_inc = list(good_l)
    l_inc[97] = 0
    dyn("literal/length incomplete", llens=l_inc, tokens=[])
    l_one = [0] * 286
    l_one[256] = 2
    dyn("literal/length one 2-bit code", llens=l_one, tokens=[])
    dyn("distance over-subscribed", dlens=[1, 1, 1], tokens=[])
    dyn("distance incomplete, two codes", dlens=[1, 2], tokens=[])
    for ln in (2, 3, 15):
        d = [0] * 30
        d[4] = ln
        dyn("distance single code of length %d" % ln, dlens=d, tokens=[])
    # invalid symbols: fixed 286 / 287, fixed distance 30 / 31, a code that is not in an incomplete code, block type 3,
    # a distance too far back, stored LEN / NLEN mismatch
    for sym in (286, 287):
        for tail in (0, 12, 40):
            s = Stream().fixed(pre + [("L", sym, 0, 0), ("bits", 0, tail)], final=True, eob=False)
            out.append(_invalid("fixed %d, %d bits after" % (sym, tail), s, trailer=False))
    # a payload that ends inside the code of 286 / 287 (the bits that are there fit no other symbol): need input, not an error
    lcodes = canonical(FIXED_LIT)
    for sym in (286, 287):
        stream_bits = [(lcodes[sym] >> (7 - i)) & 1 for i in range(8)]
        for k in range(1, 8):
            n9 = (-(3 + k)) % 8                      # 9-bit literals to put the payload's end right behind the k bits
            v = sum(b << i for i, b in enumerate(stream_bits[:k]))
            s = Stream().fixed(pre + [200] * n9 + [("bits", v, k)], eob=False)
            assert s.w.n % 8 == 0
            out.append(_invalid("ends %d bits into fixed %d" % (k, sym), s, trailer=False))
    for dc in (30, 31):
        for tail in (0, 3, 9, 40):
            s = Stream().fixed(pre + [("L", 258, 0, 0), ("D", dc, 0, 0), ("bits", 0, tail)], final=True, eob=False)
            out.append(_invalid("fixed distance %d, %d bits after" % (dc, tail), s, trailer=False))
    for tail in (0, 1, 7, 20):
        d = [0] * 30
        d[0] = 1
        s = Stream().fixed(pre)
        s.dynamic([97, ("L", 260, 0, 0), ("bits", 1, 1), ("bits", 0, tail)], good_l, d, final=True, eob=False)
        s.valid = False
        out.append(_invalid("missing code of a lone distance code, %d bits after" % tail, s, trailer=False))
        s = Stream().fixed(pre)
        s.dynamic([97, ("L", 260, 0, 0), ("bits", 0, tail)], good_l, [0], final=True, eob=False)
        s.valid = False
        out.append(_invalid("a match with no distance codes, %d bits after" % tail, s, trailer=False))
        one = [0] * 286
        one[256] = 1
        s = Stream().fixed(pre)
        s.dynamic([("bits", 1, 1), ("bits", 0, tail)], one, [0], final=True, eob=False)
        s.valid = False
        out.append(_invalid("missing code of a lone 1-bit literal/length code, %d bits after" % tail, s, trailer=False))
    s = Stream().fixed(pre)
    s.w.put(1, 1)
    s.w.put(3, 2)
    s.w.put(0, 16)
    s.valid = False
    out.append(_invalid("block type 3", s))
    for extra in (1, 2, 100):
        s = Stream().fixed([1, 2, 3, ("m", 5, 3 + extra)], final=True)
        out.append(_invalid("distance %d past the output" % extra, s))
    s = Stream().stored(b"abc", nlen=0x1234)
    out.append(_invalid("stored NLEN mismatch", s))
    s = Stream().stored(b"abcdef" * 10, final=True)
    p = s.payload(trailer=False)
    out += [Case("c", "stored cut %d" % k, p[:k], False) for k in (3, 4, 5, 6, 7, 8, 30)]
    # bad zlib headers
    for name, h in (("FDICT", zlib_header(fdict=True)), ("CINFO 8", zlib_header(cinfo=8)), ("CINFO 15", zlib_header(cinfo=15)),
                    ("FCHECK wrong", (0x78, 0x9D)), ("method 7", (0x77, 0x9C - 0x1F + (31 - ((0x77 << 8) + 0x7D) % 31) % 31))):
        s = Stream(header=h).fixed([1, 2, 3], final=True)
        out.append(Case("c", "header " + name, s.payload(), False))
    out.append(Case("c", "empty payload", b"", False))
    out.append(Case("c", "header only", b"\x78\x9c", False))
    out.append(Case("c", "one byte", b"\x78", False))
    return out


def group_d(seed):
    rng = random.Random(seed + 3)
    out = []
    # exactly 65 535 bytes, the last symbol a 258 match
    for form in ("fixed", "dynamic"):
        s = Stream()
        toks = tokens_for(rng, 60000, range(256), range(257, 286), range(30))
        n = sum(1 if isinstance(t, int) else t[1] for t in toks)
        rest = CHUNK - 258 - n
        while rest > 258 + 3:
            toks.append(("m", 258, rng.randint(1, 30000)))
            rest -= 258
        toks += [rng.randrange(256) for _ in range(rest)]
        toks.append(("m", 258, 1000))
        if form == "fixed":
            s.fixed(toks, final=True)
        else:
            s.dynamic(toks, random_code(rng, 286, 286, 12, must=(256,)), random_code(rng, 30, 30, 9), final=True)
        assert len(s.data) == CHUNK
        out.append(_valid("65535 bytes ending in a 258 match (%s)" % form, s, group="d"))
        # and one byte more, as a literal / as a match / as a stored byte
        for tail, name in (([7], "literal"), ([("m", 3, 1)], "match")):
            s2 = Stream()
            s2.fixed(toks + tail, final=True) if form == "fixed" else s2.dynamic(toks + tail, random_code(rng, 286, 286, 12, must=(256,)),
                                                                                  random_code(rng, 30, 30, 9), final=True)
            out.append(Case("d", "65535 + %s (%s)" % (name, form), s2.payload(), True, bytes(s2.data), s2.body()))
    # a 258 match that crosses 65 535; stored bytes that cross it
    s = Stream().fixed([5] + [("m", 258, 1)] * 254 + [("m", 258, 1)], final=True)
    out.append(Case("d", "258 match across 65535", s.payload(), True, bytes(s.data), s.body()))
    s = Stream().fixed([5] + [("m", 258, 1)] * 253).stored(rng.randbytes(1000), final=True)
    out.append(Case("d", "stored block across 65535", s.payload(), True, bytes(s.data), s.body()))
    s = Stream().fixed([6] + [("m", 258, 1)] * 400, final=True)
    out.append(Case("d", "far past 65535", s.payload(), True, bytes(s.data), s.body()))
    # distance 32 768, and the distances equal to / one past the output so far, at several sizes
    s = Stream().stored(rng.randbytes(40000)).fixed([("m", 258, 32768), ("m", 3, 32768), ("m", 100, 32767)], final=True)
    out.append(_valid("distance 32768", s, group="d"))
    for n in (1, 2, 3, 4, 5, 100, 32767, 32768):
        s = Stream().stored(rng.randbytes(n)).fixed([("m", 20, n)], final=True)
        out.append(_valid("distance = output %d" % n, s, group="d"))
        if n == 32768:
            continue
        s = Stream().stored(rng.randbytes(n)).fixed([("m", 20, n + 1)], final=True)
        out.append(_invalid("distance = output %d + 1" % n, s, group="d"))
    # zlib: enough text to decode past 65 535 from a payload that fits
    data = text(rng, 200000)
    z = zlib.compress(data, 9)
    assert len(z) <= CHUNK
    out.append(Case("d", "zlib 200 000 bytes", z, True, data, z[2:-4]))
    return out


def group_e(seed):
    rng = random.Random(seed + 4)
    out = []
    srcs = []
    s = Stream().fixed([1, 2, 3, ("m", 9, 2)]).stored(b"xyz")
    random_dynamic(rng, s, 120, maxbits=9, final=False)
    s.stored(b"", final=False).fixed([("m", 30, 7)], final=True)
    srcs.append(("fixed+stored+dynamic", s.payload()))
    srcs.append(("zlib sync-flushed", zlib_stream(rng, text(rng, 3000), 6, 8, 15, 0, zlib.Z_SYNC_FLUSH)[:CHUNK]))
    s = Stream()
    random_dynamic(rng, s, 200, final=True)
    srcs.append(("random dynamic", s.payload()))
    for name, p in srcs:
        out += [Case("e", "%s cut %d" % (name, k), p[:k], body=p[2:k] if 2 <= k <= len(p) - 4 else None) for k in range(len(p))]
        bits = range(16, 8 * len(p)) if len(p) < 120 else sorted(rng.sample(range(16, 8 * len(p)), 600))
        for bit in bits:
            b = bytearray(p)
            b[bit >> 3] ^= 1 << (bit & 7)
            out.append(Case("e", "%s flip %d" % (name, bit), bytes(b)))
    # the invalid-symbol streams of group c cut at every byte
    for c in group_c(seed):
        if c.name.startswith(("fixed 286", "fixed distance 30", "missing code", "a match with no")):
            out += [Case("e", "%s cut %d" % (c.name, k), c.payload[:k]) for k in range(len(c.payload) - 8, len(c.payload))]
    return out


def conformance_corpus(seed=2026, n_zlib=1500):
    cases = group_a(seed, n_zlib) + group_b(seed) + group_c(seed) + group_d(seed) + group_e(seed)
    for c in cases:
        assert len(c.payload) <= CHUNK, (c.group, c.name, len(c.payload))
    return cases
