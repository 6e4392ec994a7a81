"""tests/piece_ref.py for streams of DEPENDENT pieces (tests/deflate_dep_ref.py): the expected bytes, checksums and seek index of very long
streams without ever compressing them whole.  Test infrastructure only.

Piece k of a dependent stream is libz's output for input bytes [32768 k, 32768 (k + 1)), primed with the 32 512 bytes in front of it.
So with an alphabet of UNITS of exactly 32 768 bytes a piece's share of the body depends only on the pair (unit in front, unit):

    alphabet   five units from tests/corpus.py: random, text, zeros, lz_heavy, skewed; 25 pair bodies and 5 first bodies (no unit in
               front: the stream's first piece), each one deflate_dep_ref.pieces call
    word       a fixed list of WORD = 256 unit indices, drawn once from a mix (a weight per unit) and a seed.  Its first body is
               chosen by the last unit of the word before it; the other 255 bodies are the word's own
    Sequence   a list of words, then up to WORD - 1 single units, then a tail shorter than a unit (its body: one pieces call)

Words and their order come from splitmix64, CRC-32 / Adler-32 from libz's crc32_combine / adler32_combine (piece_ref.Sums).  The index
is section 22's format through index_ref.compose: entries by deflate_dep_ref.entries_of's rule, taken from the cumulative body
lengths; the window of the entry at a unit's start is the last 32 512 bytes of the unit before it.  tests/test_dep_piece_ref_cpu.py
holds all of it to deflate_dep_ref on whole inputs; the GPU tests beyond 2^32 bytes rest on that.
"""
import struct

import numpy as np

import corpus
import deflate_dep_ref
import index_ref
from deflate_dep_ref import D, P, WRAP_ID
from piece_ref import FINAL, HOST_LIMIT, Sums

WORD = 256
RANDOM, TEXT, ZEROS, LZ, SKEWED = range(5)
NAMES = ("random", "text", "zeros", "lz_heavy", "skewed")
TRAILER = {"raw": 0, "zlib": 4, "gzip": 8}


def _tensor(torch, b):
    return torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).cuda() if b else torch.empty(0, dtype=torch.uint8, device="cuda")


class _Alphabet:
    """units[u]: the bytes; sums[u]; first[u]: the body of u as a stream's first piece; pair[p][u]: the body of u behind p;
    lens[p + 1][u]: the length of that body (row 0: first)."""
    def __init__(self):
        self.units = [corpus.random_bytes(9101, P), corpus.text_like(9102, P), bytes(P), corpus.lz_heavy(9103, P), corpus.skewed(9104, P)]
        self.sums = [Sums.of(u) for u in self.units]
        self.first = [deflate_dep_ref.pieces(u)[0] for u in self.units]
        self.pair = [[deflate_dep_ref.pieces(p + u)[1] for u in self.units] for p in self.units]
        self.lens = np.array([[len(b) for b in row] for row in [self.first] + self.pair], dtype=np.int64)
        self._dev = {}

    def body(self, prev, u):
        return self.first[u] if prev < 0 else self.pair[prev][u]

    def dev(self, torch, what, prev, u=0):
        """("data", u) or ("body", prev, u) as a CUDA uint8 tensor, made once"""
        key = (what, prev, u)
        if key not in self._dev:
            self._dev[key] = _tensor(torch, self.units[prev] if what == "data" else self.body(prev, u))
        return self._dev[key]


_alphabet = None


def alphabet():
    global _alphabet
    if _alphabet is None:
        _alphabet = _Alphabet()
    return _alphabet


class _Word:
    """256 units in a row: their bytes, the bodies of units 1 .. 255 (unit 0's depends on the word in front), sums"""
    def __init__(self, idx):
        a = alphabet()
        self.idx = idx
        self.data = b"".join(a.units[i] for i in idx)
        self.rest = b"".join(a.pair[p][u] for p, u in zip(idx[:-1], idx[1:]))
        s = Sums()
        for i in idx:
            s = s + a.sums[i]
        self.sums = s
        self._dev = {}

    def dev(self, torch, what):
        if what not in self._dev:
            self._dev[what] = _tensor(torch, getattr(self, what))
        return self._dev[what]


_words = {}


def word(mix, seed):
    """The word of this mix (five weights, alphabet order) and seed.  Cached."""
    key = (tuple(mix), seed)
    if key not in _words:
        cdf = np.cumsum(np.array(mix, dtype=np.float64))
        u = (corpus.splitmix64(seed ^ 0xDE9, WORD) >> np.uint64(11)).astype(np.float64) / float(1 << 53)
        _words[key] = _Word(np.minimum(np.searchsorted(cdf / cdf[-1], u, side="right"), 4).astype(np.int64))
    return _words[key]


def drop_device_copies():
    """Forget every cached CUDA tensor (a test calls this before torch.cuda.empty_cache())."""
    if _alphabet is not None:
        _alphabet._dev = {}
    for w in _words.values():
        w._dev = {}


MIX_ALL = (1, 1, 1, 1, 1)
MIX_HALF = (4, 2, 1, 1, 2)            # the stream is about half of the input: random units are stored, the others shrink


class Sequence:
    """words: [_Word] in order; extra: unit indices of the single units behind them; tail: the last bytes (< P)."""

    def __init__(self, words, extra=(), tail=b""):
        assert len(tail) < P
        a = alphabet()
        self.words, self.extra, self.tail = list(words), [int(i) for i in extra], bytes(tail)
        parts = [w.idx for w in self.words] + [np.array(self.extra, dtype=np.int64)]
        self.indices = np.concatenate(parts)
        self.prev = np.concatenate([[-1], self.indices])[:-1].astype(np.int64)       # the unit in front of every unit, -1: none
        self.n_full = int(self.indices.size)
        self.n_pieces = self.n_full + (1 if tail else 0)
        self.in_len = self.n_full * P + len(tail)
        last = int(self.indices[-1]) if self.n_full else -1
        front = a.units[last] if last >= 0 else b""
        self.tail_body = deflate_dep_ref.pieces(front + self.tail)[1 if front else 0] if tail else b""
        self.body_lens = np.concatenate([a.lens[self.prev + 1, self.indices], [len(self.tail_body)] if tail else []]).astype(np.int64)
        self.body_len = int(self.body_lens.sum())
        self._sums = None

    @classmethod
    def of_length(cls, n, mixes, seed, tail_kind="text"):
        """A sequence of exactly n input bytes, in the manner of piece_ref.Sequence.of_length"""
        units, t = divmod(n, P)
        nw, ne = divmod(units, WORD)
        pick = corpus.splitmix64(seed, nw + 1) % np.uint64(len(mixes))
        variant = corpus.splitmix64(seed ^ 0xABCD, nw + 1) % np.uint64(3)
        words = [word(mixes[int(pick[i])], int(variant[i])) for i in range(nw)]
        extra = word(mixes[int(pick[nw])], 7 + int(variant[nw])).idx[:ne]
        return cls(words, extra, corpus.make(tail_kind, seed + 1, t))

    # ---- host side ---------------------------------------------------------------------------------------------------------------
    def pairs(self):
        """the ordered pairs (unit in front, unit) that occur"""
        return set(zip(self.prev[1:].tolist(), self.indices[1:].tolist()))

    def sums(self):
        if self._sums is None:
            a = alphabet()
            s = Sums()
            for w in self.words:
                s = s + w.sums
            for i in self.extra:
                s = s + a.sums[i]
            self._sums = s + Sums.of(self.tail)
        return self._sums

    def crc32(self):
        return self.sums().crc

    def adler32(self):
        return self.sums().adler

    def header(self, wrap):
        return deflate_dep_ref.header(wrap)

    def trailer(self, wrap):
        if wrap == "zlib":
            return struct.pack(">I", self.adler32())
        return struct.pack("<II", self.crc32(), self.in_len & 0xFFFFFFFF) if wrap == "gzip" else b""

    def stream_len(self, wrap):
        return len(self.header(wrap)) + self.body_len + len(FINAL) + TRAILER[wrap]

    def out_offsets(self, wrap):
        """offset of every piece's body in the stream (n_pieces + 1 entries: the last is where 03 00 stands)"""
        return len(self.header(wrap)) + np.concatenate([[0], np.cumsum(self.body_lens)])

    def entries(self, wrap, span):
        """deflate_dep_ref.entries_of's rule over the cumulative body lengths -> [(bit, off, hist)]"""
        at = self.out_offsets(wrap)
        k = np.arange(1, self.n_pieces, dtype=np.int64)
        k = k[(k * P < self.in_len) & (k * P // span > (k - 1) * P // span)]
        return [(8 * int(at[0]), 0, 0)] + [(8 * int(at[i]), int(i) * P, D) for i in k]

    def window(self, k):
        """the window of the entry at piece k >= 1: the last 32 512 bytes of unit k - 1"""
        return alphabet().units[int(self.indices[k - 1])][P - D:]

    def index(self, wrap, span):
        """The expected index, as host bytes"""
        entries = self.entries(wrap, span)
        w = WRAP_ID[wrap]
        check = self.crc32() if wrap == "gzip" else self.adler32() if wrap == "zlib" else 0
        n = self.stream_len(wrap)
        end_bit = 8 * (n - TRAILER[wrap] - 2) + 10
        windows = [b""] + [self.window(off // P) for _, off, _ in entries[1:]]
        return index_ref.compose(index_ref.Index(w, span, n, self.in_len, end_bit, check, entries, windows))

    def host_input(self):
        assert self.in_len <= HOST_LIMIT
        a = alphabet()
        return b"".join(w.data for w in self.words) + b"".join(a.units[i] for i in self.extra) + self.tail

    def host_stream(self, wrap):
        assert self.body_len <= HOST_LIMIT
        a = alphabet()
        out, prev = [self.header(wrap)], -1
        for w in self.words:
            out += [a.body(prev, int(w.idx[0])), w.rest]
            prev = int(w.idx[-1])
        for i in self.extra:
            out.append(a.body(prev, i))
            prev = i
        return b"".join(out) + self.tail_body + FINAL + self.trailer(wrap)

    # ---- device side -------------------------------------------------------------------------------------------------------------
    def _dev(self, torch, total, parts, out):
        """parts: host bytes or CUDA tensors in order, copied one after the other into `out` (made here, with the length rounded up to
        16 and the slack zeroed, when None) -> (tensor, bytes used)"""
        if out is None:
            out = torch.empty((total + 15) // 16 * 16 or 16, dtype=torch.uint8, device="cuda")
            out[total:].zero_()
        assert out.numel() >= total
        o = 0
        for p in parts:
            t = _tensor(torch, p) if isinstance(p, bytes) else p
            out[o:o + t.numel()].copy_(t)
            o += t.numel()
        assert o == total
        return out, total

    def dev_input(self, torch, out=None):
        a = alphabet()
        parts = [w.dev(torch, "data") for w in self.words] + [a.dev(torch, "data", i) for i in self.extra] + [self.tail]
        return self._dev(torch, self.in_len, parts, out)

    def dev_stream(self, torch, wrap, out=None):
        """the expected stream, written word by word: a word's first body is chosen by the last unit of the word before it"""
        a = alphabet()
        parts, prev = [self.header(wrap)], -1
        for w in self.words:
            parts += [a.dev(torch, "body", prev, int(w.idx[0])), w.dev(torch, "rest")]
            prev = int(w.idx[-1])
        for i in self.extra:
            parts.append(a.dev(torch, "body", prev, i))
            prev = i
        parts.append(self.tail_body + FINAL + self.trailer(wrap))
        return self._dev(torch, self.stream_len(wrap), parts, out)


# the sequence tests/test_gpu_index_beyond_4gib.py sends through zwz_deflate_dep_streams_index_dev: more than 139 000 pieces
GPU_LEN = (1 << 32) + (1 << 28) + 5 * P + 12345


def gpu_sequence():
    return Sequence.of_length(GPU_LEN, [MIX_HALF, MIX_ALL], 81)
