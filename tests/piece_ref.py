"""A libz reference that composes: the expected bytes of very long streams without ever compressing them whole.  Test infrastructure only.

A full flush with all input consumed clears libz's hash and window, so the level-6 full-flush stream of a long input
(tests/deflate_stream_ref.py) is a header, then one BODY per 65 280-byte piece,

    c = compressobj(6, DEFLATED, -15);  body = c.compress(piece) + c.flush(Z_FULL_FLUSH)

then 03 00 and the trailer -- and the body of a piece depends on that piece alone.  So an input made of pieces from a small ALPHABET has
a stream made of that alphabet's bodies, and lengths, offsets, checksums and the bytes themselves follow from six calls of libz.

    alphabet   six pieces of 65 280 bytes from tests/corpus.py: two random (stored: 65 305-byte bodies), text, zeros, lz_heavy, skewed
    word       a fixed list of WORD = 256 alphabet indices, drawn once from a mix (a weight per alphabet piece) and a seed
    Sequence   a list of words, then up to WORD - 1 single pieces, then a tail of fewer than 65 280 bytes: the input they spell

Words and the order of words come from splitmix64 (tests/corpus.py), so nothing repeats with a period and a piece put in the wrong
place changes the bytes.  CRC-32 and Adler-32 of the whole input come from libz's own crc32_combine / adler32_combine over per-piece
and per-word sums, word by word (one call a word: a few hundred for 4 GiB).  tests/test_piece_ref_cpu.py checks all of it against
libz on whole inputs at a size where that is cheap; the GPU tests beyond 2^32 bytes rest on that.

Host side: lengths, offsets, header and trailer bytes, BGZF members.  Device side: the input, the stream and the BGZF file as CUDA
tensors, written word by word from per-word tensors (no host buffer of the whole thing ever exists).
"""
import ctypes
import struct
import zlib

import numpy as np

import bgzf_ref
import corpus
import libz_ref

PIECE = 65280
WORD = 256
RANDOM_A, RANDOM_B, TEXT, ZEROS, LZ, SKEWED = range(6)
HEADER = {"raw": b"", "zlib": b"\x78\x9c", "gzip": bytes.fromhex("1f8b0800000000000003")}
FINAL = b"\x03\x00"                   # the empty final block behind the last flush
HOST_LIMIT = 1 << 30                  # no host buffer of a whole sequence above this


def full_flush_body(piece: bytes) -> bytes:
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    return c.compress(piece) + c.flush(zlib.Z_FULL_FLUSH)


def bgzf_member(piece: bytes) -> bytes:
    return bgzf_ref.member(piece, zlib.compress(piece, 6)[2:-4])


_combine = None


def _libz_combine():
    """(crc32_combine, adler32_combine) of the libz behind tests/libz_ref.py"""
    global _combine
    if _combine is None:
        z = libz_ref.lib()
        fns = []
        for name in ("crc32_combine", "adler32_combine"):
            f = getattr(z, name)
            f.restype = ctypes.c_ulong
            f.argtypes = [ctypes.c_ulong, ctypes.c_ulong, ctypes.c_long]
            fns.append(f)
        _combine = tuple(fns)
    return _combine


class Sums:
    """CRC-32 and Adler-32 of a run of bytes, and its length; a + b is the run a followed by the run b (one libz call each)."""
    calls = 0                         # combine calls made so far (the CPU test bounds them)

    def __init__(self, crc=0, adler=1, n=0):
        self.crc, self.adler, self.n = crc, adler, n

    @classmethod
    def of(cls, data: bytes):
        return cls(zlib.crc32(data), zlib.adler32(data), len(data))

    def __add__(self, other):
        if other.n == 0:
            return self
        cc, ac = _libz_combine()
        Sums.calls += 1
        return Sums(int(cc(self.crc, other.crc, other.n)), int(ac(self.adler, other.adler, other.n)), self.n + other.n)


class _Unit:
    """One run of input bytes with everything derived from it: raw body, BGZF bytes, sums."""
    def __init__(self, data, body, bgzf, sums):
        self.data, self.body, self.bgzf, self.sums = data, body, bgzf, sums
        self._dev = {}

    def dev(self, torch, what):
        """data / body / bgzf as a CUDA uint8 tensor, made once"""
        if what not in self._dev:
            b = getattr(self, what)
            self._dev[what] = torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).cuda() if b else torch.empty(0, dtype=torch.uint8, device="cuda")
        return self._dev[what]

    def drop_dev(self):
        self._dev = {}


def _unit_of_piece(p: bytes):
    return _Unit(p, full_flush_body(p) if p else b"", bgzf_member(p) if p else b"", Sums.of(p))


_alphabet = None


def alphabet():
    """The six pieces (as _Unit), made once."""
    global _alphabet
    if _alphabet is None:
        make = [lambda: corpus.random_bytes(9001, PIECE), lambda: corpus.random_bytes(9002, PIECE), lambda: corpus.text_like(9003, PIECE),
                lambda: bytes(PIECE), lambda: corpus.lz_heavy(9004, PIECE), lambda: corpus.skewed(9005, PIECE)]
        _alphabet = [_unit_of_piece(f()) for f in make]
    return _alphabet


_words = {}


def word(mix, seed):
    """The word of this mix (six weights, alphabet order) and seed: (indices, _Unit of the 256 pieces in a row).  Cached."""
    key = (tuple(mix), seed)
    if key not in _words:
        cdf = np.cumsum(np.array(mix, dtype=np.float64))
        u = (corpus.splitmix64(seed ^ 0x5EED, WORD) >> np.uint64(11)).astype(np.float64) / float(1 << 53)
        idx = np.minimum(np.searchsorted(cdf / cdf[-1], u, side="right"), 5).astype(np.int64)
        a = alphabet()
        sums = Sums()
        for i in idx:
            sums = sums + a[i].sums
        _words[key] = (idx, _Unit(b"".join(a[i].data for i in idx), b"".join(a[i].body for i in idx), b"".join(a[i].bgzf for i in idx), sums))
    return _words[key]


def drop_device_copies():
    """Forget every cached CUDA tensor (a test calls this before torch.cuda.empty_cache())."""
    for u in (_alphabet or []):
        u.drop_dev()
    for _, u in _words.values():
        u.drop_dev()


MIX_STORED = (1, 1, 0, 0, 0, 0)                         # random pieces only: every body a stored block, longer than its piece
MIX_MOSTLY_RANDOM = (7, 7, 0.5, 0.5, 0.5, 0.5)          # about one piece in eight compressible
MIX_MOSTLY_ZEROS = (0.2, 0.2, 0.4, 14, 0.8, 0.4)
MIX_ZEROS_LZ = (0, 0, 0, 3, 1, 0)
MIX_ALL = (1, 1, 1, 1, 1, 1)


class Sequence:
    """words: [(indices, _Unit)] in order; extra: alphabet indices of the single pieces behind them; tail: the last bytes (< PIECE)."""

    def __init__(self, words, extra=(), tail=b""):
        assert len(tail) < PIECE
        self.words, self.extra, self.tail = list(words), [int(i) for i in extra], _unit_of_piece(bytes(tail))
        a = alphabet()
        self.units = [u for _, u in self.words] + [a[i] for i in self.extra] + ([self.tail] if tail else [])
        self.indices = np.concatenate([idx for idx, _ in self.words] + [np.array(self.extra, dtype=np.int64)]) if (self.words or self.extra) \
            else np.zeros(0, dtype=np.int64)
        self.n_full = int(self.indices.size)                       # pieces of 65 280 bytes
        self.n_pieces = self.n_full + (1 if tail else 0)
        self.in_len = self.n_full * PIECE + len(tail)
        self.body_len = sum(len(u.body) for u in self.units)
        self.bgzf_len = sum(len(u.bgzf) for u in self.units) + len(bgzf_ref.EOF)
        self._sums = None

    @classmethod
    def of_length(cls, n, mixes, seed, tail_kind="text"):
        """A sequence of exactly n input bytes: whole words while they fit, their mix drawn by splitmix64 from `mixes`, single pieces
        drawn from the last word's mix, and a tail of n % PIECE bytes of `tail_kind`."""
        pieces, t = divmod(n, PIECE)
        nw, ne = divmod(pieces, WORD)
        pick = corpus.splitmix64(seed, nw + 1) % np.uint64(len(mixes))
        # (distinct words are few -- a word is 16 MiB of input on the host -- but which comes where does not repeat)
        variant = corpus.splitmix64(seed ^ 0xABCD, nw + 1) % np.uint64(3)
        words = [word(mixes[int(pick[i])], int(variant[i])) for i in range(nw)]
        extra = word(mixes[int(pick[nw])], 7 + int(variant[nw]))[0][:ne]
        return cls(words, extra, corpus.make(tail_kind, seed + 1, t))

    # ---- host side ---------------------------------------------------------------------------------------------------------------
    def sums(self):
        if self._sums is None:
            s = Sums()
            for u in self.units:
                s = s + u.sums
            self._sums = s
        return self._sums

    def crc32(self):
        return self.sums().crc

    def adler32(self):
        return self.sums().adler

    def header(self, wrap):
        return HEADER[wrap]

    def trailer(self, wrap):
        """zlib: Adler-32, big-endian; gzip: CRC-32 and ISIZE = length mod 2^32, little-endian"""
        if wrap == "zlib":
            return struct.pack(">I", self.adler32())
        if wrap == "gzip":
            return struct.pack("<II", self.crc32(), self.in_len & 0xFFFFFFFF)
        return b""

    def stream_len(self, wrap):
        return len(HEADER[wrap]) + self.body_len + len(FINAL) + (0, 4, 8)[("raw", "zlib", "gzip").index(wrap)]

    def piece_lengths(self):
        """(input bytes, body bytes, BGZF member bytes) of every piece in order, the tail's included: three int64 arrays"""
        a = alphabet()
        cols = []
        for what in ("data", "body", "bgzf"):
            per = np.array([len(getattr(u, what)) for u in a], dtype=np.int64)
            v = per[self.indices]
            cols.append(np.concatenate([v, [len(getattr(self.tail, what))]]) if self.tail.data else v)
        return cols

    def in_offsets(self):
        """offset of every piece in the input (n_pieces + 1 entries: the last is in_len)"""
        return np.concatenate([[0], np.cumsum(self.piece_lengths()[0])])

    def out_offsets(self, wrap):
        """offset of every piece's body in the stream (n_pieces + 1 entries: the last is where 03 00 stands)"""
        return len(HEADER[wrap]) + np.concatenate([[0], np.cumsum(self.piece_lengths()[1])])

    def bgzf_offsets(self):
        """offset of every member in the BGZF file (n_pieces + 1 entries: the last is the EOF member's)"""
        return np.concatenate([[0], np.cumsum(self.piece_lengths()[2])])

    def gzi_entries(self):
        """(compressed, decoded) offsets of every member after the first and before the EOF member: what zwz_bgzf_gzi writes"""
        c, u = self.bgzf_offsets(), self.in_offsets()
        return [(int(c[i]), int(u[i])) for i in range(1, self.n_pieces)]

    def index(self, wrap, span):
        """The seek index zwz_deflate_streams_index_dev writes with the stream, as host bytes: the points are the piece starts at
        65 280 k (and the empty one behind the last flush), the entries flush_index_ref.entries_of's, no windows, and the end bit
        is behind the 03 00 that follows the last marker"""
        import flush_index_ref
        import index_ref
        w = ("raw", "zlib", "gzip").index(wrap)
        entries = flush_index_ref.entries_of(list(zip(self.out_offsets(wrap).tolist(), self.in_offsets().tolist())), self.in_len, span)
        n = self.stream_len(wrap)
        check = self.crc32() if wrap == "gzip" else self.adler32() if wrap == "zlib" else 0
        end_bit = 8 * (n - len(self.trailer(wrap)) - 2) + 10
        return index_ref.compose(index_ref.Index(w, span, n, self.in_len, end_bit, check, entries, [b""] * len(entries)))

    def _host(self, what, before=b"", after=b""):
        total = len(before) + sum(len(getattr(u, what)) for u in self.units) + len(after)
        assert total <= HOST_LIMIT, "no host buffer of %d bytes" % total
        return before + b"".join(getattr(u, what) for u in self.units) + after

    def host_input(self):
        return self._host("data")

    def host_stream(self, wrap):
        return self._host("body", HEADER[wrap], FINAL + self.trailer(wrap))

    def host_bgzf(self):
        return self._host("bgzf", b"", bgzf_ref.EOF)

    # ---- device side -------------------------------------------------------------------------------------------------------------
    def _dev(self, torch, what, before=b"", after=b"", out=None):
        """The units' bytes in a row, copied unit by unit into `out` (a CUDA uint8 tensor of at least that many bytes; made here, with
        the length rounded up to 16 and the slack zeroed, when None) -> (tensor, bytes used)"""
        total = len(before) + sum(len(getattr(u, what)) for u in self.units) + len(after)
        if out is None:
            out = torch.empty((total + 15) // 16 * 16 or 16, dtype=torch.uint8, device="cuda")
            out[total:].zero_()
        assert out.numel() >= total
        put = lambda o, b: out[o:o + len(b)].copy_(torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()))
        o = 0
        if before:
            put(0, before); o = len(before)
        for u in self.units:
            t = u.dev(torch, what)
            out[o:o + t.numel()].copy_(t)
            o += t.numel()
        if after:
            put(o, after); o += len(after)
        assert o == total
        return out, total

    def dev_input(self, torch, out=None):
        return self._dev(torch, "data", out=out)

    def dev_body(self, torch, out=None):
        """the raw bodies alone, no final block: what stands between two ZIP headers is dev_stream(torch, "raw")"""
        return self._dev(torch, "body", out=out)

    def dev_stream(self, torch, wrap, out=None):
        return self._dev(torch, "body", HEADER[wrap], FINAL + self.trailer(wrap), out=out)

    def dev_bgzf(self, torch, out=None):
        return self._dev(torch, "bgzf", b"", bgzf_ref.EOF, out=out)


def tune_tail(kind, seed, body_len, lo=1, hi=PIECE - 1):
    """A tail of `kind` whose full-flush body is exactly body_len bytes (the body grows with the tail, a byte or two a step): the
    bisection's landing point and its neighbours are tried.  AssertionError if none fits."""
    whole = corpus.make(kind, seed, hi)
    size = lambda t: len(full_flush_body(whole[:t]))
    a, b = lo, hi
    while a < b:
        mid = (a + b) // 2
        if size(mid) < body_len:
            a = mid + 1
        else:
            b = mid
    for d in range(0, 400):
        for t in (a + d, a - d):
            if lo <= t <= hi and size(t) == body_len:
                return whole[:t]
    raise AssertionError("no %s tail with a body of %d bytes" % (kind, body_len))
