"""Streams for the tests of the decode in legs, built with Python's zlib and by hand, with the bytes they decode to: what is expected
comes from libz and from how a stream was put together, never from the product.  Test infrastructure."""
import random
import struct
import zlib

import deflate_gen
import index_ref
import stream_corpus
from index_ref import GZIP, RAW, ZLIB

LETTERS = b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789+/"


def grainy(seed=23, pieces=72):
    """Bytes that libz cuts into a block every 20 to 30 KB: letters with little to match, a slice of text every 4 KiB."""
    rng = random.Random(seed)
    text = deflate_gen.text(rng, 200_000)
    return b"".join(bytes(rng.choices(LETTERS, k=4096)) + text[1500 * i:1500 * i + 1500] for i in range(pieces))


def deflate(data, wrap, level=6, flush_every=None, flush=zlib.Z_SYNC_FLUSH):
    c = zlib.compressobj(level, zlib.DEFLATED, index_ref.WBITS[wrap])
    if flush_every is None:
        return c.compress(data) + c.flush()
    return b"".join(c.compress(data[i:i + flush_every]) + c.flush(flush) for i in range(0, len(data), flush_every)) + c.flush()


def stored(data, final=False):
    """One stored block on a byte boundary."""
    assert len(data) < 65536
    return bytes([1 if final else 0]) + struct.pack("<HH", len(data), len(data) ^ 0xffff) + data


def gz(body, data, flg=0, extra=b"", name=b""):
    """A gzip member around a raw body that decodes to `data`."""
    return stream_corpus.gz_member(data, flg=flg, extra=extra, name=name, body=body)


def z_block_stream(rng, total=400_000, lo=16_400, hi=17_400):
    """A raw stream of short blocks ended with Z_BLOCK: the headers fall at any bit.  -> (stream, data)"""
    data = bytes(rng.choices(LETTERS, k=total))
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    parts, at = [], 0
    while at < len(data):
        n = rng.randrange(lo, hi)
        parts.append(c.compress(data[at:at + n]) + c.flush(zlib.Z_BLOCK))
        at += n
    return b"".join(parts) + c.flush(), data


def edge_streams(seed=8, edge=4096):
    """gzip streams built so that byte `edge` -- the end of a first input window of that many bytes -- falls inside a dynamic block
    header, a stored block's header byte, LEN and NLEN, its body, the trailer before each of its eight bytes, the second member's header
    (magic, XLEN, FEXTRA, FNAME), and a first header longer than the window.  -> (names, streams, datas)"""
    rng = random.Random(seed)
    text = deflate_gen.text(rng, 60_000)
    fill = lambda n: bytes(rng.choices(LETTERS, k=n))
    names, streams, datas = [], [], []

    def add(name, stream, data):
        names.append(name); streams.append(stream); datas.append(data)

    def stored_run(total):
        """Stored blocks whose bytes, headers included, add up to `total`."""
        blocks, data = [], []
        while total:
            n = min(total, 1005)
            if 0 < total - n <= 5:
                n = total - 6                          # (what is left must hold a block of its own)
            assert n > 5
            d = fill(n - 5)
            blocks.append(stored(d)); data.append(d)
            total -= n
        return b"".join(blocks), b"".join(data)

    tail = zlib.compressobj(6, zlib.DEFLATED, -15)
    dyn = tail.compress(text) + tail.flush()
    assert (dyn[0] >> 1) & 3 == 2, "a dynamic block first"
    for back in (3, 20, 60):
        run, d = stored_run(edge - 10 - back)
        add("dynamic header %d" % back, gz(run + dyn, d + text), d + text)
    for back in (1, 2, 3, 4):
        run, d = stored_run(edge - 10 - back)
        more = fill(3000)
        add("len nlen %d" % back, gz(run + stored(more) + dyn, d + more + text), d + more + text)
    run, d = stored_run(edge - 10 - 700)
    more = fill(3000)
    add("stored body", gz(run + stored(more) + dyn, d + more + text), d + more + text)
    for cut in range(8):
        run, d = stored_run(edge - 10 - 5 - cut)
        add("trailer %d" % cut, gz(run + stored(b"", final=True), d), d)
        assert len(streams[-1]) == edge - cut + 8
    for back in (2, 11, 14, 30):
        run, d = stored_run(edge - 10 - 5 - 8 - back)
        second = gz(dyn, text, flg=4 | 8, extra=b"AB\x08\x00" + b"x" * 8, name=b"a name that goes on for a while.txt")
        add("member header %d" % back, gz(run + stored(b"", final=True), d) + second, d + text)
    add("a first header longer than the window", gz(dyn, text, flg=8, name=b"n" * (edge + 900)), text)
    return names, streams, datas


def member_streams(seed=9):
    """gzip streams of several members -> (streams, capacities, expected (status, decoded bytes or None))"""
    rng = random.Random(seed)
    parts = [deflate_gen.text(rng, 120_000), bytes(rng.choices(LETTERS, k=80_000)), deflate_gen.text(rng, 60_000)]
    m = [deflate(p, GZIP, 6) for p in parts]
    whole = b"".join(parts)
    streams = [m[0] + m[1] + m[2],                                                # boundaries in different legs
               m[0] + bytes(5000) + m[1] + bytes(4096) + m[2] + bytes(33),         # zero padding across window ends
               m[0] + bytes(9000),                                                # padding to the end
               m[0] + bytes(5000) + b"x"]                                         # garbage behind the padding
    caps = [len(whole), len(whole), len(parts[0]), len(parts[0])]
    expect = [(0, whole), (0, whole), (0, parts[0]), (35, parts[0])]
    # a bad CRC in member 1 with a data error in member 3: the checksum beats the later stop
    bad_body = bytearray(deflate(parts[2], RAW, 6))
    bad_body[len(bad_body) // 2] ^= 0xff
    broken = stream_corpus.gz_member(parts[2], body=bytes(bad_body))
    streams += [stream_corpus.gz_member(parts[0], crc=7) + m[1] + broken, m[0] + m[1] + broken]
    caps += [len(whole), len(whole)]
    expect += [(33, None), (None, None)]                                          # (the second: whatever libz says of the damage)
    # a match in member 2 that reaches before the member's first byte, right behind a restart point 20 000 bytes into it
    # (the two alphabets share no letter: nothing of `head` matches the dictionary)
    dic = bytes(rng.choices(LETTERS[:32], k=10_000))
    head = bytes(rng.choices(LETTERS[32:], k=20_000))
    c = zlib.compressobj(6, zlib.DEFLATED, -15, 8, zlib.Z_DEFAULT_STRATEGY, dic)
    body = c.compress(head) + c.flush(zlib.Z_SYNC_FLUSH) + c.compress(dic[:3000]) + c.flush()
    streams.append(m[0] + stream_corpus.gz_member(head + dic[:3000], body=body))
    caps.append(len(parts[0]) + 23_000)
    expect.append((2, parts[0] + head))
    return streams, caps, expect
