"""Archives for the ZIP tests (tests/test_zip_cpu.py, tests/test_gpu_zip.py): a handful of entries, and every form of archive that
Python's zipfile writes from them, plus the forms it does not (a foreign extra field in front of the ZIP64 one, a comment of the
greatest length that holds end-record signatures)."""
import io
import struct
import zipfile

import corpus
import zip_ref


def small_entries():
    return [("a.txt", corpus.text_like(1, 1000)), ("dir/b.bin", corpus.random_bytes(2, 70000)), ("empty", b""),
            ("déjà/vu.txt", corpus.lz_heavy(3, 200000)), ("x" * 300, b"x")]


class Unseekable(io.RawIOBase):
    """A sink that cannot seek: zipfile then writes data descriptors (flag bit 3)."""

    def __init__(self):
        self.buf = io.BytesIO()

    def writable(self):
        return True

    def write(self, b):
        return self.buf.write(b)

    def flush(self):
        pass


def zipfile_archives():
    ents = small_entries()
    out = {}

    def build(name, comp, level=None, comment=b"", sink=None, mutate=None):
        raw = sink or io.BytesIO()
        with zipfile.ZipFile(raw, "w", comp, compresslevel=level) as zf:
            for n, d in ents:
                info = zipfile.ZipInfo(n, (2021, 3, 4, 5, 6, 8))
                info.compress_type = comp
                info.external_attr = 0o100640 << 16
                if mutate:
                    mutate(info)
                zf.writestr(info, d, compresslevel=level)
            zf.comment = comment
        out[name] = (sink.buf if sink else raw).getvalue()

    build("stored", zipfile.ZIP_STORED)
    for level in (1, 6, 9):
        build("deflated%d" % level, zipfile.ZIP_DEFLATED, level)
    build("descriptors", zipfile.ZIP_DEFLATED, 6, sink=Unseekable())
    build("comment", zipfile.ZIP_DEFLATED, 6, comment=b"hello, archive")
    # A comment of the greatest length that itself holds end-record signatures (whose own comment lengths do not reach the end).
    # zipfile takes the last signature it finds, so the entries are compared with zipfile's of the same archive without the comment.
    comment = (b"PK\x05\x06" + b"\x00" * 18 + b"!!") * 2730 + b"." * 15
    assert len(comment) == 65535
    out["comment65535"] = (out["deflated6"][:-2] + b"\xff\xff" + comment, out["deflated6"])
    build("foreign_extra", zipfile.ZIP_DEFLATED, 6, mutate=lambda i: setattr(i, "extra", b"\x99\x99\x04\x00abcd"))
    # a foreign field in front of the ZIP64 field of every central record (zipfile itself writes the ZIP64 field first)
    base = zip_ref.write(ents, force64=True)
    cd0, cd1 = base.index(b"PK\x01\x02"), base.index(b"PK\x06\x06")
    recs, p, foreign = [], cd0, b"\x99\x99\x04\x00abcd"
    while p < cd1:
        nlen, xlen = struct.unpack_from("<HH", base, p + 28)
        recs.append(base[p:p + 30] + struct.pack("<H", xlen + len(foreign)) + base[p + 32:p + 46 + nlen] + foreign + base[p + 46 + nlen:p + 46 + nlen + xlen])
        p += 46 + nlen + xlen
    cd = b"".join(recs)
    out["foreign_before_zip64"] = base[:cd0] + cd + zip_ref.end_records(len(ents), len(cd), cd0, True)
    raw = io.BytesIO()
    with zipfile.ZipFile(raw, "w", zipfile.ZIP_DEFLATED) as zf:
        for n, d in ents:
            with zf.open(zipfile.ZipInfo(n, (1999, 12, 31, 23, 59, 58)), "w", force_zip64=True) as f:
                f.write(d)
    out["force_zip64"] = raw.getvalue()
    raw = io.BytesIO()
    with zipfile.ZipFile(raw, "w", zipfile.ZIP_DEFLATED) as zf:
        zf.writestr(zipfile.ZipInfo("d/"), b"")
        zf.writestr("d/e/", b"")
        zf.writestr("d/e/f.txt", b"content")
    out["directories"] = raw.getvalue()
    raw = io.BytesIO()
    with zipfile.ZipFile(raw, "w", zipfile.ZIP_STORED) as zf:
        for i in range(66000):
            zf.writestr("f/%05d" % i, b"q" * (i % 17))
    out["66000"] = raw.getvalue()
    raw = io.BytesIO()
    zipfile.ZipFile(raw, "w").close()
    out["empty"] = raw.getvalue()
    return out
