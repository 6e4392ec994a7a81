"""CPU checks of the MD5 route-matrix fixtures (tests/md5_routes.py, zwz_records.build_shard): the matrix the GPU test runs
takes every verdict route, and the crafted shards mean what they claim -- the reference's decoder (the CPU oracle) agrees
with every stored verdict."""
import hashlib
import os

import corpus
import md5_routes
import zwz_records


def test_route_matrix_takes_every_route():
    taken = set()
    for k, h, t in md5_routes.CELLS:
        _, files = md5_routes.routes(k, h, t)
        taken |= {f[3] for f in files} | {f[4] for f in files}
    assert taken == md5_routes.ALL_ROUTES


def test_route_matrix_has_the_layouts_that_hang_or_mislead():
    cells = md5_routes.CELLS
    # one host worker and a file spanning three or more slices: the trailing hash used to take the only worker
    assert any(t == 1 and any((g + n - 1) // cap - g // cap >= 2 for _, g, n, _, _ in md5_routes.routes(k, h, t)[1])
               for k, h, t in cells for cap in [md5_routes.routes(k, h, t)[0]])
    # a file spanning four or more slices, with and without the trailing hash
    for threads in (None, 1):
        assert any(t == threads and any((g + n - 1) // cap - g // cap >= 3 for _, g, n, _, _ in files)
                   for k, h, t in cells for cap, files in [md5_routes.routes(k, h, t)])
    # a file ending exactly on a slice boundary, in front of the next file
    assert any(any((g + n) % cap == 0 and n > 1 and (g + n) < 265 for _, g, n, _, _ in files)
               for k, h, t in cells for cap, files in [md5_routes.routes(k, h, t)])
    # a repeated path right behind a spanning file that ends in the same slice (its hash must be complete before the
    # repeated path is written): with the trailing hash
    def shared_behind_trailing(cap, files):
        for a, b in zip(files, files[1:]):
            if a[4] == "decode-trailing" and b[4] == "decode-shared" and (a[1] + a[2] - 1) // cap == b[1] // cap:
                return True
        return False
    assert any(shared_behind_trailing(*md5_routes.routes(k, h, t)) for k, h, t in cells)
    # sizes: 0 bytes, one chunk, 64 chunks (63 x 65 535 and 64 x 65 535 - 1), 65 chunks (64 x 65 535 and more)
    sizes = {n for _, n in md5_routes.sizes()}
    assert {0, 63 * 65535, 64 * 65535 - 1, 64 * 65535, 64 * 65535 + 1000} <= sizes
    assert len(md5_routes.sizes()) > len({p for p, _ in md5_routes.sizes()})


def test_build_shard_round_trip(oracle, tmp_path):
    """build_shard's records parse back as given; the oracle's decoder reports exactly the files stored wrong, and decodes
    every file to what its payloads inflate to -- a cut middle payload included, whose file still verifies when right."""
    text = corpus.text_like(1, 3 * 65535)
    full = [oracle.payload(text[i * 65535:(i + 1) * 65535]) for i in range(3)]
    files = [
        (b"x/a.txt", [full[0], full[1][:len(full[1]) // 2], full[2]], "right"),      # cut middle: decodes short, verifies
        (b"x/b.txt", [b"", oracle.payload(b"abc"), b"", oracle.payload(b"")], "wrong"),
        (b"c.bin", [oracle.payload(corpus.random_bytes(2, 65535))], "right"),       # a truncated reference chunk
        (b"x/a.txt", [oracle.payload(b"again")], "wrong"),                           # the path again, other content
        (b"d.txt", [oracle.payload(b"")], "right"),
    ]
    blob, table = zwz_records.build_shard(oracle, files, str(tmp_path / "work"))
    recs = zwz_records.parse(blob)
    assert zwz_records.serialise(recs) == blob
    assert [(r[0], r[1], r[2], r[3]) for r in recs] == [(p, s, int(s + 1 == len(pl)), x) for p, pl, _ in files for s, x in enumerate(pl)]
    assert [r[4] for r in recs if r[2]] == [t[2] for t in table]
    for (path, payloads, digest), (tpath, decoded, stored, verdict) in zip(files, table):
        assert tpath == path and verdict == ("match" if digest == "right" else "mismatch")
        assert decoded == b"".join(oracle.inflate(p)[0] for p in payloads)
        assert (hashlib.md5(decoded).hexdigest().encode() == stored) == (digest == "right")
        assert len(stored) == 32 and sum(a != b for a, b in zip(stored, hashlib.md5(decoded).hexdigest().encode())) == (digest == "wrong")
    assert len(table[0][1]) < 3 * 65535
    shard = tmp_path / "s.zwz"
    shard.write_bytes(blob)
    assert oracle.decompress_shard(str(shard), str(tmp_path / "out")) == 2
    assert (tmp_path / "out" / "x" / "a.txt").read_bytes() == table[3][1]          # the later instance wins, in shard order
    assert [t[3] for t in zwz_records.verdicts(oracle, blob, str(tmp_path / "v"))] == [t[3] for t in table]


def test_route_shards_agree_with_the_oracle(oracle, tmp_path):
    """The route matrix's shards: the oracle's own shard of the layout, and the three crafted ones.  Per-instance verdicts
    (zwz_records.verdicts) count what the oracle's decoder counts, and its decoded tree is the last instance of every path."""
    src = tmp_path / "src"
    lst = md5_routes.write_tree(str(src))
    sizes = md5_routes.sizes()
    for path, n in sizes:
        assert os.path.getsize(src / path) == n
    good_dir = tmp_path / "good"
    good_dir.mkdir()
    assert oracle.compress_shard(str(src), str(good_dir), lst, 0, 1) == 0
    good = (good_dir / "compressed_0.zwz").read_bytes()
    inst = zwz_records.instances(good)
    assert [(p.decode(), len(pl)) for p, pl, _ in inst] == [(p, n // 65535 + 1) for p, n in sizes]
    shards = {"good": (good, zwz_records.verdicts(oracle, good, str(tmp_path / "vg")))}
    for v in md5_routes.VARIANTS:
        shards[v] = md5_routes.crafted_shard(oracle, good, v, str(tmp_path / ("w_" + v)))
    verdict_sets = {}
    for name, (blob, table) in shards.items():
        assert [(p, len(pl)) for p, pl, _ in zwz_records.instances(blob)] == [(p, len(pl)) for p, pl, _ in inst], name
        f = tmp_path / (name + ".zwz")
        f.write_bytes(blob)
        out = tmp_path / ("out_" + name)
        bad = oracle.decompress_shard(str(f), str(out))
        assert bad == sum(t[3] == "mismatch" for t in table), name
        last = {t[0]: t[1] for t in table}
        for path, data in last.items():
            assert (out / path.decode()).read_bytes() == data, (name, path)
        verdict_sets[name] = [t[3] for t in table]
    assert set(verdict_sets["right"]) == {"match"} and set(verdict_sets["wrong"]) == {"mismatch"}
    assert set(verdict_sets["mixed"]) == {"match", "mismatch"}
    assert set(verdict_sets["good"]) == {"match", "mismatch"}            # b/c64m1.bin has truncated chunks: lossy
