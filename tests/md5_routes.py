"""Where each file's MD5 verdict comes from, for the route-matrix tests (test_gpu_md5_paths.py, test_md5_routes_cpu.py).

A file's digest takes one of several routes through csrc/zwz_pipeline.cpp, decided by its chunk count, where the slice
boundaries fall and two environment switches.  `routes()` replays that decision in Python for a layout, so that the tests
can show which routes a parameter cell takes, and the CPU suite can check that the matrix takes every one of them.

  compress side (the digest stored in the shard)
    compress-gpu       whole inside one slice, at most 64 chunks: md5_files_kernel over the input slots
    compress-reader    the same file under ZWZ_HOST_MD5=1: hashed by the task that reads it
    compress-rehash    cut by a slice boundary, or more than 64 chunks: CompressJob::hash_whole_file re-reads it
  decode side (the digest checked against the stored one)
    decode-gpu         all records inside one slice, at most 64, path not repeated: md5_files_kernel over the output slots
    decode-writer      inside one slice but more than 64 records, or ZWZ_HOST_MD5=1: the task that writes it
    decode-shared      a path that occurs twice in the shard: written and hashed on the caller's thread, in shard order
    decode-trailing    spans slices: DecodeSink::hash_trailing reads it from disk while later slices are written
    decode-from-disk   spans slices with one host worker: DecodeSink::hash_from_disk after its last record
"""
CHUNK = 65535
SLICE_MAX = 2048            # kSliceChunks

# (path, content, size).  Content "text" is corpus.text_like; "mixed" is text with random chunks at 3 and 40 (their payloads
# reach the 65 535-byte cap and are cut: lossy, like the reference).  a/one.txt is listed three times: a repeated path,
# twice right behind a file that ends in the same slice and spans slices at k = 64 / 1024.  Chunk positions (T = 265):
#   0 a/empty.bin        1 chunk (empty)
#   1 a/one.txt          1
#   2..65 b/c63.txt      64 (63 full + an empty last chunk)   ends on a slice boundary at k = 1, 2, 3
#   66..129 b/c64m1.bin  64
#   130 a/one.txt        repeat
#   131..195 c/c64.txt   65 (the last one empty)
#   196 c/small.bin      1 (3 bytes)
#   197..261 c/c65.txt   65
#   262 a/one.txt        repeat
#   263..264 d/tail.txt  2
LAYOUT = [
    ("a/empty.bin", "text", 0),
    ("a/one.txt", "text", 40000),
    ("b/c63.txt", "text", 63 * CHUNK),
    ("b/c64m1.bin", "mixed", 64 * CHUNK - 1),
    ("a/one.txt", None, None),
    ("c/c64.txt", "text", 64 * CHUNK),
    ("c/small.bin", "random", 3),
    ("c/c65.txt", "text", 64 * CHUNK + 1000),
    ("a/one.txt", None, None),
    ("d/tail.txt", "text", 70000),
]


def sizes(layout=LAYOUT):
    """-> [(path, size)] in list order, a repeated path with the size of its first listing."""
    first = {}
    out = []
    for path, _, n in layout:
        if n is not None:
            first[path] = n
        out.append((path, first[path]))
    return out


def cap_for(total, k):
    """Chunks per slice, as both directory paths size it (csrc/pipeline_core.h: slice_cap): min(max_batch, 2048, (T + 1) / 2 + 1)."""
    return max(1, min(k, SLICE_MAX, (total + 1) // 2 + 1))


def routes(k, host_md5=False, threads=None, layout=LAYOUT):
    """-> (cap, [(path, first chunk, chunks, compress route, decode route)]) for Codec(0, k) with ZWZ_HOST_MD5 set or not and
    ZWZ_HOST_THREADS = threads (None: unset, i.e. at least two workers)."""
    files = sizes(layout)
    counts = [n // CHUNK + 1 for _, n in files]
    total = sum(counts)
    cap = cap_for(total, k)
    repeated = {p for p, _ in files if sum(q == p for q, _ in files) > 1}
    out, g = [], 0
    for (path, _), n in zip(files, counts):
        whole = g // cap == (g + n - 1) // cap
        if whole and n <= 64:
            comp = "compress-reader" if host_md5 else "compress-gpu"
        else:
            comp = "compress-rehash"
        if path in repeated:
            dec = "decode-shared"
        elif not whole:
            dec = "decode-from-disk" if threads == 1 else "decode-trailing"
        elif n <= 64 and not host_md5:
            dec = "decode-gpu"
        else:
            dec = "decode-writer"
        out.append((path, g, n, comp, dec))
        g += n
    return cap, out


ALL_ROUTES = {"compress-gpu", "compress-reader", "compress-rehash", "decode-gpu", "decode-writer", "decode-shared",
              "decode-trailing", "decode-from-disk"}


def write_tree(root, layout=LAYOUT):
    """The layout's source files under root, and its file list (one line per listing) -> list file path."""
    import os
    import corpus
    for i, (path, kind, n) in enumerate(layout):
        if n is None:
            continue
        if kind == "mixed":
            data = b"".join(corpus.random_bytes(9100 + c, CHUNK) if c in (3, 40) else corpus.text_like(9100 + c, CHUNK)
                            for c in range(n // CHUNK + 1))[:n]
        else:
            data = corpus.make(kind, 9000 + i, n)
        p = os.path.join(root, path)
        os.makedirs(os.path.dirname(p), exist_ok=True)
        with open(p, "wb") as f:
            f.write(data)
    lst = os.path.join(os.path.dirname(os.path.abspath(root)), os.path.basename(root) + ".list")
    with open(lst, "w") as f:
        f.write("".join(path + "\n" for path, _, _ in layout))
    return lst


VARIANTS = ("right", "wrong", "mixed")


def crafted_files(oracle, good_blob):
    """The good shard's files with irregular chunks put in, record counts unchanged (so each file keeps its route):
    empty payloads (leading, a run of three, trailing), payloads that decode to 1-5, 63-65 and 65 509 bytes, payloads cut
    short (a text chunk's, a stored block's), and a second listing of a/one.txt with other content.
    -> [(path, [payload, ...])] in shard order, for zwz_records.build_shard."""
    import corpus
    import zwz_records
    pay = oracle.payload
    out = []
    seen = {}
    for path, payloads, _ in zwz_records.instances(good_blob):
        p = list(payloads)
        name = path.decode()
        if name == "b/c63.txt":
            p[0] = b""
            p[10] = p[10][:len(p[10]) // 2]
            p[20:23] = [b"", b"", b""]
            p[30:35] = [pay(b"x"), pay(b"yz"), pay(b"abc"), pay(b"wxyz"), pay(b"12345")]
            p[40:43] = [pay(corpus.text_like(40, 63)), pay(corpus.text_like(41, 64)), pay(corpus.text_like(42, 65))]
            p[50] = pay(corpus.text_like(50, 65509))
            p[62] = b""
        elif name == "b/c64m1.bin":
            p[10] = p[40][:30001]                      # a stored block cut inside its data
            p[63] = b""
        elif name == "c/c64.txt":
            p[0] = pay(b"ab")
            p[63] = b""
        elif name == "c/c65.txt":
            p[5] = p[5][:len(p[5]) // 3]
        elif name == "a/one.txt":
            seen[name] = seen.get(name, 0) + 1
            if seen[name] == 2:
                p = [pay(corpus.text_like(77, 100))]
        out.append((path, p))
    return out


def crafted_shard(oracle, good_blob, variant, workdir):
    """crafted_files with every digest right, every digest wrong, or a mixture (odd positions wrong) -> build_shard's result."""
    import zwz_records
    files = crafted_files(oracle, good_blob)
    pick = {"right": lambda i: "right", "wrong": lambda i: "wrong", "mixed": lambda i: "wrong" if i % 2 else "right"}[variant]
    return zwz_records.build_shard(oracle, [(path, p, pick(i)) for i, (path, p) in enumerate(files)], workdir)


# The route matrix the GPU test runs, (k, ZWZ_HOST_MD5, ZWZ_HOST_THREADS): every combination for k in {1, 2, 3, 64}, the
# default thread count for 7 and 1024 (between them those two add nothing but the two-slice layout of k = 1024).
CELLS = [(k, h, t) for k in (1, 2, 3, 64) for h in (False, True) for t in (None, 1, 2)] + \
        [(k, h, None) for k in (7, 1024) for h in (False, True)]


def cell_id(cell):
    k, h, t = cell
    return "k%d-%s-threads%s" % (k, "hostmd5" if h else "gpumd5", "default" if t is None else t)
