"""Every route a file's MD5 verdict can take (tests/md5_routes.py), on the GPU.

1. md5_files_kernel against hashlib on irregular slot layouts: slots of any length from 0 to 65 535 (decoded chunks are not
   all 65 535 bytes: a truncated reference chunk decodes to 65 513, an empty payload to nothing), runs of empty slots,
   words that straddle two or three slot boundaries, every total length mod 64, offsets that are not k * 65 536.
2. The route matrix: one small tree whose files sit on every route at several slice sizes, compressed and decompressed in
   a child process per cell (ZWZ_VERBOSE is read once per process; a hang is a time-out, not a stuck session), the
   shard bit-exact with the oracle's and every verdict line equal to the Python-side verdict of its file instance.
3. The same verdicts through the two-rank CLI split decoder."""
import collections
import ctypes
import hashlib
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import corpus
import md5_routes
import zwz_records

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "parallel-data-compression-and-decompression_amd"


@pytest.fixture(scope="module")
def zwz():
    import importlib
    return importlib.import_module(PKG)


@pytest.fixture(scope="module")
def codec(zwz):
    c = zwz.Codec(0, 1024)
    yield c
    c.close()


# ---------------------------------------------------------------------------------------------- 1. the kernel
def _md5_files(codec, buf, offs, lens, table):
    """zwz_md5_files_dev over device copies of (buf, offs, lens, table) -> 16 bytes per table entry."""
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    hip.hipFree.argtypes = [ctypes.c_void_p]

    class Dev:
        def __init__(self, host, count=0):
            self.p, self.count = ctypes.c_void_p(), count
            assert hip.hipMalloc(ctypes.byref(self.p), max(host.nbytes, 16)) == 0
            assert hip.hipMemcpy(self.p, host.ctypes.data, host.nbytes, 1) == 0          # hipMemcpyHostToDevice
        def data_ptr(self):
            return self.p.value
        def numel(self):
            return self.count
    h_dig = np.zeros(16 * (len(table) // 2), dtype=np.uint8)
    devs = [Dev(buf), Dev(offs), Dev(lens), Dev(table, len(table)), Dev(h_dig)]
    try:
        codec.md5_files_dev(*devs)
        codec.sync()
        assert hip.hipMemcpy(h_dig.ctypes.data, devs[4].p, h_dig.nbytes, 2) == 0        # hipMemcpyDeviceToHost
    finally:
        for d in devs:
            hip.hipFree(d.p)
    return h_dig.tobytes()


def _irregular_files(rng):
    """-> list of files, each a list of slot lengths.  More than 64 files: several workgroups."""
    files = []
    for m in (0, 1, 2, 3, 4, 5, 63, 64, 65, 65509, 65513, 65535):      # a middle slot of every interesting length
        files.append([65535, m, 65535, 1000])
        files.append([7, m, 3, m, 60])
    files += [[0], [], [0, 0, 0], [0, 0, 5, 0, 0, 0, 100, 0, 0], [0, 0, 0, 65535, 0, 0, 0], [1, 0, 1, 0, 1, 0, 1]]   # empty slots
    files += [[rng.choice((0, 1, 2, 3, 61, 1000, 65513, 65535)) for _ in range(64)] for _ in range(3)]     # exactly 64 slots
    files.append([65535] * 63 + [0])
    files.append([65535] * 63 + [65534])
    for r in range(64):                                 # every total length mod 64: a long slot among slots of 0 to 7 bytes
        total = 64 * rng.randrange(1, 4) + r
        slots = [rng.randrange(0, 8) for _ in range(rng.randrange(0, 9))]
        slots.insert(rng.randrange(0, len(slots) + 1), total - sum(slots))
        files.append(slots)
    files += [[1, 1, 1, 1, 2, 1, 3, 1, 1, 2, 2, 2], [3, 1, 3, 1, 3, 1, 55, 1, 1, 1, 5], [2, 2, 2, 2, 2, 2, 2, 2, 2, 1]]   # words across 2-3 boundaries
    return files


@pytest.mark.parametrize("layout", ["stride", "packed"])
def test_md5_files_kernel_irregular_slots_match_hashlib(codec, layout):
    """One launch over every file of _irregular_files: the slots of all files in one slot array, their bytes at k * 65 536
    (the pipeline's layout) or packed back to back at odd offsets in a shuffled order; the files table in shuffled order,
    plus entries that re-read slices of other files' slots.  All 16 digest bytes of every file against hashlib."""
    rng = random.Random(20261016 if layout == "stride" else 61016)
    files = _irregular_files(rng)
    lens, data, first = [], [], []
    for i, f in enumerate(files):
        first.append(len(lens))
        for j, n in enumerate(f):
            lens.append(n)
            data.append(corpus.make(("text", "random", "lz")[(i + j) % 3], 100 * i + j, n))
    # extra table entries over other files' slots (files may share slots: the kernel only reads them)
    entries = [(first[i], len(f)) for i, f in enumerate(files)]
    for _ in range(16):
        a = rng.randrange(0, len(lens)); b = rng.randrange(a, min(len(lens), a + 70) + 1)
        entries.append((a, b - a))
    order = list(range(len(entries)))
    rng.shuffle(order)
    entries = [entries[i] for i in order]
    offs = np.zeros(len(lens), dtype=np.uint64)
    if layout == "stride":
        buf = bytearray(65536 * len(lens))
        for s, d in enumerate(data):
            offs[s] = 65536 * s
            buf[65536 * s:65536 * s + len(d)] = d
    else:
        place = list(range(len(lens)))
        rng.shuffle(place)
        buf = bytearray()
        for s in place:
            buf += bytes([0xA5]) * rng.choice((1, 2, 3, 5))        # junk between slots: never part of a digest
            offs[s] = len(buf)
            buf += data[s]
        buf += bytes([0x5A]) * 7
        assert any(int(o) % 4 for o in offs) and not all(int(o) % 65536 == 0 for o in offs)
    table = np.array([x for e in entries for x in e], dtype=np.uint32)
    got = _md5_files(codec, np.frombuffer(bytes(buf), dtype=np.uint8), offs, np.array(lens, dtype=np.uint32), table)
    assert len(entries) > 64                                      # several workgroups of 64 lanes
    bad = []
    for i, (s0, ns) in enumerate(entries):
        want = hashlib.md5(b"".join(data[s0:s0 + ns])).digest()
        if got[16 * i:16 * i + 16] != want:
            bad.append((i, s0, ns, lens[s0:s0 + ns][:12]))
    assert not bad, bad[:10]


# ---------------------------------------------------------------------------------------------- 2. the route matrix
@pytest.fixture(scope="module")
def route_shards(oracle, tmp_path_factory):
    """The layout's tree and list, the oracle's shard of it and its decoded tree, and the crafted shards (right, wrong,
    mixed), each in a directory of its own with the per-instance verdicts the Python side expects."""
    base = tmp_path_factory.mktemp("routes")
    src = base / "src"
    lst = md5_routes.write_tree(str(src))
    good_dir = base / "good"
    good_dir.mkdir()
    assert oracle.compress_shard(str(src), str(good_dir), lst, 0, 1) == 0
    good = (good_dir / "compressed_0.zwz").read_bytes()
    shards = {"good": (good, zwz_records.verdicts(oracle, good, str(base / "vg")))}
    for v in md5_routes.VARIANTS:
        shards[v] = md5_routes.crafted_shard(oracle, good, v, str(base / ("w_" + v)))
    dirs = {}
    for name, (blob, table) in shards.items():
        d = base / ("shard_" + name)
        d.mkdir(exist_ok=True)
        (d / "compressed_0.zwz").write_bytes(blob)
        dirs[name] = str(d)
    oracle_out = base / "oracle_out"
    oracle_bad = oracle.decompress_shard(str(good_dir / "compressed_0.zwz"), str(oracle_out))
    return {"src": str(src), "list": lst, "good": good, "dirs": dirs, "tables": {n: t for n, (_, t) in shards.items()},
            "oracle_tree": _tree(str(oracle_out)), "oracle_bad": oracle_bad, "base": base}


def _tree(root):
    out = {}
    for d, _, names in os.walk(root):
        for n in names:
            p = os.path.join(d, n)
            out[os.path.relpath(p, root)] = hashlib.sha256(open(p, "rb").read()).hexdigest()
    return out


def _expected(table):
    return collections.Counter((path.decode(), verdict) for path, _, _, verdict in table)


def _seen(text, prefix, marker, verdict):
    """Verdict lines of one output directory: "MD5 match for file: <dst>/<rel>" -> (rel, verdict)."""
    out = collections.Counter()
    for line in text.splitlines():
        if line.startswith(marker) and line[len(marker):].startswith(prefix + "/"):
            out[(line[len(marker) + len(prefix) + 1:], verdict)] += 1
    return out


CHILD = r"""
import ctypes, importlib, json, sys
job = json.load(open(sys.argv[1]))
sys.path.insert(0, job["root"])
z = importlib.import_module(job["pkg"])
c = z.Codec(0, job["k"])
res = {}
c.do_compression(job["src"], job["zdir"], job["list"], 0, 1)
for name, src, dst in job["decode"]:
    try:
        res[name] = [0, c.do_decompression(src, dst)]
    except z.ZwzError as e:
        res[name] = [e.status, e.md5_mismatches]
c.close()
ctypes.CDLL(None).fflush(None)          # the verdict lines are C stdio's: out before the result file says "done"
json.dump(res, open(job["result"], "w"))
"""


@pytest.mark.parametrize("cell", md5_routes.CELLS, ids=md5_routes.cell_id)
def test_verdict_routes(route_shards, tmp_path, cell):
    """One cell of the route matrix (md5_routes.routes(k, host_md5, threads) names each file's route), in a child process:
    compress the layout -- the shard must be the oracle's byte for byte, which pins both compress-side routes (the stored
    MD5s are in it) -- then decompress the good shard and the three crafted ones.  Every "MD5 match" / "MD5 mismatch"
    line must be the Python-side verdict of its file instance (as a multiset: a repeated path has one line per instance),
    the returned count the number of mismatches, the decoded tree the last instance of every path."""
    k, host_md5, threads = cell
    cap, files = md5_routes.routes(k, host_md5, threads)
    zdir = tmp_path / "zwz"
    zdir.mkdir()
    decode = []
    for name in ("good",) + md5_routes.VARIANTS:
        out = tmp_path / ("out_" + name)
        out.mkdir()
        decode.append((name, route_shards["dirs"][name], str(out)))
    job = {"root": ROOT, "pkg": PKG, "k": k, "src": route_shards["src"], "zdir": str(zdir), "list": route_shards["list"],
           "decode": decode, "result": str(tmp_path / "result.json")}
    (tmp_path / "job.json").write_text(json.dumps(job))
    env = {n: v for n, v in os.environ.items() if n not in ("ZWZ_HOST_MD5", "ZWZ_HOST_THREADS", "ZWZ_TIMELINE")}
    env["ZWZ_VERBOSE"] = "1"
    if host_md5:
        env["ZWZ_HOST_MD5"] = "1"
    if threads is not None:
        env["ZWZ_HOST_THREADS"] = str(threads)
    r = subprocess.run([sys.executable, "-c", CHILD, str(tmp_path / "job.json")], env=env, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    res = json.load(open(tmp_path / "result.json"))
    routes = [(p, g, n, c, d) for p, g, n, c, d in files]
    assert (zdir / "compressed_0.zwz").read_bytes() == route_shards["good"], routes
    for name, _, out in decode:
        table = route_shards["tables"][name]
        status, bad = res[name]
        want = _expected(table)
        got = _seen(r.stdout, out, "MD5 match for file: ", "match") + _seen(r.stderr, out, "MD5 mismatch for file: ", "mismatch")
        assert got == want, (name, sorted((got - want).items()), sorted((want - got).items()), routes)
        assert status == 0 and bad == sum(n for (_, v), n in want.items() if v == "mismatch"), (name, status, bad)
        last = {path.decode(): hashlib.sha256(decoded).hexdigest() for path, decoded, _, _ in table}
        assert _tree(out) == last, name
        if name == "good":
            assert _tree(out) == route_shards["oracle_tree"] and bad == route_shards["oracle_bad"]


# ---------------------------------------------------------------------------------------------- 3. the split decoder
def test_cli_split_decode_reports_crafted_verdicts(oracle, route_shards, tmp_path):
    """The crafted mixed shard without its repeated path (a shard with one is not split) through two CLI ranks that split it
    into record ranges and may keep only four chunks on the device between the phases: the verdict lines of both ranks
    together are the Python-side verdicts, and so is the sum of the mismatches they report."""
    files = []
    seen = set()
    for i, (path, payloads) in enumerate(md5_routes.crafted_files(oracle, route_shards["good"])):
        if path not in seen:
            seen.add(path)
            files.append((path, payloads, "wrong" if i % 2 else "right"))
    blob, table = zwz_records.build_shard(oracle, files, str(tmp_path / "work"))
    zdir = tmp_path / "zwz"
    zdir.mkdir()
    (zdir / "compressed_0.zwz").write_bytes(blob)
    back = tmp_path / "back"
    cli = os.path.join(ROOT, PKG, "main")
    procs = []
    for r in range(2):
        env = dict(os.environ, ZWZ_RANK=str(r), ZWZ_NRANKS="2", ZWZ_DEVICE="0", ZWZ_RENDEZVOUS_TIMEOUT="120",
                   ZWZ_MAX_RANGE_CHUNKS="4", ZWZ_VERBOSE="1")
        procs.append(subprocess.Popen([cli, "decompress", str(zdir), str(back)], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.PIPE, text=True))
    outs = [p.communicate(timeout=300) for p in procs]
    assert all(p.returncode == 0 for p in procs), outs
    assert any("split decode: rank" in o[1] for o in outs)
    want = _expected(table)
    got = collections.Counter()
    for o in outs:
        got += _seen(o[0], str(back), "MD5 match for file: ", "match") + _seen(o[1], str(back), "MD5 mismatch for file: ", "mismatch")
    assert got == want, (sorted((got - want).items()), sorted((want - got).items()))
    assert sum(o[1].count("MD5 mismatch for file:") for o in outs) == sum(t[3] == "mismatch" for t in table) > 0
    assert _tree(str(back)) == {path.decode(): hashlib.sha256(decoded).hexdigest() for path, decoded, _, _ in table}
