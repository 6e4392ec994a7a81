"""bench.py's CPU-side helpers (no GPU): the reference-binary baseline on a small tree, the guarded time-out, the top-level text fields."""
import importlib.util
import os
import subprocess
import sys
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("zwz_bench", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    argv, sys.argv = sys.argv, ["bench.py"]
    try:
        spec.loader.exec_module(m)
    finally:
        sys.argv = argv
    return m


def test_cpu_baseline_tree_times_the_reference_on_a_small_tree(bench):
    """The baseline `--workload small_files | one_file` put on the line: the reference binary itself on a bounded sample; without
    the binary (the GPU box of a checkout that never built it) the entry says so instead of substituting anything."""
    import corpus

    def populate(src):
        total = 0
        for i, n in enumerate((70000, 1000, 0, 131070)):
            b = corpus.text_like(900 + i, n)
            total += len(b)
            with open(os.path.join(src, "f%d.txt" % i), "wb") as f:
                f.write(b)
        return total

    r = bench.cpu_baseline_tree(populate, "four small files", [1, 2])
    assert r["kind"] == "reference" and r["unit"] == "GB/s" and r["sample"] == "four small files"
    if os.path.exists(bench.REF_MAIN):
        assert r["value"] > 0 and r["compress_GBps"] > 0 and r["decompress_GBps"] > 0 and r["ranks"]["1"]["bytes"] == 202070
        assert r["ranks"]["1"]["compress_banner_s"] is not None          # the reference's own "Time Taken" was found on its stdout
        if "2" in r["ranks"] and "error" not in r["ranks"]["2"]:
            assert r["ranks"]["2"]["compress_banner_s"] is not None      # ... and with two ranks sharing a stdout: from rank 0's own file
    else:
        assert r["value"] is None and "absent" in r["note"]


def test_run_timed_kills_the_whole_process_group(bench):
    """A reference run that overstays is killed with everything it started (mpiexec's ranks hold the stdout pipe: killing the launcher alone left
    read() waiting) and reported as a failed command, not as a measurement."""
    t0 = time.perf_counter()
    with pytest.raises(subprocess.CalledProcessError):
        bench._run_timed(["bash", "-c", "sleep 30 & sleep 30"], limit_s=0.5)
    assert time.perf_counter() - t0 < 10


def _fake_step_outputs(torch, n, seed):
    """Device-layout buffers like one timed step leaves them: [chunk][65536] payloads and decoded bytes with garbage past each length."""
    import numpy as np
    rng = np.random.RandomState(seed)
    d_out = torch.from_numpy(rng.randint(0, 256, n * 65536).astype(np.uint8))
    d_back = torch.from_numpy(rng.randint(0, 256, n * 65536).astype(np.uint8))
    d_olen = torch.from_numpy(rng.randint(0, 65536, n).astype(np.int32))
    d_blen = torch.from_numpy(rng.randint(0, 65537, n).astype(np.int32))
    d_stat = torch.from_numpy(rng.randint(0, 3, n).astype(np.int32))
    return d_out, d_olen, d_back, d_blen, d_stat


def test_dump_outputs_writes_the_step_outputs_as_float_arrays(bench, tmp_path):
    """--dump-outputs: every array is float32/float64, lengths/status per chunk, checksums and sampled bytes count the valid bytes
    only (what lies past a chunk's length is not output), and the same buffers give the same files."""
    import numpy as np
    import torch
    n = 40
    d_out, d_olen, d_back, d_blen, d_stat = _fake_step_outputs(torch, n, 5)
    nbytes = bench.dump_outputs(torch, str(tmp_path / "a"), "text", True, d_out, d_olen, d_back, d_blen, d_stat)
    got = {f[len("text_"):-4]: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    assert sorted(got) == sorted(["chunk_index", "sample_index", "inflate_status", "payload_len", "payload_sums", "payload_sample",
                                  "decoded_len", "decoded_sums", "decoded_sample"])
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert nbytes == sum(a.nbytes for a in got.values())
    assert (got["chunk_index"] == np.arange(n)).all() and (got["payload_len"] == d_olen.numpy()).all()
    assert (got["decoded_len"] == d_blen.numpy()).all() and (got["inflate_status"] == d_stat.numpy()).all()
    pick = got["sample_index"].astype(np.int64)
    assert len(pick) == min(n, bench.DUMP_SAMPLE_CHUNKS) and (np.diff(pick) > 0).all()
    for nm, buf, lens in (("payload", d_out, d_olen.numpy()), ("decoded", d_back, d_blen.numpy())):
        rows = buf.numpy().reshape(n, 65536).astype(np.int64)
        for i in range(n):
            valid = rows[i, :lens[i]]
            assert got[nm + "_sums"][i, 0] == valid.sum() and got[nm + "_sums"][i, 1] == (valid * np.arange(1, lens[i] + 1)).sum()
        for j, i in enumerate(pick):
            assert (got[nm + "_sample"][j, :lens[i]] == rows[i, :lens[i]]).all() and not got[nm + "_sample"][j, lens[i]:].any()
    bench.dump_outputs(torch, str(tmp_path / "b"), "text", True, d_out, d_olen, d_back, d_blen, d_stat)
    for f in os.listdir(tmp_path / "a"):
        assert (np.load(tmp_path / "a" / f) == np.load(tmp_path / "b" / f)).all(), f


def test_dump_outputs_samples_large_batches_within_the_budget(bench, tmp_path, monkeypatch):
    """A batch beyond DUMP_MAX_CHUNKS is covered by a fixed, seeded sample of chunks; an inflate-only step writes no payload
    arrays; two workloads at the largest sizes the constants allow stay within the 64 MB the option promises."""
    import numpy as np
    import torch
    per_workload = (bench.DUMP_MAX_CHUNKS * (8 + 2 * (4 + 16) + 4) + bench.DUMP_SAMPLE_CHUNKS * (8 + 2 * 65536 * 4))
    assert 2 * per_workload <= bench.DUMP_LIMIT_BYTES
    monkeypatch.setattr(bench, "DUMP_MAX_CHUNKS", 16)
    d_out, d_olen, d_back, d_blen, d_stat = _fake_step_outputs(torch, 50, 6)
    for sub in ("a", "b"):
        bench.dump_outputs(torch, str(tmp_path / sub), "one_file", False, d_out, d_olen, d_back, d_blen, d_stat)
    names = sorted(os.listdir(tmp_path / "a"))
    assert not any("payload" in f for f in names) and "one_file_decoded_sums.npy" in names
    idx = np.load(tmp_path / "a" / "one_file_chunk_index.npy").astype(np.int64)
    assert len(idx) == 16 and (np.diff(idx) > 0).all() and idx.max() < 50
    assert (np.load(tmp_path / "a" / "one_file_decoded_len.npy") == d_blen.numpy()[idx]).all()
    for f in names:
        assert (np.load(tmp_path / "a" / f) == np.load(tmp_path / "b" / f)).all(), f
