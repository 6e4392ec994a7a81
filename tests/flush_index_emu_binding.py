"""Host build of the index at full-flush points (tests/emu_flush_index/flush_index_emu.cpp).  Test infrastructure."""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FAULTS = ("ok", "magic", "length", "crc", "window_sum", "order", "hist", "end_bit", "field")      # index_core.h: IndexFault


def load():
    so = os.path.join(HERE, "emu_flush_index", "libflush_index_emu.so")
    src = os.path.join(HERE, "emu_flush_index", "flush_index_emu.cpp")
    csrc = os.path.join(HERE, "..", "parallel-data-compression-and-decompression_amd", "csrc")
    deps = [src] + [os.path.join(csrc, f) for f in ("index_core.h", "dstream_core.h", "stream_core.h", "crc_core.h", "huff_core.h", "zwz_common.h")]
    deps = [d for d in deps if os.path.exists(d)]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, src])
    lib = ctypes.CDLL(so)
    u32, u64, vp = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p
    lib.emu_flush_bound.restype = u64
    lib.emu_flush_bound.argtypes = [u64, u32]
    lib.emu_flush_parse.restype = u32
    lib.emu_flush_parse.argtypes = [ctypes.c_char_p, u64, vp]
    lib.emu_flush_index.restype = u64
    lib.emu_flush_index.argtypes = [u32, u32, u64, u64, u64, u32, vp, u64, vp, u64]
    lib.emu_flush_writer.restype = u64
    lib.emu_flush_writer.argtypes = [u32, u32, u64, vp, u32, u32, u32, vp, u64]
    return lib


def parse(lib, idx):
    """-> (fault name, fields or None)"""
    f = (ctypes.c_uint64 * 8)()
    r = lib.emu_flush_parse(idx, len(idx), f)
    keys = ("wrap", "span", "stream_len", "decoded_len", "count", "end_bit", "check", "win_off")
    return FAULTS[r], dict(zip(keys, [int(x) for x in f])) if r == 0 else None


def index(lib, wrap, span, stream_len, decoded_len, end_bit, check, points, cap=None):
    """The compaction of a list of points [(byte, offset)] -> index bytes (b"" if it does not fit cap)"""
    pts = np.ascontiguousarray(np.array(points, dtype=np.uint64).reshape(-1, 2))
    if cap is None:
        cap = lib.emu_flush_bound(decoded_len, span)
    out = ctypes.create_string_buffer(b"\xa5" * (cap + 16))
    n = lib.emu_flush_index(wrap, span, stream_len, decoded_len, end_bit, check, pts.ctypes.data, len(pts), out, cap)
    assert out.raw[cap:] == b"\xa5" * 16 + b"\x00"
    return out.raw[:n]


def writer(lib, wrap, span, n, slen, check, m=1 << 20, lead=0, cap=None):
    """The writer's loops over slices of m pieces -> index bytes (b"" if it does not fit cap)"""
    sl = np.ascontiguousarray(np.array(slen, dtype=np.uint32))
    if cap is None:
        cap = lib.emu_flush_bound(n, span)
    out = ctypes.create_string_buffer(b"\xa5" * (cap + 16))
    k = lib.emu_flush_writer(wrap, span, n, sl.ctypes.data, m, lead, check, out, cap)
    assert out.raw[cap:] == b"\xa5" * 16 + b"\x00"
    return out.raw[:k]
