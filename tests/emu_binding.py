"""Host build of the product's portable codec cores (tests/emu/zwz_emu.cpp).  Test infrastructure."""
import ctypes
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def load():
    so = os.path.join(HERE, "emu", "libzwz_emu.so")
    src = os.path.join(HERE, "emu", "zwz_emu.cpp")
    csrc = os.path.join(HERE, "..", "parallel-data-compression-and-decompression_amd", "csrc")
    deps = [src] + [os.path.join(csrc, f) for f in ("lz_core.h", "lz_band.h", "lz_lazy.h", "huff_core.h", "zwz_common.h", "inflate_core.h")]
    deps = [d for d in deps if os.path.exists(d)]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, src])
    lib = ctypes.CDLL(so)
    lib.emu_chunk_stream.restype = ctypes.c_uint32
    lib.emu_chunk_stream.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_uint32,
                                     ctypes.c_void_p, ctypes.c_void_p]
    lib.emu_inflate.restype = ctypes.c_uint32
    lib.emu_inflate.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_uint32,
                                ctypes.POINTER(ctypes.c_uint32)]
    lib.emu_inflate_bytewise.restype = ctypes.c_uint32
    lib.emu_inflate_bytewise.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_uint32,
                                         ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint32]
    lib.emu_inflate_bytewise_mapped.restype = ctypes.c_uint32
    lib.emu_inflate_bytewise_mapped.argtypes = lib.emu_inflate_bytewise.argtypes + [ctypes.c_uint32]
    lib.emu_copy_counters.restype = None
    lib.emu_copy_counters.argtypes = [ctypes.POINTER(ctypes.c_uint64), ctypes.c_int]
    lib.emu_band_records.restype = ctypes.c_uint32
    lib.emu_band_records.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    lib.emu_plan_split_check.restype = ctypes.c_uint32
    lib.emu_plan_split_check.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int, ctypes.c_uint32]
    lib.emu_overflow_hits.restype = ctypes.c_uint64
    lib.emu_packed_window_check.restype = ctypes.c_uint32
    lib.emu_packed_window_check.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
    lib.emu_chunk_is_dense.restype = ctypes.c_int
    lib.emu_chunk_is_dense.argtypes = [ctypes.c_char_p, ctypes.c_uint32]
    lib.emu_lazy_check.restype = ctypes.c_uint32
    lib.emu_lazy_check.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p]
    lib.emu_parse_blocks_check.restype = ctypes.c_int
    lib.emu_parse_blocks_check.argtypes = [ctypes.c_char_p, ctypes.c_uint32]
    return lib


def chunk_stream(lib, data: bytes) -> bytes:
    cap = 70000
    out = ctypes.create_string_buffer(cap)
    n = lib.emu_chunk_stream(data, len(data), out, cap, None, None)
    assert n != 0xFFFFFFFF, "block plan mispredicted the body size"
    assert n != 0xFFFFFFFD, "the plan stage's decomposition (heap / depths / runs) disagrees with plan_block"
    return out.raw[:n]


def inflate(lib, payload: bytes, cap: int = 65535):
    out = ctypes.create_string_buffer(cap + 8)
    st = ctypes.c_uint32()
    n = lib.emu_inflate(payload, len(payload), out, cap, ctypes.byref(st))
    return out.raw[:n], st.value


def inflate_bytewise(lib, payload: bytes, cap: int = 65535, batch_syms: int = 64):
    """emu_inflate with the kernel's batch copy (one output byte per lane, owners by binary search)."""
    out = ctypes.create_string_buffer(cap + 8)
    st = ctypes.c_uint32()
    n = lib.emu_inflate_bytewise(payload, len(payload), out, cap, ctypes.byref(st), batch_syms)
    return out.raw[:n], st.value


def inflate_bytewise_mapped(lib, payload: bytes, cap: int = 65535, batch_syms: int = 64, own_cap: int = 1024):
    """The same with the kernel's per-byte owner map for batches of at most own_cap bytes (0: every batch searches)."""
    out = ctypes.create_string_buffer(cap + 8)
    st = ctypes.c_uint32()
    n = lib.emu_inflate_bytewise_mapped(payload, len(payload), out, cap, ctypes.byref(st), batch_syms, own_cap)
    return out.raw[:n], st.value


COPY_COUNTERS = ("deepest_chase", "batches_above_cap", "batches_mapped", "self_overlap_in_batch", "slow_matches")


def copy_counters(lib, reset=True):
    """What the byte-wise copies since the last reset went through -> {name: count} (COPY_COUNTERS)."""
    v = (ctypes.c_uint64 * 5)()
    lib.emu_copy_counters(v, int(reset))
    return dict(zip(COPY_COUNTERS, [int(x) for x in v]))
