"""MI355X-native chunk codec: Python host mirror of the reference's C++ seam (process.hpp:37-42)
over the C ABI in include/zwz.h (libzwz_hip.so, hand-written HIP for gfx950).

Names and argument meaning follow the reference:
    sort_files_by_size(path)                                   file_sort.cpp:24
    count_non_empty_lines(file_path)                           file_tools.cpp:6
    do_compression(input_dir, output_dir, file_record, rank)   compression.cpp:161
    do_decompression(input_dir, output_dir)                    decompression.cpp:165
    md5_of_file(file_path)                                     verification.cpp:6
plus the batch form of the two zlib call sites (compression.cpp:119-134, decompression.cpp:16-36):
    Codec.deflate_chunks / Codec.inflate_chunks                (host bytes)
    Codec.deflate_dev / Codec.inflate_dev                      (device-resident torch tensors)
and BGZF (blocked gzip, readable by gzip / zcat / htslib; no reference counterpart):
    Codec.bgzf_compress / Codec.bgzf_decompress                (bytes or a CUDA uint8 tensor)
    Codec.bgzf_compress_file / Codec.bgzf_decompress_file      (whole files, streamed)
    bgzf_gzi / bgzf_gzi_file                                   (the .gzi index, host only)
    Codec.bgzf_read_ranges / Codec.bgzf_read_ranges_file       (random access: decoded byte ranges)
    Codec.bgzf_index_dev / Codec.bgzf_gzi                      (the member walk on the GPU, for a CUDA tensor)
    Codec.bgzf_read_chunks / _file / Codec.bgzf_chunk_sizes    (random access: chunks (vbeg, vend) of virtual offsets, no index)
    bgzf_voffsets                                              (decoded offsets -> virtual offsets by a .gzi, host only)
and ordinary DEFLATE data of any size, a batch of independent streams in one launch (no reference counterpart):
    Codec.inflate_streams / Codec.inflate_streams_dev          (raw, zlib or gzip; bytes or device tensors)
    Codec.inflate_stream / Codec.inflate_split_streams_dev     (one long stream with full-flush points: a wave per piece)
    Codec.inflate_stream_file                                  (one file of any size, in slices; `main gunzip`)
    Codec.inflate_split_index_file                             (the same with the file's seek index; `main gunzip --split --write-index`,
                                                               `main gzindex --split`)
    Codec.inflate_stream_index / Codec.inflate_split_streams_index_dev
                                                               (the split decode that also writes the seek index of the flush points)
    Codec.inflate_index / Codec.inflate_indexed / Codec.read_ranges
                                                               (the seek index of one ordinary stream: a wave per segment)
    Codec.inflate_indexed_batch / Codec.read_ranges_batch, pack_indexes
                                                               (many indexed streams in one launch; the _dev forms)
    Codec.inflate_legs / Codec.inflate_legs_dev                (streams of ANY length, decoded and indexed in legs; one wave a stream)
    Codec.inflate_legs_file                                    (one file of ANY length through leg windows: its bytes and / or its index)
    Codec.deflate_streams / Codec.deflate_streams_dev          (the way there: libz's level-6 full-flush streams, any size)
    Codec.deflate_stream_file, deflate_stream_bound            (one file as one .gz / zlib / raw stream)
    Codec.deflate_streams_index / Codec.deflate_streams_index_dev, Codec.deflate_stream_file_index, deflate_stream_index_bound
                                                               (the same, with the seek index of the flush points written alongside)
    Codec.deflate_dep_streams / Codec.deflate_dep_streams_dev  (streams of dependent pieces, pigz's default: smaller, no cut for a reader)
    Codec.deflate_dep_stream_file, deflate_dep_stream_bound    (one file as one such stream; `main gzip --dependent`)
    Codec.deflate_dep_streams_index / Codec.deflate_dep_streams_index_dev, Codec.deflate_dep_stream_file_index,
    deflate_dep_stream_index_bound                             (the same, with the seek index, windows included, written alongside)
and ZIP archives, a batch of entries per launch (what unzip, zipfile and file managers open; no reference counterpart):
    Codec.zip / Codec.unzip                                    ([(name, bytes)] -> archive bytes and back)
    Codec.zip_dev / Codec.unzip_dev                            (device tensors)
    Codec.zip_dir / Codec.unzip_file, zip_index, zip_bound     (a directory as one .zip and back; the host-only index)

and libz's compression level of every writer above (4, 5 or 6, byte for byte libz's output at that level; default 6):
    Codec.set_level / Codec.level                              (ZWZ_LEVEL sets a codec's default)

and libz's two search-free strategies for every writer, byte for byte libz's output whatever the level (entropy coding only; runs of a byte only):
    Codec.set_strategy("huffman" | "rle" | "default") / Codec.strategy      (ZWZ_STRATEGY sets a codec's default)

There is no CPU fallback: importing works anywhere (so the build can be checked), but every codec
call needs the HIP library and a GPU and raises ZwzError otherwise.
"""
import ctypes
import os

CHUNK_SIZE = 65535          # process.hpp:12
DEV_STRIDE = 65536
NUM_STAGES = 7
STAGE_NAMES = ("lz_links", "lz_match", "lz_parse", "blockify", "plan", "encode", "inflate")

LOSSLESS_CHUNK_SIZE = 65509  # opt-in, never default (include/zwz.h: zwz_ctx_set_chunk_size)
# zwz_allgather_u64_fn: int (*)(void *user, const uint64_t *mine, uint64_t *all, uint32_t count)
ALLGATHER_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64),
                                ctypes.c_uint32)

_HERE = os.path.dirname(os.path.abspath(__file__))
# (ZWZ_LIB: another build of the same library -- tools/gpu.sh's instrumented libzwz_hip_exp.so; such a build announces itself on stderr)
LIB_PATH = os.environ.get("ZWZ_LIB") or os.path.join(_HERE, "libzwz_hip.so")
_lib = None


class ZwzError(RuntimeError):
    """A non-zero status from the C ABI.  .status is the zwz_status code; a failed do_decompression also carries
    .md5_mismatches (a damaged shard is decoded up to the damage before ZWZ_E_FORMAT is returned)."""
    status = None
    md5_mismatches = None


def lib():
    """The C-ABI library; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ZwzError("libzwz_hip.so is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(or make -C %s); this package has no CPU fallback" % _HERE)
        L = ctypes.CDLL(LIB_PATH)
        c = ctypes
        vp, u32, u64 = c.c_void_p, c.c_uint32, c.c_uint64
        L.zwz_strerror.restype = c.c_char_p
        L.zwz_strerror.argtypes = [c.c_int]
        L.zwz_last_error.restype = c.c_char_p
        L.zwz_device_count.argtypes = [c.POINTER(c.c_int)]
        L.zwz_ctx_create.argtypes = [c.c_int, u32, c.POINTER(vp)]
        L.zwz_ctx_destroy.argtypes = [vp]
        L.zwz_ctx_destroy.restype = None
        L.zwz_ctx_stream.argtypes = [vp]
        L.zwz_ctx_stream.restype = vp
        L.zwz_ctx_sync.argtypes = [vp]
        L.zwz_deflate_batch_dev.argtypes = [vp, vp, vp, vp, u32, vp, u64, vp]
        L.zwz_inflate_batch_dev.argtypes = [vp, vp, vp, vp, u32, vp, u64, vp, vp]
        L.zwz_deflate_batch.argtypes = [vp, vp, vp, vp, u32, vp, vp]
        L.zwz_inflate_batch.argtypes = [vp, vp, vp, vp, u32, vp, vp, vp]
        L.zwz_ctx_set_profiling.argtypes = [vp, c.c_int]
        L.zwz_ctx_stage_ms.argtypes = [vp, c.POINTER(c.c_float), c.c_int]
        L.zwz_sort_files_by_size.argtypes = [c.c_char_p, c.c_char_p, c.c_size_t]
        L.zwz_count_non_empty_lines.argtypes = [c.c_char_p]
        L.zwz_md5_of_file.argtypes = [c.c_char_p, c.c_char_p]
        L.zwz_md5_files_dev.argtypes = [vp, vp, vp, vp, vp, u32, vp]
        L.zwz_compress_dir.argtypes = [vp, c.c_char_p, c.c_char_p, c.c_char_p, c.c_int, c.c_int]
        L.zwz_decompress_dir.argtypes = [vp, c.c_char_p, c.c_char_p, c.POINTER(c.c_int)]
        L.zwz_decompress_dir_ranked.argtypes = [vp, c.c_char_p, c.c_char_p, c.c_int, c.c_int, ALLGATHER_FN, vp, c.POINTER(c.c_int)]
        L.zwz_ctx_set_chunk_size.argtypes = [vp, u32]
        L.zwz_ctx_set_level.argtypes = [vp, c.c_int]
        L.zwz_ctx_level.argtypes = [vp]
        L.zwz_ctx_index_span.restype = u32
        L.zwz_ctx_index_span.argtypes = [vp]
        L.zwz_ctx_set_strategy.argtypes = [vp, c.c_int]
        L.zwz_ctx_strategy.argtypes = [vp]
        L.zwz_ctx_set_option.argtypes = [vp, c.c_char_p, c.c_char_p]
        L.zwz_bgzf_bound.restype = u64
        L.zwz_bgzf_bound.argtypes = [u64]
        L.zwz_bgzf_compress_dev.argtypes = [vp, vp, u64, vp, u64, vp]
        L.zwz_bgzf_index.argtypes = [vp, u64, vp, u32, c.POINTER(u32), c.POINTER(u64)]
        L.zwz_bgzf_decompress_dev.argtypes = [vp, vp, u64, vp, u32, vp, vp, vp]
        L.zwz_bgzf_compress_file.argtypes = [vp, c.c_char_p, c.c_char_p]
        L.zwz_bgzf_decompress_file.argtypes = [vp, c.c_char_p, c.c_char_p]
        L.zwz_bgzf_gzi.argtypes = [vp, u64, vp, u64, c.POINTER(u64)]
        L.zwz_bgzf_gzi_file.argtypes = [c.c_char_p, c.c_char_p]
        L.zwz_bgzf_read_ranges_dev.argtypes = [vp, vp, u64, vp, u64, vp, u32, vp]
        L.zwz_bgzf_read_ranges_file.argtypes = [vp, c.c_char_p, c.c_char_p, vp, u32, vp]
        L.zwz_bgzf_index_dev.argtypes = [vp, vp, u64, vp, u32, c.POINTER(u32), c.POINTER(u64)]
        L.zwz_bgzf_gzi_dev.argtypes = [vp, vp, u64, vp, u64, c.POINTER(u64)]
        L.zwz_bgzf_voffsets.argtypes = [vp, u64, vp, u32, vp]
        L.zwz_bgzf_chunk_sizes_dev.argtypes = [vp, vp, u64, vp, u32, vp]
        L.zwz_bgzf_read_chunks_dev.argtypes = [vp, vp, u64, vp, u32, vp, u64, vp]
        L.zwz_bgzf_chunk_sizes_file.argtypes = [c.c_char_p, vp, u32, vp]
        L.zwz_bgzf_read_chunks_file.argtypes = [vp, c.c_char_p, vp, u32, vp, u64, vp]
        L.zwz_inflate_streams_dev.argtypes = [vp, c.c_int, vp, vp, vp, u32, vp, vp, vp, vp, vp]
        L.zwz_inflate_split_streams_dev.argtypes = [vp, c.c_int, vp, vp, vp, u32, vp, vp, vp, vp, vp, vp]
        L.zwz_inflate_stream_file.argtypes = [vp, c.c_int, c.c_char_p, c.c_char_p]
        L.zwz_inflate_split_index_file.argtypes = [vp, c.c_int, c.c_char_p, c.c_char_p, c.c_char_p]
        L.zwz_inflate_split_streams_index_dev.argtypes = [vp, c.c_int, vp, vp, vp, u32, vp, vp, vp, vp, vp, vp, u32, vp, vp, vp, vp]
        L.zwz_inflate_index_bound.restype = u64
        L.zwz_inflate_index_bound.argtypes = [u64, u32]
        L.zwz_inflate_streams_index_dev.argtypes = [vp, c.c_int, vp, vp, vp, u32, vp, vp, vp, vp, vp, u32, vp, vp, vp, vp]
        L.zwz_inflate_indexed_dev.argtypes = [vp, vp, u64, vp, u64, vp, vp, u64, vp, vp, vp]
        L.zwz_inflate_legs_dev.argtypes = [vp, c.c_int, vp, vp, vp, u32, vp, vp, vp, vp, vp, u32, vp, vp, vp, vp, vp]
        L.zwz_inflate_read_ranges_dev.argtypes = [vp, vp, u64, vp, u64, vp, vp, u32, vp]
        L.zwz_inflate_indexed_batch_dev.argtypes = [vp, vp, vp, vp, u32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.zwz_inflate_read_ranges_batch_dev.argtypes = [vp, vp, vp, vp, u32, vp, vp, vp, vp, vp, u32, vp]
        L.zwz_inflate_index_info.argtypes = [vp, u64, c.POINTER(c.c_int), c.POINTER(u64), c.POINTER(u64), c.POINTER(u32)]
        L.zwz_inflate_index_file.argtypes = [vp, c.c_int, c.c_char_p, c.c_char_p]
        L.zwz_inflate_legs_file.argtypes = [vp, c.c_int, c.c_char_p, c.c_char_p, c.c_char_p, vp]
        L.zwz_inflate_read_ranges_file.argtypes = [vp, c.c_char_p, c.c_char_p, vp, u32, vp]
        L.zwz_inflate_stream_file_indexed.argtypes = [vp, c.c_char_p, c.c_char_p, c.c_char_p]
        L.zwz_deflate_stream_bound.restype = u64
        L.zwz_deflate_stream_bound.argtypes = [u64, c.c_int]
        L.zwz_deflate_streams_dev.argtypes = [vp, c.c_int, vp, vp, vp, u32, vp, vp, vp, vp, vp]
        L.zwz_deflate_stream_file.argtypes = [vp, c.c_int, c.c_char_p, c.c_char_p]
        L.zwz_deflate_stream_file_index.argtypes = [vp, c.c_int, c.c_char_p, c.c_char_p, c.c_char_p]
        L.zwz_deflate_stream_index_bound.restype = u64
        L.zwz_deflate_stream_index_bound.argtypes = [u64, u32]
        L.zwz_deflate_streams_index_dev.argtypes = [vp, c.c_int, vp, vp, vp, u32, vp, vp, vp, vp, vp, u32, vp, vp, vp, vp]
        L.zwz_deflate_dep_stream_bound.restype = u64
        L.zwz_deflate_dep_stream_bound.argtypes = [u64, c.c_int]
        L.zwz_deflate_dep_streams_dev.argtypes = [vp, c.c_int, vp, vp, vp, u32, vp, vp, vp, vp, vp]
        L.zwz_deflate_dep_stream_file.argtypes = [vp, c.c_int, c.c_char_p, c.c_char_p]
        L.zwz_deflate_dep_stream_index_bound.restype = u64
        L.zwz_deflate_dep_stream_index_bound.argtypes = [u64, u32]
        L.zwz_deflate_dep_streams_index_dev.argtypes = [vp, c.c_int, vp, vp, vp, u32, vp, vp, vp, vp, vp, u32, vp, vp, vp, vp]
        L.zwz_deflate_dep_stream_file_index.argtypes = [vp, c.c_int, c.c_char_p, c.c_char_p, c.c_char_p]
        L.zwz_zip_index.argtypes = [vp, u64, vp, u32, c.POINTER(u32)]
        L.zwz_zip_bound.restype = u64
        L.zwz_zip_bound.argtypes = [vp, vp, u32]
        L.zwz_zip_dev.argtypes = [vp, vp, vp, vp, vp, vp, u32, vp, u64, vp, vp]
        L.zwz_unzip_dev.argtypes = [vp, vp, u64, vp, u32, vp, vp, vp, vp, vp]
        L.zwz_zip_dir.argtypes = [vp, c.c_char_p, c.c_char_p]
        L.zwz_unzip_file.argtypes = [vp, c.c_char_p, c.c_char_p]
        _lib = L
    return _lib


E_INVALID = -1
E_IO = -4
E_FORMAT = -6
E_CHECKSUM = -7
BGZF_BLOCK_SIZE = 65280     # raw bytes per BGZF member (htslib's BGZF_BLOCK_SIZE)
# per-member status of zwz_bgzf_decompress_dev beyond the inflate codes (include/zwz.h)
BGZF_BAD_MEMBER, BGZF_ISIZE_MISMATCH, BGZF_CRC_MISMATCH = 16, 17, 18
# zwz_inflate_streams_dev (include/zwz.h): wrappers, and per-stream statuses beyond the inflate codes 0..3
WRAP_RAW, WRAP_ZLIB, WRAP_GZIP = 0, 1, 2
WRAPS = {"raw": WRAP_RAW, "zlib": WRAP_ZLIB, "gzip": WRAP_GZIP}
STRATEGY_DEFAULT, STRATEGY_HUFFMAN, STRATEGY_RLE = 0, 2, 3      # libz's numbers (include/zwz.h: zwz_ctx_set_strategy)
STRATEGIES = {"default": STRATEGY_DEFAULT, "huffman": STRATEGY_HUFFMAN, "rle": STRATEGY_RLE}
STREAM_END, STREAM_NEED_INPUT, STREAM_DATA_ERROR, STREAM_OVERFLOW = 0, 1, 2, 3
STREAM_BAD_HEADER, STREAM_CHECKSUM, STREAM_LENGTH, STREAM_TRAILING, STREAM_TOO_LARGE = 32, 33, 34, 35, 36
STREAM_INDEX = 37           # the stream did not decode as its seek index says (inflate_indexed)
STREAM_MAX_IN, STREAM_MAX_OUT = 1 << 29, 1 << 32
# per-entry status of zwz_unzip_dev beyond the inflate codes and STREAM_TOO_LARGE (include/zwz.h)
ZIP_UNSUPPORTED, ZIP_BAD_ENTRY, ZIP_SIZE_MISMATCH, ZIP_CRC_MISMATCH = 48, 49, 50, 51


class ZipEntry(ctypes.Structure):
    """zwz_zip_entry: one central-directory record as zip_index reads it."""
    _fields_ = [("header_off", ctypes.c_uint64), ("data_off", ctypes.c_uint64), ("csize", ctypes.c_uint64), ("usize", ctypes.c_uint64),
                ("name_off", ctypes.c_uint64), ("crc32", ctypes.c_uint32), ("external_attr", ctypes.c_uint32), ("name_len", ctypes.c_uint16),
                ("method", ctypes.c_uint16), ("flags", ctypes.c_uint16), ("dos_time", ctypes.c_uint16), ("dos_date", ctypes.c_uint16),
                ("made_by", ctypes.c_uint16)]


class ZipMeta(ctypes.Structure):
    """zwz_zip_meta: what an entry's headers say beyond name, sizes and CRC."""
    _fields_ = [("dos_time", ctypes.c_uint16), ("dos_date", ctypes.c_uint16), ("external_attr", ctypes.c_uint32)]


def _check(rc, what, **extra):
    if rc != 0:
        L = lib()
        err = ZwzError("%s: %s (%s)" % (what, L.zwz_strerror(rc).decode(), L.zwz_last_error().decode()))
        err.status = rc
        for k, v in extra.items():
            setattr(err, k, v)
        raise err


def device_count():
    n = ctypes.c_int(0)
    lib().zwz_device_count(ctypes.byref(n))
    return n.value


class Codec:
    """One GPU, one HIP stream, one workspace (zwz_ctx)."""

    def __init__(self, device=0, max_batch_chunks=0):
        self._h = ctypes.c_void_p()
        _check(lib().zwz_ctx_create(device, max_batch_chunks, ctypes.byref(self._h)), "zwz_ctx_create")
        self.device = device

    def close(self):
        if self._h:
            lib().zwz_ctx_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    @property
    def stream(self):
        return lib().zwz_ctx_stream(self._h)

    def sync(self):
        _check(lib().zwz_ctx_sync(self._h), "zwz_ctx_sync")

    def set_profiling(self, on):
        _check(lib().zwz_ctx_set_profiling(self._h, int(on)), "zwz_ctx_set_profiling")

    def stage_ms(self, reset=True):
        arr = (ctypes.c_float * NUM_STAGES)()
        _check(lib().zwz_ctx_stage_ms(self._h, arr, int(reset)), "zwz_ctx_stage_ms")
        return dict(zip(STAGE_NAMES, list(arr)))

    # ---- host bytes ---------------------------------------------------------------------------
    def deflate_chunks(self, chunks):
        """[bytes <= 65535] -> [payload bytes]: what consumer() stores per Chunk (compression.cpp:118-134)."""
        import numpy as np
        n = len(chunks)
        blob = b"".join(chunks)
        lens = np.array([len(c) for c in chunks], dtype=np.uint32)
        offs = np.zeros(n, dtype=np.uint64)
        if n:
            offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
        src = np.frombuffer(blob, dtype=np.uint8) if blob else np.zeros(1, dtype=np.uint8)
        out = np.empty(max(n, 1) * CHUNK_SIZE, dtype=np.uint8)
        olen = np.zeros(max(n, 1), dtype=np.uint32)
        _check(lib().zwz_deflate_batch(self._h, src.ctypes.data, offs.ctypes.data, lens.ctypes.data, n, out.ctypes.data,
                                       olen.ctypes.data), "zwz_deflate_batch")
        return [out[i * CHUNK_SIZE:i * CHUNK_SIZE + int(olen[i])].tobytes() for i in range(n)]

    def inflate_chunks(self, payloads):
        """[payload bytes] -> ([decoded bytes], [status]): decompress_chunk() per record (decompression.cpp:11-37)."""
        import numpy as np
        n = len(payloads)
        blob = b"".join(payloads)
        lens = np.array([len(c) for c in payloads], dtype=np.uint32)
        offs = np.zeros(n, dtype=np.uint64)
        if n:
            offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
        src = np.frombuffer(blob, dtype=np.uint8) if blob else np.zeros(1, dtype=np.uint8)
        out = np.empty(max(n, 1) * CHUNK_SIZE, dtype=np.uint8)
        olen = np.zeros(max(n, 1), dtype=np.uint32)
        st = np.zeros(max(n, 1), dtype=np.uint32)
        _check(lib().zwz_inflate_batch(self._h, src.ctypes.data, offs.ctypes.data, lens.ctypes.data, n, out.ctypes.data,
                                       olen.ctypes.data, st.ctypes.data), "zwz_inflate_batch")
        return ([out[i * CHUNK_SIZE:i * CHUNK_SIZE + int(olen[i])].tobytes() for i in range(n)], [int(s) for s in st[:n]])

    def md5_files_dev(self, d_in, d_off, d_len, d_files, d_digests):
        """MD5 of whole files from their chunk slots in device memory: d_files = int32 pairs (first slot, slots),
        d_digests = 16 bytes per file (md5_of_file(), verification.cpp:6-30, batched).  Asynchronous."""
        n_files = d_files.numel() // 2
        _check(lib().zwz_md5_files_dev(self._h, d_in.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), d_files.data_ptr(), n_files,
                                       d_digests.data_ptr()), "zwz_md5_files_dev")

    # ---- device-resident torch tensors (asynchronous on self.stream) ---------------------------
    # self.stream is the context's own non-blocking HIP stream, NOT torch's current stream: work torch has queued on the
    # tensors (a torch.zeros fill, a copy) must be complete before these calls -- torch.cuda.synchronize(), or an event --
    # and self.sync() must precede any torch read of the results.
    def deflate_dev(self, d_in, d_off, d_len, d_out, d_out_len, out_stride=DEV_STRIDE):
        n = d_len.numel()
        _check(lib().zwz_deflate_batch_dev(self._h, d_in.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), n, d_out.data_ptr(),
                                           out_stride, d_out_len.data_ptr()), "zwz_deflate_batch_dev")

    def inflate_dev(self, d_in, d_off, d_len, d_out, d_out_len, d_status, out_stride=DEV_STRIDE):
        n = d_len.numel()
        _check(lib().zwz_inflate_batch_dev(self._h, d_in.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), n, d_out.data_ptr(),
                                           out_stride, d_out_len.data_ptr(), d_status.data_ptr()), "zwz_inflate_batch_dev")

    def inflate_streams_dev(self, wrap, d_in, d_in_off, d_in_len, d_out, d_out_off, d_out_cap, d_out_len, d_status):
        """zwz_inflate_streams_dev on device tensors (offsets, lengths, capacities and d_out_len int64, d_status int32; include/zwz.h
        has the alignment rules).  wrap: "raw" | "zlib" | "gzip" or WRAP_*.  Asynchronous; never raises for a stream's status."""
        n = d_in_len.numel()
        _check(lib().zwz_inflate_streams_dev(self._h, WRAPS.get(wrap, wrap), d_in.data_ptr(), d_in_off.data_ptr(), d_in_len.data_ptr(), n,
                                             d_out.data_ptr(), d_out_off.data_ptr(), d_out_cap.data_ptr(), d_out_len.data_ptr(),
                                             d_status.data_ptr()), "zwz_inflate_streams_dev")

    def inflate_split_streams_dev(self, wrap, d_in, d_in_off, d_in_len, d_out, d_out_off, d_out_cap, d_out_len, d_status, d_segments=None):
        """zwz_inflate_split_streams_dev: arguments and per-stream results exactly those of inflate_streams_dev; a stream with full-flush
        points (what deflate_streams writes, pigz -i, libz callers that flush fully) is decoded by one wave per piece.  d_segments
        (int32, optional) receives the pieces decoded in parallel, 0 for a stream that took the one-wave path.  Waits for the
        context's stream while it runs; the results are complete after sync()."""
        n = d_in_len.numel()
        _check(lib().zwz_inflate_split_streams_dev(self._h, WRAPS.get(wrap, wrap), d_in.data_ptr(), d_in_off.data_ptr(), d_in_len.data_ptr(), n,
                                                   d_out.data_ptr(), d_out_off.data_ptr(), d_out_cap.data_ptr(), d_out_len.data_ptr(),
                                                   d_status.data_ptr(), d_segments.data_ptr() if d_segments is not None else None),
               "zwz_inflate_split_streams_dev")

    def inflate_stream(self, data, wrap="gzip", out_size=None):
        """bytes -> decoded bytes of ONE raw / zlib / gzip stream through the split decode: as fast as a batch when the stream has
        full-flush points, the one-wave path otherwise.  Capacity guessed and regrown as inflate_streams does; raises ZwzError
        (.stream_status) as inflate_streams does."""
        return self.inflate_streams([data], wrap, None if out_size is None else [out_size], split=True)[0]

    def inflate_split_streams_index_dev(self, wrap, d_in, d_in_off, d_in_len, d_out, d_out_off, d_out_cap, d_out_len, d_status, d_segments, d_idx,
                                        d_idx_off, d_idx_cap, d_idx_len, span=0):
        """zwz_inflate_split_streams_index_dev: inflate_split_streams_dev's arguments and results (d_segments may be None), and the seek
        index of stream i at d_idx + d_idx_off[i] as inflate_streams_index_dev lays it out.  A stream that splits gets the index of its
        flush points (no windows), built at the split decode's rate; any other stream the one-wave decode's index.  The results are
        complete after sync()."""
        n = d_in_len.numel()
        _check(lib().zwz_inflate_split_streams_index_dev(self._h, WRAPS.get(wrap, wrap), d_in.data_ptr(), d_in_off.data_ptr(), d_in_len.data_ptr(), n,
                                                         d_out.data_ptr(), d_out_off.data_ptr(), d_out_cap.data_ptr(), d_out_len.data_ptr(),
                                                         d_status.data_ptr(), d_segments.data_ptr() if d_segments is not None else None, int(span),
                                                         d_idx.data_ptr(), d_idx_off.data_ptr(), d_idx_cap.data_ptr(), d_idx_len.data_ptr()),
               "zwz_inflate_split_streams_index_dev")

    def inflate_stream_index(self, data, wrap="gzip", span=None, out_size=None):
        """bytes of ONE raw / zlib / gzip stream -> (decoded bytes, index bytes, segments) through the split decode: a stream with
        full-flush points is decoded by a wave per piece (segments > 0) and gets the index of those points, without windows; any other
        stream is decoded by one wave (segments 0) and gets inflate_index's index (b"" for a gzip stream of several members).
        Capacity and errors as inflate_index."""
        return self._inflate_index("inflate_stream_index", True, data, wrap, span, out_size)

    def _inflate_index(self, who, split, data, wrap, span, out_size):
        """inflate_index (split False) and inflate_stream_index (split True): one stream with its capacity guessed and doubled while it
        overflows -> (decoded bytes, index bytes, segments)"""
        import numpy as np
        import torch
        w = WRAPS.get(wrap, wrap)
        data = bytes(data)
        span = int(span or 0)
        cap = min(int(out_size), STREAM_MAX_OUT - 1) if out_size is not None else _guess_cap(data, w)
        dev = torch.device("cuda", self.device)
        d_in = _device_input(torch, data, self.device)
        while True:
            bound = lib().zwz_inflate_index_bound(cap, span)
            if bound == 0:
                raise ValueError("span must be a power of two in 16 KiB .. 1 GiB")
            d_out = torch.empty((cap + 15) // 16 * 16 or 16, dtype=torch.uint8, device=dev)
            d_idx = torch.empty(bound, dtype=torch.uint8, device=dev)
            par = torch.from_numpy(np.array([0, len(data), 0, cap, 0, bound, 0, 0], dtype=np.int64)).to(dev)
            d_st = torch.zeros(1, dtype=torch.int32, device=dev)
            d_seg = torch.zeros(1, dtype=torch.int32, device=dev)
            streams = (w, d_in, par[0:1], par[1:2], d_out, par[2:3], par[3:4], par[6:7], d_st)
            torch.cuda.synchronize(dev)
            if split:
                self.inflate_split_streams_index_dev(*streams, d_seg, d_idx, par[4:5], par[5:6], par[7:8], span)
            else:
                self.inflate_streams_index_dev(*streams, d_idx, par[4:5], par[5:6], par[7:8], span)
            self.sync()
            st, olen, ilen = int(d_st.item()), int(par[6].item()), int(par[7].item())
            if st == STREAM_OVERFLOW and out_size is None and cap < STREAM_MAX_OUT - 1:
                cap = min(2 * cap, STREAM_MAX_OUT - 1)
                continue
            if st != STREAM_END:
                raise _stream_error(who, st)
            return d_out[:olen].cpu().numpy().tobytes(), d_idx[:ilen].cpu().numpy().tobytes(), int(d_seg.item())

    def _with_span(self, span, call):
        """call() with the context option "index_span_bytes" at span (None: as it is); afterwards the option is what the context
        itself held before (zwz_ctx_index_span), however it was set"""
        if not span:
            return call()
        if lib().zwz_inflate_index_bound(1, int(span)) == 0:
            raise ValueError("span must be a power of two in 16 KiB .. 1 GiB")
        before = str(lib().zwz_ctx_index_span(self._h))
        self.set_option("index_span_bytes", str(int(span)))
        try:
            return call()
        finally:
            self.set_option("index_span_bytes", before)

    def inflate_split_index_file(self, src, dst, dst_idx, wrap="gzip", span=None):
        """inflate_stream_file that also writes the file's seek index to dst_idx (zwz_inflate_split_index_file; `main gunzip --split
        --write-index`, `main gzindex --split`); dst None: the index only.  A file with full-flush points gets their index, without
        windows, at the split decode's rate; any other file inflate_legs_file's.  span: for this call.  Both files appear on success only."""
        self._with_span(span, lambda: _check(lib().zwz_inflate_split_index_file(self._h, WRAPS.get(wrap, wrap), os.fsencode(src),
                                                                                os.fsencode(dst) if dst is not None else None, os.fsencode(dst_idx)),
                                             "zwz_inflate_split_index_file"))

    def inflate_stream_file(self, src, dst, wrap="gzip"):
        """One file holding one raw / zlib / gzip stream of any size -> dst (zwz_inflate_stream_file; `main gunzip`).  ZwzError with
        status E_FORMAT / E_CHECKSUM on a damaged file; dst then does not appear."""
        _check(lib().zwz_inflate_stream_file(self._h, WRAPS.get(wrap, wrap), os.fsencode(src), os.fsencode(dst)), "zwz_inflate_stream_file")

    def inflate_streams_index_dev(self, wrap, d_in, d_in_off, d_in_len, d_out, d_out_off, d_out_cap, d_out_len, d_status, d_idx, d_idx_off,
                                  d_idx_cap, d_idx_len, span=0):
        """zwz_inflate_streams_index_dev: inflate_streams_dev's arguments and results, and the seek index of stream i at d_idx +
        d_idx_off[i] (int64 device tensors of offsets, capacities and lengths; a length of 0 where no index was made).  span: decoded
        bytes between checkpoints, a power of two in 16 KiB .. 1 GiB; 0: the context option "index_span_bytes".  Asynchronous."""
        n = d_in_len.numel()
        _check(lib().zwz_inflate_streams_index_dev(self._h, WRAPS.get(wrap, wrap), d_in.data_ptr(), d_in_off.data_ptr(), d_in_len.data_ptr(), n,
                                                   d_out.data_ptr(), d_out_off.data_ptr(), d_out_cap.data_ptr(), d_out_len.data_ptr(),
                                                   d_status.data_ptr(), int(span), d_idx.data_ptr(), d_idx_off.data_ptr(), d_idx_cap.data_ptr(),
                                                   d_idx_len.data_ptr()), "zwz_inflate_streams_index_dev")

    def inflate_legs_dev(self, wrap, d_in, in_off, in_len, d_out, out_off, out_cap, d_out_len, d_status, span=0, d_idx=None, idx_off=None,
                         idx_cap=None, d_idx_len=None, legs=None):
        """zwz_inflate_legs_dev: inflate_streams_index_dev for streams of any length, decoded in legs.  in_off, in_len, out_off, out_cap,
        idx_off, idx_cap: HOST sequences or numpy arrays of one element per stream; d_in, d_out, d_idx: 16-byte aligned CUDA uint8 tensors;
        d_out_len, d_idx_len (int64), d_status (int32): CUDA tensors of n.  d_idx None: decode only.  legs: a numpy uint32 array of 3 n
        that receives per stream the legs run, the legs rewound and the windows grown, or None.  The results are complete after sync()."""
        import numpy as np
        arr, n = _u64_arrays(np, "in_off, in_len, out_off and out_cap must have one element per stream", (in_off, in_len, out_off, out_cap))
        ia = None
        if d_idx is not None:
            what = "idx_off, idx_cap and d_idx_len go with d_idx, one element per stream"
            ia, _ = _u64_arrays(np, what, (idx_off, idx_cap), n)
            if d_idx_len is None:
                raise ValueError(what)
        if legs is not None and (legs.dtype != np.uint32 or legs.size != 3 * n or not legs.flags["C_CONTIGUOUS"]):
            raise ValueError("legs must be a contiguous uint32 array of 3 n")
        _check(lib().zwz_inflate_legs_dev(self._h, WRAPS.get(wrap, wrap), d_in.data_ptr(), arr[0].ctypes.data, arr[1].ctypes.data, n, d_out.data_ptr(),
                                          arr[2].ctypes.data, arr[3].ctypes.data, d_out_len.data_ptr(), d_status.data_ptr(), int(span),
                                          d_idx.data_ptr() if d_idx is not None else None, ia[0].ctypes.data if ia else None,
                                          ia[1].ctypes.data if ia else None, d_idx_len.data_ptr() if d_idx is not None else None,
                                          legs.ctypes.data if legs is not None else None), "zwz_inflate_legs_dev")

    def inflate_legs(self, datas, wrap="gzip", span=None, index=True, out_caps=None, with_legs=False):
        """[bytes of one stream each] -> [(decoded bytes, index bytes or b"", status)] through the decode in legs: streams of any length,
        at the context's "leg_bytes" / "leg_out_bytes".  Nothing is raised for a failing stream: its status (STREAM_*) is returned with
        what was decoded before the stop.  index=False decodes only.  out_caps: the capacity of every stream (None: guessed from the
        input and regrown while any stream ends with STREAM_OVERFLOW).  with_legs: also return an (n, 3) array of the legs run, the legs
        rewound and the windows grown per stream."""
        import numpy as np
        import torch
        w = WRAPS.get(wrap, wrap)
        datas = [bytes(d) for d in datas]
        n = len(datas)
        span = int(span or 0)
        if n == 0:
            return ([], np.zeros((0, 3), dtype=np.uint32)) if with_legs else []
        if lib().zwz_inflate_index_bound(1, span) == 0:
            raise ValueError("span must be a power of two in 16 KiB .. 1 GiB")
        dev = torch.device("cuda", self.device)
        d_in, offs, lens = self._batch_input(torch, np, datas)
        caps = np.array([max(4 * len(d), 1 << 16) for d in datas] if out_caps is None else [int(x) for x in out_caps], dtype=np.uint64)
        while True:
            ooff, total = _layout(np, caps, slack=16)
            d_out = torch.empty(total, dtype=torch.uint8, device=dev)
            d_len = torch.zeros(n, dtype=torch.int64, device=dev)
            d_st = torch.zeros(n, dtype=torch.int32, device=dev)
            d_idx = ioff = icap = d_ilen = None
            if index:
                icap = np.array([lib().zwz_inflate_index_bound(int(x), span) for x in caps], dtype=np.uint64)
                ioff, itotal = _layout(np, icap)            # (a bound is a multiple of 16: the slots are the bounds)
                d_idx = torch.empty(itotal, dtype=torch.uint8, device=dev)
                d_ilen = torch.zeros(n, dtype=torch.int64, device=dev)
            legs = np.zeros(3 * n, dtype=np.uint32)
            torch.cuda.synchronize(dev)
            self.inflate_legs_dev(w, d_in, offs, lens, d_out, ooff, caps, d_len, d_st, span, d_idx, ioff, icap, d_ilen, legs)
            self.sync()
            st = d_st.cpu().numpy()
            if out_caps is None and (st == STREAM_OVERFLOW).any():
                caps = np.where(st == STREAM_OVERFLOW, caps * np.uint64(2), caps)
                continue
            olen = d_len.cpu().numpy()
            ilen = d_ilen.cpu().numpy() if index else np.zeros(n, dtype=np.int64)
            res = []
            for i in range(n):
                dec = d_out[int(ooff[i]):int(ooff[i]) + int(olen[i])].cpu().numpy().tobytes()
                idx = d_idx[int(ioff[i]):int(ioff[i]) + int(ilen[i])].cpu().numpy().tobytes() if index and ilen[i] else b""
                res.append((dec, idx, int(st[i])))
            return (res, legs.reshape(n, 3)) if with_legs else res

    def inflate_indexed_dev(self, d_in, in_len, index, d_out, out_cap, d_out_len, d_status, d_segments=None, d_idx=None):
        """zwz_inflate_indexed_dev: ONE stream (a 16-byte aligned CUDA uint8 tensor, in_len bytes) decoded whole with its index (bytes),
        a wave per segment, into d_out, which may start at any byte.  d_idx: the index on the device (None: uploaded).  d_out_len
        (int64), d_status (int32), d_segments (int32, optional): one element each.  The results are complete after sync()."""
        index = bytes(index)
        _check(lib().zwz_inflate_indexed_dev(self._h, d_in.data_ptr(), int(in_len), index, len(index), d_idx.data_ptr() if d_idx is not None else None,
                                             d_out.data_ptr(), int(out_cap), d_out_len.data_ptr(), d_status.data_ptr(),
                                             d_segments.data_ptr() if d_segments is not None else None), "zwz_inflate_indexed_dev")

    def inflate_index(self, data, wrap="gzip", span=None, out_size=None):
        """bytes of ONE ordinary raw / zlib / gzip stream -> (decoded bytes, index bytes): the one-wave decode that also keeps a
        checkpoint every `span` decoded bytes (None: the context's "index_span_bytes", 1 MiB).  The index is b"" where none is made
        (a gzip stream of several members).  Capacity as inflate_streams guesses and regrows it; raises ZwzError as it does."""
        return self._inflate_index("inflate_index", False, data, wrap, span, out_size)[:2]

    def inflate_indexed(self, data, index):
        """bytes of one stream and its index (inflate_index's, or any index of the layout in include/zwz.h) -> decoded bytes, one
        wave per indexed segment.  Raises ZwzError (.stream_status: STREAM_INDEX when the stream does not decode as the index says,
        STREAM_CHECKSUM, ...) for a verdict other than 0, and with status E_FORMAT for a malformed index."""
        import torch
        index = bytes(index)
        total = index_info(index)["decoded_len"]                # (validated before anything is sized by it)
        dev = torch.device("cuda", self.device)
        d_in = _device_input(torch, data, self.device)
        d_out = torch.empty((total + 15) // 16 * 16 or 16, dtype=torch.uint8, device=dev)
        d_len = torch.zeros(1, dtype=torch.int64, device=dev)
        d_st = torch.zeros(1, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        self.inflate_indexed_dev(d_in, len(data), index, d_out, total, d_len, d_st)
        self.sync()
        st = int(d_st.item())
        if st != STREAM_END:
            raise _stream_error("inflate_indexed", st)
        return d_out[:int(d_len.item())].cpu().numpy().tobytes()

    def read_ranges_dev(self, d_in, in_len, index, ranges, d_out, d_idx=None):
        """zwz_inflate_read_ranges_dev: the decoded byte ranges (a (k, 2) uint64 array of offset, length) of one stream on the device,
        concatenated into d_out.  Only the touched segments are decoded; no checksum verdict.  Synchronous."""
        index = bytes(index)
        _check(lib().zwz_inflate_read_ranges_dev(self._h, d_in.data_ptr(), int(in_len), index, len(index), d_idx.data_ptr() if d_idx is not None else None,
                                                 ranges.ctypes.data, len(ranges), d_out.data_ptr()), "zwz_inflate_read_ranges_dev")

    def inflate_indexed_batch_dev(self, d_in, in_off, in_len, indexes, d_out, out_off, out_cap, d_out_len, d_status, d_segments=None, d_idx=None,
                                  idx_off=None):
        """zwz_inflate_indexed_batch_dev: n streams (stream i: in_len[i] bytes at in_off[i], a multiple of 16, of the 16-byte aligned CUDA
        uint8 tensor d_in) decoded whole with their indexes in ONE call, output i to d_out[out_off[i]:], any byte offset, of capacity
        out_cap[i].  in_off, in_len, out_off, out_cap: HOST sequences or numpy arrays.  indexes: a list of index bytes, or
        pack_indexes' result (made once for repeated calls); idx_off: where each index lies in the packed host buffer and in d_idx,
        multiples of 16 (None: one behind the other).  d_idx: the same buffer on the device (None: uploaded).  d_out_len (int64),
        d_status (int32), d_segments (int32, optional): n elements each, complete after sync().  ZwzError with status E_FORMAT,
        naming the stream, for a malformed index."""
        import numpy as np
        what = "in_off, in_len, out_off, out_cap and the indexes must have one element per stream"
        arr, n = _u64_arrays(np, what, (in_off, in_len, out_off, out_cap))
        pk = indexes if isinstance(indexes, PackedIndexes) else pack_indexes(indexes, idx_off)
        if pk.n != n:
            raise ValueError(what)
        _check(lib().zwz_inflate_indexed_batch_dev(self._h, d_in.data_ptr(), arr[0].ctypes.data, arr[1].ctypes.data, n, pk.blob.ctypes.data, pk.off.ctypes.data,
                                                   pk.len.ctypes.data, d_idx.data_ptr() if d_idx is not None else None, d_out.data_ptr(),
                                                   arr[2].ctypes.data, arr[3].ctypes.data, d_out_len.data_ptr(), d_status.data_ptr(),
                                                   d_segments.data_ptr() if d_segments is not None else None), "zwz_inflate_indexed_batch_dev")

    def read_ranges_batch_dev(self, d_in, in_off, in_len, indexes, ranges, d_out, d_idx=None, idx_off=None):
        """zwz_inflate_read_ranges_batch_dev: the decoded byte ranges (a (k, 3) uint64 array of stream number, offset, length) of the
        streams of a batch laid out as inflate_indexed_batch_dev's, concatenated into d_out.  Only the touched segments are decoded;
        only the indexes of named streams are read; no checksum verdict.  Synchronous."""
        import numpy as np
        what = "in_off, in_len and the indexes must have one element per stream"
        arr, n = _u64_arrays(np, what, (in_off, in_len))
        pk = indexes if isinstance(indexes, PackedIndexes) else pack_indexes(indexes, idx_off)
        if pk.n != n:
            raise ValueError(what)
        _check(lib().zwz_inflate_read_ranges_batch_dev(self._h, d_in.data_ptr(), arr[0].ctypes.data, arr[1].ctypes.data, n, pk.blob.ctypes.data,
                                                       pk.off.ctypes.data, pk.len.ctypes.data, d_idx.data_ptr() if d_idx is not None else None,
                                                       ranges.ctypes.data, len(ranges), d_out.data_ptr()), "zwz_inflate_read_ranges_batch_dev")

    def _batch_input(self, torch, np, datas):
        """[bytes or CUDA uint8 tensor] -> (one 16-byte aligned CUDA tensor holding them at multiples of 16, offsets, lengths)"""
        dev = torch.device("cuda", self.device)
        if not any(isinstance(d, torch.Tensor) for d in datas):
            blob, offs, lens = _pack_host(np, datas)
            return torch.from_numpy(blob).to(dev), offs, lens
        lens = np.array([d.numel() if isinstance(d, torch.Tensor) else len(d) for d in datas], dtype=np.uint64)
        offs, total = _layout(np, lens)
        d_in = torch.zeros(max(total, 16), dtype=torch.uint8, device=dev)
        for d, o, n in zip(datas, offs.tolist(), lens.tolist()):
            d_in[o:o + n].copy_(d.reshape(-1) if isinstance(d, torch.Tensor) else torch.frombuffer(bytearray(d), dtype=torch.uint8))
        return d_in, offs, lens

    def inflate_indexed_batch(self, datas, indexes):
        """[bytes of one stream each] and their indexes -> [decoded bytes], every segment of every stream in one launch; the streams
        may mix raw, zlib and gzip.  Raises ZwzError for the first failing stream, naming it (.index, .stream_status), as
        inflate_streams does, and with status E_FORMAT for a malformed index."""
        import numpy as np
        import torch
        datas = [bytes(d) for d in datas]
        indexes = [bytes(x) for x in indexes]
        if len(datas) != len(indexes):
            raise ValueError("one index per stream")
        n = len(datas)
        if n == 0:
            return []
        totals = np.array([index_info(x)["decoded_len"] for x in indexes], dtype=np.uint64)      # (validated before anything is sized by it)
        ooff, total = _layout(np, totals)
        dev = torch.device("cuda", self.device)
        d_in, offs, lens = self._batch_input(torch, np, datas)
        d_out = torch.empty(max(total, 16), dtype=torch.uint8, device=dev)
        d_len = torch.zeros(n, dtype=torch.int64, device=dev)
        d_st = torch.zeros(n, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        self.inflate_indexed_batch_dev(d_in, offs, lens, indexes, d_out, ooff, totals, d_len, d_st)
        self.sync()
        st, olen, host = d_st.cpu().numpy(), d_len.cpu().numpy(), d_out.cpu().numpy()
        for i in range(n):
            if st[i] != STREAM_END:
                raise _stream_error("inflate_indexed_batch", st[i], i)
        return _cut(host, ooff, olen)

    def read_ranges_batch(self, datas, indexes, ranges):
        """Decoded byte ranges [(stream, offset, length), ...] out of a batch of ordinary streams with their seek indexes, in one call:
        [bytes] -> a list of bytes; CUDA uint8 tensors -> one CUDA tensor of the ranges concatenated.  Only the segments holding a
        requested byte are decoded.  A stream number past the batch or a range past its stream's end raises ZwzError (status E_INVALID)."""
        import numpy as np
        import torch
        as_tensor = any(isinstance(d, torch.Tensor) for d in datas)
        indexes = [bytes(x) for x in indexes]
        if len(datas) != len(indexes):
            raise ValueError("one index per stream")
        rng = _ranges(np, ranges, 3)
        d_in, offs, lens = self._batch_input(torch, np, datas)
        return self._ranges_dev(torch, rng, as_tensor, lambda d_out: self.read_ranges_batch_dev(d_in, offs, lens, indexes, rng, d_out))

    def _ranges_dev(self, torch, rng, as_tensor, call):
        """The tail of the range and chunk reads on the device: room for what the rows' last column sums to, call(d_out) -- a
        synchronous call, nothing to wait for behind it --, then the CUDA tensor of the ranges concatenated or the list of their bytes"""
        total = int(rng[:, -1].sum()) if len(rng) else 0
        dev = torch.device("cuda", self.device)
        d_out = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        call(d_out)
        return d_out[:total] if as_tensor else _split(d_out[:total].cpu().numpy().tobytes(), rng)

    def inflate_index_file(self, src, dst_idx, wrap="gzip", span=None):
        """One file holding one ordinary stream -> its seek index at dst_idx (zwz_inflate_index_file; `main gzindex`).  span: as
        inflate_index (sets the context option "index_span_bytes").  A file of 2^29 compressed bytes or more goes through
        inflate_legs_file's loop, at the one-wave rate."""
        if span:
            self.set_option("index_span_bytes", str(int(span)))
        _check(lib().zwz_inflate_index_file(self._h, WRAPS.get(wrap, wrap), os.fsencode(src), os.fsencode(dst_idx)), "zwz_inflate_index_file")

    LEGS_FILE_STATS = ("legs", "rewound", "grown", "commits", "max_in_window", "max_out_window", "index_entries", "allocated_bytes")

    def inflate_legs_file(self, src, dst=None, idx=None, wrap="gzip"):
        """One file holding one raw, zlib or gzip stream of ANY length -> its decoded bytes at dst and / or its seek index (at the
        context's "index_span_bytes") at idx, decoded in legs through staging windows of "leg_file_bytes" compressed and
        "leg_file_out_bytes" decoded bytes (zwz_inflate_legs_file; `main gunzip --legs`, `main gzindex --legs`).  Memory is bounded by the
        windows, not by the file.  It makes no stream faster: one wave decodes it, about 36 s a decoded GiB.  Returns the call's stats
        as a dict (LEGS_FILE_STATS); ZwzError with status E_FORMAT / E_CHECKSUM / E_IO, with .stats, and then neither file appears."""
        import numpy as np
        st = np.zeros(8, dtype=np.uint64)
        rc = lib().zwz_inflate_legs_file(self._h, WRAPS.get(wrap, wrap), os.fsencode(src), None if dst is None else os.fsencode(dst),
                                         None if idx is None else os.fsencode(idx), st.ctypes.data)
        stats = dict(zip(self.LEGS_FILE_STATS, (int(x) for x in st)))
        _check(rc, "zwz_inflate_legs_file", stats=stats)
        return stats

    def inflate_stream_file_indexed(self, src, index_path, dst):
        """One file of any size decoded whole with its index, a wave per segment (zwz_inflate_stream_file_indexed; `main gunzip
        --index`).  ZwzError with status E_FORMAT / E_CHECKSUM; dst then does not appear."""
        _check(lib().zwz_inflate_stream_file_indexed(self._h, os.fsencode(src), os.fsencode(index_path), os.fsencode(dst)),
               "zwz_inflate_stream_file_indexed")

    def read_ranges_file(self, src, index_path, ranges):
        """Decoded byte ranges of a file holding one ordinary stream -> a list of bytes; only the compressed bytes of the touched
        segments are read (zwz_inflate_read_ranges_file)."""
        import numpy as np
        rng = _ranges(np, ranges)
        return _ranges_host(np, rng, lambda out: _check(lib().zwz_inflate_read_ranges_file(
            self._h, os.fsencode(src), os.fsencode(index_path), rng.ctypes.data, len(rng), out.ctypes.data), "zwz_inflate_read_ranges_file"))

    def read_ranges(self, data, index, ranges):
        """Decoded byte ranges [(offset, length), ...] of an ordinary stream with its seek index: bytes -> a list of bytes; a CUDA uint8
        tensor -> one CUDA tensor of the ranges concatenated (as bgzf_read_ranges).  Only the segments holding a requested byte are
        decoded.  A range past the end raises ZwzError (status E_INVALID)."""
        import numpy as np
        import torch
        as_tensor = isinstance(data, torch.Tensor)
        rng = _ranges(np, ranges)
        d_in = _device_input(torch, data, self.device)
        n = data.numel() if as_tensor else len(data)
        return self._ranges_dev(torch, rng, as_tensor, lambda d_out: self.read_ranges_dev(d_in, n, index, rng, d_out))

    def _streams_once(self, torch, np, wrap, streams, caps, split=False):
        """One call over host streams with the given capacities -> (statuses, [bytes])."""
        n = len(streams)
        dev = torch.device("cuda", self.device)
        blob, offs, lens = _pack_host(np, streams)
        ooff, total_out = _layout(np, caps)
        d_in = torch.from_numpy(blob).to(dev)
        d_out = torch.empty(max(total_out, 16), dtype=torch.uint8, device=dev)
        t = lambda a: torch.from_numpy(np.asarray(a).astype(np.int64)).to(dev)      # (this family reads device arrays: int64 tensors)
        d_off, d_len, d_ooff, d_cap = t(offs), t(lens), t(ooff), t(caps)
        d_olen = torch.zeros(max(n, 1), dtype=torch.int64, device=dev)
        d_st = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        (self.inflate_split_streams_dev if split else self.inflate_streams_dev)(wrap, d_in, d_off, d_len, d_out, d_ooff, d_cap, d_olen, d_st)
        self.sync()
        st = d_st[:n].cpu().numpy()
        olen = d_olen[:n].cpu().numpy()
        host = d_out.cpu().numpy()
        return [int(x) for x in st], _cut(host, ooff, olen)

    def inflate_streams(self, streams, wrap="gzip", out_sizes=None, split=False):
        """[bytes] -> [decoded bytes]: a batch of independent raw / zlib / gzip streams of any size in one pass on the GPU.  Raises
        ZwzError for the first failing stream, naming its index and status (.index, .stream_status), as zlib.decompress raises.
        out_sizes: each stream's decoded size if known; without it capacities are guessed (gzip: ISIZE from the last 4 bytes; zlib,
        raw: max(4 x input, 64 KiB)), and streams that come back with status 3 are decoded again by themselves with double the
        capacity, up to 2^32 - 1.  split: through zwz_inflate_split_streams_dev (same results)."""
        import numpy as np
        import torch
        w = WRAPS.get(wrap, wrap)
        if w not in (WRAP_RAW, WRAP_ZLIB, WRAP_GZIP):
            raise ValueError("wrap must be raw, zlib or gzip")
        streams = [bytes(s) for s in streams]
        if out_sizes is not None:
            caps, grow = [int(c) for c in out_sizes], False
        else:
            caps, grow = [_guess_cap(s, w) for s in streams], True
        st, out = self._streams_once(torch, np, w, streams, caps, split)
        for i in range(len(streams)):
            while grow and st[i] == STREAM_OVERFLOW and caps[i] < STREAM_MAX_OUT - 1:
                caps[i] = min(2 * caps[i], STREAM_MAX_OUT - 1)
                s1, o1 = self._streams_once(torch, np, w, [streams[i]], [caps[i]], split)
                st[i], out[i] = s1[0], o1[0]
            if st[i] != STREAM_END:
                raise _stream_error("inflate_streams", st[i], i)
        return out

    def deflate_streams_dev(self, wrap, d_in, in_off, in_len, d_out, out_off, out_cap, d_out_len, d_status):
        """zwz_deflate_streams_dev: d_in / d_out uint8 device tensors, d_out_len int64 and d_status int32 device tensors; in_off, in_len,
        out_off, out_cap HOST sequences or numpy arrays (include/zwz.h has the alignment rules).  wrap: "raw" | "zlib" | "gzip" or
        WRAP_*.  Asynchronous; an output that does not fit is status 3 with the needed length in d_out_len, never an exception."""
        self._deflate_streams_dev("zwz_deflate_streams_dev", wrap, d_in, in_off, in_len, d_out, out_off, out_cap, d_out_len, d_status)

    def _deflate_streams_dev(self, fn, wrap, d_in, in_off, in_len, d_out, out_off, out_cap, d_out_len, d_status):
        """the C function `fn` of zwz_deflate_streams_dev's arguments: either piece form"""
        import numpy as np
        arr, n = _u64_arrays(np, "in_off, in_len, out_off and out_cap must have one entry per stream", (in_off, in_len, out_off, out_cap))
        _check(getattr(lib(), fn)(self._h, WRAPS.get(wrap, wrap), d_in.data_ptr(), arr[0].ctypes.data, arr[1].ctypes.data, n, d_out.data_ptr(),
                                  arr[2].ctypes.data, arr[3].ctypes.data, d_out_len.data_ptr(), d_status.data_ptr()), fn)

    def _deflate_streams_index_dev(self, fn, wrap, d_in, in_off, in_len, d_out, out_off, out_cap, d_out_len, d_status, d_idx, idx_off, idx_cap,
                                   d_idx_len, span):
        """the C function `fn` of zwz_deflate_streams_index_dev's arguments: either piece form"""
        import numpy as np
        arr, n = _u64_arrays(np, "in_off, in_len, out_off, out_cap, idx_off and idx_cap must have one entry per stream",
                             (in_off, in_len, out_off, out_cap, idx_off, idx_cap))
        _check(getattr(lib(), fn)(self._h, WRAPS.get(wrap, wrap), d_in.data_ptr(), arr[0].ctypes.data, arr[1].ctypes.data, n, d_out.data_ptr(),
                                  arr[2].ctypes.data, arr[3].ctypes.data, d_out_len.data_ptr(), d_status.data_ptr(), int(span), d_idx.data_ptr(),
                                  arr[4].ctypes.data, arr[5].ctypes.data, d_idx_len.data_ptr()), fn)

    def _deflate_streams(self, dep, index, buffers, wrap, span):
        """deflate_streams, deflate_streams_index and their deflate_dep_ forms: the buffers packed into one blob, every stream given its
        bound, one call of the piece form's _dev wrapper -> [stream bytes], or [(stream bytes, index bytes)] with index"""
        import numpy as np
        import torch
        if dep:
            form, bound, index_bound = "deflate_dep_streams", deflate_dep_stream_bound, deflate_dep_stream_index_bound
            call, index_call = self.deflate_dep_streams_dev, self.deflate_dep_streams_index_dev
        else:
            form, bound, index_bound = "deflate_streams", deflate_stream_bound, deflate_stream_index_bound
            call, index_call = self.deflate_streams_dev, self.deflate_streams_index_dev
        who = form + "_index" if index else form
        w = WRAPS.get(wrap, wrap)
        if w not in (WRAP_RAW, WRAP_ZLIB, WRAP_GZIP):
            raise ValueError("wrap must be raw, zlib or gzip")
        span = int(span or 0)
        if index and index_bound(1, span) == 0:
            raise ValueError("span must be a power of two in 16 KiB .. 1 GiB")
        buffers = [bytes(b) for b in buffers]
        n = len(buffers)
        if n == 0:
            return []
        dev = torch.device("cuda", self.device)
        blob, offs, lens = _pack_host(np, buffers)
        caps = np.array([bound(k, w) for k in lens.tolist()], dtype=np.uint64)
        ooff, total = _layout(np, caps)
        d_in = torch.from_numpy(blob).to(dev)
        d_out = torch.empty(total, dtype=torch.uint8, device=dev)
        d_olen = torch.zeros(n, dtype=torch.int64, device=dev)
        d_st = torch.zeros(n, dtype=torch.int32, device=dev)
        if index:
            # (with span 0 the context's span applies, which may be below the default: the smallest span bounds them all)
            icap = np.array([index_bound(k, span or 16384) for k in lens.tolist()], dtype=np.uint64)
            ioff, itotal = _layout(np, icap)
            d_idx = torch.empty(itotal, dtype=torch.uint8, device=dev)
            d_ilen = torch.zeros(n, dtype=torch.int64, device=dev)
        torch.cuda.synchronize(dev)
        if index:
            index_call(w, d_in, offs, lens, d_out, ooff, caps, d_olen, d_st, d_idx, ioff, icap, d_ilen, span)
        else:
            call(w, d_in, offs, lens, d_out, ooff, caps, d_olen, d_st)
        self.sync()
        st, olen, ilen = d_st.cpu().numpy(), d_olen.cpu().numpy(), d_ilen.cpu().numpy() if index else None
        for i in range(n):
            if st[i] != 0:      # (the dependent form has named deflate_dep_streams here for both of its calls since it was written)
                raise ZwzError("%s: stream %d needs %d bytes, above its bound of %d" % (form if dep else who, i, olen[i], caps[i]))
            if index and ilen[i] == 0:
                raise ZwzError("%s: the index of stream %d does not fit its bound of %d bytes" % (who, i, icap[i]))
        out = _cut(d_out.cpu().numpy(), ooff, olen)
        return list(zip(out, _cut(d_idx.cpu().numpy(), ioff, ilen))) if index else out

    def deflate_streams(self, buffers, wrap="gzip"):
        """[bytes] -> [bytes]: every buffer as one raw / zlib / gzip stream of its own, all in one pass on the GPU.  Each is what libz
        writes at level 6 (or at this codec's level: set_level) with a full flush after every 65 280 bytes, so zlib.decompress /
        gzip.decompress read it."""
        return self._deflate_streams(False, False, buffers, wrap, None)

    def deflate_streams_index_dev(self, wrap, d_in, in_off, in_len, d_out, out_off, out_cap, d_out_len, d_status, d_idx, idx_off, idx_cap,
                                  d_idx_len, span=0):
        """zwz_deflate_streams_index_dev: deflate_streams_dev's arguments and results, and the seek index of stream i -- an entry at the
        first piece start in every `span` decoded bytes, no windows -- at d_idx + idx_off[i] (d_idx a 16-byte aligned CUDA uint8 tensor,
        idx_off and idx_cap HOST sequences, d_idx_len an int64 device tensor: 0 with status 3 or a capacity too small).  span: a power of
        two in 16 KiB .. 1 GiB; 0: the context option "index_span_bytes".  Asynchronous."""
        self._deflate_streams_index_dev("zwz_deflate_streams_index_dev", wrap, d_in, in_off, in_len, d_out, out_off, out_cap, d_out_len, d_status,
                                        d_idx, idx_off, idx_cap, d_idx_len, span)

    def deflate_streams_index(self, buffers, wrap="gzip", span=None):
        """[bytes] -> [(stream, index)]: deflate_streams, and with every stream the seek index of its full-flush points, written as
        the stream is (nothing is decoded): what inflate_indexed, read_ranges and their batch and file forms take.  span: decoded
        bytes an entry covers at least, a power of two in 16 KiB .. 1 GiB (None: the context's "index_span_bytes", 1 MiB)."""
        return self._deflate_streams(False, True, buffers, wrap, span)

    def deflate_stream_file(self, src, dst, wrap="gzip"):
        """One file of any size as one gzip (.gz), zlib or raw DEFLATE stream, streamed through the GPU in slices."""
        _check(lib().zwz_deflate_stream_file(self._h, WRAPS.get(wrap, wrap), os.fsencode(src), os.fsencode(dst)), "zwz_deflate_stream_file")

    def deflate_stream_file_index(self, src, dst, dst_idx, wrap="gzip", span=None):
        """deflate_stream_file that also writes the seek index of the stream's flush points to dst_idx, as it writes the stream
        (zwz_deflate_stream_file_index; `main gzip --write-index`).  span: as deflate_streams_index, for this call (the context option
        "index_span_bytes" is put back afterwards).  Both files appear on success only."""
        self._with_span(span, lambda: _check(lib().zwz_deflate_stream_file_index(self._h, WRAPS.get(wrap, wrap), os.fsencode(src), os.fsencode(dst),
                                                                                 os.fsencode(dst_idx)), "zwz_deflate_stream_file_index"))

    # ---- dependent pieces: pigz's default (include/zwz.h: zwz_deflate_dep_*) ----------------------
    def deflate_dep_streams_dev(self, wrap, d_in, in_off, in_len, d_out, out_off, out_cap, d_out_len, d_status):
        """zwz_deflate_dep_streams_dev: deflate_streams_dev's arguments and results; every piece of 32 768 bytes is compressed with the
        32 512 bytes in front of it as its dictionary.  Needs the default strategy (ZwzError with status E_INVALID otherwise)."""
        self._deflate_streams_dev("zwz_deflate_dep_streams_dev", wrap, d_in, in_off, in_len, d_out, out_off, out_cap, d_out_len, d_status)

    def deflate_dep_streams_index_dev(self, wrap, d_in, in_off, in_len, d_out, out_off, out_cap, d_out_len, d_status, d_idx, idx_off, idx_cap,
                                      d_idx_len, span=0):
        """zwz_deflate_dep_streams_index_dev: deflate_streams_index_dev's arguments and results for streams of dependent pieces; every
        entry but the first carries the 32 512 input bytes in front of it as its window."""
        self._deflate_streams_index_dev("zwz_deflate_dep_streams_index_dev", wrap, d_in, in_off, in_len, d_out, out_off, out_cap, d_out_len, d_status,
                                        d_idx, idx_off, idx_cap, d_idx_len, span)

    def deflate_dep_streams(self, buffers, wrap="gzip"):
        """[bytes] -> [bytes]: every buffer as one raw / zlib / gzip stream of dependent pieces, pigz's default: pieces of 32 768 bytes,
        each primed with the 32 512 bytes in front of it and closed with a sync flush.  Smaller than deflate_streams' (5 % on text,
        almost half on data with long-range repeats) and as parallel to write; zlib.decompress / gzip.decompress read it, the split
        decode finds no cut in it -- write its index along with it (deflate_dep_streams_index) for parallel reads."""
        return self._deflate_streams(True, False, buffers, wrap, None)

    def deflate_dep_streams_index(self, buffers, wrap="gzip", span=None):
        """[bytes] -> [(stream, index)]: deflate_dep_streams, and with every stream its seek index, written as the stream is: an entry
        at the first piece start in every `span` decoded bytes, each but the first with the 32 512 input bytes in front of it as its
        window.  What inflate_indexed, read_ranges and their batch and file forms take.  span: as deflate_streams_index."""
        return self._deflate_streams(True, True, buffers, wrap, span)

    def deflate_dep_stream_file(self, src, dst, wrap="gzip"):
        """One file of any size as one stream of dependent pieces (`main gzip --dependent`)."""
        _check(lib().zwz_deflate_dep_stream_file(self._h, WRAPS.get(wrap, wrap), os.fsencode(src), os.fsencode(dst)), "zwz_deflate_dep_stream_file")

    def deflate_dep_stream_file_index(self, src, dst, dst_idx, wrap="gzip", span=None):
        """deflate_dep_stream_file that also writes the stream's seek index, windows included, to dst_idx (`main gzip --dependent
        --write-index`).  span: as deflate_stream_file_index.  Both files appear on success only."""
        self._with_span(span, lambda: _check(lib().zwz_deflate_dep_stream_file_index(self._h, WRAPS.get(wrap, wrap), os.fsencode(src), os.fsencode(dst),
                                                                                     os.fsencode(dst_idx)), "zwz_deflate_dep_stream_file_index"))

    # ---- ZIP archives (include/zwz.h: zwz_zip_*) ------------------------------------------------
    def zip_dev(self, d_in, in_off, in_len, names, d_out, d_out_len, d_status, meta=None, out_cap=None):
        """zwz_zip_dev: d_in / d_out uint8 device tensors, d_out_len an int64 and d_status an int32 device tensor of one element;
        in_off, in_len HOST sequences; names a list of bytes (or str, stored as UTF-8); meta None or a list of (dos_time, dos_date,
        external_attr).  Asynchronous; an archive that does not fit out_cap (default: d_out's size) is status 3, never an exception."""
        import numpy as np
        what = "in_off, in_len, names and meta must have one entry per buffer"
        (off, ln), n = _u64_arrays(np, what, (in_off, in_len), len(names))
        if meta is not None and len(meta) != n:
            raise ValueError(what)
        c_names = _c_names(names)
        c_meta = (ZipMeta * max(n, 1))(*[ZipMeta(*m) for m in meta]) if meta is not None else None
        _check(lib().zwz_zip_dev(self._h, d_in.data_ptr() if n else None, off.ctypes.data, ln.ctypes.data, c_names, c_meta, n, d_out.data_ptr(),
                                 d_out.numel() if out_cap is None else out_cap, d_out_len.data_ptr(), d_status.data_ptr()), "zwz_zip_dev")

    def zip(self, entries, meta=None):
        """[(name, bytes)] -> the bytes of one ZIP archive, every entry deflated on the GPU in one pass."""
        import numpy as np
        import torch
        entries = [(n, bytes(b)) for n, b in entries]
        dev = torch.device("cuda", self.device)
        blob, offs, lens = _pack_host(np, [b for _, b in entries])
        names = [e[0] for e in entries]
        cap = zip_bound(lens, names)
        d_in = torch.from_numpy(blob).to(dev)
        d_out = torch.empty((cap + 15) // 16 * 16, dtype=torch.uint8, device=dev)
        d_len = torch.zeros(1, dtype=torch.int64, device=dev)
        d_st = torch.zeros(1, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        self.zip_dev(d_in, offs, lens, names, d_out, d_len, d_st, meta, cap)
        self.sync()
        if int(d_st.item()) != 0:
            raise ZwzError("zwz_zip_dev: status %d, %d bytes needed above the bound of %d" % (int(d_st.item()), int(d_len.item()), cap))
        return d_out[:int(d_len.item())].cpu().numpy().tobytes()

    def unzip_dev(self, d_zip, zip_len, entries, d_out, out_off, d_out_len, d_status, d_segments=None):
        """zwz_unzip_dev: d_zip / d_out uint8 device tensors; entries a ctypes array of ZipEntry (zip_index's) and out_off a HOST
        sequence; d_out_len int64, d_status and d_segments int32 device tensors.  Waits for the context's stream while it runs; the
        results are complete after sync().  Never raises for an entry's status."""
        import numpy as np
        (off,), n = _u64_arrays(np, "out_off must have one entry per entry", (out_off,), len(entries))
        _check(lib().zwz_unzip_dev(self._h, d_zip.data_ptr(), zip_len, ctypes.addressof(entries) if n else None, n, d_out.data_ptr(), off.ctypes.data,
                                   d_out_len.data_ptr(), d_status.data_ptr(), d_segments.data_ptr() if d_segments is not None else None),
               "zwz_unzip_dev")

    def unzip(self, data, with_segments=False):
        """ZIP archive bytes -> [(name bytes, decoded bytes, status)] in directory order; status 0 or a verdict (ZIP_*, STREAM_*, 1, 2)
        with whatever was decoded.  with_segments: a fourth item, the pieces decoded in parallel."""
        import numpy as np
        import torch
        data = bytes(data)
        ents = zip_index(data)
        n = len(ents)
        if n == 0:
            return []
        dev = torch.device("cuda", self.device)
        ooff, total = _layout(np, [e.usize for e in ents])
        d_zip = _device_input(torch, data, self.device)
        d_out = torch.zeros(max(total, 16), dtype=torch.uint8, device=dev)
        d_len = torch.zeros(n, dtype=torch.int64, device=dev)
        d_st = torch.zeros(n, dtype=torch.int32, device=dev)
        d_seg = torch.zeros(n, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        self.unzip_dev(d_zip, len(data), ents, d_out, ooff, d_len, d_st, d_seg)
        self.sync()
        olen, st, seg = d_len.cpu().numpy(), d_st.cpu().numpy(), d_seg.cpu().numpy()
        out = []
        for i, (e, dec) in enumerate(zip(ents, _cut(d_out.cpu().numpy(), ooff, olen))):
            item = (data[e.name_off:e.name_off + e.name_len], dec, int(st[i]))
            out.append(item + (int(seg[i]),) if with_segments else item)
        return out

    def zip_dir(self, src_dir, dst_zip):
        """The regular files under src_dir as one ZIP archive (zwz_zip_dir; `main zip`); dst_zip appears only on success."""
        _check(lib().zwz_zip_dir(self._h, os.fsencode(src_dir), os.fsencode(dst_zip)), "zwz_zip_dir")

    def unzip_file(self, src_zip, dst_dir):
        """Extracts src_zip below dst_dir (zwz_unzip_file; `main unzip`).  ZwzError with status E_FORMAT / E_CHECKSUM on a damaged archive
        or a name that would leave dst_dir."""
        _check(lib().zwz_unzip_file(self._h, os.fsencode(src_zip), os.fsencode(dst_dir)), "zwz_unzip_file")

    # ---- directory level -----------------------------------------------------------------------
    def do_compression(self, input_dir, output_dir, file_record, world_rank, world_size=1):
        _check(lib().zwz_compress_dir(self._h, os.fsencode(input_dir), os.fsencode(output_dir), os.fsencode(file_record),
                                      world_rank, world_size), "zwz_compress_dir")

    def do_decompression(self, input_dir, output_dir, world_rank=0, world_size=1, allgather=None):
        """do_decompression(), decompression.cpp:165-178, shared by world_size ranks (one GPU each): whole shards round-robin,
        or record ranges of a shard when there are fewer shards than ranks.  `allgather(values) -> list of every rank's
        values, rank-major` is the launcher's exchange (cli.py passes torch.distributed's); returns the number of files
        this rank found with a wrong MD5."""
        bad = ctypes.c_int(0)

        def _cb(_user, mine, out, count):
            try:
                flat = allgather([int(mine[i]) for i in range(count)])
                for i, v in enumerate(flat):
                    out[i] = int(v)
                return 0
            except Exception:          # never unwind through the C frames
                import traceback
                traceback.print_exc()
                return -1

        cb = ALLGATHER_FN(_cb) if allgather is not None else ctypes.cast(None, ALLGATHER_FN)
        rc = lib().zwz_decompress_dir_ranked(self._h, os.fsencode(input_dir), os.fsencode(output_dir), world_rank, world_size,
                                             cb, None, ctypes.byref(bad))
        _check(rc, "zwz_decompress_dir", md5_mismatches=bad.value)
        return bad.value

    # ---- BGZF (include/zwz.h: zwz_bgzf_*) -------------------------------------------------------
    # bgzf_compress / bgzf_decompress hold their buffers in torch tensors.  torch loads its own HIP runtime, which must open the GPU
    # before this codec's library does: touch the device through torch (torch.zeros(1, device="cuda")) before creating the Codec.
    def bgzf_compress(self, data):
        """bytes -> BGZF bytes; a CUDA uint8 tensor -> a CUDA uint8 tensor of the BGZF stream (on this codec's device)."""
        import torch
        as_tensor = isinstance(data, torch.Tensor)
        d_in = _device_input(torch, data, self.device)
        n = data.numel() if as_tensor else len(data)
        cap = lib().zwz_bgzf_bound(n)
        d_out = torch.empty(cap, dtype=torch.uint8, device=d_in.device)
        d_len = torch.zeros(1, dtype=torch.int64, device=d_in.device)
        torch.cuda.synchronize(d_in.device)
        _check(lib().zwz_bgzf_compress_dev(self._h, d_in.data_ptr(), n, d_out.data_ptr(), cap, d_len.data_ptr()), "zwz_bgzf_compress_dev")
        self.sync()
        n_out = int(d_len.item())
        if n_out < 0:       # ~0: a member body reached the deflate slot's length (include/zwz.h; not producible from 65 280-byte blocks)
            raise ZwzError("zwz_bgzf_compress_dev: a member body was cut")
        out = d_out[:n_out]
        return out if as_tensor else out.cpu().numpy().tobytes()

    def bgzf_decompress(self, data):
        """BGZF bytes -> bytes; a CUDA uint8 tensor -> a CUDA uint8 tensor.  The member headers of bytes are walked on the host, those
        of a tensor on the GPU (nothing of it is copied to the host); everything else runs on the GPU.  ZwzError with status E_FORMAT /
        E_CHECKSUM on damage."""
        import torch
        if isinstance(data, torch.Tensor):
            d_gz, n = _device_input(torch, data, self.device), data.numel()
            d_off, raw = self._bgzf_index_dev(torch, d_gz, n, "zwz_bgzf_index")
            return self._bgzf_decompress_dev(torch, d_gz, n, d_off, raw)
        host = bytes(data)
        offs, raw = bgzf_index(host)
        d_off = torch.tensor(offs, dtype=torch.int64, device=torch.device("cuda", self.device))
        return self._bgzf_decompress_dev(torch, _device_input(torch, host, self.device), len(host), d_off, raw).cpu().numpy().tobytes()

    def _bgzf_decompress_dev(self, torch, d_gz, n, d_off, raw):
        """zwz_bgzf_decompress_dev over the members at d_off (an int64 CUDA tensor) of a stream that decodes to raw bytes, and its
        verdict -> a CUDA tensor of the decoded bytes.  Only the statuses and the first bad member's offset come to the host."""
        count = d_off.numel()
        dev = d_gz.device
        if not count:
            d_off = torch.zeros(1, dtype=torch.int64, device=dev)
        d_out = torch.empty(max(raw, 1), dtype=torch.uint8, device=dev)
        d_len = torch.zeros(1, dtype=torch.int64, device=dev)
        d_st = torch.zeros(max(count, 1), dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        _check(lib().zwz_bgzf_decompress_dev(self._h, d_gz.data_ptr(), n, d_off.data_ptr(), count, d_out.data_ptr(), d_len.data_ptr(),
                                             d_st.data_ptr()), "zwz_bgzf_decompress_dev")
        self.sync()
        bad = torch.nonzero(d_st[:count])
        if bad.numel():
            i = int(bad[0].item())
            s = int(d_st[i].item())
            err = ZwzError("zwz_bgzf_decompress_dev: member %d at byte offset %d: status %d" % (i, int(d_off[i].item()), s))
            err.status = E_CHECKSUM if s in (BGZF_ISIZE_MISMATCH, BGZF_CRC_MISMATCH) else E_FORMAT
            raise err
        return d_out[:int(d_len.item())]

    def _bgzf_index_dev(self, torch, d_gz, n, what):
        """zwz_bgzf_index_dev on an aligned CUDA tensor -> (int64 CUDA tensor of the member offsets, decoded size).  The offsets go
        into a guessed room first (a member per 512 bytes); only a stream of smaller members is walked a second time."""
        count, raw = ctypes.c_uint32(0), ctypes.c_uint64(0)
        cap = n // 512 + 64
        torch.cuda.synchronize(d_gz.device)
        for _ in range(2):
            d_off = torch.empty(cap, dtype=torch.int64, device=d_gz.device)
            torch.cuda.synchronize(d_gz.device)
            rc = lib().zwz_bgzf_index_dev(self._h, d_gz.data_ptr(), n, d_off.data_ptr(), cap, ctypes.byref(count), ctypes.byref(raw))
            if rc == E_INVALID and count.value > cap:
                cap = count.value
                continue
            break
        _check(rc, what)
        return d_off[:count.value], raw.value

    def bgzf_index_dev(self, gz):
        """The member walk of a BGZF stream in a CUDA uint8 tensor, on the GPU: (int64 CUDA tensor of the members' byte offsets, decoded
        size).  ZwzError with status E_FORMAT and the words of bgzf_index for anything that is not a whole member."""
        import torch
        d_gz = _device_input(torch, gz, self.device)
        return self._bgzf_index_dev(torch, d_gz, gz.numel(), "zwz_bgzf_index_dev")

    def bgzf_gzi(self, gz, _what="zwz_bgzf_gzi_dev"):
        """The .gzi bytes of a BGZF stream in a CUDA uint8 tensor (as the module's bgzf_gzi gives them for bytes), walked on the GPU."""
        import torch
        d_gz = _device_input(torch, gz, self.device)
        n = gz.numel()
        torch.cuda.synchronize(d_gz.device)
        size = ctypes.c_uint64(0)
        cap = 8 + 16 * (n // 512 + 64)
        for _ in range(2):
            buf = (ctypes.c_uint8 * cap)()
            rc = lib().zwz_bgzf_gzi_dev(self._h, d_gz.data_ptr(), n, buf, cap, ctypes.byref(size))
            if rc == E_INVALID and size.value > cap:
                cap = size.value
                continue
            break
        _check(rc, _what)
        return ctypes.string_at(buf, size.value)

    def _chunks_dev(self, gz, chunks):
        import numpy as np
        import torch
        d_gz = _device_input(torch, gz, self.device)
        n = gz.numel() if isinstance(gz, torch.Tensor) else len(gz)
        ch = _ranges(np, chunks)
        sizes = np.zeros(max(len(ch), 1), dtype=np.uint64)
        torch.cuda.synchronize(d_gz.device)
        return torch, np, d_gz, n, ch, sizes

    def bgzf_chunk_sizes(self, gz, chunks):
        """Decoded bytes of every chunk (vbeg, vend) of virtual offsets, from the members' ISIZE fields: a list of ints.  gz: BGZF bytes,
        a CUDA uint8 tensor, or the path of a file (str or os.PathLike; read on the host, no GPU work)."""
        if isinstance(gz, (str, os.PathLike)):
            return bgzf_chunk_sizes_file(gz, chunks)
        torch, np, d_gz, n, ch, sizes = self._chunks_dev(gz, chunks)
        _check(lib().zwz_bgzf_chunk_sizes_dev(self._h, d_gz.data_ptr(), n, ch.ctypes.data, len(ch), sizes.ctypes.data), "zwz_bgzf_chunk_sizes_dev")
        return [int(x) for x in sizes[:len(ch)]]

    def bgzf_read_chunks(self, gz, chunks):
        """Chunks [(vbeg, vend), ...] of virtual offsets (compressed offset of a member << 16 | offset inside its decoded block; what
        .bai / .csi / .tbi indexes hold) of a BGZF stream, without an index: bytes -> a list of bytes; a CUDA uint8 tensor -> (one CUDA
        tensor of the chunks concatenated, their sizes).  The member headers between a chunk's compressed offsets are walked on the
        GPU; members holding a requested byte are decoded and checked.  include/zwz.h says what a valid chunk is."""
        torch, np, d_gz, n, ch, sizes = self._chunks_dev(gz, chunks)
        _check(lib().zwz_bgzf_chunk_sizes_dev(self._h, d_gz.data_ptr(), n, ch.ctypes.data, len(ch), sizes.ctypes.data), "zwz_bgzf_chunk_sizes_dev")
        szs, as_tensor = sizes[:len(ch)].reshape(-1, 1), isinstance(gz, torch.Tensor)         # (a view: the read writes the sizes again)
        total = int(szs.sum())
        res = self._ranges_dev(torch, szs, as_tensor, lambda d_out: _check(lib().zwz_bgzf_read_chunks_dev(
            self._h, d_gz.data_ptr(), n, ch.ctypes.data, len(ch), d_out.data_ptr(), total, sizes.ctypes.data), "zwz_bgzf_read_chunks_dev"))
        return (res, [int(x) for x in szs[:, 0]]) if as_tensor else res

    def bgzf_read_chunks_file(self, src, chunks):
        """Chunks of virtual offsets of a BGZF file -> a list of bytes.  Only the file's bytes between a chunk's compressed offsets (and
        the member its end lies in) are read; no .gzi is needed."""
        import numpy as np
        ch = _ranges(np, chunks)
        sizes = np.zeros(max(len(ch), 1), dtype=np.uint64)
        _check(lib().zwz_bgzf_chunk_sizes_file(os.fsencode(src), ch.ctypes.data, len(ch), sizes.ctypes.data), "zwz_bgzf_chunk_sizes_file")
        szs = sizes[:len(ch)].reshape(-1, 1)
        total = int(szs.sum())
        return _ranges_host(np, szs, lambda out: _check(lib().zwz_bgzf_read_chunks_file(
            self._h, os.fsencode(src), ch.ctypes.data, len(ch), out.ctypes.data, total, sizes.ctypes.data), "zwz_bgzf_read_chunks_file"))

    def bgzf_compress_file(self, src, dst):
        """src -> dst as BGZF, streamed through pinned staging (any size); dst appears only on success."""
        _check(lib().zwz_bgzf_compress_file(self._h, os.fsencode(src), os.fsencode(dst)), "zwz_bgzf_compress_file")

    def bgzf_decompress_file(self, src, dst):
        _check(lib().zwz_bgzf_decompress_file(self._h, os.fsencode(src), os.fsencode(dst)), "zwz_bgzf_decompress_file")

    def bgzf_read_ranges(self, gz, ranges, gzi=None):
        """Decoded byte ranges [(offset, length), ...] of a BGZF stream: bytes -> a list of bytes; a CUDA uint8 tensor -> one CUDA tensor
        of the ranges concatenated.  gzi: the stream's .gzi bytes (None: built from the stream -- on the host for bytes, on the GPU for
        a tensor).  Only the members holding a requested byte are decoded and checked."""
        import numpy as np
        import torch
        as_tensor = isinstance(gz, torch.Tensor)
        if gzi is None:
            gzi = self.bgzf_gzi(gz, _what="zwz_bgzf_gzi") if as_tensor else bgzf_gzi(bytes(gz))
        rng = _ranges(np, ranges)
        d_gz = _device_input(torch, gz, self.device)
        n = gz.numel() if as_tensor else len(gz)
        return self._ranges_dev(torch, rng, as_tensor, lambda d_out: _check(lib().zwz_bgzf_read_ranges_dev(
            self._h, d_gz.data_ptr(), n, bytes(gzi), len(gzi), rng.ctypes.data, len(rng), d_out.data_ptr()), "zwz_bgzf_read_ranges_dev"))

    def bgzf_read_ranges_file(self, src, ranges, gzi=None):
        """Decoded byte ranges of a BGZF file -> a list of bytes.  gzi: path of its .gzi (only the touched members are read); None:
        the member headers are walked up to the last requested byte."""
        import numpy as np
        rng = _ranges(np, ranges)
        return _ranges_host(np, rng, lambda out: _check(lib().zwz_bgzf_read_ranges_file(
            self._h, os.fsencode(src), None if gzi is None else os.fsencode(gzi), rng.ctypes.data, len(rng), out.ctypes.data), "zwz_bgzf_read_ranges_file"))

    def set_option(self, name, value):
        """Test / experiment switches of this context (include/zwz.h: zwz_ctx_set_option): "match" = auto | walk | band | lazy |
        autoband | autolazy, "plan" = wave | serial, "inflate_header" = wave | serial.  Every choice produces the same bytes; a form that
        failed its self-test on this device is refused.  "split_min_bytes", "split_budget", "split_max_candidates" (decimal strings):
        the limits of inflate_split_streams_dev.  "leg_bytes", "leg_out_bytes": the windows of inflate_legs_dev; "leg_file_bytes" (default
        67108864; 4096 .. 2^29 - 16) and "leg_file_out_bytes" (default 268435456; 65536 .. 2^32 - 65536), multiples of 16: the staging
        windows of inflate_legs_file.  An empty string restores a default."""
        _check(lib().zwz_ctx_set_option(self._h, name.encode(), value.encode()), "zwz_ctx_set_option")

    def set_chunk_size(self, nbytes):
        """Raw bytes per Chunk for do_compression (0 = the reference's 65535).  Opt-in, not bit-exact with the reference's
        shards; LOSSLESS_CHUNK_SIZE never truncates."""
        _check(lib().zwz_ctx_set_chunk_size(self._h, nbytes), "zwz_ctx_set_chunk_size")

    def set_level(self, level):
        """libz's compression level of every writer of this codec (include/zwz.h: zwz_ctx_set_level): 4, 5 or 6, byte for byte what
        libz 1.2.11 writes at that level; 0 restores the default (6, or ZWZ_LEVEL).  Any other level raises ZwzError (status E_INVALID)
        and leaves the level as it was.  Readers are not affected."""
        _check(lib().zwz_ctx_set_level(self._h, int(level)), "zwz_ctx_set_level")

    @property
    def level(self):
        return lib().zwz_ctx_level(self._h)

    def set_strategy(self, strategy):
        """libz's strategy of every writer of this codec (include/zwz.h: zwz_ctx_set_strategy): "default" / 0, "huffman" / 2 (Z_HUFFMAN_ONLY:
        entropy coding only) or "rle" / 3 (Z_RLE: runs of a byte only), byte for byte what libz 1.2.11 writes under it at any level.  While
        one is set the level and the match option change no byte.  Anything else (1 = Z_FILTERED and 4 = Z_FIXED included) raises ZwzError
        (status E_INVALID) and leaves the strategy as it was.  Readers are not affected."""
        if isinstance(strategy, str):
            if strategy not in STRATEGIES:
                raise ValueError("strategy %r: one of %s" % (strategy, ", ".join(sorted(STRATEGIES))))
            strategy = STRATEGIES[strategy]
        _check(lib().zwz_ctx_set_strategy(self._h, int(strategy)), "zwz_ctx_set_strategy")

    @property
    def strategy(self):
        """The strategy as libz's number: 0 (default), 2 (huffman) or 3 (rle)."""
        return lib().zwz_ctx_strategy(self._h)


def _device_input(torch, data, device):
    """A 16-byte aligned CUDA uint8 tensor holding `data` and readable up to its length rounded up to 16 (the kernels read whole
    16-byte vectors): a suitable tensor as it is, anything else copied."""
    if isinstance(data, torch.Tensor):
        if data.dtype != torch.uint8 or not data.is_cuda:
            raise ValueError("expected a CUDA uint8 tensor")
        t = data.reshape(-1)
        room = t.untyped_storage().nbytes() - t.storage_offset()
        if t.is_contiguous() and t.data_ptr() % 16 == 0 and room >= (t.numel() + 15) // 16 * 16 and t.device.index == device:
            return t
        out = torch.empty((t.numel() + 15) // 16 * 16 or 16, dtype=torch.uint8, device=torch.device("cuda", device))
        out[:t.numel()].copy_(t)
        return out
    n = len(data)
    buf = torch.zeros((n + 15) // 16 * 16 or 16, dtype=torch.uint8)
    if n:
        buf[:n] = torch.frombuffer(bytearray(data), dtype=torch.uint8)
    return buf.to(torch.device("cuda", device))


def _c_names(names):
    """[bytes or str] -> a char*[] for the C ABI (the array keeps the byte strings alive)."""
    raw = [n.encode("utf-8") if isinstance(n, str) else bytes(n) for n in names]
    return (ctypes.c_char_p * max(len(raw), 1))(*raw)


def _ranges(np, ranges, width=2):
    """[(offset, length), ...] -> a C-contiguous (k, 2) uint64 array (ZwzError for a negative value); width 3: (stream, offset, length)."""
    rows = [tuple(int(x) for x in r) for r in ranges]
    if any(len(r) != width for r in rows):
        raise ValueError("every range has %d elements" % width)
    if any(x < 0 for r in rows for x in r):
        err = ZwzError("ranges: stream numbers, offsets and lengths are not negative")
        err.status = E_INVALID
        raise err
    return np.ascontiguousarray(np.array(rows, dtype=np.uint64).reshape(-1, width))


def _split(blob, rng):
    out, o = [], 0
    for n in rng[:, -1].tolist():
        out.append(blob[o:o + n])
        o += n
    return out


def _ranges_host(np, rng, call):
    """The tail of the range and chunk reads of a file: room on the host for what the rows' last column sums to, call(out), then the
    list of the ranges' bytes"""
    total = int(rng[:, -1].sum()) if len(rng) else 0
    out = np.empty(max(total, 1), dtype=np.uint8)
    call(out)
    return _split(out[:total].tobytes(), rng)


def _layout(np, sizes, align=16, slack=0):
    """Slots one behind the other, slot i of sizes[i] rounded up to `align` plus `slack` bytes -> (uint64 offsets, total bytes; 0
    without a slot).  The one batch layout of this file: a caller that needs a minimum takes max(total, 16).  Sizes may come from
    untrusted headers (a ZIP directory), so the sums are Python integers, which do not wrap: OverflowError for a negative slot or a
    total of 2^64 or more, before anything is sized by an offset."""
    off, total = [], 0
    for s in (sizes.tolist() if hasattr(sizes, "tolist") else sizes):
        slot = (int(s) + align - 1) // align * align + slack
        if slot < 0:
            raise OverflowError("batch layout: a slot of %d bytes" % slot)
        off.append(total)
        total += slot
    if total >= 1 << 64:
        raise OverflowError("batch layout: the slots take %d bytes, which 64 bits do not hold" % total)
    return np.array(off, dtype=np.uint64), total


def _blob(np, size, bufs, offs):
    """A zeroed uint8 host array of `size` bytes holding bufs[i] at offs[i] (zeroed: the kernels read whole 16-byte vectors past a
    buffer's end)"""
    blob = np.zeros(size, dtype=np.uint8)
    for b, o in zip(bufs, offs.tolist()):
        blob[o:o + len(b)] = np.frombuffer(bytes(b), dtype=np.uint8)
    return blob


def _pack_host(np, bufs):
    """[bytes] -> (one zeroed blob of at least 16 bytes holding them at multiples of 16, uint64 offsets, uint64 lengths)"""
    lens = np.array([len(b) for b in bufs], dtype=np.uint64)
    offs, total = _layout(np, lens)
    return _blob(np, max(total, 16), bufs, offs), offs, lens


def _cut(host, offs, lens):
    """[the lens[i] bytes at offs[i] of a host array]"""
    return [host[o:o + n].tobytes() for o, n in zip(offs.tolist(), lens.tolist())]


def _u64_arrays(np, what, seqs, n=None):
    """Host sequences -> (contiguous uint64 arrays as the C ABI reads them, n); ValueError(what) unless each has n elements (None: as
    many as the first)"""
    arr = [np.ascontiguousarray(a, dtype=np.uint64) for a in seqs]
    n = arr[0].size if n is None else n
    if any(a.size != n for a in arr):
        raise ValueError(what)
    return arr, n


def _guess_cap(stream, w):
    """The decoded capacity to try first for a stream of unknown size: gzip's ISIZE, else max(4 x input, 64 KiB); below 2^32"""
    guess = max(4 * len(stream), 1 << 16)
    if w == WRAP_GZIP and len(stream) >= 4:
        guess = max(int.from_bytes(stream[-4:], "little"), 1)
    return min(guess, STREAM_MAX_OUT - 1)


def _stream_error(who, st, i=None):
    """The ZwzError of a stream that ended with status st (stream i of a batch; None: the call's only one)"""
    err = ZwzError("%s: status %d" % (who, st) if i is None else "%s: stream %d: status %d" % (who, i, st))
    err.status, err.index, err.stream_status = E_FORMAT, i or 0, int(st)
    return err


def sort_files_by_size(path):
    buf = ctypes.create_string_buffer(4096)
    _check(lib().zwz_sort_files_by_size(os.fsencode(path), buf, len(buf)), "zwz_sort_files_by_size")
    return buf.value.decode()


def count_non_empty_lines(file_path):
    return lib().zwz_count_non_empty_lines(os.fsencode(file_path))


def md5_of_file(file_path):
    buf = ctypes.create_string_buffer(33)
    lib().zwz_md5_of_file(os.fsencode(file_path), buf)
    return buf.value.decode()


_default = None


def _codec():
    global _default
    if _default is None:
        _default = Codec(int(os.environ.get("LOCAL_RANK", "0")))
    return _default


def do_compression(input_dir, output_dir, file_record, world_rank, world_size=1):
    _codec().do_compression(input_dir, output_dir, file_record, world_rank, world_size)


def do_decompression(input_dir, output_dir, world_rank=0, world_size=1, allgather=None):
    return _codec().do_decompression(input_dir, output_dir, world_rank, world_size, allgather)


def inflate_stream(data, wrap="gzip", out_size=None):
    return _codec().inflate_stream(data, wrap, out_size)


def inflate_stream_index(data, wrap="gzip", span=None, out_size=None):
    return _codec().inflate_stream_index(data, wrap, span, out_size)


def inflate_split_index_file(src, dst, dst_idx, wrap="gzip", span=None):
    return _codec().inflate_split_index_file(src, dst, dst_idx, wrap, span)


def deflate_stream_file_index(src, dst, dst_idx, wrap="gzip", span=None):
    return _codec().deflate_stream_file_index(src, dst, dst_idx, wrap, span)


class PackedIndexes:
    """The seek indexes of a batch in one host buffer (pack_indexes): .blob (uint8), .off and .len (uint64, one element a stream)."""
    def __init__(self, blob, off, length):
        self.blob, self.off, self.len, self.n = blob, off, length, len(off)


def pack_indexes(indexes, idx_off=None):
    """[index bytes] -> PackedIndexes: index i at idx_off[i] of one host buffer (multiples of 16; None: one behind the other), the
    layout Codec.inflate_indexed_batch_dev and Codec.read_ranges_batch_dev take, and their d_idx on the device."""
    import numpy as np
    lens = np.array([len(x) for x in indexes], dtype=np.uint64)
    if idx_off is None:
        off, _ = _layout(np, lens)
    else:
        off = np.ascontiguousarray(idx_off, dtype=np.uint64)
        if len(off) != len(lens):
            raise ValueError("one offset per index")
    return PackedIndexes(_blob(np, int((off + lens).max()) + 16 if len(lens) else 16, indexes, off), off, lens)


def index_info(index):
    """A seek index checked as every reader checks it (ZwzError with status E_FORMAT) -> {"wrap", "stream_len", "decoded_len", "count"}.
    Needs no GPU."""
    index = bytes(index)
    w, n, d, k = ctypes.c_int(0), ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint32(0)
    _check(lib().zwz_inflate_index_info(index, len(index), ctypes.byref(w), ctypes.byref(n), ctypes.byref(d), ctypes.byref(k)), "zwz_inflate_index_info")
    return {"wrap": w.value, "stream_len": n.value, "decoded_len": d.value, "count": k.value}


def inflate_stream_file(src, dst, wrap="gzip"):
    return _codec().inflate_stream_file(src, dst, wrap)


def deflate_stream_bound(n, wrap="gzip"):
    """Worst-case size of one stream of n input bytes from Codec.deflate_streams (about 1.0009 n); needs no GPU."""
    return lib().zwz_deflate_stream_bound(n, WRAPS.get(wrap, wrap))


def deflate_stream_index_bound(n, span=None):
    """Worst-case size of the index Codec.deflate_streams_index writes for a stream of n input bytes: 64 + 24 (n // span + 1) rounded
    up to 16 (span None: 1 MiB); 0 for a span that is not allowed.  Needs no GPU."""
    return lib().zwz_deflate_stream_index_bound(n, int(span or 0))


def deflate_dep_stream_bound(n, wrap="gzip"):
    """Worst-case size of one stream of n input bytes from Codec.deflate_dep_streams (about 1.002 n); needs no GPU."""
    return lib().zwz_deflate_dep_stream_bound(n, WRAPS.get(wrap, wrap))


def deflate_dep_stream_index_bound(n, span=None):
    """The exact size of the index Codec.deflate_dep_streams_index writes for a stream of n input bytes: with step = max(span, 32 768)
    and count = ceil(n / step) entries (1 for n = 0), 64 + 24 count + 32 512 (count - 1) rounded up to 16 (span None: 1 MiB); 0 for a
    span that is not allowed.  Needs no GPU."""
    return lib().zwz_deflate_dep_stream_index_bound(n, int(span or 0))


def zip_index(data):
    """The entries of a ZIP archive in memory, walked on the host (no GPU): a ctypes array of ZipEntry in directory order.  ZwzError
    with status E_FORMAT names the entry and the byte offset."""
    data = bytes(data)
    count = ctypes.c_uint32(0)
    _check(lib().zwz_zip_index(data, len(data), None, 0, ctypes.byref(count)), "zwz_zip_index")
    ents = (ZipEntry * count.value)()
    if count.value:
        _check(lib().zwz_zip_index(data, len(data), ctypes.addressof(ents), count.value, ctypes.byref(count)), "zwz_zip_index")
    return ents


def zip_bound(lengths, names):
    """Worst-case archive size for buffers of these lengths under these names; needs no GPU."""
    import numpy as np
    ln = np.ascontiguousarray(lengths, dtype=np.uint64)
    if ln.size != len(names):
        raise ValueError("one length per name")
    return lib().zwz_zip_bound(ln.ctypes.data, _c_names(names), len(names))


def zip_dir(src_dir, dst_zip):
    _codec().zip_dir(src_dir, dst_zip)


def unzip_file(src_zip, dst_dir):
    _codec().unzip_file(src_zip, dst_dir)


def bgzf_bound(n):
    """Worst-case BGZF size of n input bytes (EOF member included); needs no GPU."""
    return lib().zwz_bgzf_bound(n)


def bgzf_index(gz):
    """(member offsets, total decoded bytes) of a BGZF byte string, walked on the host (no GPU)."""
    import numpy as np
    count, raw = ctypes.c_uint32(0), ctypes.c_uint64(0)
    _check(lib().zwz_bgzf_index(gz, len(gz), None, 0, ctypes.byref(count), ctypes.byref(raw)), "zwz_bgzf_index")
    offs = np.zeros(max(count.value, 1), dtype=np.uint64)
    _check(lib().zwz_bgzf_index(gz, len(gz), offs.ctypes.data, count.value, ctypes.byref(count), ctypes.byref(raw)), "zwz_bgzf_index")
    return [int(o) for o in offs[:count.value]], raw.value


def bgzf_compress(data):
    return _codec().bgzf_compress(data)


def bgzf_decompress(data):
    return _codec().bgzf_decompress(data)


def bgzf_compress_file(src, dst):
    _codec().bgzf_compress_file(src, dst)


def bgzf_decompress_file(src, dst):
    _codec().bgzf_decompress_file(src, dst)


def bgzf_gzi(gz):
    """The .gzi index (include/zwz.h) of a BGZF byte string, built on the host (no GPU)."""
    gz = bytes(gz)
    n = ctypes.c_uint64(0)
    _check(lib().zwz_bgzf_gzi(gz, len(gz), None, 0, ctypes.byref(n)), "zwz_bgzf_gzi")
    buf = ctypes.create_string_buffer(n.value)
    _check(lib().zwz_bgzf_gzi(gz, len(gz), buf, n.value, ctypes.byref(n)), "zwz_bgzf_gzi")
    return buf.raw[:n.value]


def bgzf_voffsets(gzi, offsets):
    """Decoded byte offsets -> virtual offsets (compressed offset of the member << 16 | offset inside its block) by a stream's .gzi
    bytes: a list of ints.  Host only.  The member of an offset is the last index entry at or below it, as range reads resolve it."""
    import numpy as np
    offs = np.ascontiguousarray(np.array([int(x) for x in offsets], dtype=np.uint64))
    out = np.zeros(max(len(offs), 1), dtype=np.uint64)
    gzi = bytes(gzi)
    _check(lib().zwz_bgzf_voffsets(gzi, len(gzi), offs.ctypes.data, len(offs), out.ctypes.data), "zwz_bgzf_voffsets")
    return [int(x) for x in out[:len(offs)]]


def bgzf_chunk_sizes_file(src, chunks):
    """Decoded bytes of every chunk (vbeg, vend) of virtual offsets of a BGZF file, from a host walk of the member headers between
    the chunks' compressed offsets: a list of ints.  No GPU."""
    import numpy as np
    ch = _ranges(np, chunks)
    sizes = np.zeros(max(len(ch), 1), dtype=np.uint64)
    _check(lib().zwz_bgzf_chunk_sizes_file(os.fsencode(src), ch.ctypes.data, len(ch), sizes.ctypes.data), "zwz_bgzf_chunk_sizes_file")
    return [int(x) for x in sizes[:len(ch)]]


def bgzf_gzi_file(src, dst):
    """src's .gzi written to dst, streamed (`bgzip -r`; no GPU); dst appears only on success."""
    _check(lib().zwz_bgzf_gzi_file(os.fsencode(src), os.fsencode(dst)), "zwz_bgzf_gzi_file")
