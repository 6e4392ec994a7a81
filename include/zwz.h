/*
 * zwz.h -- C ABI of the MI355X-native chunk codec: the drop-in boundary for the reference's hot path.
 *
 * The reference (JoernZheng/parallel-data-compression-and-decompression) has no plugin/FFI
 * surface; its seams are C++ prototypes in process.hpp:37-42 and two inline zlib call sites.
 * Each entry point below names the reference interface it replaces:
 *
 *   zwz_deflate_batch*     the zlib call pair in consumer(), compression.cpp:119-134
 *                          (deflateInit level 6 / deflate(Z_FINISH) into a 65535-byte buffer /
 *                          deflateEnd), once per Chunk (process.hpp:21-28) -- here for a batch
 *   zwz_inflate_batch*     decompress_chunk(), decompression.cpp:11-37 (inflateInit / inflate
 *                          loop / inflateEnd, return codes ignored), once per CompressedChunk
 *                          (process.hpp:30-35) -- here for a batch
 *   zwz_compress_dir       do_compression(input_dir, output_dir, file_record, world_rank),
 *                          process.hpp:39 / compression.cpp:161-194 (+ the rank < file_count
 *                          guard of compress(), main.cpp:44-51)
 *   zwz_decompress_dir     do_decompression(input_dir, output_dir), process.hpp:40 /
 *                          decompression.cpp:165-178
 *   zwz_sort_files_by_size sort_files_by_size(path), process.hpp:37 / file_sort.cpp:24-43
 *   zwz_count_non_empty_lines  count_non_empty_lines(file), process.hpp:38 / file_tools.cpp:6-23
 *   zwz_md5_of_file        md5_of_file(path), process.hpp:41 / verification.cpp:6-30
 *   zwz_md5_files_dev      the same digest for many files at once, from their chunks in device memory
 *                          (the call sites compression.cpp:98 and decompression.cpp:136 batched)
 *
 * Conventions: plain pointers and sizes, no exceptions across the boundary, 0 = success and
 * negative zwz_status codes otherwise, caller owns every buffer.  A context binds one GPU, one
 * HIP stream and a device workspace; calls on one context are serialised by the caller, distinct
 * contexts are independent.  There is no CPU fallback: without a usable GPU zwz_ctx_create fails.
 *
 * Bit-exactness contract: for every chunk, out[0..out_len) equals the first min(len, 65535)
 * bytes of zlib 1.2.11's level-6 stream of that chunk -- what the reference stores in a .zwz
 * record.
 */
#ifndef ZWZ_H
#define ZWZ_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZWZ_CHUNK_SIZE 65535u      /* process.hpp:12 CHUNK_SIZE */
#define ZWZ_DEV_STRIDE 65536u      /* chunk slot stride in device buffers (16-byte aligned slots) */
#define ZWZ_MD5_HEX_LEN 32u        /* process.hpp:14 MD5_DATA_SIZE */
#define ZWZ_LOSSLESS_CHUNK_SIZE 65509u /* opt-in: largest chunk whose stream always fits 65535 bytes: 4 stored blocks, n + 26 */

typedef enum zwz_status {
    ZWZ_OK = 0,
    ZWZ_E_INVALID = -1,   /* bad argument (null pointer, misaligned device slot, size > 65535) */
    ZWZ_E_HIP = -2,       /* a HIP runtime call failed; zwz_last_error() has the text */
    ZWZ_E_NO_DEVICE = -3, /* no usable gfx950 device (none visible, or it fails every one of zwz_ctx_create's self-tests: see zwz_ctx_set_option) */
    ZWZ_E_IO = -4,        /* file system error */
    ZWZ_E_NOMEM = -5,
    ZWZ_E_FORMAT = -6,    /* malformed .zwz shard, or input that is not BGZF (zwz_bgzf_*) */
    ZWZ_E_CHECKSUM = -7   /* a BGZF member's CRC-32 or ISIZE does not match its decoded bytes */
} zwz_status;

/* Per-chunk status written by the inflate entry points (the reference ignores zlib's return
 * codes, decompression.cpp:31; these only report, they never suppress output). */
typedef enum zwz_inflate_status {
    ZWZ_INF_END = 0,         /* final block reached */
    ZWZ_INF_NEED_INPUT = 1,  /* payload ended early (reference-truncated chunk): partial output kept */
    ZWZ_INF_DATA_ERROR = 2,  /* invalid stream: output up to the error kept */
    ZWZ_INF_OVERFLOW = 3     /* stream decodes past 65535 bytes (not producible by the reference) */
} zwz_inflate_status;

/* Per-member status of zwz_bgzf_decompress_dev beyond the inflate codes above (0 = the member decoded and matched). */
typedef enum zwz_bgzf_member_status {
    ZWZ_BGZF_BAD_MEMBER = 16,      /* the member's header or size does not parse (an offset list not made by zwz_bgzf_index) */
    ZWZ_BGZF_ISIZE_MISMATCH = 17,  /* decoded length differs from the stored ISIZE */
    ZWZ_BGZF_CRC_MISMATCH = 18     /* CRC-32 of the decoded bytes differs from the stored one */
} zwz_bgzf_member_status;

typedef struct zwz_ctx zwz_ctx;

const char *zwz_strerror(int status);
const char *zwz_last_error(void);               /* thread-local detail for ZWZ_E_HIP / ZWZ_E_IO */
int zwz_device_count(int *count);

/* max_batch_chunks bounds the device workspace (~680 KiB per chunk); larger batches are
 * processed in slices.  0 selects the default (8192). */
int zwz_ctx_create(int device, uint32_t max_batch_chunks, zwz_ctx **ctx);
void zwz_ctx_destroy(zwz_ctx *ctx);
void *zwz_ctx_stream(zwz_ctx *ctx);             /* the context's hipStream_t */
int zwz_ctx_sync(zwz_ctx *ctx);

/* ---- device-resident batches (asynchronous on the context's stream) ------------------------
 * d_in + d_in_off[i] is chunk i: d_in_len[i] <= 65535 bytes, d_in and every d_in_off[i] multiples
 * of 16, and the slot readable up to its length rounded up to 16 (the kernels stream whole 16-byte
 * vectors; the extra bytes never influence a result).  Chunk i's result goes to
 * d_out + i * out_stride (out_stride % 16 == 0, >= 65536) with its length in d_out_len[i].
 * All pointers are device memory on the context's GPU.
 * Level (zwz_ctx_set_level): a chunk's deflate output is the first min(len, 65535) bytes of libz 1.2.11's level-N zlib stream of the
 * chunk, N = the context's level (6 unless set; the header is 78 9c at 6, 78 5e at 4 and 5).  Inflate reads every level. */
int zwz_deflate_batch_dev(zwz_ctx *ctx, const uint8_t *d_in, const uint64_t *d_in_off, const uint32_t *d_in_len,
                          uint32_t n, uint8_t *d_out, uint64_t out_stride, uint32_t *d_out_len);
int zwz_inflate_batch_dev(zwz_ctx *ctx, const uint8_t *d_in, const uint64_t *d_in_off, const uint32_t *d_in_len,
                          uint32_t n, uint8_t *d_out, uint64_t out_stride, uint32_t *d_out_len, uint32_t *d_status);

/* ---- host-buffer batches (synchronous; staged through pinned memory) ------------------------
 * in + in_off[i] is chunk i; results at out + i * 65535, lengths in out_len[i]. */
int zwz_deflate_batch(zwz_ctx *ctx, const uint8_t *in, const uint64_t *in_off, const uint32_t *in_len, uint32_t n,
                      uint8_t *out, uint32_t *out_len);
int zwz_inflate_batch(zwz_ctx *ctx, const uint8_t *in, const uint64_t *in_off, const uint32_t *in_len, uint32_t n,
                      uint8_t *out, uint32_t *out_len, uint32_t *status);

/* ---- stage timing (HIP events on the context's stream) -------------------------------------
 * With profiling on, every deflate slice records events around its 6 stages; the accumulated
 * milliseconds since the last reset are returned in ms[0..6) in pipeline order -- links (marks of the
 * chain-heavy chunks, chain links of the others, the sorted arrays: lz_dense_list, lz_lists, lz_links,
 * lz_sort, lz_place), match (lz_match, lz_match_band), parse, blockify, plan (three kernels), encode
 * (two kernels) --, ms[6] = inflate (its launch order + the kernel). */
#define ZWZ_NUM_STAGES 7
int zwz_ctx_set_profiling(zwz_ctx *ctx, int on);
int zwz_ctx_stage_ms(zwz_ctx *ctx, float *ms, int reset);

/* MD5 (RFC 1321) of n_files files whose bytes already sit in device chunk slots: file i is the concatenation
 * of slots d_files[2i] .. d_files[2i] + d_files[2i+1] - 1 (slot k = d_in_len[k] bytes at d_in + d_in_off[k]).
 * d_digests receives 16 bytes per file (4-byte aligned).  Asynchronous on the context's stream.  One lane per
 * file: meant for many small and medium files; hash very large files on the host (zwz_md5_of_file). */
int zwz_md5_files_dev(zwz_ctx *ctx, const uint8_t *d_in, const uint64_t *d_in_off, const uint32_t *d_in_len,
                      const uint32_t *d_files, uint32_t n_files, uint8_t *d_digests);

/* ---- directory level (the reference's per-rank pipeline) ------------------------------------ */
int zwz_sort_files_by_size(const char *src_dir, char *record_path_out, size_t cap);
int zwz_count_non_empty_lines(const char *file_path);
int zwz_md5_of_file(const char *path, char hex_out[33]);
/* Shard `rank` of `nranks`: lines i of file_record with i % nranks == rank, written to
 * <dst>/compressed_<rank>.zwz.  Ranks >= the number of listed files write nothing. */
int zwz_compress_dir(zwz_ctx *ctx, const char *src_dir, const char *dst_dir, const char *file_record, int rank,
                     int nranks);
/* Every <src>/ *.zwz -> files under <dst>; md5_mismatches (optional) counts files whose MD5
 * differs from the stored one (the reference only prints them, decompression.cpp:140-146).
 * A shard that ends inside a record is decoded up to the damage (as the reference's reader would) and the
 * call returns ZWZ_E_FORMAT. */
int zwz_decompress_dir(zwz_ctx *ctx, const char *src_dir, const char *dst_dir, int *md5_mismatches);

/* The same job shared by nranks processes, one GPU each (the reference parallelises over shards only,
 * decompression.cpp:165-178, and decodes inside a shard serially, :65-154).  Shards are taken in name order: with at
 * least nranks of them, shard j belongs to rank j % nranks and no rank talks to another.  With fewer (BASELINE config 5:
 * one shard holding one huge file) every shard is split: rank r inflates the r-th contiguous range of its records, and
 * the ranks all-gather how many bytes each decoded (a chunk's place in its file is the sum of the decoded lengths in
 * front of it).  `exchange` is that all-gather: every rank calls it with `count` values in `mine` and receives
 * nranks * count values, rank-major, in `all`; it returns 0 on success.  It doubles as the barrier before MD5
 * verification, is called the same number of times on every rank, and may be NULL when nranks == 1 or there is a shard
 * per rank.  The launcher supplies it: torch.distributed / RCCL (cli.py), marker files (csrc/main.cpp).  <dst> must be
 * one file system for all ranks.  md5_mismatches counts the files THIS rank verified. */
typedef int (*zwz_allgather_u64_fn)(void *user, const uint64_t *mine, uint64_t *all, uint32_t count);
int zwz_decompress_dir_ranked(zwz_ctx *ctx, const char *src_dir, const char *dst_dir, int rank, int nranks,
                              zwz_allgather_u64_fn exchange, void *user, int *md5_mismatches);

/* "A final gather of per-shard .zwz blobs" (north star; the reference has none: every MPI rank writes compressed_<rank>.zwz itself,
 * compression.cpp:151-170).  The protocol, stated once for every launcher (csrc/main.cpp: RCCL; cli.py: torch.distributed): sizes and
 * readiness by all-gather, then every rank's shard travels to rank 0 in pieces of at most piece_bytes (0: 64 MiB), one send for one
 * receive; an I/O failure on either side marks a shard bad without leaving any send unmatched.  Rank 0 writes
 * <out_dir>/compressed_<r>.zwz (through a .part name).  my_shard_path: this rank's shard, "" or NULL = nothing to contribute (rank 0, an
 * idle or failed rank).  Returns 1 only if every rank saw every transfer and every write succeed -- only then may a sender delete its
 * copy.  The hooks move HOST memory; all of them return 0 on success; a failing send / recv / all-gather means the transport is gone.
 * prepare / release (optional): the transport's own staging for pieces of that size.  No GPU call is made by the library here. */
typedef struct zwz_gather_hooks {
    void *user;
    int (*allgather_u64)(void *user, const uint64_t *mine, uint64_t *all, uint32_t count);
    int (*send)(void *user, const void *buf, uint64_t nbytes, int to_rank);
    int (*recv)(void *user, void *buf, uint64_t nbytes, int from_rank);
    int (*prepare)(void *user, uint64_t piece_bytes);
    void (*release)(void *user);
} zwz_gather_hooks;
int zwz_gather_shards(int rank, int nranks, const char *my_shard_path, const char *out_dir, uint64_t piece_bytes,
                      const zwz_gather_hooks *hooks);

/* Opt-in, never the default, NOT bit-exact with the reference's shards: raw bytes per Chunk for
 * zwz_compress_dir, 1..65535; 0 restores the reference's 65535 (process.hpp:12).  ZWZ_LOSSLESS_CHUNK_SIZE (65509) is the
 * largest size whose level-6 stream always fits the reference's 65535-byte payload buffer (compression.cpp:127-132), so
 * nothing is truncated and every file round-trips with a matching MD5; the container is unchanged and the reference's
 * decoder reads such shards.  The environment variables ZWZ_LOSSLESS=1 / ZWZ_CHUNK_SIZE=<n> do the same for the CLI. */
int zwz_ctx_set_chunk_size(zwz_ctx *ctx, uint32_t bytes);

/* The compression level of EVERY writer of this context -- zwz_deflate_batch(_dev), zwz_compress_dir, zwz_bgzf_compress_dev / _file,
 * zwz_deflate_streams_dev / zwz_deflate_stream_file, zwz_zip_dev / zwz_zip_dir -- and of no reader.  4, 5 and 6 select libz 1.2.11's level of that
 * number: the output is byte for byte what libz writes at it (deflateInit(level); gzip -N, bgzip -l N, zip -N).  0 restores the default, 6.
 * Any other value is ZWZ_E_INVALID, zwz_last_error() says why, and the level stays what it was:
 *   1-3  libz's deflate_fast skips hash insertions inside matches, so the chains depend on the parse and the position-parallel search does not hold;
 *   7-9  need chains of 256-4096 candidates and max_lazy up to 258: past the 128-wide band, its key field and the 13-position parse step;
 *   0    is a different encoder (stored blocks only).
 * Levels 4 and 5 run level 6's algorithm (deflate_slow + longest_match) with smaller numbers -- good_length / max_lazy / nice_length / max_chain
 * 4 / 4 / 16 / 16 and 8 / 16 / 32 / 32 against 8 / 16 / 128 / 128 -- about 3 % of ratio on text for less search; DESIGN.md section 20 has the
 * measured table.  The default comes from the environment variable ZWZ_LEVEL, read once in zwz_ctx_create (a value that is not understood is
 * reported on stderr and ignored).  Calls on a context are serialised by the caller, so the level may change between any two calls.
 * Wrappers as libz writes them: the zlib header is 78 5e at 4 and 5 (FLEVEL 1) and 78 9c at 6; gzip, BGZF and ZIP headers do not depend on the
 * level, nor do zwz_bgzf_bound, zwz_deflate_stream_bound and zwz_zip_bound (their worst case is stored blocks).
 * For zwz_compress_dir a level other than 6 is opt-in and NOT bit-exact with the reference's shards, exactly like the chunk size: the container is
 * unchanged, and the reference's decoder and `main decompress` read such shards.  zwz_ctx_level returns the current level. */
int zwz_ctx_set_level(zwz_ctx *ctx, int level);
int zwz_ctx_level(zwz_ctx *ctx);

/* libz's compression STRATEGY of every writer of this context (the same writers as the level's), and of no reader.  The numbers are libz's:
 *   ZWZ_STRATEGY_DEFAULT (0)  deflate_slow at the context's level, as above;
 *   ZWZ_STRATEGY_HUFFMAN (2)  Z_HUFFMAN_ONLY: every byte a literal, entropy coding only (pigz -H, PNG writers);
 *   ZWZ_STRATEGY_RLE     (3)  Z_RLE: matches at distance 1 only -- runs of a byte (pigz -U).
 * Under 2 and 3 the output is byte for byte what libz 1.2.11 writes after deflateInit2(level, Z_DEFLATED, wbits, 8, strategy) for ANY level
 * 1-9: the level stays settable and readable and changes no byte until the strategy is 0 again, and the "match" option chooses nothing.  No
 * chain is built and nothing is searched: one memory-bound kernel stands in for the search and the parse (DESIGN.md section 21 has the measured
 * table).  Wrappers as libz writes them: the zlib header is 78 01 (FLEVEL 0), the gzip header's XFL byte is 04 (1f 8b 08 00 00 00 00 00 04 03);
 * BGZF and ZIP headers do not change, nor do the .gzi index, zwz_bgzf_bound, zwz_deflate_stream_bound and zwz_zip_bound (their worst case is
 * stored blocks, and a chunk still has at most five).  Ordinary DEFLATE: every reader here and elsewhere decodes it.
 * 1 (Z_FILTERED) and 4 (Z_FIXED) -- and any other value -- are ZWZ_E_INVALID, zwz_last_error() says why, and the strategy stays what it was:
 * Z_FILTERED changes which short matches the lazy parse accepts (three parse forms at three levels), Z_FIXED the plan's choice of block type (its
 * three forms); each is its own piece of work.  The default comes from the environment variable ZWZ_STRATEGY=huffman|rle|default, read once in
 * zwz_ctx_create (a value that is not understood is reported on stderr and ignored).  For zwz_compress_dir a strategy is opt-in and NOT bit-exact
 * with the reference's shards, exactly like the level.  zwz_ctx_strategy returns the current strategy. */
#define ZWZ_STRATEGY_DEFAULT 0
#define ZWZ_STRATEGY_HUFFMAN 2
#define ZWZ_STRATEGY_RLE 3
int zwz_ctx_set_strategy(zwz_ctx *ctx, int strategy);
int zwz_ctx_strategy(zwz_ctx *ctx);

/* Test and diagnosis switches of one context; no reference counterpart (the reference's zlib has one code path,
 * compression.cpp:119-134 / decompression.cpp:16-36) and no effect on any byte produced -- they choose between kernels that compute
 * the same thing, so that tests can drive each of them and a device that fails a self-test at zwz_ctx_create still gets a codec:
 *   "match"           "auto" (default: per chunk, by a sample of its trigrams) | "walk" (chain links + walk) | "band" (sort + banded search)
 *                     | "lazy" (sort + lz_lazy: search and lazy parse in one kernel, the searches on demand) | "autoband" / "autolazy"
 *                     (the per-chunk choice with the band / lz_lazy for chain-heavy chunks; "auto" is "autoband")
 *   "plan"            "wave" (default) | "serial"   block flush: a lane per heap + a wave per block, or all of it on one lane
 *   "inflate_header"  "wave" (default) | "serial"   a block's decoding tables by the whole wave, or by lane 0
 * Defaults come from ZWZ_MATCH / ZWZ_PLAN / ZWZ_INFLATE_HEADER, read once in zwz_ctx_create (never per launch; a value that is not
 * understood is reported on stderr and ignored).  ZWZ_E_INVALID for an unknown name or value; ZWZ_E_NO_DEVICE for a kernel form
 * that failed its self-test on this device at zwz_ctx_create -- it stays off ("auto" / "" then mean what the device can run).
 * "split_min_bytes", "split_budget" and "split_max_candidates" (decimal numbers) belong to zwz_inflate_split_streams_dev and are
 * described there; they decide which streams are decoded in pieces, never what is decoded. */
int zwz_ctx_set_option(zwz_ctx *ctx, const char *name, const char *value);

/* ---- BGZF (blocked gzip, SAM/BAM specification section 4.1): .gz files that gzip, zcat and htslib read -----------------------
 * Compression cuts the input into blocks of 65280 bytes (htslib's BGZF_BLOCK_SIZE; the last one shorter, none for an empty input)
 * and writes each as one gzip member: 1f 8b 08 04 | 00000000 | 00 ff | 06 00 | 'B' 'C' 02 00 | BSIZE-1 (u16 LE) | raw deflate |
 * CRC-32 (LE) | ISIZE (LE), the raw deflate being bytes [2, len - 4) of the block's zlib 1.2.11 level-6 stream (the bytes of
 * zwz_deflate_batch_dev; level-N under zwz_ctx_set_level(N) -- headers, block size and zwz_bgzf_bound do not change), then the standard 28-byte EOF member.  Decompression accepts any BGZF: other extra subfields around BC,
 * any deflate level, empty members anywhere (two BGZF files one after the other), a missing EOF member; it rejects (ZWZ_E_FORMAT,
 * zwz_last_error() naming the member and its byte offset) a member without BC, a BSIZE past the end, trailing bytes that are not
 * a member and ISIZE > 65535.  A CRC-32 or ISIZE mismatch is ZWZ_E_CHECKSUM.  All of it runs on the GPU; the header walk has a host
 * form (zwz_bgzf_index) and a device form (zwz_bgzf_index_dev, below). */
uint64_t zwz_bgzf_bound(uint64_t n);   /* worst-case compressed bytes for n input bytes, EOF member included */
/* Asynchronous on the context's stream.  d_in 16-byte aligned and readable up to n rounded up to 16 (as every slot of
 * zwz_deflate_batch_dev); out_cap >= zwz_bgzf_bound(n) (else ZWZ_E_INVALID).  *d_out_len (device u64) receives the total length. */
int zwz_bgzf_compress_dev(zwz_ctx *ctx, const uint8_t *d_in, uint64_t n, uint8_t *d_out, uint64_t out_cap, uint64_t *d_out_len);
/* Host-only walk of a BGZF file in memory (no GPU): member_off[0..*n_members) and the total decoded size *raw_len.  member_off may
 * be NULL to count only; with fewer than *n_members entries of cap the call is ZWZ_E_INVALID (*n_members, *raw_len still set). */
int zwz_bgzf_index(const uint8_t *gz, uint64_t n, uint64_t *member_off, uint32_t cap, uint32_t *n_members, uint64_t *raw_len);
/* Asynchronous.  d_gz (gz_len bytes, 16-byte aligned) and d_member_off (device copies of zwz_bgzf_index's offsets) describe the
 * members; d_out holds raw_len bytes; *d_out_len (device u64) receives the decoded length; d_status[i] per member: 0, an inflate
 * code (zwz_inflate_status) or a zwz_bgzf_member_status. */
int zwz_bgzf_decompress_dev(zwz_ctx *ctx, const uint8_t *d_gz, uint64_t gz_len, const uint64_t *d_member_off, uint32_t n_members,
                            uint8_t *d_out, uint64_t *d_out_len, uint32_t *d_status);
/* Whole files of any size, streamed in slices through pinned staging (reading, the GPU and writing overlap).  dst is written as
 * <dst>.part and renamed only on success; on failure no dst is left. */
int zwz_bgzf_compress_file(zwz_ctx *ctx, const char *src, const char *dst);
int zwz_bgzf_decompress_file(zwz_ctx *ctx, const char *src, const char *dst);

/* ---- BGZF random access: the .gzi index and range reads ---------------------------------------------------------------------
 * .gzi (htslib's bgzf_index_dump layout; what `bgzip -i` / `bgzip -r` write): a u64 LE count, then count pairs of u64 LE
 * (compressed offset of a member, decoded offset of its first byte).  The first member, (0, 0), is implied and not stored.
 * Written here: one entry for every member after the first, in file order, except a last member that decodes to nothing (the EOF
 * member); empty members elsewhere (the EOF member of the first of two concatenated files) get one.  Read here: indexes with or
 * without entries for empty members, a trailing EOF member's included.  A .gzi whose length is not 8 + 16 * count, whose
 * compressed offsets are not strictly increasing from above 0, or whose decoded offsets decrease is ZWZ_E_FORMAT. */
/* Host only (no GPU): the .gzi bytes of a BGZF buffer; gzi == NULL gives the size in *gzi_len only (cap too small: ZWZ_E_INVALID).
 * The same strict walk and ZWZ_E_FORMAT messages as zwz_bgzf_index. */
int zwz_bgzf_gzi(const uint8_t *gz, uint64_t n, uint8_t *gzi, uint64_t cap, uint64_t *gzi_len);
/* The same for a file of any size, streamed in bounded memory (`bgzip -r`); written as <dst_gzi>.part, renamed on success. */
int zwz_bgzf_gzi_file(const char *src, const char *dst_gzi);
/* ranges: k pairs (decoded offset, length) in host memory.  d_out (device) receives their bytes concatenated in the given order:
 * sum of the lengths.  Ranges may overlap, repeat, come in any order and be empty; an empty range at the very end is valid.  A
 * range past the end of the decoded data, or whose offset + length overflows, is ZWZ_E_INVALID naming the range.  Only members
 * holding a requested byte are read, decoded and checked (header, BSIZE within gz_len, inflate, CRC-32, ISIZE, and the decoded
 * length against the next index entry).  d_gz as for zwz_bgzf_decompress_dev.  Synchronous: returns after the GPU work, with the
 * first bad touched member reported as zwz_bgzf_decompress_file reports it (ZWZ_E_CHECKSUM / ZWZ_E_FORMAT). */
int zwz_bgzf_read_ranges_dev(zwz_ctx *ctx, const uint8_t *d_gz, uint64_t gz_len, const uint8_t *gzi, uint64_t gzi_len,
                             const uint64_t *ranges, uint32_t k, uint8_t *d_out);
/* The same from a file into host memory.  With a .gzi only the touched members are read (one pread per run of consecutive
 * entries); gzi_path == NULL walks the member headers from the start until the last requested byte is covered. */
int zwz_bgzf_read_ranges_file(zwz_ctx *ctx, const char *src, const char *gzi_path, const uint64_t *ranges, uint32_t k, uint8_t *out);

/* ---- BGZF: the member walk on the device, and chunks by virtual offset -----------------------------------------------------------
 * The walk of the member headers as a parallel job (candidate scan, parse, pointer jumping over the chain of BSIZE links), so that a
 * stream in device memory -- the output of zwz_bgzf_compress_dev, say -- is indexed and decoded without a copy to the host.
 *
 * A VIRTUAL OFFSET (what .bai / .csi / .tbi indexes and htslib's bgzf_tell speak in) is
 *     compressed offset of a member << 16 | offset inside its decoded block.
 * Write U(c) for the decoded offset of the member that starts at compressed offset c; the position of virtual offset v is
 * P(v) = U(v >> 16) + (v & 0xffff), and the CHUNK (vbeg, vend) is the decoded bytes [P(vbeg), P(vend)).  With cbeg = vbeg >> 16 and
 * cend = vend >> 16 a chunk is valid when vbeg <= vend, a member parses at cbeg, the chain of members from cbeg hits cend exactly
 * (or cend == gz_len), each offset inside a block is at most that member's ISIZE (equality is the block's end, which bgzf_tell can
 * return) and is 0 where cend == gz_len.  vbeg > vend, an offset inside a block above ISIZE, a cend the chain from cbeg steps over
 * and a cbeg at or past gz_len are ZWZ_E_INVALID, zwz_last_error() naming the chunk and the reason.  A cbeg that is no member, or a
 * broken member on the way, is ZWZ_E_FORMAT in the words of zwz_bgzf_index (member numbers count from cbeg).  Chunks may overlap,
 * repeat, be empty and come in any order; the compressed spans [cbeg, cend] of chunks that overlap or touch are walked as one chain
 * from the lowest cbeg, and a cbeg that is not on that chain is ZWZ_E_FORMAT.  Members holding a requested byte are decoded and fully
 * checked (inflate, CRC-32, ISIZE) as range reads check them; a member that is only passed over contributes its header and ISIZE
 * on trust.  No .gzi is needed: the compressed offsets are in the request. */
/* zwz_bgzf_index for a buffer in device memory: same counts, offsets, raw_len, same ZWZ_E_FORMAT and zwz_last_error() text.
 * d_member_off (device, may be NULL to count) receives min(cap, *n_members) offsets; fewer than *n_members: ZWZ_E_INVALID with
 * the counts set.  d_gz 16-byte aligned (else ZWZ_E_INVALID).  Synchronous. */
int zwz_bgzf_index_dev(zwz_ctx *ctx, const uint8_t *d_gz, uint64_t gz_len, uint64_t *d_member_off, uint32_t cap,
                       uint32_t *n_members, uint64_t *raw_len);
/* zwz_bgzf_gzi for a buffer in device memory: byte for byte the same .gzi, into HOST memory (what zwz_bgzf_read_ranges_dev takes) */
int zwz_bgzf_gzi_dev(zwz_ctx *ctx, const uint8_t *d_gz, uint64_t gz_len, uint8_t *gzi, uint64_t cap, uint64_t *gzi_len);
/* Host only (no GPU): decoded offsets -> virtual offsets by a .gzi (the member is the last entry at or below the offset, as range
 * reads resolve it; an offset whose member starts at or above 2^48, or lies 65536 or more bytes past its entry: ZWZ_E_INVALID) */
int zwz_bgzf_voffsets(const uint8_t *gzi, uint64_t gzi_len, const uint64_t *offsets, uint32_t k, uint64_t *voffsets);
/* chunks: k pairs (vbeg, vend) of virtual offsets in host memory.  sizes[k] (host): decoded bytes of each chunk, from the members'
 * ISIZE fields (on trust until read).  Only headers and trailers between the chunks' compressed offsets are looked at. */
int zwz_bgzf_chunk_sizes_dev(zwz_ctx *ctx, const uint8_t *d_gz, uint64_t gz_len, const uint64_t *chunks, uint32_t k, uint64_t *sizes);
/* The chunks' bytes concatenated in the given order into d_out (device; sum of sizes > out_cap: ZWZ_E_INVALID, sizes still set).
 * Needs no index.  Synchronous; damage reported as zwz_bgzf_read_ranges_dev reports it (member numbers count the members walked). */
int zwz_bgzf_read_chunks_dev(zwz_ctx *ctx, const uint8_t *d_gz, uint64_t gz_len, const uint64_t *chunks, uint32_t k,
                             uint8_t *d_out, uint64_t out_cap, uint64_t *sizes);
/* The same for a file.  The headers are walked on the host, from each chunk's cbeg: nothing in front of a chunk's first member or
 * more than 65 536 bytes behind the start of its last one is read, in bounded memory.  zwz_bgzf_chunk_sizes_file needs no GPU. */
int zwz_bgzf_chunk_sizes_file(const char *src, const uint64_t *chunks, uint32_t k, uint64_t *sizes);
int zwz_bgzf_read_chunks_file(zwz_ctx *ctx, const char *src, const uint64_t *chunks, uint32_t k, uint8_t *out, uint64_t out_cap,
                              uint64_t *sizes);

/* ---- DEFLATE streams of any size: raw, zlib and gzip ---------------------------------------------------------------------------
 * Decodes a batch of n independent streams in one pass on the GPU, one wave per stream (a single stream is not faster than one
 * wave; the call pays off on batches of thousands).  Stream i is d_in_len[i] bytes at d_in + d_in_off[i], wrapped as `wrap` says:
 *   ZWZ_WRAP_RAW   RFC 1951 DEFLATE data alone; bytes after the final block are ignored
 *   ZWZ_WRAP_ZLIB  RFC 1950: header, DEFLATE data, Adler-32; bytes after the Adler-32 are ignored
 *   ZWZ_WRAP_GZIP  RFC 1952: one or more members, each a header (FEXTRA, FNAME, FCOMMENT, FHCRC), DEFLATE data, CRC-32 and ISIZE.
 *                  Zero bytes between and after members are skipped; a following 1f 8b starts another member, any other byte is
 *                  ZWZ_STREAM_TRAILING.  Every member starts with an empty window.  An input with no member (empty, or zeros only)
 *                  is status 1.
 * Output i goes to d_out + d_out_off[i], at most d_out_cap[i] bytes; d_out_len[i] receives the decoded length (also on failure:
 * everything decoded before the stop, as libz emits it) and d_status[i] the verdict, libz 1.2.11's:
 * 0..3 as in zwz_inflate_status, 3 meaning that the output would pass d_out_cap[i], or a zwz_stream_status.  A checksum mismatch in an earlier
 * member beats whatever stopped a later one, as libz stops at the first bad member.  A byte outside
 * [d_out_off[i], d_out_off[i] + d_out_cap[i]) is never written.
 * Limits (the kernel's 32-bit bit and byte positions): d_in_len[i] < 2^29 and d_out_cap[i] < 2^32, else ZWZ_STREAM_TOO_LARGE with
 * nothing read or written.
 * Alignment: d_in, d_out and every d_in_off[i], d_out_off[i] are multiples of 16; stream i is readable up to its length rounded up to
 * 16; output ranges do not overlap.  All arrays are device memory on the context's GPU.  Asynchronous on the context's stream.
 * ZWZ_E_INVALID for a null pointer, a misaligned d_in / d_out or an unknown wrap; problems of one stream only through d_status.
 * Preset dictionaries (FDICT) are ZWZ_STREAM_BAD_HEADER.  The context's "inflate_header" option applies here too. */
#define ZWZ_WRAP_RAW  0
#define ZWZ_WRAP_ZLIB 1
#define ZWZ_WRAP_GZIP 2
typedef enum zwz_stream_status {      /* 0..3 mean what zwz_inflate_status means */
    ZWZ_STREAM_BAD_HEADER = 32,   /* not this wrapper, FDICT set, unknown method or flags, window > 32K, header CRC mismatch */
    ZWZ_STREAM_CHECKSUM   = 33,   /* Adler-32 / CRC-32 mismatch */
    ZWZ_STREAM_LENGTH     = 34,   /* gzip ISIZE mismatch */
    ZWZ_STREAM_TRAILING   = 35,   /* gzip: bytes after a member that are neither zero padding nor another member */
    ZWZ_STREAM_TOO_LARGE  = 36,   /* d_in_len[i] >= 2^29 or d_out_cap[i] >= 2^32: nothing read or written */
    ZWZ_STREAM_INDEX      = 37    /* zwz_inflate_indexed_dev: the stream did not decode as its index says (a bit offset, decoded offset, hist or
                                     end bit that is not the stream's, or a stream of another length) */
} zwz_stream_status;
int zwz_inflate_streams_dev(zwz_ctx *ctx, int wrap, const uint8_t *d_in, const uint64_t *d_in_off, const uint64_t *d_in_len,
                            uint32_t n, uint8_t *d_out, const uint64_t *d_out_off, const uint64_t *d_out_cap,
                            uint64_t *d_out_len, uint32_t *d_status);

/* ---- One long stream, decoded in parallel at its full-flush points ------------------------------------------------------------
 * Arguments, alignment rules, limits (ZWZ_STREAM_TOO_LARGE included) and PER-STREAM RESULTS exactly those of
 * zwz_inflate_streams_dev: the same decoded bytes, d_out_len[i] and d_status[i] for every input, good or damaged.  What differs is
 * the time a long stream takes.  A flush point is an empty stored block, 00 00 ff ff on a byte boundary, and after a FULL flush
 * nothing refers back across it, so a stream that has such points -- what zwz_deflate_streams_dev and `main gzip` write (one every
 * 65280 input bytes), pigz -i, libz callers that use Z_FULL_FLUSH -- is decoded by one wave per piece between two of them instead
 * of one wave in all.  Per stream: the candidates (the body's first byte and every byte behind the four marker bytes) are found by
 * a scan of the input; one wave per candidate decodes from there with an empty window and only counts; the chain of true piece
 * starts is followed from the body's first byte; if it reaches the final block, the trailer is fine and the counts fit the
 * capacity, one wave per piece writes its bytes in place and the checksum is computed from pieces of the output in parallel.
 * Every other stream -- no flush points, sync flushes (the pieces refer back), a damaged or cut stream, a second gzip member or
 * trailing bytes, a header other than fine, an output above the capacity -- is decoded by zwz_inflate_streams_dev's own path and
 * gets that path's results.
 * d_segments (device, n entries, may be NULL): the pieces of stream i decoded in parallel, 0 for a stream that took the other path.
 * Context options (zwz_ctx_set_option, decimal values, "" restores the default; "split_slice_bytes" belongs to the file function below):
 *   "split_min_bytes"       65536    streams shorter than this are not scanned
 *   "split_budget"          4194304  input bytes one measuring wave may read; a piece longer than this sends its stream the other way
 *   "split_max_candidates"  131072   a stream with more candidates is not measured (2^32 output bytes in pieces of 65280 are 65794)
 * so the work on hostile input is bounded by candidates x budget per stream, whatever its length.  Device memory beyond input and
 * output: 12 bytes per 4096 input bytes for the scan, 20 + log2(candidates of the longest chain) words per candidate that is
 * measured, 40 bytes per piece decoded and 16 per 65280 output bytes for the checksum.  One call measures at most 8 Mi candidates
 * (streams beyond that take the other path): about 1.2 GB at the worst.  The context keeps its largest workspace until it is
 * destroyed.
 * NOT asynchronous: the launch sizes depend on what the scan finds, so the call waits for the context's stream three times; the
 * last kernels are still queued when it returns (zwz_ctx_sync before reading results, as for zwz_inflate_streams_dev). */
int zwz_inflate_split_streams_dev(zwz_ctx *ctx, int wrap, const uint8_t *d_in, const uint64_t *d_in_off, const uint64_t *d_in_len,
                                  uint32_t n, uint8_t *d_out, const uint64_t *d_out_off, const uint64_t *d_out_cap,
                                  uint64_t *d_out_len, uint32_t *d_status, uint32_t *d_segments);
/* zwz_inflate_split_streams_dev that also writes every stream's seek index (the layout below, under "A seek index for ordinary
 * streams").  The first twelve arguments, the decoded bytes, d_out_len, d_status and d_segments are exactly that call's; span, d_idx,
 * d_idx_off, d_idx_cap and d_idx_len are zwz_inflate_streams_index_dev's (device arrays).  A stream that SPLITS gets the index of its
 * flush points by the rule of zwz_deflate_streams_index_dev (further down): the points are the chain's piece starts, which the
 * split decode has found and proved with their decoded offsets, so the index costs a flag per piece, a scan and the entries -- hist
 * 0, no windows, 24 bytes an entry -- and is built at the split decode's rate.  For what zwz_deflate_streams_index_dev wrote it is,
 * byte for byte, the index that call wrote.  d_idx_len[i] = 0 where the final status is not 0 (a checksum mismatch included) or the
 * capacity is too small.  A stream that does not split goes through zwz_inflate_streams_index_dev's marking form instead of the plain
 * stream form and gets exactly that call's bytes, lengths, status and index (none for a stream of several members).
 * zwz_inflate_index_bound(d_out_cap[i], span) always fits either way.  NOT asynchronous, as zwz_inflate_split_streams_dev. */
int zwz_inflate_split_streams_index_dev(zwz_ctx *ctx, int wrap, const uint8_t *d_in, const uint64_t *d_in_off,
                                        const uint64_t *d_in_len, uint32_t n, uint8_t *d_out, const uint64_t *d_out_off,
                                        const uint64_t *d_out_cap, uint64_t *d_out_len, uint32_t *d_status, uint32_t *d_segments,
                                        uint32_t span, uint8_t *d_idx, const uint64_t *d_idx_off, const uint64_t *d_idx_cap,
                                        uint64_t *d_idx_len);
/* One file of any size holding ONE raw, zlib or gzip stream -> its decoded bytes: the way back from zwz_deflate_stream_file and
 * `main gzip`.  The compressed file passes through the device in slices of "split_slice_bytes" (context option, default 67108864,
 * 4096 .. 2^28); per slice the pieces that end inside it are found and decoded as above and written, and the next slice starts where
 * the chain stands.  Sizes are 64-bit: no 2^29 or 2^32 limit for a file that splits; a piece must fit a slice and its decoded bytes
 * four slices (at least 4 MiB).  A file in which no piece ends cleanly before any byte was written (no flush points, sync flushes,
 * another wrapper) is decoded as one stream by zwz_inflate_streams_dev's path if it is shorter than 2^29 bytes, and in legs by
 * zwz_inflate_legs_file's loop (below) if it is longer or that path ends at its largest capacity: any .gz decodes, a long one that
 * does not split at the one-wave rate.  If the chain breaks after bytes were written (a cut or damaged file), ZWZ_E_FORMAT with
 * zwz_last_error() naming the compressed offset.  A CRC-32, Adler-32 or ISIZE that does not match is ZWZ_E_CHECKSUM.  When bytes
 * other than zeros follow the first gzip member of a file that splits, the file is decoded again from its first byte: by the
 * one-stream path if it is shorter than 2^29 bytes (which reads further members and names garbage), in legs otherwise.  dst is
 * written as dst.part and renamed on success only.  Synchronous. */
int zwz_inflate_stream_file(zwz_ctx *ctx, int wrap, const char *src, const char *dst);
/* zwz_inflate_stream_file that also writes the file's seek index to dst_idx, at the context's "index_span_bytes"; dst may be NULL
 * (index only).  A file that splits gets the index of its flush points (zwz_inflate_split_streams_index_dev's, byte for byte what
 * zwz_deflate_stream_file_index wrote for a file of its own): every slice hands back the starts of the pieces it decoded, the host
 * applies the rule with the last point carried from slice to slice and seals the header once the trailer is known.  A file that does
 * not split before any byte was written (or is one piece in all), or in which bytes other than zeros follow the first gzip member, goes through
 * zwz_inflate_legs_file(ctx, wrap, src, dst, dst_idx, NULL) and gets that call's index.  A chain that breaks after bytes were
 * written is ZWZ_E_FORMAT, as above.  dst_idx is written as <dst_idx>.part and renamed behind dst: a failure leaves neither. */
int zwz_inflate_split_index_file(zwz_ctx *ctx, int wrap, const char *src, const char *dst, const char *dst_idx);

/* ---- A seek index for ordinary streams: parallel and ranged inflate ----------------------------------------------------------------
 * An ordinary stream -- gzip, zlib.compress, pigz without -i, git, PNG, anything with sync flushes -- offers no cut: every block may
 * refer 32 KiB back.  It is decoded ONCE at the one-wave rate, and that decode keeps CHECKPOINTS: a block header's first bit, the
 * decoded offset there and the up to 32 KiB of output in front of it.  From then on the stream decodes with one wave per segment between
 * two checkpoints, and a batch of byte ranges decodes only the segments it touches.  Building runs at the one-wave rate (about 36 s
 * per decoded GiB of a single stream): the index pays off from the second access on, or on batches.
 * The index of one stream, all little-endian: a 64-byte header, `count` entries of 24 bytes, the windows back to back in entry
 * order, zero padding to a multiple of 16.
 *   header   0 "ZWZIDX\0\1"   8 u32 wrap   12 u32 span   16 u64 stream length, wrapper included   24 u64 decoded length   32 u32 count
 *           36 u32 flags, 0   40 u64 end bit: the first bit behind the final block   48 u32 stored CRC-32 / Adler-32, 0 for raw
 *           52 u32 CRC-32 of the index from byte 64 to its end   56 u64 0
 *   entry    0 u64 bit offset of a block header's first bit, counted from the stream's first byte   8 u64 decoded offset
 *           16 u32 hist: bytes of window kept, <= min(32768, decoded offset)   20 u32 0
 * Entry 0 is the body's first block (decoded offset 0, hist 0); bit offsets rise strictly, decoded offsets do not fall.  A hist below
 * its bound is a promise that no match of the segment reaches further back, and the decode checks it.  Anyone may write such an
 * index: after every Z_SYNC_FLUSH of a libz writer the next block starts on a byte boundary at a known decoded offset.  An index
 * with a wrong magic, length, index CRC or window sum, entries out of order, a hist over its bound, an end bit beyond the stream or a
 * header field out of range (a decoded length above 1032 times the stream's, which no DEFLATE data reaches, among them) is
 * ZWZ_E_FORMAT wherever one is read.
 * Readable extents: the byte copies read whole aligned 4-byte words, so an index on the device and every output range are readable up
 * to their length rounded up to 16 (an index's length is a multiple of 16 already).
 * Not in this version: an index for a gzip stream of several members (none is made), compressed windows, decoding a touched segment
 * only as far as the last byte asked for.  (A stream of 2^29 compressed bytes or more gets its index from zwz_inflate_legs_dev below,
 * a file of that size from zwz_inflate_legs_file, which zwz_inflate_index_file and zwz_inflate_stream_file call where one launch ends.) */
/* The most an index of a stream that decodes to decoded_cap bytes takes at this span (0: 1 MiB); 0 for a span that is not allowed. */
uint64_t zwz_inflate_index_bound(uint64_t decoded_cap, uint32_t span);
/* The context option "index_span_bytes" as it stands (0 for a null context): what the calls with span 0 and the file calls take */
uint32_t zwz_ctx_index_span(zwz_ctx *ctx);
/* zwz_inflate_streams_dev that also writes every stream's index.  The first eleven arguments, the decoded bytes, d_out_len and
 * d_status are exactly that call's.  span: decoded bytes between checkpoints at least, a power of two in 16 KiB .. 1 GiB; 0 takes
 * the context option "index_span_bytes" (default 1048576).  The index of stream i goes to d_idx + d_idx_off[i] (device arrays;
 * d_idx and every offset multiples of 16), at most d_idx_cap[i] bytes, and d_idx_len[i] receives its length: 0 where none was made --
 * a status other than 0, a second gzip member (zero padding behind the member is fine), or a capacity too small
 * (zwz_inflate_index_bound(d_out_cap[i], span) always fits).  Asynchronous on the context's stream. */
int zwz_inflate_streams_index_dev(zwz_ctx *ctx, int wrap, const uint8_t *d_in, const uint64_t *d_in_off, const uint64_t *d_in_len,
                                  uint32_t n, uint8_t *d_out, const uint64_t *d_out_off, const uint64_t *d_out_cap,
                                  uint64_t *d_out_len, uint32_t *d_status, uint32_t span, uint8_t *d_idx,
                                  const uint64_t *d_idx_off, const uint64_t *d_idx_cap, uint64_t *d_idx_len);
/* zwz_inflate_streams_index_dev for streams of ANY length, in LEGS.  A leg is one launch of a stream's wave over a window of its input
 * and a window of its output that fit the kernel's 32-bit positions; everything 64 bits wide is carried from leg to leg.  While it
 * decodes, the wave keeps its latest RESTART POINT: the last block header at which a checkpoint was due (by the index's rule and span,
 * whether or not an index is made) or the last gzip member start.  A leg whose window runs out before the stream does is rewound: the
 * next leg starts at the restart point, with the up to 32 KiB of output in front of it as its window, and decodes again what lay behind
 * it.  A leg that is rewound to the very point it started from gets double the window that ran out; past 2^29 - 16 input or 2^32 - 16
 * output bytes the stream is ZWZ_STREAM_TOO_LARGE with d_out_len[i] = the last restart point's decoded offset, so the limits hold for
 * one stretch between two restart points, not for the stream.
 * in_off, in_len, out_off, out_cap, idx_off and idx_cap are HOST arrays of n (zwz_deflate_streams_dev's convention), lengths and
 * capacities 64-bit and not limited; d_in, d_out, d_idx, d_out_len, d_status and d_idx_len are device memory.  Alignment rules are
 * zwz_inflate_streams_dev's.  d_idx may be NULL (with idx_off, idx_cap, d_idx_len): decode only; restart points are then still taken at
 * `span` (0: the context's "index_span_bytes").
 * For every stream within the one-launch limits, whatever the leg sizes, the decoded bytes, d_out_len[i], d_status[i], d_idx_len[i]
 * and the index bytes are exactly zwz_inflate_streams_index_dev's -- damaged and cut streams and streams of several members
 * included -- and no byte outside [out_off[i], out_off[i] + out_cap[i]) is written.  Checkpoints are due by the same rule and the same
 * running offset as in one launch: nothing is forced at a leg's end.  Entries carry 64-bit bit and decoded offsets, and ISIZE is
 * checked against the member's length mod 2^32.  The checksum is taken from pieces of the whole output in parallel once every stream
 * has ended.  An index of 2^32 bytes or more is not made.
 * legs (HOST, 3 n words, may be NULL): per stream the legs run, the legs rewound and the windows grown.
 * One launch per round holds one wave per unfinished stream, and the call waits for the context's stream every round: NOT
 * asynchronous; the last kernels are still queued when it returns (zwz_ctx_sync before reading results).
 * Context options (zwz_ctx_set_option, decimal, "" restores the default):
 *   "leg_bytes"      268435456      4096 .. 2^29 - 16, a multiple of 16   compressed bytes a leg may read
 *   "leg_out_bytes"  2^32 - 65536   65536 .. that value                   decoded bytes a leg may write
 * A stream runs at the one-wave rate, and a rewind pays for what it decodes twice: this call removes a limit, it makes nothing faster. */
int zwz_inflate_legs_dev(zwz_ctx *ctx, int wrap, const uint8_t *d_in, const uint64_t *in_off, const uint64_t *in_len, uint32_t n,
                         uint8_t *d_out, const uint64_t *out_off, const uint64_t *out_cap, uint64_t *d_out_len, uint32_t *d_status,
                         uint32_t span, uint8_t *d_idx, const uint64_t *idx_off, const uint64_t *idx_cap, uint64_t *d_idx_len,
                         uint32_t *legs);
/* ONE stream of any length (d_in, in_len bytes, 16-byte aligned, readable up to its length rounded up to 16) decoded whole with its
 * index, one wave per segment: the 2^29 / 2^32 limits hold for a single segment only (else ZWZ_STREAM_TOO_LARGE).  idx (idx_len
 * bytes) is HOST memory, for planning; d_idx is the same bytes on the device (16-byte aligned), or NULL: the call then uploads them.
 * The wrapper comes from the index.  d_out may start at ANY byte; no byte outside [d_out, d_out + decoded length) is written.
 * *d_out_len, *d_status, *d_segments (device; d_segments may be NULL): the decoded length, the verdict, the segments decoded.
 * Verdicts: 0; 3 with nothing written when out_cap is below the indexed decoded length; ZWZ_STREAM_INDEX when in_len is not the
 * index's or a segment does not end exactly at its end bit with exactly its indexed count; ZWZ_STREAM_CHECKSUM when the decoded
 * bytes' CRC-32 / Adler-32 (computed from pieces in parallel) is not BOTH the index's stored value and the stream's own trailer
 * (gzip: ISIZE too), or when a window of the index is not the bytes that precede its checkpoint.  The windows are put at their final
 * places in the output before the waves start; the wave of the segment before writes the same bytes there later.
 * NOT asynchronous (the call waits for the context's stream before it fills its staging); the last kernels are still queued when it
 * returns: zwz_ctx_sync before reading results -- and, with d_idx NULL, before idx is freed or changed: its upload may still be queued.
 * ZWZ_E_FORMAT for a malformed index. */
int zwz_inflate_indexed_dev(zwz_ctx *ctx, const uint8_t *d_in, uint64_t in_len, const uint8_t *idx, uint64_t idx_len,
                            const uint8_t *d_idx, uint8_t *d_out, uint64_t out_cap, uint64_t *d_out_len, uint32_t *d_status,
                            uint32_t *d_segments);
/* ranges and the result layout are zwz_bgzf_read_ranges_dev's: k pairs (decoded offset, length) in host memory, their bytes
 * concatenated in d_out; a range past the decoded length is ZWZ_E_INVALID naming it.  Only the segments holding a requested byte are
 * decoded, each whole, into scratch the context keeps (its window in front of it; slices of at most 256 MiB of scratch).  With d_idx
 * NULL only the windows of touched segments are uploaded.  Range reads carry NO checksum verdict: a segment is checked to end at its
 * end bit with its indexed count (else ZWZ_E_FORMAT naming the segment), the bytes themselves are not; damage inside a segment no
 * range touches is not seen.  Synchronous. */
int zwz_inflate_read_ranges_dev(zwz_ctx *ctx, const uint8_t *d_in, uint64_t in_len, const uint8_t *idx, uint64_t idx_len,
                                const uint8_t *d_idx, const uint64_t *ranges, uint32_t k, uint8_t *d_out);
/* zwz_inflate_indexed_dev for n streams in ONE call: the segments of all of them are one launch, and so are the placing and the
 * comparing of their windows, their checksum pieces and their verdicts (zwz_inflate_indexed_dev is this call with n = 1).
 * in_off, in_len, idx_off, idx_len, out_off and out_cap are HOST arrays of n (zwz_deflate_streams_dev's convention; they may be
 * reused when the call returns); d_in, d_out, d_out_len, d_status and d_segments (which may be NULL) are device memory, the last three
 * of n elements.  Stream i is in_len[i] bytes at d_in + in_off[i] (d_in and every in_off[i] multiples of 16, readable up to the
 * length rounded up to 16).  Index i is idx_len[i] bytes at idx + idx_off[i] in HOST memory and, with d_idx given, the same bytes at
 * d_idx + idx_off[i] (d_idx and every idx_off[i] multiples of 16): the layout zwz_inflate_streams_index_dev writes, so what it built is
 * decoded with the same offsets after one copy to the host.  With d_idx NULL the call uploads the indexes.  The wrapper of stream i
 * comes from its index: one batch may mix raw, zlib and gzip.
 * Output i goes to d_out + out_off[i], ANY byte address; no byte outside [out_off[i], out_off[i] + decoded length) is written; the
 * ranges must not overlap.  d_out_len[i], d_status[i] and d_segments[i] are exactly what zwz_inflate_indexed_dev gives for stream i
 * alone (0; 3 with nothing written; ZWZ_STREAM_INDEX; ZWZ_STREAM_TOO_LARGE; ZWZ_STREAM_CHECKSUM), and the verdicts are independent: a
 * stream that fails changes no byte and no verdict of another.
 * A malformed index is ZWZ_E_FORMAT for the whole call, zwz_last_error() naming the stream number and the rule; nothing is launched
 * or written.  n == 0 is ZWZ_OK.  More than 2^32 - 1 segments or checksum pieces in one call is ZWZ_E_INVALID.  Synchronisation as
 * zwz_inflate_indexed_dev's. */
int zwz_inflate_indexed_batch_dev(zwz_ctx *ctx, const uint8_t *d_in, const uint64_t *in_off, const uint64_t *in_len, uint32_t n,
                                  const uint8_t *idx, const uint64_t *idx_off, const uint64_t *idx_len, const uint8_t *d_idx,
                                  uint8_t *d_out, const uint64_t *out_off, const uint64_t *out_cap,
                                  uint64_t *d_out_len, uint32_t *d_status, uint32_t *d_segments);
/* zwz_inflate_read_ranges_dev across the n streams of a batch laid out as zwz_inflate_indexed_batch_dev's: ranges is k TRIPLES
 * (stream number, decoded offset, length) in host memory, in any order, overlapping, repeated or empty; d_out receives their bytes
 * concatenated in the given order.  The touched segments of all streams are decoded together, each whole, in slices of at most
 * 256 MiB of scratch; with d_idx NULL only their windows are uploaded.  No checksum verdict.  Synchronous.
 * ZWZ_E_INVALID names the range for a stream number >= n, a range past its stream's decoded length or an overflowing end;
 * ZWZ_E_FORMAT names the stream for a malformed index or an in_len other than indexed, and the stream and the segment for a segment
 * that does not decode as indexed.  Only the indexes of streams that a range names are read. */
int zwz_inflate_read_ranges_batch_dev(zwz_ctx *ctx, const uint8_t *d_in, const uint64_t *in_off, const uint64_t *in_len, uint32_t n,
                                      const uint8_t *idx, const uint64_t *idx_off, const uint64_t *idx_len, const uint8_t *d_idx,
                                      const uint64_t *ranges, uint32_t k, uint8_t *d_out);
/* Host only (no GPU): checks an index as every reader does (ZWZ_E_FORMAT, zwz_last_error() naming the rule) and returns its wrapper,
 * the stream's length, the decoded length and the number of entries; any of the four pointers may be NULL. */
int zwz_inflate_index_info(const uint8_t *idx, uint64_t idx_len, int *wrap, uint64_t *stream_len, uint64_t *decoded_len, uint32_t *count);
/* One file holding one stream -> its index at dst_idx (written as dst_idx.part, renamed on success).  A file shorter than 2^29 bytes
 * goes through zwz_inflate_streams_index_dev whole, at the context's "index_span_bytes"; a longer one, or one whose decoded bytes end
 * that launch at its largest capacity, through zwz_inflate_legs_file's loop (below), at the one-wave rate.  A stream that does not decode
 * is ZWZ_E_FORMAT (ZWZ_E_CHECKSUM for a checksum or ISIZE mismatch); so is a gzip file of several members, for which no index is made.
 * Synchronous. */
int zwz_inflate_index_file(zwz_ctx *ctx, int wrap, const char *src, const char *dst_idx);
/* One file holding one raw, zlib or gzip stream of ANY length (gzip: any number of members with zero padding, as zwz_inflate_legs_dev
 * reads them) -> its decoded bytes at dst and its seek index, at the context's "index_span_bytes", at dst_idx, from one decode in LEGS.
 * Either of dst and dst_idx may be NULL, not both (ZWZ_E_INVALID).  The compressed file passes through one pinned buffer and one device
 * window; the decoded bytes through one device window, with the up to 32 KiB in front of a restart point carried to the head of the next
 * leg's; what a leg has made final -- the bytes below its restart point, all of them once the stream has ended -- is copied to one of two
 * pinned buffers and written by a writer thread while the next leg runs, its checksum joined from pieces onto a running value, and the
 * index entries below the restart point's own leave the device with their windows, which wait in a spool file (dst_idx.part.windows).
 * Memory is bounded by the windows, not by the file; windows grow as in zwz_inflate_legs_dev, past its limits ZWZ_E_FORMAT naming
 * ZWZ_STREAM_TOO_LARGE and the last restart point.  It makes no stream faster: ONE wave decodes the stream, about 36 s a decoded GiB, and
 * what lies behind a restart point is decoded twice.  What it buys is that any .gz can be decoded and indexed; with the index,
 * zwz_inflate_stream_file_indexed and zwz_inflate_read_ranges_file then work on it at the parallel rate.
 * Both files are written through .part names and renamed on success only; on any failure no dst, dst_idx, .part or spool file is left.
 * ZWZ_OK for stream status 0; ZWZ_E_CHECKSUM for a checksum or ISIZE mismatch (a mismatch beats any later stop); ZWZ_E_FORMAT for any
 * other status, zwz_last_error() naming the status, the decoded bytes and the COMPRESSED BYTE OFFSET at which the decoder stopped;
 * with dst_idx given also for a gzip file of several members and for an index of 2^32 bytes or more (neither is an obstacle to dst
 * alone); ZWZ_E_IO as the other file calls.  For every file within the one-launch limits the return code is zwz_inflate_stream_file's /
 * zwz_inflate_index_file's, and the index bytes are the latter's.
 * stats (may be NULL), 8 words: legs run; legs rewound; windows grown; commits that wrote bytes; largest input window; largest output
 * window; index entries; bytes of device plus pinned memory the call allocated (at their peak).
 * Context options (zwz_ctx_set_option, decimal, "" restores the default; also read from the environment at zwz_ctx_create):
 *   "leg_file_bytes"      67108864    4096 .. 2^29 - 16, a multiple of 16       ZWZ_LEG_FILE_BYTES      the input window
 *   "leg_file_out_bytes"  268435456   65536 .. 2^32 - 65536, a multiple of 16   ZWZ_LEG_FILE_OUT_BYTES  the output window
 * Synchronous: every wait is a join of a thread that only does file I/O, or a stream synchronisation. */
int zwz_inflate_legs_file(zwz_ctx *ctx, int wrap, const char *src, const char *dst, const char *dst_idx, uint64_t *stats);
/* zwz_inflate_read_ranges_dev from a file into host memory: the index is read from idx_path, and of src only the compressed bytes of
 * the touched segments (one pread per run of consecutive index entries).  A file of another length than indexed is ZWZ_E_FORMAT. */
int zwz_inflate_read_ranges_file(zwz_ctx *ctx, const char *src, const char *idx_path, const uint64_t *ranges, uint32_t k, uint8_t *out);
/* One file of any size decoded whole with its index: the compressed file is read in slices of consecutive index entries (their decoded
 * bytes at most four times "split_slice_bytes", one entry at least), every segment of a slice by a wave of its own, the bytes written
 * by a writer thread while the next slice runs.  The CRC-32 / Adler-32 joined from the slices' pieces is checked against the index's
 * stored value and the file's own trailer (gzip: ISIZE too): ZWZ_E_CHECKSUM; a segment that does not decode as indexed: ZWZ_E_FORMAT.
 * dst is written as dst.part and renamed on success only.  Synchronous. */
int zwz_inflate_stream_file_indexed(zwz_ctx *ctx, const char *src, const char *idx_path, const char *dst);

/* ---- DEFLATE streams of any size, written: raw, zlib and gzip ------------------------------------------------------------------
 * Compresses a batch of n independent inputs into n ordinary streams that any inflate reads.  Stream i is, byte for byte, what
 * libz 1.2.11 writes at level 6 (windowBits -15 / 15 / 31 for ZWZ_WRAP_RAW / _ZLIB / _GZIP) when every 65280 bytes of input are
 * followed by deflate(Z_FULL_FLUSH) and the last by deflate(Z_FINISH): every piece of 65280 bytes is compressed by itself (the bytes of
 * zwz_deflate_batch_dev), its last block made non-final and followed by an empty stored block (00 00 ff ff on a byte boundary), and
 * the stream ends with 03 00 and the trailer.  zlib: 78 9c ... Adler-32; gzip: 1f 8b 08 00 00 00 00 00 00 03 ... CRC-32, ISIZE; an
 * empty input is header, 03 00, trailer.  The pieces of one long stream are as parallel as a batch of short ones.
 * Under zwz_ctx_set_level(N), N = 4 or 5, read "level N" for "level 6": the same full-flush structure of 65280-byte pieces, the zlib header 78 5e,
 * the gzip header unchanged (XFL 0), the same bound.
 * Input i is in_len[i] bytes at d_in + in_off[i]; output i goes to d_out + out_off[i], at most out_cap[i] bytes.  d_out_len[i]
 * receives the length the stream needs, whether it fitted or not, and d_status[i] 0 or ZWZ_INF_OVERFLOW (3) when that is more than
 * out_cap[i]; what then lies in the range is undefined, and no byte outside [out_off[i], out_off[i] + out_cap[i]) is ever written.
 * out_cap[i] >= zwz_deflate_stream_bound(in_len[i], wrap) never overflows.  (Status 2 would mean that the codec's own block records
 * contradict the stream it wrote from them; no input is known to cause it.)
 * in_off, in_len, out_off, out_cap are HOST arrays (the launch sizes depend on them; they may be reused when the call returns);
 * d_in, d_out, d_out_len and d_status are device memory.  Asynchronous on the context's stream.
 * Alignment: d_in, d_out and every in_off[i], out_off[i] are multiples of 16; input i is readable up to its length rounded up to 16;
 * output ranges do not overlap.  Lengths are 64-bit and not limited; pieces are counted in 64 bits, and a call may hold at most
 * 2^46 of them (2^62 bytes).  ZWZ_E_INVALID for a null pointer, a misaligned pointer or offset, or an unknown wrap. */
uint64_t zwz_deflate_stream_bound(uint64_t n, int wrap);   /* worst-case output bytes for one stream of n input bytes; 1.0009 n */
int zwz_deflate_streams_dev(zwz_ctx *ctx, int wrap, const uint8_t *d_in, const uint64_t *in_off, const uint64_t *in_len, uint32_t n,
                            uint8_t *d_out, const uint64_t *out_off, const uint64_t *out_cap, uint64_t *d_out_len,
                            uint32_t *d_status);
/* One file of any size as one stream, in slices through pinned staging (reading, the GPU and writing overlap; the checksum and the
 * position carry from slice to slice).  dst is written as <dst>.part and renamed only on success; on failure no dst is left. */
int zwz_deflate_stream_file(zwz_ctx *ctx, int wrap, const char *src, const char *dst);
/* zwz_deflate_streams_dev that also writes every stream's seek index (the layout above, under "A seek index for ordinary streams") as
 * it writes the stream: nothing is decoded.  Every piece starts behind a full-flush marker, where nothing refers back, so the entries
 * have hist 0 and the index holds no windows: 24 bytes an entry.  The POINTS of a stream are the body's first block (decoded offset 0)
 * and every block that starts behind a flush marker, in stream order; entry 0 is the first point, and a later point at decoded offset
 * o is an entry when o < the decoded length and floor(o / span) is above that of the point in front of it -- the first point in each
 * span-sized bucket of the output.  The end bit is 10 bits into the 03 00 behind the last marker.  Every reader of an index takes it:
 * zwz_inflate_indexed_dev, zwz_inflate_read_ranges_dev, the batch calls and the file forms.
 * The first eleven arguments, the stream bytes, d_out_len and d_status are exactly zwz_deflate_streams_dev's.  span: a power of two
 * in 16 KiB .. 1 GiB; 0 takes the context option "index_span_bytes".  The index of stream i goes to d_idx + idx_off[i] (d_idx device
 * memory; idx_off and idx_cap HOST arrays of n, d_idx and every offset multiples of 16), at most idx_cap[i] bytes, and d_idx_len[i]
 * (device) receives its length: 0 with status 3 or a capacity too small; no byte outside [idx_off[i], idx_off[i] + idx_cap[i]) is
 * written.  Asynchronous on the context's stream.
 * zwz_deflate_stream_index_bound: the exact worst case for n input bytes, 64 + 24 (n / span + 1) rounded up to 16 (span 0: 1 MiB);
 * 0 for a span that is not allowed.
 * zwz_deflate_stream_file_index: zwz_deflate_stream_file that also writes the stream's index to dst_idx, for files of any size, at
 * the context's "index_span_bytes".  The entries of each slice come from the same kernels, told the decoded bytes and the stream
 * bytes in front of the slice; the host appends them and seals the header once the trailer is known.  dst_idx is written as
 * <dst_idx>.part and renamed behind dst: a failure leaves neither file. */
uint64_t zwz_deflate_stream_index_bound(uint64_t n, uint32_t span);
int zwz_deflate_stream_file_index(zwz_ctx *ctx, int wrap, const char *src, const char *dst, const char *dst_idx);
int zwz_deflate_streams_index_dev(zwz_ctx *ctx, int wrap, const uint8_t *d_in, const uint64_t *in_off, const uint64_t *in_len, uint32_t n,
                                  uint8_t *d_out, const uint64_t *out_off, const uint64_t *out_cap, uint64_t *d_out_len,
                                  uint32_t *d_status, uint32_t span, uint8_t *d_idx, const uint64_t *idx_off,
                                  const uint64_t *idx_cap, uint64_t *d_idx_len);

/* ---- DEFLATE streams of dependent pieces, written: pigz's default ---------------------------------------------------------------
 * zwz_deflate_streams_dev gives every piece an empty history, which is what lets a reader cut the stream at the markers and costs
 * ratio: 5 % on text, almost half the file on data with long-range repeats.  Here the pieces stay independent WORK and stop being
 * independent streams.  Stream i is, byte for byte, what libz 1.2.11 writes in this way: the input is cut into pieces of 32 768 bytes;
 * piece k is compressed by a raw deflate stream of its own (windowBits -15, memLevel 8, the default strategy, the context's level)
 * that was given the 32 512 input bytes in front of the piece -- fewer for nothing in front of piece 0 -- with deflateSetDictionary,
 * takes the piece in one deflate call and is ended with deflate(Z_SYNC_FLUSH), whose bytes (00 00 ff ff on a byte boundary) are a
 * full flush's; the pieces' outputs follow one another and 03 00 ends the body.  The wrapper is zwz_deflate_streams_dev's: nothing for
 * ZWZ_WRAP_RAW; 78 9c (78 5e at levels 4 and 5) and the Adler-32 of the whole input; 1f 8b 08 00 00 00 00 00 00 03 and the CRC-32 and
 * ISIZE of the whole input.  No FDICT bit is set: the result is an ordinary stream that gzip -d, zlib.decompress and pigz read.  An
 * empty input is header, 03 00, trailer.
 * Arguments, results, alignment, statuses and the refusals are zwz_deflate_streams_dev's; input i is read, as there, up to its length
 * rounded up to 16, and nowhere else: a piece's dictionary is the caller's own bytes in front of it, nothing is copied.  out_cap[i]
 * >= zwz_deflate_dep_stream_bound(in_len[i], wrap) never overflows (1.002 n).  Under zwz_ctx_set_strategy(2 or 3) these calls return
 * ZWZ_E_INVALID with the reason in zwz_last_error(): there is nothing to gain there.  Every value of the "match" option and the levels
 * 4, 5 and 6 write the same bytes as libz at that level.
 * A reader without an index finds sync markers and no cut where nothing refers back: zwz_inflate_streams_dev and the decode in legs read
 * such a stream with one wave, and the split decode falls back to that.  So the writer can hand the reader the index along with the
 * stream, decoding nothing (zwz_deflate_dep_streams_index_dev): the points are the piece starts, bit 8 * byte and decoded offset
 * 32 768 k, chosen by zwz_deflate_streams_index_dev's rule; entry 0 has hist 0, every later entry hist 32 512, and its window is the
 * input [offset - 32 512, offset), which the writer holds.  The layout is "A seek index for ordinary streams" as it stands, windows
 * included, and every reader of an index takes it.  The entries are every max(span, 32 768) / 32 768-th piece, so their number is
 * ceil(n / max(span, 32 768)) (1 for n = 0), and zwz_deflate_dep_stream_index_bound(n, span) = 64 + 24 count + 32 512 (count - 1)
 * rounded up to 16 is exact: the index has that length (span 0: 1 MiB; 0 for a span that is not allowed).  With span 0 the call takes
 * the context option "index_span_bytes".  d_idx_len[i] is 0 with status 3 or a capacity too small, and then nothing of the index is
 * promised; no byte outside [idx_off[i], idx_off[i] + idx_cap[i]) is written.
 * The file forms run zwz_deflate_stream_file's slice loop, the last 32 512 input bytes of a slice carried in front of the next; with
 * dst_idx the slices' entries and windows are appended by the host and sealed at the end.  A failure leaves neither file.
 * Memory of the _file_index form: the windows are kept on the host until the index is sealed, 32 512 bytes an entry -- 1/32 of the
 * input at the default span of 1 MiB, about the size of the input at a span of 32 KiB or less -- and the call's small device and
 * pinned buffers hold a slice's windows, up to 16.6 MB each.  Choose the span with that in mind for files of many GiB. */
uint64_t zwz_deflate_dep_stream_bound(uint64_t n, int wrap);
int zwz_deflate_dep_streams_dev(zwz_ctx *ctx, int wrap, const uint8_t *d_in, const uint64_t *in_off, const uint64_t *in_len, uint32_t n,
                                uint8_t *d_out, const uint64_t *out_off, const uint64_t *out_cap, uint64_t *d_out_len,
                                uint32_t *d_status);
int zwz_deflate_dep_stream_file(zwz_ctx *ctx, int wrap, const char *src, const char *dst);
uint64_t zwz_deflate_dep_stream_index_bound(uint64_t n, uint32_t span);
int zwz_deflate_dep_streams_index_dev(zwz_ctx *ctx, int wrap, const uint8_t *d_in, const uint64_t *in_off, const uint64_t *in_len, uint32_t n,
                                      uint8_t *d_out, const uint64_t *out_off, const uint64_t *out_cap, uint64_t *d_out_len,
                                      uint32_t *d_status, uint32_t span, uint8_t *d_idx, const uint64_t *idx_off,
                                      const uint64_t *idx_cap, uint64_t *d_idx_len);
int zwz_deflate_dep_stream_file_index(zwz_ctx *ctx, int wrap, const char *src, const char *dst, const char *dst_idx);

/* ---- ZIP archives ---------------------------------------------------------------------------------------------------------------
 * One raw DEFLATE stream per entry, a CRC-32 per entry and a directory at the end: what unzip, Python's zipfile and every file manager
 * open.  Written here: method 8 always; the data of entry i is, byte for byte, zwz_deflate_streams_dev's ZWZ_WRAP_RAW stream of buffer i
 * (an empty buffer is 03 00), at the context's level (zwz_ctx_set_level; flags, versions and zwz_zip_bound do not depend on it); the header fields are fixed (csrc/zip_core.h has the table), so an archive's bytes are a function of its
 * entries alone; ZIP64 records appear where a size, an offset or the count needs them (>= 0xFFFFFFFF, >= 0xFFFF entries), or everywhere
 * with the context option "zip_force_zip64" = "1" (default "0"; "" restores it).  Read here: methods 0 (stored) and 8, ZIP64, data
 * descriptors (sizes and CRC come from the central directory), archive comments.  Not supported: data prepended to the archive,
 * multi-disk archives, encryption, other methods, appending; on the writing side symlinks, empty directories and storing what deflate
 * does not shrink. */
typedef struct zwz_zip_entry {        /* one central-directory record, as zwz_zip_index reads it */
    uint64_t header_off, data_off;    /* local header; first byte of the entry's data (from the LOCAL header's name and extra lengths) */
    uint64_t csize, usize;            /* ZIP64 extra field applied */
    uint64_t name_off;                /* the name's bytes inside the archive (the central directory's copy) */
    uint32_t crc32, external_attr;
    uint16_t name_len, method, flags, dos_time, dos_date, made_by;
} zwz_zip_entry;
typedef struct zwz_zip_meta { uint16_t dos_time, dos_date; uint32_t external_attr; } zwz_zip_meta;
typedef enum zwz_zip_entry_status {   /* beyond 0..3 (zwz_inflate_status) */
    ZWZ_ZIP_UNSUPPORTED = 48,    /* method other than 0 / 8, or encrypted (flag bit 0): nothing read or written */
    ZWZ_ZIP_BAD_ENTRY = 49,      /* data range outside the archive, or stored with csize != usize */
    ZWZ_ZIP_SIZE_MISMATCH = 50,  /* decodes to fewer or more bytes than usize */
    ZWZ_ZIP_CRC_MISMATCH = 51
} zwz_zip_entry_status;
/* Host only (no GPU), with zwz_bgzf_index's convention: e == NULL counts; fewer than *n_entries entries of cap is ZWZ_E_INVALID
 * (*n_entries still set).  Finds the end record behind an archive comment of up to 65535 bytes, follows the ZIP64 locator and record,
 * reads every central record (ZIP64 extra field 0x0001 applied, other extra fields skipped) and every local header (signature; data_off).
 * ZWZ_E_FORMAT, zwz_last_error() naming the entry and the byte offset: no end record, a disk number other than 0, a record or name
 * past the archive, a wrong signature, a count that disagrees with the records present, a local header or data range outside
 * [0, directory start), a stated directory offset that is not where the directory is (prepended data).  An unsupported method or
 * encryption is not an index error: it is that entry's status in zwz_unzip_dev. */
int zwz_zip_index(const uint8_t *zip, uint64_t n, zwz_zip_entry *e, uint32_t cap, uint32_t *n_entries);
/* Worst-case archive bytes for n buffers of these lengths under these names; needs no GPU. */
uint64_t zwz_zip_bound(const uint64_t *in_len, const char *const *names, uint32_t n);
/* n buffers in device memory -> one complete archive at d_out: local header and data of entry 0 .. n-1 tightly packed, the central
 * directory, the end records.  in_off, in_len, names (NUL-terminated, 1..65535 bytes, stored as they are; flag 0x0800 iff a byte is
 * >= 0x80) and meta are HOST arrays and may be reused when the call returns; meta == NULL: time 0, date 0x0021 (1980-01-01), attribute
 * 0100644 << 16.  d_in, d_out and every in_off[i] are multiples of 16; buffer i is readable up to its length rounded up to 16.
 * *d_out_len (device) receives the length the archive needs, whether it fitted or not, and *d_status (device) 0, or 3 when that is
 * more than out_cap: the contents are then undefined and nothing outside [0, out_cap) is written.  out_cap >= zwz_zip_bound(...) never
 * overflows.  Asynchronous on the context's stream.  The entries are compressed as gzip streams into staging the context keeps (about
 * the input's size again) and copied to their places from there.  ZWZ_E_INVALID for a name of length 0 or above 65535, a misaligned
 * pointer or offset, a null pointer. */
int zwz_zip_dev(zwz_ctx *ctx, const uint8_t *d_in, const uint64_t *in_off, const uint64_t *in_len, const char *const *names,
                const zwz_zip_meta *meta, uint32_t n, uint8_t *d_out, uint64_t out_cap, uint64_t *d_out_len, uint32_t *d_status);
/* The archive in device memory (d_zip 16-byte aligned, readable up to zip_len rounded up to 16, never read past that) and n entries
 * of zwz_zip_index, or any others, in HOST memory.  Entry i decodes to d_out + out_off[i] (host array, multiples of 16): the range
 * holds exactly entries[i].usize bytes and no byte outside it is ever written.  d_out_len[i] (device u64): the bytes decoded.
 * d_status[i] (device): 0 or the first of ZWZ_ZIP_UNSUPPORTED, ZWZ_ZIP_BAD_ENTRY, ZWZ_STREAM_TOO_LARGE (a DEFLATED entry with csize >=
 * 2^29 or usize >= 2^32: zwz_inflate_split_streams_dev's limits; stored entries have none), inflate's 1 / 2, ZWZ_ZIP_SIZE_MISMATCH
 * (inflate's overflow status 3 included), ZWZ_ZIP_CRC_MISMATCH.  d_segments (device, may be NULL): as zwz_inflate_split_streams_dev
 * reports it -- an entry this library wrote has a flush point every 65280 bytes and is decoded a wave per piece --, 0 for stored
 * entries.  Data moves and the CRC-32 are dealt by tiles of 65280 bytes, never by entry.  NOT asynchronous, exactly as
 * zwz_inflate_split_streams_dev (zwz_ctx_sync before reading results). */
int zwz_unzip_dev(zwz_ctx *ctx, const uint8_t *d_zip, uint64_t zip_len, const zwz_zip_entry *entries, uint32_t n, uint8_t *d_out,
                  const uint64_t *out_off, uint64_t *d_out_len, uint32_t *d_status, uint32_t *d_segments);
/* The regular files under src_dir (no symlinks, no empty directories) as one archive: names relative to src_dir with '/', in bytewise
 * name order; time and date from st_mtime in local time (year clamped to 1980..2107, seconds halved), attribute st_mode << 16.  Files
 * pass through pinned staging in slices of whole files of "zip_slice_bytes" (context option, default 268435456; a larger file is a
 * slice of its own); reading, the GPU and writing overlap; the central directory is kept on the host and written at the end.  An
 * empty directory gives the valid 22-byte archive.  Written as <dst_zip>.part and renamed on success only. */
int zwz_zip_dir(zwz_ctx *ctx, const char *src_dir, const char *dst_zip);
/* Extracts an archive below dst_dir (created if missing), in slices of consecutive entries by the same option.  Before anything is
 * created every name is checked: an empty or absolute name, a `..` component, a backslash, a NUL or a duplicate is ZWZ_E_FORMAT naming
 * the entry; so is a deflated entry above zwz_unzip_dev's limits.  A name ending in '/' with size 0 is a directory.  Files get mode
 * (external_attr >> 16) & 0777 when made_by's high byte is 3 and that is not zero, and the entry's time.  An entry whose status is not
 * 0 ends the call after its slice: ZWZ_E_CHECKSUM for a CRC or size mismatch, ZWZ_E_FORMAT otherwise; its file is not left behind. */
int zwz_unzip_file(zwz_ctx *ctx, const char *src_zip, const char *dst_dir);

#ifdef __cplusplus
}
#endif
#endif
