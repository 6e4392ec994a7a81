// zwz_api_internal.h -- context object behind include/zwz.h.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/zwz.h"
#include "index_core.h"
#include "split_core.h"
#include "zwz_kernels.h"

namespace zwz {

// A grow-only allocation of the context, in device memory or pinned on the host.  `count` is the number of elements (chunks, members,
// pieces, streams) the arrays in it were laid out for: a layout is always carved by that capacity, never by the current call's size.
struct Buffer {
    void* p = nullptr;
    size_t bytes = 0, count = 0;
    bool pinned = false;
    // Returns at once if `count` elements and `bytes` bytes are reserved already.  Otherwise waits for the context's stream (queued
    // work may still use the old allocation), frees it and allocates anew; on failure everything is left at zero.
    int reserve(zwz_ctx* c, size_t count, size_t bytes);
    void release();
    template <class T> T* as() const { return static_cast<T*>(p); }
};

enum BufId {
    kBufWorkspace,       // deflate: carve_workspace's arrays, per chunk
    kBufInfOrder,        // inflate's launch order ((offset, length, chunk) by payload length), a uint4 per chunk, stream or segment
    kBufStreamRec,       // zwz_inflate_streams_dev: a StreamRecord per stream
    kBufStageDev,        // staging of the host-buffer entry points and the directory pipeline (stage_view), and its pinned twin
    kBufCrcTables,       // built on first use (ensure_crc_tables)
    kBufBgzf,            // BGZF (zwz_bgzf.cpp): slots and per-member arrays
    kBufRangeDev,        // range reads: the packed plan of one call, and its pinned twin
    kBufPieces,          // stream deflate (zwz_dstream.cpp): slots and per-piece arrays
    kBufStreamsDev,      // stream deflate: the per-stream arrays of one call, and their pinned twin
    kBufSplit0, kBufSplit1, kBufSplit2,      // split inflate (zwz_split.cpp): per stream and scan tile / per candidate / per chain segment and checksum piece
    kBufZipStage,        // ZIP (zwz_zip.cpp): the entries' gzip streams on the way in, their gathered data on the way out
    kBufZipDev,          // ZIP: the per-entry and per-tile arrays of one call, and their pinned twin
    kBufIndex0,          // seek index (zwz_index.cpp): segment records, window moves, checksum pieces and flags of one call, and its pinned twin
    kBufIndex1,          // seek index: an index uploaded for a call, or the scratch slots of a range read
    kBufLegs,            // decode in legs (zwz_legs.cpp): the per-stream arrays of one call, and their pinned twin
    kBufLegPieces,       // decode in legs: the checksum pieces of one call
    kBufWalk0, kBufWalk1,                    // BGZF member walk (zwz_bgzf_walk.hip): per span and scan tile / per candidate and member
    kNumDeviceBufs,
    kBufStageHost = kNumDeviceBufs, kBufRangeHost, kBufStreamsHost,
    kBufSplitHost,       // split inflate: the per-stream arrays a call uploads (read by copies that may still be queued when it returns)
    kBufZipHost,
    kBufIndexHost,
    kBufLegsHost,
    kBufWalkHost,        // BGZF member walk: the spans a call uploads and the results it brings back
    kNumBufs
};

}  // namespace zwz

struct zwz_ctx {
    int device = 0;
    uint32_t max_batch = 0;
    hipStream_t stream = nullptr;
    uint32_t cu_count = 0;
    uint32_t chunk_bytes = 0;        // raw bytes per Chunk for zwz_compress_dir; 0 = default (see chunk_bytes_for)
    uint32_t level = 6;              // libz's compression level of every writer: 4, 5 or 6 (zwz_ctx_set_level; default from ZWZ_LEVEL at zwz_ctx_create)
    uint32_t strategy = 0;           // libz's strategy of every writer: 0 (default), 2 (Z_HUFFMAN_ONLY) or 3 (Z_RLE) (zwz_ctx_set_strategy; default from ZWZ_STRATEGY);
                                     // while it is 2 or 3 the level is kept and changes no byte
    // Switches (zwz_ctx_set_option; defaults from ZWZ_MATCH / ZWZ_PLAN / ZWZ_INFLATE_HEADER read ONCE at zwz_ctx_create, or forced by a
    // failed self-test there).  Every setting produces the same bytes; they differ in which kernels run.
    uint32_t match_mode = 0;             // zwz::kMatchAuto | kMatchWalk | kMatchBand
    uint32_t plan_serial = 0;            // 1: lane-serial block flush
    uint32_t inflate_serial_header = 0;  // 1: block headers and tables on lane 0
    // Kernel forms this device failed a self-test of at zwz_ctx_create (kForbid*): zwz_ctx_set_option refuses to switch them back on
    uint32_t forbidden = 0;
    bool profiling = false;
    hipEvent_t ev[zwz::kNumDeflateStages + 1] = {};
    hipEvent_t ev_inf[2] = {};
    float stage_ms[ZWZ_NUM_STAGES] = {};
    hipEvent_t ds_copied = nullptr;  // stream deflate: the last call's copy out of the pinned per-stream arrays (kBufStreamsHost) has run
    // split inflate (zwz_split.cpp): options "split_min_bytes", "split_budget", "split_max_candidates" (split_core.h's defaults)
    uint32_t split_min_bytes = zwz::kSplitMinBytes, split_budget = zwz::kSplitBudget, split_max_candidates = zwz::kSplitMaxCandidates;
    uint32_t split_slice_bytes = zwz::kSplitSliceBytes;      // zwz_inflate_stream_file: "split_slice_bytes"
    uint32_t index_span_bytes = zwz::kIdxSpanDefault;        // zwz_inflate_streams_index_dev with span 0: "index_span_bytes"
    // decode in legs (zwz_legs.cpp): options "leg_bytes" and "leg_out_bytes" (leg_core.h's defaults)
    uint64_t leg_bytes = zwz::kLegBytesDefault, leg_out_bytes = zwz::kLegOutBytesDefault;
    // the file loop (zwz_legs_file.cpp): options "leg_file_bytes" and "leg_file_out_bytes" (legfile_core.h's defaults), the staging windows
    uint64_t leg_file_bytes = zwz::kLegFileBytesDefault, leg_file_out_bytes = zwz::kLegFileOutBytesDefault;
    // ZIP (zwz_zip.cpp): options "zip_force_zip64" and "zip_slice_bytes"; the last call's copy out of kBufZipHost has run
    uint32_t zip_force_zip64 = 0;
    uint64_t zip_slice_bytes = 268435456ull;
    hipEvent_t zip_copied = nullptr;
    // Every allocation that outlives a call: grown lazily to the largest call seen (Buffer::reserve), released by zwz_ctx_destroy
    zwz::Buffer buf[zwz::kNumBufs];
    zwz_ctx() { for (int i = zwz::kNumDeviceBufs; i < zwz::kNumBufs; i++) buf[i].pinned = true; }
};

namespace zwz {

enum : uint32_t { kForbidLinks = 1u, kForbidSort = 2u, kForbidPlanWave = 4u, kForbidInflateWave = 8u };   // zwz_ctx::forbidden

void set_error(const char* fmt, ...);
int hip_fail(hipError_t e, const char* what);
int ensure_workspace(zwz_ctx* c, uint32_t chunks);
void carve_workspace(zwz_ctx* c, DeflateArgs& a);
// zwz_deflate_batch_dev with a start offset per chunk (d_skip, device memory, or null: none): chunk i's first d_skip[i] bytes are a dictionary,
// searched against and never coded (zwz_kernels.h: DeflateArgs::skip).  The slot's Adler-32 still covers the whole chunk.  Internal: the
// stream writer's dependent pieces (zwz_dstream.cpp); the public call has no such argument.
int deflate_batch_dev_skip(zwz_ctx* c, const uint8_t* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len, const uint32_t* d_skip, uint32_t n,
                           uint8_t* d_out, uint64_t out_stride, uint32_t* d_out_len);
int ensure_staging(zwz_ctx* c, uint32_t chunks);
int ensure_inf_order(zwz_ctx* c, uint32_t n);
int ensure_crc_tables(zwz_ctx* c);            // builds the tables on first use, on the context's stream

#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return hip_fail(e_, #x); } while (0)

inline size_t round_up(size_t v, size_t a) { return (v + a - 1) & ~(a - 1); }   // a: a power of two

// little-endian fields of a host buffer (le32_at / be32_at: stream_core.h)
inline uint32_t le16_at(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
inline uint64_t le64_at(const uint8_t* p) { return (uint64_t)le32_at(p) | (uint64_t)le32_at(p + 4) << 32; }

// Lays arrays out one after the other from `base`, each at a multiple of 256 bytes.  Every workspace has ONE layout function that
// takes a Carver: run over base 0 it gives the bytes to reserve (layout_bytes), run over the buffer it gives the pointers, so the two
// cannot disagree.  Offsets are integers: nothing is added to a null pointer.
struct Carver {
    uintptr_t base;
    size_t used = 0;
    explicit Carver(const void* p) : base(reinterpret_cast<uintptr_t>(p)) {}
    template <class T> T* take(size_t count, size_t slack = 0) {
        T* r = reinterpret_cast<T*>(base + used);
        used += round_up(count * sizeof(T) + slack, 256);
        return r;
    }
};
template <class F> size_t layout_bytes(F&& layout) { Carver w(nullptr); layout(w); return w.used; }

// One staging slice: input slots, output slots, offsets/lengths/status; same layout on host and device.
struct StageView {
    uint8_t *h_in, *h_out; uint64_t* h_off; uint32_t *h_len, *h_olen, *h_status;
    uint8_t *d_in, *d_out; uint64_t* d_off; uint32_t *d_len, *d_olen, *d_status;
};

// The staging arrays from chunk `first` on (the buffers are laid out for kBufStageDev's count)
StageView stage_view(zwz_ctx* c, uint32_t first);

}  // namespace zwz
