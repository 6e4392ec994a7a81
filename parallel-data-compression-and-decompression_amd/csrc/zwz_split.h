// zwz_split.h -- launcher interface of zwz_split.hip: the scan, resolve and checksum kernels of zwz_inflate_split_streams_dev
// (split_core.h has the method; the measuring and the segment decode are forms of inflate_kernel, zwz_kernels.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "split_core.h"

namespace zwz {

struct CrcTables;

// The batch as the caller gave it, plus what the head kernel found
struct SplitStreams {
    const uint8_t* in; const uint64_t* in_off; const uint64_t* in_len; const uint64_t* out_cap; uint32_t n;
    uint32_t wrap;
    uint32_t* body;            // n: first byte of the DEFLATE data, kSplitNil for a stream that is not scanned
    const uint32_t* tile_first;   // n + 1: a stream's first scan tile (host; no tiles for a stream the sizes rule out)
    uint32_t n_tiles;
    uint32_t* tile_cnt;        // per tile: candidates in it
    uint64_t* tile_off;        // per tile: candidates in front of it (exclusive scan)
    uint64_t* base;            // [0]: all candidates; [1] (as uint32): the scan's error word, unused
    uint64_t* cfirst;          // n + 1: candidates in front of a stream
    const uint32_t* kbase;     // n + 1 (host): kept candidates in front of a stream; a stream that is not kept has none
};
// Per kept candidate
struct SplitCands {
    uint32_t m;
    uint32_t* pos;             // stream offset p, ascending within a stream
    uint4* seg;                // inflate_kernel's segment record, measuring form
    uint64_t* in_off; uint64_t* in_len;   // the measuring wave's input
    uint4* meas;               // SegMeasure
    uint32_t* jump;            // levels * m: node 2^level steps down the chain, kSplitNil behind its end
    uint32_t* mark;            // 1: on the chain of its stream
    uint32_t* ostart;          // marked: output bytes of the stream in front of the segment
    uint32_t* rank;            // marked: chain segments in front of it
};
// Per stream, after resolve: (splits, chain segments, decoded bytes, expected checksum)
struct SplitDecode {
    const uint4* res; const uint32_t* dbase;   // n + 1 (host): chain segments of splitting streams in front of a stream
    uint64_t* in_off; uint64_t* in_len; uint4* seg;   // per chain segment: the segment form's input and record
};
// zwz_inflate_split_streams_index_dev: where the indexes go (device arrays, as the caller gave them), and per stream its entries
struct SplitIndex { uint8_t* idx; const uint64_t *idx_off, *idx_cap; uint64_t* idx_len; uint32_t* count; uint32_t span; };
struct SplitPieces {
    const uint32_t* pbase;     // n + 1 (host): checksum pieces of splitting streams in front of a stream
    uint32_t p;
    uint64_t* off; uint32_t* len; uint32_t* val;
};

hipError_t launch_split_head(const SplitStreams& S, uint32_t min_bytes, hipStream_t s);
hipError_t launch_split_count(const SplitStreams& S, hipStream_t s);                    // tile_cnt, tile_off, base, cfirst
hipError_t launch_split_write(const SplitStreams& S, const SplitCands& C, uint32_t budget, hipStream_t s);
// partial != 0 (one slice of a file): res = the longest prefix of the chain that ended cleanly and fits pcap, res2 = (its end, how it ended,
// a final block's end bit within its byte); partial == 0: res2 = the same of the chain's last segment
hipError_t launch_split_resolve(const SplitStreams& S, const SplitCands& C, uint32_t levels, uint4* res, uint32_t partial, uint64_t pcap, uint4* res2,
                                hipStream_t s);
hipError_t launch_split_emit(const SplitStreams& S, const SplitCands& C, const SplitDecode& D, hipStream_t s);
// piece checksums of the splitting streams' output, joined per stream; writes out_len, status and (if not null) segments of those streams;
// chk_out not null: the checksum itself goes there and is not compared
hipError_t launch_split_finish(const SplitStreams& S, const SplitDecode& D, const SplitPieces& P, const CrcTables* tab, const uint8_t* out,
                               const uint64_t* out_off, const uint32_t* bad, uint64_t* out_len, uint32_t* status, uint32_t* segments,
                               uint32_t* chk_out, uint32_t cu_count, hipStream_t s);
// The index at the chain's piece starts (index_core.h: the index at full-flush points).  index: behind emit, the entries of every
// splitting stream and their count; seal: behind finish, the header, the padding, the index CRC and idx_len (0 where the final status
// is not 0 or the capacity is too small) of every splitting stream; the others keep what the fallback gave them.
hipError_t launch_split_index(const SplitStreams& S, const SplitDecode& D, const SplitIndex& X, hipStream_t s);
hipError_t launch_split_seal(const SplitStreams& S, const SplitDecode& D, const SplitIndex& X, const uint4* res2, const CrcTables* tab, const uint32_t* status,
                             uint32_t cu_count, hipStream_t s);

}  // namespace zwz
