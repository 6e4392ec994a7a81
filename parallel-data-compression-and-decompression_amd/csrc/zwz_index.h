// zwz_index.h -- launcher interface of zwz_index.hip: the kernels around inflate_kernel's marking and indexed-segment forms
// (index_core.h has the layout and the method; the two forms themselves are in zwz_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "index_core.h"
#include "zwz_bgzf.h"

namespace zwz {

// After the marking decode and its checksum: per stream, the windows out of the decoded output into the index, the header, the
// index CRC; idx_len[i] = 0 where the stream's status is not 0.
struct IndexBuild {
    const uint8_t* out; const uint64_t* out_off; const uint64_t* in_len; const uint32_t* status; uint32_t n, wrap, span;
    uint8_t* idx; const uint64_t* idx_off; uint64_t* idx_len;
};
hipError_t launch_index_windows(const CrcTables* tab, const IndexBuild& b, hipStream_t s);

// One window to place: `len` bytes at `src` of the index buffer go to `dst` of the output (or of the scratch slots); `stream`: whose
// flag a difference sets
struct IndexMove { uint64_t src, dst; uint32_t len, stream; };
hipError_t launch_index_place(const uint8_t* idx, uint8_t* out, const IndexMove* mv, uint32_t m, hipStream_t s);
// The file loop's commit: window i, mv[i].len bytes at mv[i].src of a leg's output staging (stage_len bytes readable), goes to mv[i].dst
// of `packed` (packed_cap bytes).  Offsets are 64-bit; a move outside either buffer is skipped.
hipError_t launch_index_gather(const uint8_t* stage, uint64_t stage_len, uint8_t* packed, uint64_t packed_cap, const IndexMove* mv, uint32_t m, hipStream_t s);
// flag[stream] |= 1 where a window differs from the bytes that now stand at its place
hipError_t launch_index_compare(const uint8_t* idx, const uint8_t* out, const IndexMove* mv, uint32_t m, uint32_t* flag, hipStream_t s);

// The checksum pieces of out[0, total): the first `head` bytes, then kPieceBytes each -- piece_off, piece_len and piece_val (the file
// call joins the slices' pieces on the host)
struct IndexPieces {
    const uint8_t* out; uint64_t total; uint32_t head, wrap;
    uint64_t* piece_off; uint32_t* piece_len; uint32_t* piece_val; uint32_t pieces;
};
hipError_t launch_index_piece_sums(const CrcTables* tab, const IndexPieces& f, uint32_t cu_count, hipStream_t s);

// One stream of a whole decode (zwz_inflate_indexed_batch_dev; the one-stream call is a batch of one).  Its bytes are in[in_off, in_off +
// in_len) with the trailer at byte `trailer` of them; its output out[out_off, out_off + total) with the checksum pieces piece0 ..
// piece0 + pieces (index_core.h's layout from `head`).  refused: a verdict the host has reached already (no segment of the stream runs).
struct IndexStream {
    uint64_t in_off, in_len, trailer, out_off, total;
    uint32_t head, wrap, expect, nseg, piece0, pieces, refused, pad;
};
// The pieces of all streams, their checksums -- the first `gzip_pieces` of the list are CRC-32's, the others Adler-32's -- and a wave
// per stream that joins its pieces and gives the verdict: refused, else bad[i] -> kStrIndex; a window that was not the stream's bytes
// (flag[i]), a checksum other than the index's or other than the stream's own trailer -> kStrChecksum; else 0.  Writes out_len[i],
// status[i] and, if given, segments[i] of every stream.
struct IndexBatch {
    const uint8_t* in; const uint8_t* out; const IndexStream* rec; uint32_t n;
    uint64_t* piece_off; uint32_t* piece_len; uint32_t* piece_val; uint32_t pieces, gzip_pieces;
    const uint32_t* bad; const uint32_t* flag;
    uint64_t* out_len; uint32_t* status; uint32_t* segments;
};
hipError_t launch_index_batch_finish(const CrcTables* tab, const IndexBatch& b, uint32_t cu_count, hipStream_t s);

// The decode in legs (zwz_inflate_legs_dev): the checksum of out[out_off, out_off + total) of every stream from the same pieces, joined
// and compared with `expect`; status[i] = ZWZ_STREAM_CHECKSUM where they differ.  Of an IndexStream it reads out_off, total (the checked
// length), head, wrap, expect, piece0, pieces, refused (the stream got its verdict from the host) and nseg (0: no checksum was read).
struct LegsCheck {
    const uint8_t* out; const IndexStream* rec; uint32_t n, wrap;
    uint64_t* piece_off; uint32_t* piece_len; uint32_t* piece_val; uint32_t pieces;
    uint32_t* status;
};
hipError_t launch_legs_check(const CrcTables* tab, const LegsCheck& b, uint32_t cu_count, hipStream_t s);

// Range reads: touched segment i's decoded bytes start at slots + slot_off[i]; its pieces row[i] .. row[i + 1], the first nlong[i] of
// them long, go to out (bgzf_verify_extract's dealing).  Pieces of a segment whose bad[i] is set are not copied.
hipError_t launch_index_extract(const uint8_t* slots, const uint64_t* slot_off, const uint32_t* row, const uint32_t* nlong, const RangePiece* pieces,
                                uint32_t m, const uint32_t* bad, uint8_t* out, uint32_t cu_count, hipStream_t s);

}  // namespace zwz
