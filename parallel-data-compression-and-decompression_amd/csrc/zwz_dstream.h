// zwz_dstream.h -- zwz_deflate_streams_dev and zwz_deflate_dep_streams_dev: the kernels that turn the deflate slots of independent or
// dependent pieces into whole raw, zlib or gzip streams (zwz_dstream.hip) and their host driver (zwz_dstream.cpp).  dstream_core.h has
// the format and the two piece forms.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dstream_core.h"
#include "zwz_kernels.h"

namespace zwz {

// Per stream, device memory.  Stream i's pieces are pfirst[i] .. pfirst[i + 1] - 1, counted over the whole call (n + 1 entries).
struct DstreamStreams {
    const uint64_t *in_off, *in_len, *out_off, *out_cap, *pfirst;
    uint64_t* xs;              // the scan's value at the stream's first piece, for its pieces in later slices
    uint32_t* chk;             // the checksum of the stream's pieces so far
    uint32_t n;
    // zwz_deflate_streams_index_dev only
    const uint64_t *idx_off, *idx_cap;
    uint64_t *rs, *cnt;        // the rank scan's value at the stream's first piece; its entries, once its last piece is known
};
// Per piece of one slice: piece p of the slice is piece g0 + p of the call.  off / len are the codec's chunk: the piece with its dictionary
// of `skip` bytes in front (dstream_core.h: dependent pieces); poff / plen are the piece alone, what its checksum covers.  Independent
// pieces have no dictionary: skip is 0 and the two are the same range.
struct DstreamPieces {
    uint8_t* slots;            // ZWZ_DEV_STRIDE bytes each: the piece's zlib stream
    uint64_t *off, *poff, *x;  // its input; bytes of spliced output in front of it (over the whole call)
    uint32_t *len, *plen, *skip, *olen, *crc, *sidx, *slen, *hbit, *ebit;   // input, slot and spliced lengths; CRC-32 (gzip) or the piece's own Adler-32 (dependent, zlib); stream; dstream_core.h's SplicePoints
    uint32_t* due;             // index: whether the piece's first block is an entry (index_core.h: index_flush_due)
    uint64_t* rank;            // index: entries in front of it (over the whole call)
};
struct DstreamOut { uint8_t* out; uint64_t* out_len; uint32_t* status; uint32_t wrap; uint32_t partial; uint32_t zflg; uint32_t xfl; };   // partial: pieces only (no header, no 03 00, no trailer); zflg: zlib_flg_of(level, strategy); xfl: gzip_xfl_of(strategy)

// The index at the pieces' starts (index_core.h).  off_base, pos_base: the decoded bytes and the stream bytes in front of a partial
// call's input and output (the file function's slices), 0 otherwise.
struct DstreamIndex { uint8_t* idx; uint64_t* idx_len; uint32_t span; uint64_t off_base, pos_base; };

// Every step takes the piece form F where the geometry matters: kPiecesAlone or kPiecesDep (dstream_core.h).
hipError_t launch_dstream_begin(const DstreamStreams& S, const DstreamOut& O, hipStream_t s);
// lead: the dictionary bytes in front of every stream's first piece (0; the dependent file call's later slices: kDepDictBytes)
hipError_t launch_dstream_layout(const DstreamStreams& S, const DstreamPieces& P, PieceForm F, uint32_t lead, uint64_t g0, uint32_t m, hipStream_t s);
// The checksum of a piece is computed from its own bytes, poff / plen, into P.crc: crc32_blocks under gzip, this under zlib for dependent
// pieces (their slot's Adler-32 covers the dictionary too; an independent piece's is read from its slot by combine)
hipError_t launch_dstream_adler(const uint8_t* in, const DstreamPieces& P, uint32_t m, uint32_t cu_count, hipStream_t s);
hipError_t launch_dstream_size(const ChunkInfo* info, const BlockInfo* blocks, const BlockOut* plans, const DstreamPieces& P, uint32_t m, uint32_t* err,
                               hipStream_t s);   // *err = 1 if a piece's records contradict its slot
// streams s0 .. s0 + ns - 1 are those with a piece in the slice
hipError_t launch_dstream_combine(const DstreamStreams& S, const DstreamPieces& P, PieceForm F, uint64_t g0, uint32_t m, uint32_t s0, uint32_t ns, uint32_t wrap,
                                  hipStream_t s);
hipError_t launch_dstream_pack(const DstreamStreams& S, const DstreamPieces& P, uint64_t g0, uint32_t m, const DstreamOut& O, const uint32_t* err,
                               hipStream_t s);
// The index of a slice: the due flags (before the rank scan) and the entries (behind it and behind pack) -- of dependent pieces the
// windows too; in: the call's input.  win_base (partial calls): where in the stream's index space the slice's windows go, back to back; a
// whole call puts them behind the entries, whose number index_dep_count gives beforehand
hipError_t launch_dstream_due(const DstreamStreams& S, const DstreamPieces& P, PieceForm F, uint64_t g0, uint32_t m, const DstreamIndex& X, hipStream_t s);
hipError_t launch_dstream_index(const uint8_t* in, const DstreamStreams& S, const DstreamPieces& P, PieceForm F, uint64_t g0, uint32_t m, const DstreamOut& O,
                                const DstreamIndex& X, uint64_t win_base, hipStream_t s);
// Behind the last slice, whole streams only: every stream's header, index CRC and idx_len
hipError_t launch_dstream_index_seal(const CrcTables* tab, const DstreamStreams& S, PieceForm F, const DstreamOut& O, const DstreamIndex& X, uint32_t cu_count,
                                     hipStream_t s);

}  // namespace zwz
