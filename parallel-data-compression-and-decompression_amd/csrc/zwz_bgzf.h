// zwz_bgzf.h -- BGZF (SAM/BAM spec section 4.1) framing kernels (zwz_bgzf.hip) and their host driver (zwz_bgzf.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace zwz {

constexpr uint32_t kBgzfBlock = 65280;        // 0xff00, htslib's BGZF_BLOCK_SIZE: raw bytes per member
constexpr uint32_t kBgzfHeader = 18;          // 1f 8b 08 04 | mtime | 00 ff | 06 00 | 'B' 'C' 02 00 | BSIZE-1
constexpr uint32_t kBgzfTrailer = 8;          // CRC-32, ISIZE
constexpr uint32_t kBgzfEofBytes = 28;
constexpr uint32_t kBgzfMaxIsize = 65535;     // the inflate slot
constexpr uint32_t kBgzfSlot = 65536;         // gathered bodies and decoded blocks: one 16-byte aligned slot each
constexpr uint32_t kBgzfThreads = 256;        // lanes of the CRC workgroup (crc_core.h's T)
// Worst case of a level-6 zlib stream of kBgzfBlock bytes: at most kMaxBlocks stored blocks (5 header bytes each), the 2 + 4 bytes of
// zlib framing, and a few bytes of bit padding where stored and coded blocks meet.  Far below the 65535-byte deflate slot, so no
// member body is ever cut; bgzf_scan still flags a stream that reaches the slot's length (the output length then reads ~0).
// The same at levels 4 and 5 (zwz_ctx_set_level): the worst case is stored blocks, and the block cuts (16 383 symbols) do not depend on the level.
static_assert(kBgzfBlock + 5u * 5u + 6u + 16u < 65535u, "a BGZF block's level-6 stream always fits the deflate slot");

// Range reads: one piece is len bytes at offset off of a touched member's decoded block, bound for out + dst
struct RangePiece { uint64_t dst; uint32_t off; uint32_t len; };
constexpr uint32_t kNoExpect = 0xffffffffu;       // no index entry follows the member: its decoded length is not known in advance
constexpr uint32_t kBgzfIndexMismatch = 32;       // member status (internal): decoded length differs from what the .gzi implies
constexpr uint32_t kWavePieceMax = 4096;          // pieces of at least this many bytes go with the workgroup, shorter ones with a wave

extern const uint8_t kBgzfEof[kBgzfEofBytes];

// CRC tables in device memory (crc_core.h): slicing tables, the lane stride's multiplier, every lane's closing shift.
struct CrcTables { uint32_t vec[16 * 256]; uint32_t mul[4 * 256]; uint32_t lane[kBgzfThreads]; };

hipError_t launch_crc_tables(CrcTables* t, hipStream_t s);
// off[i] = (first + i) * kBgzfBlock, len[i] = min(kBgzfBlock, n - off[i])
hipError_t launch_bgzf_layout(uint64_t* off, uint32_t* len, uint64_t first, uint32_t m, uint64_t n, hipStream_t s);
// crc[i] = crc32(in + off[i], len[i]); in + off[i] 16-byte aligned, nothing read past len[i]
hipError_t launch_crc32_blocks(const CrcTables* t, const uint8_t* in, const uint64_t* off, const uint32_t* len, uint32_t m, uint32_t* crc,
                               uint32_t cu_count, hipStream_t s);
// off[i] = *base + sum_{j<i} (v[j] + add); *base += the total; *err = 1 if some v[j] > limit
hipError_t launch_bgzf_scan(const uint32_t* v, uint32_t m, uint32_t add, uint32_t limit, uint64_t* off, uint64_t* base, uint32_t* err, hipStream_t s);
// member i at out + moff[i]: header, deflate slot i's bytes [2, olen - 4), crc[i], isize[i]
hipError_t launch_bgzf_pack(const uint8_t* slots, const uint32_t* olen, const uint32_t* crc, const uint32_t* isize, const uint64_t* moff,
                            uint32_t m, uint8_t* out, hipStream_t s);
// eof: the EOF member at out + *base and *out_len = *base + 28; else *out_len = *base.  *err != 0: *out_len = ~0
hipError_t launch_bgzf_finish(uint8_t* out, const uint64_t* base, const uint32_t* err, uint64_t* out_len, int eof, hipStream_t s);
// members first .. first + m - 1 of gz: body behind 78 9c in slot i, in_off / in_len for inflate, stored crc / isize; status[i] = 0 or
// ZWZ_BGZF_BAD_MEMBER (then in_len = 2, isize = 0)
hipError_t launch_bgzf_gather(const uint8_t* gz, uint64_t gz_len, const uint64_t* member_off, uint32_t n_members, uint32_t first, uint32_t m,
                              uint8_t* slots, uint64_t* in_off, uint32_t* in_len, uint32_t* crc, uint32_t* isize, uint32_t* status, hipStream_t s);
// checks decoded slot i against crc / isize (status[i]: first failure wins) and copies min(olen, isize) bytes to out + ooff[i]
hipError_t launch_bgzf_verify_compact(const CrcTables* t, const uint8_t* slots, const uint32_t* olen, const uint32_t* inf_status, const uint32_t* crc,
                                      const uint32_t* isize, const uint64_t* ooff, uint32_t m, uint8_t* out, uint32_t* status, uint32_t cu_count,
                                      hipStream_t s);

// touched members: member i at gz + moff[i], readable up to min(mend[i], gz_len) (mend may be null: gz_len).  The header is parsed
// and bounds-checked on the device; then as launch_bgzf_gather for slot i (status[i] = 0 or ZWZ_BGZF_BAD_MEMBER)
hipError_t launch_bgzf_gather_list(const uint8_t* gz, uint64_t gz_len, const uint64_t* moff, const uint64_t* mend, uint32_t m, uint8_t* slots,
                                   uint64_t* in_off, uint32_t* in_len, uint32_t* crc, uint32_t* isize, uint32_t* status, hipStream_t s);
// checks decoded slot i (status[i]: first failure wins; kBgzfIndexMismatch when the length is not expect[i]) and copies its pieces
// [row[i], row[i + 1]) -- the first nlong[i] of them >= kWavePieceMax bytes -- to out; bad_piece[i] = smallest piece past the block's end
hipError_t launch_bgzf_verify_extract(const CrcTables* t, const uint8_t* slots, const uint32_t* olen, const uint32_t* inf_status, const uint32_t* crc,
                                      const uint32_t* isize, const uint32_t* expect, const uint32_t* row, const uint32_t* nlong, const RangePiece* pieces,
                                      uint32_t m, uint8_t* out, uint32_t* status, uint32_t* bad_piece, uint32_t cu_count, hipStream_t s);

}  // namespace zwz
