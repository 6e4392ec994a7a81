// dstream_core.h -- the portable half of zwz_deflate_streams_dev: how the streams of independent pieces (level 6, or the context's level) become one raw, zlib
// or gzip stream of any size.  Host + device, so that a CPU build (tests/emu_dstream) pins every formula here against libz.
//
// The output is what libz 1.2.11 writes when every kPieceBytes of input are followed by deflate(Z_FULL_FLUSH) and the last by
// deflate(Z_FINISH).  A full flush with all input consumed clears libz's hash and window, so each piece is compressed as if alone,
// and its share of the output differs from its own Z_FINISH raw stream -- bytes [2, len - 4) of zwz_deflate_batch_dev's slot -- in
// two places only:
//   * the BFINAL bit of its last block's header is 0;
//   * after the last block's end-of-block code (or a stored block's last data byte) come the three header bits 000 of an empty
//     stored block, zero bits up to a byte boundary, and LEN / NLEN = 00 00 ff ff.  The Z_FINISH stream pads with zero bits at the
//     same place, so its bytes are kept and the marker adds 4 bytes when the block ends 1 to 5 bits into a byte, else 5.
// After the last piece's marker Z_FINISH writes 03 00 (an empty final static block, padded) and the wrapper's trailer.
#pragma once
#include "crc_core.h"
#include "huff_core.h"
#include "stream_core.h"

namespace zwz {

constexpr uint32_t kPieceBytes = 65280;       // input bytes per piece: BGZF's block, whose level-6 stream always fits the deflate slot
constexpr uint32_t kGzipHeaderBytes = 10;     // 1f 8b 08 00 | mtime 0 | 00 | 03 (libz's deflate with no gz_header: OS_CODE 3)

ZWZ_HD uint32_t dstream_header_bytes(uint32_t wrap) { return wrap == kWrapZlib ? 2u : wrap == kWrapGzip ? kGzipHeaderBytes : 0u; }
ZWZ_HD uint32_t dstream_trailer_bytes(uint32_t wrap) { return wrap == kWrapZlib ? 4u : wrap == kWrapGzip ? 8u : 0u; }
// flg: the zlib header's second byte, zlib_flg(level) -- 9c at level 6, 5e at 4 and 5, 01 under a strategy (rle_core.h: zlib_flg_of).  The gzip header does
// not depend on the level: libz's XFL is 0 but at 1 and 9 -- and under Z_HUFFMAN_ONLY and Z_RLE, where it is 4 (xfl: gzip_xfl_of).
ZWZ_HD uint32_t dstream_header_byte(uint32_t wrap, uint32_t i, uint32_t flg = 0x9cu, uint32_t xfl = 0u) {
    if (wrap == kWrapZlib) return i == 0 ? 0x78u : flg;
    return i == 0 ? 0x1fu : i == 1 ? 0x8bu : i == 2 ? 0x08u : i == 8 ? xfl : i == 9 ? 0x03u : 0u;
}
// Byte i of what follows the last marker: 03 00, then Adler-32 big-endian (zlib) or CRC-32 and ISIZE little-endian (gzip).
ZWZ_HD uint32_t dstream_tail_byte(uint32_t wrap, uint32_t i, uint32_t check, uint64_t total_in) {
    if (i < 2) return i == 0 ? 0x03u : 0u;
    i -= 2;
    if (wrap == kWrapZlib) return (check >> (24u - 8u * i)) & 255u;
    return i < 4 ? (check >> (8u * i)) & 255u : ((uint32_t)total_in >> (8u * (i - 4u))) & 255u;
}
ZWZ_HD uint32_t dstream_check_init(uint32_t wrap) { return wrap == kWrapZlib ? 1u : 0u; }     // adler32("") / crc32("")

// Where a piece's zlib stream is spliced, in bits from the start of its slot (the 16 bits of 78 9c included): the header of its last
// block (whose first bit is BFINAL), and the end of that block before the final padding.  Walks the blocks as the encoder lays them
// out (encode_kernel's thread 0): headers bit-contiguous, a stored block's LEN at the next byte boundary.
struct SplicePoints { uint32_t hdr_bit, end_bit; };
template <class BlockFn>    // block(b, type, hdr_bits, body_bits, stored_bytes)
ZWZ_HD SplicePoints splice_points(uint32_t n_blocks, BlockFn&& block) {
    uint64_t bit = 16;
    SplicePoints sp{16u, 16u};
    for (uint32_t b = 0; b < n_blocks; b++) {
        uint32_t type, hdr_bits, body_bits, stored_bytes;
        block(b, type, hdr_bits, body_bits, stored_bytes);
        sp.hdr_bit = (uint32_t)bit;
        bit += hdr_bits;
        if (type == kStored) bit = ((bit + 7) & ~7ull) + 32u + 8ull * stored_bytes;
        else bit += body_bits;
    }
    sp.end_bit = (uint32_t)bit;
    return sp;
}
// Bytes a piece contributes: its raw stream through the marker's padding, then 00 00 ff ff.  The source bytes are slot[2, 2 + n - 4)
// with the BFINAL bit cleared; where the marker's three bits open a new byte that byte is zero.
ZWZ_HD uint32_t spliced_bytes(uint32_t end_bit) { return (end_bit - 16u + 3u + 7u) / 8u + 4u; }
ZWZ_HD uint32_t spliced_source_bytes(uint32_t end_bit) { return (end_bit - 16u + 7u) / 8u; }

// Worst case of spliced_bytes for a piece of L <= kPieceBytes input bytes.  A piece has at most L / kSymsPerBlock + 1 blocks (one per
// kSymsPerBlock symbols, and a symbol covers at least a byte).  libz stores a block of n bytes unless the coded form is shorter than
// n + 4 bytes, header bits included, so a block takes at most 3 + 7 + 32 + 8n = 8n + 42 bits (stored, behind up to 7 bits of
// padding).  The exception is a block that may not be stored because the window has slid: it is flushed at or after kSlidePos
// and starts before kWSize, so only a piece of at least kSlidePos bytes has one, it has only one, and that block holds
// n > kSlidePos - kWSize = 32 506 bytes in S <= kSymsPerBlock symbols.  libz takes the static code when that is shorter, so the
// block costs at most its static length: 3 header bits, 7 for the end-of-block code, at most 9 for a literal -- one more than its
// byte -- and for a match of length l at most 22 bits for l = 3 (farther than kTooFar it is not taken), 25 for l <= 10 and 31
// above: always at least l - 1 bits less than its 8 l.  With m matches the literals add at most S - m bits and the matches save at
// least n - S, so the block takes at most 8n + 10 + 2 * 16 383 - 32 507 = 8n + 269 bits: 227 more than the 8n + 42 counted already.
ZWZ_HD uint32_t piece_bound(uint32_t L) {
    const uint32_t nb = L / kSymsPerBlock + 1u;
    const uint32_t bits = 42u * nb + (L >= kSlidePos ? 227u : 0u);
    return L + (bits + 3u + 7u) / 8u + 4u;
}
// header + pieces * (worst piece + marker) + 03 00 + trailer; an empty input has no piece.  1.0009 n for large n.
ZWZ_HD uint64_t dstream_bound(uint64_t n, uint32_t wrap) {
    const uint64_t full = n / kPieceBytes;
    const uint32_t rest = (uint32_t)(n % kPieceBytes);
    return dstream_header_bytes(wrap) + full * piece_bound(kPieceBytes) + (rest ? piece_bound(rest) : 0u) + 2u + dstream_trailer_bytes(wrap);
}

// ---- dependent pieces (zwz_deflate_dep_streams_dev) ------------------------------------------------------------
// pigz's default: pieces of kDepPieceBytes, each compressed with the kDepDictBytes of input in front of it as a preset dictionary
// (deflateSetDictionary on a raw stream, no FDICT) and closed with Z_SYNC_FLUSH, which writes the bytes of a full flush; 03 00 behind the
// last.  A piece and its dictionary are ONE chunk of the codec, [dictionary | piece], at most kDepDictBytes + kDepPieceBytes = kPieceBytes
// bytes: libz puts the dictionary at window position 0, so window and chunk positions coincide, it inserts every dictionary position
// into the chains, and it reads the whole piece in one fill_window (room 65 536 - 32 512 >= 32 768) -- the chains, the distance rules
// and the one slide at strstart >= kSlidePos are those of the whole chunk.  What differs is where the walk starts: at position
// `skip` = the dictionary's length, fresh (prev_length 2, no match pending), and symbols, blocks and the checksum count from there.
// kDepDictBytes >= kMaxDist, so no match libz could reach with a 32 768-byte dictionary is lost; it is a multiple of 64 (lz_parse's
// blocks), of 128 (lz_lazy's segments) and of 256 (a wave's trip of lz_match's screening pass).
constexpr uint32_t kDepPieceBytes = 32768, kDepDictBytes = 32512;
static_assert(kDepDictBytes + kDepPieceBytes == kPieceBytes && kDepDictBytes >= kMaxDist && kDepDictBytes % 256u == 0, "a dependent piece and its dictionary are one chunk");

// The dictionary of piece k of a stream whose first piece has `lead` dictionary bytes in front of it (0 but in the file call's later slices)
ZWZ_HD uint32_t dep_skip(uint64_t k, uint32_t lead) { return k ? kDepDictBytes : lead; }

// A piece form: the input bytes of a piece and of the dictionary in front of it.  The kernels around the codec (zwz_dstream.hip) and
// their host driver take one of these two and are otherwise the same code for both.
struct PieceForm {
    uint32_t piece, dict;
    ZWZ_HD uint32_t skip(uint64_t k, uint32_t lead) const { return k ? dict : lead; }      // dep_skip; 0 for independent pieces, whose lead is 0
};
constexpr PieceForm kPiecesAlone{kPieceBytes, 0u}, kPiecesDep{kDepPieceBytes, kDepDictBytes};

// Worst case of spliced_bytes for a dependent piece of L <= kDepPieceBytes input bytes behind `skip` dictionary bytes: piece_bound's
// count, in chunk coordinates.  At most L / kSymsPerBlock + 1 blocks of at most 8n + 42 bits.  The block that may not be stored starts
// before kWSize -- behind a dictionary that is the piece's FIRST block, at skip = 32 512, and no other: the next one starts 16 383
// symbols on -- and is flushed at or after kSlidePos, so the piece has skip + L >= kSlidePos: every full piece behind a dictionary
// whose first block reaches 65 274, and on compressible data a full piece is one block.  Such a block holds n >= kSlidePos - skip
// = 32 762 bytes, so piece_bound's count gives 8n + 10 + 2 * 16 383 - 32 762 = 8n + 14 bits for it; the 227 bits piece_bound adds for
// its own case (n > 32 506) are carried here all the same, for every such piece: one rule for both writers, 28 bytes a piece.
ZWZ_HD uint32_t dep_piece_bound(uint32_t L, uint32_t skip) {
    const uint32_t nb = L / kSymsPerBlock + 1u;
    const uint32_t bits = 42u * nb + (skip + L >= kSlidePos ? 227u : 0u);
    return L + (bits + 3u + 7u) / 8u + 4u;
}
// header + the first piece (no dictionary) + the full pieces behind it + the last + 03 00 + trailer; an empty input has no piece
ZWZ_HD uint64_t dep_stream_bound(uint64_t n, uint32_t wrap) {
    uint64_t b = dstream_header_bytes(wrap) + 2u + dstream_trailer_bytes(wrap);
    if (!n) return b;
    const uint64_t pieces = (n + kDepPieceBytes - 1u) / kDepPieceBytes;
    const uint32_t last = (uint32_t)(n - (pieces - 1u) * kDepPieceBytes);
    if (pieces == 1u) return b + dep_piece_bound(last, 0u);
    return b + dep_piece_bound(kDepPieceBytes, 0u) + (pieces - 2u) * dep_piece_bound(kDepPieceBytes, kDepDictBytes) + dep_piece_bound(last, kDepDictBytes);
}

// ---- checksums of a concatenation -----------------------------------------------------------------------------------------------
// Both checksums are monoids under "append": join(l, r, p) is the checksum of A || B from those of A and B and a parameter p that
// depends on |B| alone; pof(n) is that parameter for n bytes and pjoin(p, q) the parameter of the two lengths added.  The identity
// (the checksum of nothing) on the left leaves r unchanged whatever p is, which is what lets a wave pad a short row of pieces
// at the front.
struct AdlerSum {       // Adler-32 as B << 16 | A; p = |B| mod 65521
    static ZWZ_HD uint32_t identity() { return 1u; }
    static ZWZ_HD uint32_t pof(uint64_t n) { return (uint32_t)(n % kAdlerMod); }
    static ZWZ_HD uint32_t pjoin(uint32_t p, uint32_t q) { return (p + q) % kAdlerMod; }
    static ZWZ_HD uint32_t join(uint32_t l, uint32_t r, uint32_t p) {
        const uint32_t a1 = l & 0xffffu, b1 = l >> 16, a2 = r & 0xffffu, b2 = r >> 16;
        const uint32_t a = (a1 + a2 + kAdlerMod - 1u) % kAdlerMod;                               // A1 + A2 - 1
        const uint32_t b = (b1 + b2 + (p * ((a1 + kAdlerMod - 1u) % kAdlerMod)) % kAdlerMod) % kAdlerMod;   // B1 + B2 + |B| (A1 - 1); p * (..) < 2^32
        return b << 16 | a;
    }
};
struct CrcSum {         // CRC-32; p = x^(8 |B|) mod P (crc_core.h: zlib's crc32_combine)
    static ZWZ_HD uint32_t identity() { return 0u; }
    static ZWZ_HD uint32_t pof(uint64_t n) { return crc_xpow8n(n); }
    static ZWZ_HD uint32_t pjoin(uint32_t p, uint32_t q) { return crc_mulmod(p, q); }
    static ZWZ_HD uint32_t join(uint32_t l, uint32_t r, uint32_t p) { return crc_mulmod(l, p) ^ r; }
};
// The parameter of k blocks of the length p stands for, by doubling
template <class Sum>
ZWZ_HD uint32_t sum_ptimes(uint32_t p, uint32_t k) {
    uint32_t r = Sum::pof(0);
    while (k) {
        if (k & 1u) r = Sum::pjoin(r, p);
        p = Sum::pjoin(p, p);
        k >>= 1;
    }
    return r;
}
// A row of kSumRow checksums of equal-length blocks (parameter p1 each), identities in front of a short row, folded as a wave folds
// it: at distance d = 1, 2, 4, ... every 2d-th entry takes in its neighbour d further on, whose d blocks have the parameter p1 d times.
constexpr uint32_t kSumRow = 64;
template <class Sum>
inline uint32_t sum_fold_row_host(uint32_t* v, uint32_t p1) {
    uint32_t pd = p1;
    for (uint32_t d = 1; d < kSumRow; d <<= 1) {
        for (uint32_t l = 0; l < kSumRow; l += 2 * d) v[l] = Sum::join(v[l], v[l + d], pd);
        pd = Sum::pjoin(pd, pd);
    }
    return v[0];
}
// dstream_combine_kernel on the host: the checksums val[0, cnt) of one stream's pieces in one slice joined onto acc.  Of all but the last,
// `piece` bytes each, K in a row per lane, the short share in front; the lanes folded; then the last piece by its own length.
template <class Sum>
inline uint32_t sum_join_slice_host(uint32_t acc, const uint32_t* val, const uint32_t* len, uint64_t cnt, uint32_t piece) {
    const uint32_t full = (uint32_t)cnt - 1u, p1 = Sum::pof(piece);
    if (full) {
        const uint32_t K = (full + kSumRow - 1u) / kSumRow, pad = K * kSumRow - full;
        uint32_t row[kSumRow];
        for (uint32_t l = 0; l < kSumRow; l++) {
            row[l] = Sum::identity();
            for (uint32_t j = 0; j < K; j++) { const uint32_t v = l * K + j; if (v >= pad) row[l] = Sum::join(row[l], val[v - pad], p1); }
        }
        acc = Sum::join(acc, sum_fold_row_host<Sum>(row, sum_ptimes<Sum>(p1, K)), sum_ptimes<Sum>(p1, full));
    }
    return Sum::join(acc, val[cnt - 1], Sum::pof(len[cnt - 1]));
}

}  // namespace zwz
