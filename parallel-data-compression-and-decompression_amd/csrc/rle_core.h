// rle_core.h -- libz's two search-free encoders, deflate_huff (Z_HUFFMAN_ONLY) and deflate_rle (Z_RLE), as a function of the position.
//
// deflate_huff tallies a literal per byte.  deflate_rle, at a fresh position p > 0 with at least three bytes left, emits a match at
// distance 1 if b[p-1] == b[p] == b[p+1] == b[p+2] -- as long as the run of that byte goes on from p, at most 258 and at most the
// bytes left -- and a literal otherwise.  A greedy parse, but one with a closed form per maximal run of R equal bytes starting at s:
//   a literal at s; floor((R - 1) / 258) matches of 258; then, with t = (R - 1) mod 258, one match of t if t >= 3, else t literals.
// So what becomes of position p follows from p and the two ends of its run alone (rle_fate), and the ends follow from the chunk's
// "equals its predecessor" bits E (bit p = b[p] == b[p-1], bit 0 clear, bits from the length on clear): the run of p starts at the
// last clear bit at or below p and ends at the first clear bit above it (rle_run_of).  Beyond p's own 64-bit word those two are a
// running maximum and a running minimum over the words (rle_word_last_clear / rle_word_first_clear), which is how runs of any length
// -- a whole chunk of one byte -- need no walk.
//
// Blocks: both encoders flush after every 16 383rd symbol, literal or match, and once more at the end -- an empty block included
// (strategy_blocks).  Neither defers a literal, so this is NOT lz_parse's rule.  Whether a block's bytes can still be stored depends
// on when fill_window may slide the window (strategy_flush_pos).
//
// Portable (host + device): tests/emu_strategy builds this header on the CPU and pins it token for token against libz.
#pragma once
#include "zwz_common.h"

namespace zwz {

// libz's strategy numbers.  Z_FILTERED (1) and Z_FIXED (4) have no kernels here.
constexpr uint32_t kStrategyDefault = 0, kStrategyHuffman = 2, kStrategyRle = 3;
ZWZ_HD constexpr bool strategy_exists(int s) { return s == (int)kStrategyDefault || s == (int)kStrategyHuffman || s == (int)kStrategyRle; }
constexpr uint32_t kRleNone = 0xffffffffu;

// The header bytes libz writes under a strategy: deflate() sets the zlib header's FLEVEL to 0 for strategy >= Z_HUFFMAN_ONLY, whatever
// the level (78 01), and gzip's XFL to 4.
ZWZ_HD constexpr uint32_t zlib_flg_of(uint32_t level, uint32_t strategy) { return strategy >= kStrategyHuffman ? 0x01u : zlib_flg(level); }
ZWZ_HD constexpr uint32_t gzip_xfl_of(uint32_t strategy) { return strategy >= kStrategyHuffman ? 4u : 0u; }

// Four E bits: byte j of `cur` against byte j of `shifted` (cur moved up a byte with its predecessor in front).
ZWZ_HD uint32_t rle_eq4(uint32_t cur, uint32_t shifted) {
    const uint32_t t = cur ^ shifted;
    const uint32_t nz = (((t & 0x7f7f7f7fu) + 0x7f7f7f7fu) | t) & 0x80808080u;      // the top bit of every byte that differs
    return (((~nz & 0x80808080u) >> 7) * 0x10204080u) >> 28;                      // bits 0, 8, 16, 24 -> bits 0..3 (no two products meet)
}
// The E bits of sixteen consecutive bytes (four little-endian words) behind the byte `prev`.
ZWZ_HD uint32_t rle_eq16(uint32_t x, uint32_t y, uint32_t z, uint32_t w, uint32_t prev) {
    return rle_eq4(x, (x << 8) | (prev & 255u)) | rle_eq4(y, (y << 8) | (x >> 24)) << 4 | rle_eq4(z, (z << 8) | (y >> 24)) << 8 |
           rle_eq4(w, (w << 8) | (z >> 24)) << 12;
}

// Per word of E: the last / first position whose bit is clear; 0 / kRleNone for a word of ones.  An inclusive running maximum of the
// first over the words gives back[w], the start of the run that the word's last position lies in (position 0 is always clear); a
// running minimum of the second from the far end gives fwd[w], the first clear bit at or behind the word's first position.
ZWZ_HD uint32_t rle_word_last_clear(uint64_t e, uint32_t w) { return ~e ? (w << 6) + 63u - (uint32_t)__builtin_clzll(~e) : 0u; }
ZWZ_HD uint32_t rle_word_first_clear(uint64_t e, uint32_t w) { return ~e ? (w << 6) + (uint32_t)__builtin_ctzll(~e) : kRleNone; }

// The run [s, e) of equal bytes that position p < L lies in.  word(w) = E's word w; back(w) / fwd(w) as above, asked for w - 1 and
// w + 1 only (fwd of the word behind the last one: any value >= L).
template <class WordFn, class BackFn, class FwdFn>
ZWZ_HD void rle_run_of(uint32_t p, uint32_t L, WordFn&& word, BackFn&& back, FwdFn&& fwd, uint32_t& s, uint32_t& e) {
    const uint32_t w = p >> 6, b = p & 63u;
    const uint64_t clear = ~word(w);
    const uint64_t lo = clear & (~0ull >> (63u - b));                 // clear bits at or below p
    s = lo ? (w << 6) + 63u - (uint32_t)__builtin_clzll(lo) : back(w - 1u);      // (word 0 has bit 0 clear: w > 0 here)
    const uint64_t hi = b == 63u ? 0ull : clear & (~0ull << (b + 1u));           // clear bits above p
    e = hi ? (w << 6) + (uint32_t)__builtin_ctzll(hi) : fwd(w + 1u);
    if (e > L) e = L;
}

// What deflate_rle makes of position p of the run [s, e): sym = a symbol starts here, mst = that symbol is a match (distance 1), of
// len bytes.  A position inside a match is neither.
struct RleFate { uint32_t sym, mst, len; };
ZWZ_HD RleFate rle_fate(uint32_t p, uint32_t s, uint32_t e) {
    RleFate f{1u, 0u, 0u};
    if (p == s) return f;                                            // the run's first byte: nothing in front of it equals it
    const uint32_t body = e - s - 1u, o = p - s - 1u;                // the bytes behind that literal, and p's place among them
    const uint32_t k = o / kMaxMatch, r = o - k * kMaxMatch, full = body / kMaxMatch, t = body - full * kMaxMatch;
    if (k < full) { f.sym = f.mst = (uint32_t)(r == 0u); f.len = kMaxMatch; }
    else if (t >= kMinMatch) { f.sym = f.mst = (uint32_t)(r == 0u); f.len = t; }
    return f;                                                        // (else one of the t < 3 literals at the run's end)
}
// True if none of the 64 positions of a word can lie in a run of four or more: no three consecutive E bits among the word's own, the
// two below it and the two above it.  Then every position is a literal.  prev / next: the neighbouring words (0 where there is none).
ZWZ_HD bool rle_word_quiet(uint64_t e, uint64_t prev, uint64_t next) {
    const uint64_t lo = (e << 2) | (prev >> 62), hi = (e >> 2) | (next << 62);
    return ((lo & (lo >> 1) & (lo >> 2)) | (hi & (hi >> 1) & (hi >> 2))) == 0ull;
}

// Blocks of a chunk of n_sym symbols: one per 16 383, and the finishing flush's, which may be empty.
ZWZ_HD uint32_t strategy_blocks(uint32_t n_sym) { return n_sym / kSymsPerBlock + 1u; }

// BlockInfo::flush_pos under a strategy: the position at which fill_window last ran before the block's flush, or 0 if it has not run
// since the start -- the plan's rule !(flush_pos >= kSlidePos && start < kWSize) then says whether the block may be stored.
// deflate_slow calls fill_window whenever the lookahead is below 262; these two do not:
//   deflate_huff  only with no lookahead at all, that is once every byte is tallied: before the LAST block's flush only;
//   deflate_rle   at a loop top -- a symbol's first position -- with at most 258 bytes left, and at the end.
// last_sym_start: the first position of the block's last symbol (not looked at for the last block).
ZWZ_HD uint32_t strategy_flush_pos(uint32_t strategy, bool last_block, uint32_t last_sym_start, uint32_t L) {
    if (last_block) return L;
    return strategy == kStrategyRle && L - last_sym_start <= kMaxMatch ? last_sym_start : 0u;
}

}  // namespace zwz
