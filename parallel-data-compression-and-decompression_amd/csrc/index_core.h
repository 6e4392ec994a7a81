// index_core.h -- the portable half of the seek index for ordinary DEFLATE streams (zwz_inflate_streams_index_dev, zwz_inflate_indexed_dev,
// zwz_inflate_read_ranges_dev).  Host + device: the parse, the plan and the rules below are one code for the host driver, the
// kernels and the CPU tests (tests/emu/index_emu.cpp, which restates the kernel's loops around them).
//
// An ordinary stream offers no cut: every block may refer 32 KiB back.  The stream is decoded ONCE by one wave, which notes CHECKPOINTS on
// its way: a block header's first bit, the decoded offset there, and -- copied out of the output afterwards -- the `hist` bytes in front of
// it.  From then on segment k, the blocks from checkpoint k to checkpoint k + 1, is decoded by a wave of its own that finds its window
// already in memory: inflate_kernel's positions are relative to an `origin`, which here lies hist bytes in front of the first output byte.
//
// The index of one stream, all little-endian: a 64-byte header, `count` entries of 24 bytes, the windows back to back in entry order,
// zero padding to a multiple of 16.
//   header   0  "ZWZIDX\0\1"       8  u32 wrap         12  u32 span      16  u64 stream length, wrapper included
//           24  u64 decoded length 32  u32 count        36  u32 flags, 0  40  u64 end bit: the first bit behind the final block
//           48  u32 stored CRC-32 / Adler-32 (raw: 0)   52  u32 CRC-32 of the index from byte 64 to its end           56  u64 0
//   entry    0  u64 bit offset of a block header's first bit, from the stream's first byte     8  u64 decoded offset
//           16  u32 hist: window bytes kept, <= min(32768, decoded offset); a promise that no match reaches further back   20  u32 0
// Entry 0 is the body's first block (decoded offset 0, hist 0); bit offsets rise strictly, decoded offsets do not fall.
#pragma once
#include "stream_core.h"

#include <algorithm>
#include <vector>

namespace zwz {

constexpr uint32_t kIdxHeader = 64, kIdxEntry = 24, kIdxWindow = 32768;
constexpr uint32_t kIdxSpanMin = 16384, kIdxSpanMax = 1u << 30, kIdxSpanDefault = 1u << 20;
constexpr uint32_t kStrIndex = 37;                  // include/zwz.h: ZWZ_STREAM_INDEX
// inflate_kernel's forms (its kSplit argument) beyond split_core.h's 1 and 2
constexpr uint32_t kFormMark = 3, kFormIndexed = 4;

ZWZ_HD uint64_t le64_of(const uint8_t* p) { return (uint64_t)le32_at(p) | (uint64_t)le32_at(p + 4) << 32; }
ZWZ_HD void put_le32(uint8_t* p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }
ZWZ_HD void put_le64(uint8_t* p, uint64_t v) { put_le32(p, (uint32_t)v); put_le32(p + 4, (uint32_t)(v >> 32)); }

// The host's tables for crc_raw_long: slice[k][b] = the register after byte b and k zero bytes (crc_core.h's T_k), built once
constexpr uint32_t kCrcHostSlices = 16;
struct CrcHostTables {
    uint32_t slice[kCrcHostSlices][256];
    CrcHostTables() {
        for (uint32_t b = 0; b < 256u; b++) slice[0][b] = crc_shift8(b);
        for (uint32_t k = 1; k < kCrcHostSlices; k++)
            for (uint32_t b = 0; b < 256u; b++) slice[k][b] = (slice[k - 1][b] >> 8) ^ slice[0][slice[k - 1][b] & 255u];
    }
};
inline const CrcHostTables& crc_host_tables() { static const CrcHostTables t; return t; }

// crc_raw_bytes over a length of 64 bits, 16 bytes a step: the register goes into the first four, every byte through the table of its
// distance from the step's end
inline uint32_t crc_raw_sliced(uint32_t c, const uint8_t* p, uint64_t n) {
    const CrcHostTables& t = crc_host_tables();
    for (; n >= kCrcHostSlices; p += kCrcHostSlices, n -= kCrcHostSlices) {
        const uint32_t w[4] = {le32_at(p) ^ c, le32_at(p + 4), le32_at(p + 8), le32_at(p + 12)};
        c = 0;
        for (uint32_t j = 0; j < 4u; j++)
            c ^= t.slice[15u - 4u * j][w[j] & 255u] ^ t.slice[14u - 4u * j][(w[j] >> 8) & 255u] ^ t.slice[13u - 4u * j][(w[j] >> 16) & 255u] ^ t.slice[12u - 4u * j][w[j] >> 24];
    }
    for (; n; p++, n--) c = t.slice[0][(c ^ *p) & 255u] ^ (c >> 8);
    return c;
}

// crc_raw_bytes over a length of 64 bits (the host through its tables; a kernel, which has crc_wg.h for anything long, bit by bit)
ZWZ_HD uint32_t crc_raw_long(uint32_t c, const uint8_t* p, uint64_t n) {
#if defined(__HIP_DEVICE_COMPILE__)
    for (uint64_t at = 0; at < n; at += 1u << 30) c = crc_raw_bytes(c, p + at, (uint32_t)(n - at < (1u << 30) ? n - at : 1u << 30));
    return c;
#else
    return crc_raw_sliced(c, p, n);
#endif
}

ZWZ_HD bool index_span_ok(uint32_t span) { return span >= kIdxSpanMin && span <= kIdxSpanMax && !(span & (span - 1u)); }
ZWZ_HD uint32_t index_hist_bound(uint64_t off) { return off < kIdxWindow ? (uint32_t)off : kIdxWindow; }

// The most an index of a stream that decodes to at most `decoded_cap` bytes takes at this span: checkpoints lie at least `span` apart
ZWZ_HD uint64_t index_bound(uint64_t decoded_cap, uint32_t span) {
    const uint64_t count = decoded_cap / span + 2u;
    return (kIdxHeader + count * (kIdxEntry + (uint64_t)kIdxWindow) + 15u) & ~15ull;
}

struct IndexEntry { uint64_t bit, off; uint32_t hist; };
// A parsed index: pointers into the caller's bytes
struct IndexView {
    uint32_t wrap, span, count, check;
    uint64_t stream_len, decoded_len, end_bit, win_off;      // win_off: where the windows start in the index
    const uint8_t* base;
    ZWZ_HD IndexEntry entry(uint32_t k) const {
        const uint8_t* e = base + kIdxHeader + (size_t)k * kIdxEntry;
        return IndexEntry{le64_of(e), le64_of(e + 8), le32_at(e + 16)};
    }
    // segment k: from entry k to entry k + 1, or to the end
    ZWZ_HD uint64_t seg_end_bit(uint32_t k) const { return k + 1u < count ? entry(k + 1u).bit : end_bit; }
    ZWZ_HD uint64_t seg_end_off(uint32_t k) const { return k + 1u < count ? entry(k + 1u).off : decoded_len; }
};

enum IndexFault : uint32_t { kIdxOk = 0, kIdxMagic, kIdxLength, kIdxCrc, kIdxWindowSum, kIdxOrder, kIdxHist, kIdxEndBit, kIdxField };
ZWZ_HD const char* index_fault_name(uint32_t f) {
    switch (f) {
        case kIdxMagic: return "wrong magic"; case kIdxLength: return "wrong length"; case kIdxCrc: return "wrong index CRC";
        case kIdxWindowSum: return "the windows do not add up to the index's length"; case kIdxOrder: return "entries out of order";
        case kIdxHist: return "hist over its bound"; case kIdxEndBit: return "end bit beyond the stream"; case kIdxField: return "a header field out of range";
        default: return "fine";
    }
}

// Everything the layout promises, checked: the first fault found, kIdxOk with *v filled otherwise.
ZWZ_HD uint32_t index_parse(const uint8_t* p, uint64_t n, IndexView* v) {
    const uint8_t magic[8] = {'Z', 'W', 'Z', 'I', 'D', 'X', 0, 1};
    if (n < kIdxHeader) return kIdxLength;
    for (uint32_t i = 0; i < 8; i++) if (p[i] != magic[i]) return kIdxMagic;
    v->base = p;
    v->wrap = le32_at(p + 8); v->span = le32_at(p + 12); v->stream_len = le64_of(p + 16); v->decoded_len = le64_of(p + 24);
    v->count = le32_at(p + 32); v->end_bit = le64_of(p + 40); v->check = le32_at(p + 48);
    if (v->wrap > kWrapGzip || !index_span_ok(v->span) || le32_at(p + 36) != 0u || le64_of(p + 56) != 0u || v->count == 0u) return kIdxField;
    if (v->decoded_len / 1032u > v->stream_len) return kIdxField;        // (DEFLATE gives at most 1032 bytes for one: 258 from a match of 2 bits)
    if ((n & 15u) || n < kIdxHeader + (uint64_t)v->count * kIdxEntry) return kIdxLength;
    if (crc_raw_long(0xffffffffu, p + kIdxHeader, n - kIdxHeader) != (le32_at(p + 52) ^ 0xffffffffu)) return kIdxCrc;
    v->win_off = kIdxHeader + (uint64_t)v->count * kIdxEntry;
    uint64_t sum = 0;
    IndexEntry prev{0, 0, 0};
    for (uint32_t k = 0; k < v->count; k++) {
        const IndexEntry e = v->entry(k);
        if (le32_at(p + kIdxHeader + (size_t)k * kIdxEntry + 20) != 0u) return kIdxField;
        if (k == 0 ? (e.off != 0u) : (e.bit <= prev.bit || e.off < prev.off)) return kIdxOrder;
        if (e.off > v->decoded_len) return kIdxOrder;
        if (e.hist > index_hist_bound(e.off)) return kIdxHist;
        sum += e.hist;
        prev = e;
    }
    if (v->end_bit <= prev.bit || v->end_bit > v->stream_len * 8u) return kIdxEndBit;
    if (((v->win_off + sum + 15u) & ~15ull) != n) return kIdxWindowSum;
    return kIdxOk;
}

// the last entry k with entry(k).off <= x, among those a byte at x can belong to: the LAST entry with that offset owns the bytes behind it
ZWZ_HD uint32_t index_segment_of(const IndexView& v, uint64_t x) {
    uint32_t lo = 0, hi = v.count;
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (v.entry(mid).off <= x) lo = mid; else hi = mid;
    }
    return lo;
}

// Planning and sealing are the host's (plain inline functions)
// One piece of a range inside one touched segment: `len` bytes at `off` of the segment's decoded bytes go to `dst` of the result
struct IndexPiece { uint64_t dst; uint32_t off, len; };
// The plan of a batch of ranges, as section 14's: the touched segments ascending, and per touched segment its pieces as compressed
// sparse rows (row[i] .. row[i + 1]), in range order.
struct IndexPlan { std::vector<uint32_t> segs, row; std::vector<IndexPiece> pieces; uint64_t total = 0; };

// -1: fine; otherwise the first range that lies past the decoded length or whose end overflows
inline int64_t index_plan(const IndexView& v, const uint64_t* ranges, uint32_t k, IndexPlan* plan) {
    plan->segs.clear(); plan->row.clear(); plan->pieces.clear(); plan->total = 0;
    struct Raw { uint32_t seg; IndexPiece p; };
    std::vector<Raw> raw;
    std::vector<uint32_t> cnt(v.count + 1u, 0);
    uint64_t dst = 0;
    for (uint32_t r = 0; r < k; r++) {
        const uint64_t a = ranges[2 * r], len = ranges[2 * r + 1];
        if (a + len < a || a + len > v.decoded_len) return r;
        uint64_t at = a, left = len;
        while (left) {
            const uint32_t s = index_segment_of(v, at);
            const uint64_t s0 = v.entry(s).off, s1 = v.seg_end_off(s);
            const uint64_t take = left < s1 - at ? left : s1 - at;
            raw.push_back(Raw{s, IndexPiece{dst, (uint32_t)(at - s0), (uint32_t)take}});
            cnt[s]++;
            at += take; dst += take; left -= take;
        }
    }
    plan->total = dst;
    std::vector<uint32_t> slot(v.count, 0);
    plan->row.push_back(0);
    for (uint32_t s = 0; s < v.count; s++) if (cnt[s]) { slot[s] = (uint32_t)plan->segs.size(); plan->segs.push_back(s); plan->row.push_back(plan->row.back() + cnt[s]); }
    plan->pieces.resize(raw.size());
    std::vector<uint32_t> fill(plan->row.begin(), plan->row.end());
    for (const Raw& q : raw) plan->pieces[fill[slot[q.seg]]++] = q.p;
    return -1;
}

// The batch (zwz_inflate_read_ranges_batch_dev): ranges are triples (stream number, decoded offset, length); the touched segments of all
// streams in one list, ascending by (stream, segment), with their pieces as compressed sparse rows in range order, as IndexPlan's.
struct IndexBatchPlan { std::vector<uint32_t> stream, segs, row; std::vector<IndexPiece> pieces; uint64_t total = 0; };

// Which streams the triples name: named[s] = 1.  -1: fine; otherwise the first range whose stream number is not below n
inline int64_t index_batch_named(const uint64_t* triples, uint32_t k, uint32_t n, std::vector<uint8_t>* named) {
    named->assign(n, 0);
    for (uint32_t r = 0; r < k; r++) {
        if (triples[3 * r] >= n) return r;
        (*named)[(size_t)triples[3 * r]] = 1;
    }
    return -1;
}

// -1: fine; otherwise the first range that lies past its stream's decoded length or whose end overflows.  Only the views of named
// streams are read (every stream number is below n: index_batch_named).
inline int64_t index_plan_batch(const IndexView* views, const uint64_t* triples, uint32_t k, IndexBatchPlan* plan) {
    plan->stream.clear(); plan->segs.clear(); plan->row.clear(); plan->pieces.clear(); plan->total = 0;
    struct Raw { uint64_t key; IndexPiece p; };                          // key: stream << 32 | segment
    std::vector<Raw> raw;
    uint64_t dst = 0;
    for (uint32_t r = 0; r < k; r++) {
        const uint64_t s = triples[3 * r], a = triples[3 * r + 1], len = triples[3 * r + 2];
        const IndexView& v = views[s];
        if (a + len < a || a + len > v.decoded_len) return r;
        uint64_t at = a, left = len;
        while (left) {
            const uint32_t g = index_segment_of(v, at);
            const uint64_t s0 = v.entry(g).off, s1 = v.seg_end_off(g);
            const uint64_t take = left < s1 - at ? left : s1 - at;
            raw.push_back(Raw{s << 32 | g, IndexPiece{dst, (uint32_t)(at - s0), (uint32_t)take}});
            at += take; dst += take; left -= take;
        }
    }
    plan->total = dst;
    // the rows: a stable sort by key keeps a row's pieces in range order
    std::vector<uint32_t> by(raw.size());
    for (uint32_t i = 0; i < by.size(); i++) by[i] = i;
    std::stable_sort(by.begin(), by.end(), [&](uint32_t x, uint32_t y) { return raw[x].key < raw[y].key; });
    plan->pieces.reserve(raw.size());
    for (size_t i = 0; i < by.size(); i++) {
        const Raw& q = raw[by[i]];
        if (i == 0 || q.key != raw[by[i - 1]].key) { plan->stream.push_back((uint32_t)(q.key >> 32)); plan->segs.push_back((uint32_t)q.key); plan->row.push_back((uint32_t)i); }
        plan->pieces.push_back(q.p);
    }
    plan->row.push_back((uint32_t)raw.size());
    return -1;
}

// The checksum pieces of a whole-stream decode whose first byte stands at an address with the low four bits `low4`: piece 0 is the
// `head` bytes up to the next 16-byte boundary (it may be empty), the others kIdxPieceBytes each, the last one what is left.
constexpr uint32_t kIdxPieceBytes = 65280;          // dstream_core.h's kPieceBytes
ZWZ_HD uint32_t index_head_bytes(uint32_t low4, uint64_t total) { const uint32_t h = (16u - low4) & 15u; return total < h ? (uint32_t)total : h; }
ZWZ_HD uint64_t index_piece_count(uint32_t wrap, uint32_t head, uint64_t total) { return wrap == kWrapRaw ? 0u : 1u + (total - head + kIdxPieceBytes - 1u) / kIdxPieceBytes; }
ZWZ_HD uint64_t index_piece_start(uint32_t head, uint64_t j) { return j ? head + (j - 1u) * kIdxPieceBytes : 0u; }
ZWZ_HD uint32_t index_piece_bytes(uint32_t head, uint64_t total, uint64_t j) {
    if (j == 0) return head;
    const uint64_t left = total - index_piece_start(head, j);
    return left < kIdxPieceBytes ? (uint32_t)left : kIdxPieceBytes;
}

// The header's fields (check: the stream's stored check value, 0 for raw; crc: the index CRC) and its sixteen little-endian words: the
// one place the header is spelled out, for every writer on the host and on the device
constexpr uint32_t kIdxMagicLo = 0x495a575au, kIdxMagicHi = 0x01005844u;      // "ZWZIDX\0\1"
struct IndexHeader { uint32_t wrap, span; uint64_t stream_len, decoded_len; uint32_t count; uint64_t end_bit; uint32_t check, crc; };
ZWZ_HD void index_header_words(uint32_t* h, const IndexHeader& f) {
    h[0] = kIdxMagicLo; h[1] = kIdxMagicHi; h[2] = f.wrap; h[3] = f.span;
    h[4] = (uint32_t)f.stream_len; h[5] = (uint32_t)(f.stream_len >> 32); h[6] = (uint32_t)f.decoded_len; h[7] = (uint32_t)(f.decoded_len >> 32);
    h[8] = f.count; h[9] = 0; h[10] = (uint32_t)f.end_bit; h[11] = (uint32_t)(f.end_bit >> 32);
    h[12] = f.check; h[13] = f.crc; h[14] = 0; h[15] = 0;
}
// The host's store of it, at any alignment
inline void index_put_header(uint8_t* p, const IndexHeader& f) {
    uint32_t h[kIdxHeader / 4];
    index_header_words(h, f);
    for (uint32_t i = 0; i < kIdxHeader / 4; i++) put_le32(p + 4u * i, h[i]);
}

// Header and index CRC of an index whose entries and windows are in place (n: its padded length)
inline void index_seal(uint8_t* p, uint64_t n, uint32_t wrap, uint32_t span, uint64_t stream_len, uint64_t decoded_len, uint32_t count, uint64_t end_bit,
                       uint32_t check) {
    index_put_header(p, IndexHeader{wrap, span, stream_len, decoded_len, count, end_bit, check, crc_raw_long(0xffffffffu, p + kIdxHeader, n - kIdxHeader) ^ 0xffffffffu});
}

// The marking form's rule at a block header (lane 0): a checkpoint when the output has moved at least `span` since the last one; the
// body's first block always.
ZWZ_HD bool index_mark_due(uint32_t marks, uint32_t out_pos, uint32_t last_mark, uint32_t span) { return marks == 0u || out_pos - last_mark >= span; }

// ---- The index at full-flush points ---------------------------------------------------------------------------
// Behind a full flush nothing refers back, so a block that starts there is a checkpoint with hist 0 and no window.  The POINTS of a
// stream are the body's first block (point 0, decoded offset 0) and, in stream order, every block that starts behind a flush marker,
// at decoded offset o_k.  Entry 0 is point 0; point k >= 1 is an entry when it is the first point in its span-sized bucket of the
// output and bytes follow it.  The comparison is with the previous POINT, not the previous entry: a flag per point, no chain.
ZWZ_HD bool index_flush_due(uint64_t prev_off, uint64_t off, uint64_t decoded_len, uint32_t span) { return off < decoded_len && off / span > prev_off / span; }
// At most one entry a bucket: the exact worst case of a stream of n decoded bytes
ZWZ_HD uint64_t index_flush_bound(uint64_t n, uint32_t span) { return (kIdxHeader + (n / span + 1u) * kIdxEntry + 15u) & ~15ull; }
ZWZ_HD uint64_t index_flush_bytes(uint64_t count) { return (kIdxHeader + count * kIdxEntry + 15u) & ~15ull; }
ZWZ_HD void index_flush_entry(uint8_t* e, uint64_t bit, uint64_t off) { put_le64(e, bit); put_le64(e + 8, off); put_le64(e + 16, 0); }
// Where the writer's own final block, the 03 00 behind the last marker, ends: ten bits into its two bytes
ZWZ_HD uint64_t index_flush_end_bit(uint64_t final_byte) { return 8u * final_byte + 10u; }
// The host's sealing of such an index: `count` entries are in place behind the header of a buffer of index_flush_bytes(count)
inline void index_flush_seal(uint8_t* p, uint32_t wrap, uint32_t span, uint64_t stream_len, uint64_t decoded_len, uint32_t count, uint64_t end_bit, uint32_t check) {
    const uint64_t n = index_flush_bytes(count);
    for (uint64_t z = kIdxHeader + (uint64_t)count * kIdxEntry; z < n; z++) p[z] = 0;
    index_seal(p, n, wrap, span, stream_len, decoded_len, count, end_bit, check);
}

// ---- The index of a stream of dependent pieces (dstream_core.h) ---------------------------------------------
// The points are the piece starts, bit 8 * byte and decoded offset kIdxDepPiece * k, chosen by index_flush_due; entry 0 has hist 0,
// every later entry hist = kIdxDepDict, and its window is the input in front of it, which the writer holds: nothing is decoded.  The
// offsets are multiples of 32 768 and a span is a power of two from 16 384 up, so the entries are every `step`-th piece and their
// number is known before a byte is written -- and with it where the windows start.
constexpr uint32_t kIdxDepPiece = 32768, kIdxDepDict = 32512;     // dstream_core.h's kDepPieceBytes, kDepDictBytes
ZWZ_HD uint64_t index_dep_step(uint32_t span) { return span > kIdxDepPiece ? span / kIdxDepPiece : 1u; }       // pieces from entry to entry
ZWZ_HD uint64_t index_dep_count(uint64_t n, uint32_t span) {
    const uint64_t reach = index_dep_step(span) * kIdxDepPiece;
    return n ? (n + reach - 1u) / reach : 1u;
}
// count entries, the first without a window: the exact length, padded
ZWZ_HD uint64_t index_dep_bytes(uint64_t count) { return (kIdxHeader + count * kIdxEntry + (count - 1u) * kIdxDepDict + 15u) & ~15ull; }
ZWZ_HD uint64_t index_dep_bound(uint64_t n, uint32_t span) { return index_dep_bytes(index_dep_count(n, span)); }

// The indexed-segment form's verdict: it must stand at the block header whose first bit is the segment's end bit (or behind the final
// block, for the last segment), with exactly the indexed count and the decoder still running.
ZWZ_HD bool index_segment_good(uint32_t status, uint32_t bit_pos, uint32_t end_bit, uint32_t out_pos, uint32_t cap, uint32_t last, uint32_t is_last) {
    return status == kInfRunning && bit_pos == end_bit && out_pos == cap && (last != 0u) == (is_last != 0u);
}

}  // namespace zwz
