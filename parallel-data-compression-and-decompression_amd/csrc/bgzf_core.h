// bgzf_core.h -- the portable half of the BGZF member walk (zwz_bgzf_walk.hip): the header parse and the steps of the parallel walk.
// Host + device, so that a CPU build (tests/emu/bgzf_walk_emu.cpp) runs the device's decomposition step by step.
//
// A BGZF stream is a chain: a member at offset o says in its BSIZE field where the next one starts.  The walk finds the chain of a
// SPAN (head, stop, limit) of the buffer without hopping along it:
//   scan      a CANDIDATE is every offset p in [head, stop) with bytes 1f 8b 08 and a FLG that has bit 2 and nothing outside bits 0
//             and 2.  False ones are expected: deflate bits, or a BGZF file stored inside a member.  Only the chain decides.
//   parse     bgzf_member_parse at every candidate: the host walk's checks in the host walk's order.  A good member links to the
//             candidate at p + BSIZE, if that lies in front of the span's stop and is one.
//   jump      pointer jumping over the links; the span's head marks the nodes of its chain.
//   resolve   the chain's last node is a failure, or ends at an offset that is the stop (fine; with `limit` the member AT the stop is
//             parsed too, directly), lies behind it (the chain steps over the stop) or is no candidate (parsed directly: it yields the
//             host walk's own failure).  The marked good members, ranked by a prefix sum, are the span's member list.
// Offsets are 64-bit; candidate indices and member counts 32-bit.
#pragma once
#include "stream_core.h"

namespace zwz {

// One code per failure message of the host walk (zwz_bgzf.cpp: bgzf_walk_each), in its order; kBgzfStepOver is the walk's own.
enum BgzfKind : uint32_t {
    kBgzfOk = 0,
    kBgzfMagic,             // "not gzip (bad magic or method)" for member 0, else "trailing bytes that are not a gzip member"
    kBgzfShortHeader,       // "truncated member header"
    kBgzfNoExtra,           // "no extra field: a plain gzip member, not BGZF"
    kBgzfFlags,             // "unsupported gzip header flags" FLG
    kBgzfExtraPast,         // "extra field runs past the end of the input"
    kBgzfExtraMalformed,    // "malformed extra field"
    kBgzfNoBc,              // "no BC subfield: not BGZF"
    kBgzfBsizeSmall,        // "BSIZE smaller than its header and trailer:" BSIZE
    kBgzfBsizePast,         // "BSIZE runs past the end of the input:" BSIZE
    kBgzfIsize,             // "ISIZE above 65535:" ISIZE
    kBgzfStepOver,          // the chain passes the span's stop offset without hitting it: value = BSIZE of the member that does
    kBgzfNumKinds
};

struct BgzfMember { uint32_t kind, xlen, bsize, isize, value; };

ZWZ_HD uint32_t bgzf_le16(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }

// The member at p, of which `avail` >= 1 bytes may be read.  kind == kBgzfOk: xlen, bsize (<= avail) and isize are its fields.
ZWZ_HD BgzfMember bgzf_member_parse(const uint8_t* p, uint64_t avail) {
    BgzfMember m{kBgzfOk, 0, 0, 0, 0};
    if (p[0] != 0x1f || (avail > 1 && p[1] != 0x8b) || (avail > 2 && p[2] != 8)) { m.kind = kBgzfMagic; return m; }
    if (avail < 12) { m.kind = kBgzfShortHeader; return m; }
    const uint32_t flg = p[3];
    if (!(flg & 4u)) { m.kind = kBgzfNoExtra; return m; }
    if (flg & ~5u) { m.kind = kBgzfFlags; m.value = flg; return m; }
    const uint32_t xlen = bgzf_le16(p + 10);
    m.xlen = xlen;
    if (avail < 12ull + xlen) { m.kind = kBgzfExtraPast; return m; }
    uint32_t bsize = 0;
    for (uint32_t x = 0; x < xlen;) {
        if (xlen - x < 4) { m.kind = kBgzfExtraMalformed; return m; }
        const uint8_t* f = p + 12 + x;
        const uint32_t slen = bgzf_le16(f + 2);
        if (4u + slen > xlen - x) { m.kind = kBgzfExtraMalformed; return m; }
        if (f[0] == 'B' && f[1] == 'C' && slen == 2) bsize = bgzf_le16(f + 4) + 1u;
        x += 4 + slen;
    }
    m.bsize = bsize;
    if (!bsize) { m.kind = kBgzfNoBc; return m; }
    if (bsize < 12u + xlen + 8u) { m.kind = kBgzfBsizeSmall; m.value = bsize; return m; }
    if (bsize > avail) { m.kind = kBgzfBsizePast; m.value = bsize; return m; }
    const uint32_t isize = le32_at(p + bsize - 4);
    if (isize > 65535u) { m.kind = kBgzfIsize; m.value = isize; return m; }
    m.isize = isize;
    return m;
}

// The cheap test in front of the parse, on the little-endian word at an offset: 1f 8b 08, then FLG = 4 or 5.  A member that parses
// always passes it.
ZWZ_HD bool bgzf_candidate_word(uint32_t w) { return (w & 0xfeffffffu) == 0x04088b1fu; }

// A span of the buffer to walk.  The chain starts at head and must hit stop exactly (stop == the buffer's length: the strict walk of
// everything behind head).  limit: the member at the stop offset is parsed as well and closes the list.
struct BgzfSpan { uint64_t head, stop; uint32_t limit, pad; };

// What the walk leaves per span.  count good members (their list starts at slot `first` of the member arrays), sum of their ISIZE;
// kind != kBgzfOk: the first failure in chain order, at member number `count`, byte offset fail_off.
struct BgzfSpanResult { uint64_t sum, fail_off, first; uint32_t count, kind, value, pad; };

constexpr uint32_t kBgzfWalkTile = 4096;            // bytes per scan workgroup: 256 lanes, 16 bytes each
constexpr uint32_t kBgzfNil = 0xffffffffu;

// Where a span's scan starts (whole 16-byte vectors) and how many tiles it takes; candidates lie in [head, min(stop, n))
ZWZ_HD uint64_t bgzf_span_base(const BgzfSpan& s) { return s.head & ~15ull; }
ZWZ_HD uint64_t bgzf_span_end(const BgzfSpan& s, uint64_t n) { return s.stop < n ? s.stop : n; }
ZWZ_HD uint64_t bgzf_span_tiles(const BgzfSpan& s, uint64_t n) {
    const uint64_t b = bgzf_span_base(s), e = bgzf_span_end(s, n);
    return e > s.head ? (e - b + kBgzfWalkTile - 1u) / kBgzfWalkTile : 0u;
}

// Candidates among the 16 offsets [o, o + 16), o a multiple of 16, as a bit mask.  w[0..3] is the vector at o, w[4] the word behind
// it (bytes past the buffer's end read as anything).  Offset p counts if lo <= p < hi and p + 4 <= n.
ZWZ_HD uint32_t bgzf_candidate_mask(const uint32_t w[5], uint64_t o, uint64_t lo, uint64_t hi, uint64_t n) {
    uint32_t mask = 0;
    for (uint32_t j = 0; j < 16; j++) {
        const uint64_t p = o + j;
        const uint32_t q = j >> 2, r = j & 3u;
        const uint32_t word = r ? (w[q] >> (8u * r)) | (w[q + 1] << (32u - 8u * r)) : w[q];
        if (bgzf_candidate_word(word) && p >= lo && p < hi && p + 4u <= n) mask |= 1u << j;
    }
    return mask;
}

// Index of the candidate at offset `target` in the ascending offsets pos[lo, hi), or kBgzfNil
ZWZ_HD uint32_t bgzf_find(const uint64_t* pos, uint32_t lo, uint32_t hi, uint64_t target) {
    const uint32_t end = hi;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (pos[mid] < target) lo = mid + 1u; else hi = mid;
    }
    return lo < end && pos[lo] == target ? lo : kBgzfNil;
}

// The parse of candidate k of span sp and its first link: meas = (kind, bsize, isize, value); the link goes to the candidate at the
// member's end if that lies in front of the span's end.  Candidates [k0, k1) are the span's.
struct BgzfMeas { uint32_t kind, bsize, isize, value; };
ZWZ_HD uint32_t bgzf_parse_link(const uint8_t* gz, uint64_t n, const BgzfSpan& sp, const uint64_t* pos, uint32_t k0, uint32_t k1, uint32_t k,
                                BgzfMeas* meas) {
    const uint64_t p = pos[k];
    const BgzfMember m = bgzf_member_parse(gz + p, n - p);
    *meas = BgzfMeas{m.kind, m.bsize, m.isize, m.value};
    if (m.kind != kBgzfOk) return kBgzfNil;
    const uint64_t next = p + m.bsize;
    return next < bgzf_span_end(sp, n) ? bgzf_find(pos, k + 1u, k1, next) : kBgzfNil;
}

// The end of a span's chain.  tail: the last marked candidate (kBgzfNil: the head is no candidate), with its parse and the rank and
// ISIZE sum of the good members in front of it within the span.  Returns the result but for `first`; *extra (offset, isize) = the
// member at the stop offset that `limit` adds, *has_extra whether there is one.
ZWZ_HD BgzfSpanResult bgzf_span_resolve(const uint8_t* gz, uint64_t n, const BgzfSpan& sp, uint64_t tail_pos, bool has_tail, const BgzfMeas& tm,
                                        uint32_t rank, uint64_t sum, bool* has_extra, uint64_t* extra_off, uint32_t* extra_isize) {
    BgzfSpanResult r{sum, 0, 0, rank, kBgzfOk, 0, 0};
    *has_extra = false;
    uint64_t cur = sp.head;
    if (has_tail) {
        if (tm.kind != kBgzfOk) { r.kind = tm.kind; r.value = tm.value; r.fail_off = tail_pos; return r; }
        r.count++; r.sum += tm.isize;
        cur = tail_pos + tm.bsize;
        if (cur > sp.stop) { r.count--; r.sum -= tm.isize; r.kind = kBgzfStepOver; r.value = tm.bsize; r.fail_off = tail_pos; return r; }
    }
    if (cur == sp.stop && !sp.limit) return r;
    if (cur >= n) {
        // the buffer ends here: fine for the strict walk; a stop or a head behind the end is the caller's to refuse
        if (cur != sp.stop) { r.kind = kBgzfMagic; r.fail_off = cur; }
        return r;
    }
    // the member at the stop offset, or an offset in front of it that is no candidate: the parse names what is wrong with it
    const BgzfMember m = bgzf_member_parse(gz + cur, n - cur);
    if (m.kind != kBgzfOk) { r.kind = m.kind; r.value = m.value; r.fail_off = cur; return r; }
    // (a good member in front of the stop is always a candidate and linked: the chain cannot end on one)
    if (cur != sp.stop) { r.kind = kBgzfNumKinds; r.fail_off = cur; return r; }
    *has_extra = true; *extra_off = cur; *extra_isize = m.isize;
    r.count++; r.sum += m.isize;
    return r;
}

// ---- virtual offsets --------------------------------------------------------------------------------------------------------------
// voffset = compressed offset of a member << 16 | offset inside its decoded block
constexpr uint64_t kBgzfVoffMaxCoff = 1ull << 48;
ZWZ_HD uint64_t bgzf_voffset(uint64_t coff, uint32_t within) { return coff << 16 | within; }

}  // namespace zwz
