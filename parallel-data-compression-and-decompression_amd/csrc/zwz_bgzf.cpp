// zwz_bgzf.cpp -- BGZF entry points of include/zwz.h: the host walk of member headers, the device drivers around the codec
// (crc32_blocks + zwz_deflate_batch_dev + bgzf_scan + bgzf_pack; bgzf_gather + inflate + bgzf_scan + bgzf_verify_compact), and
// whole-file streaming through pinned staging with reading, the GPU and writing overlapped.  Random access: the .gzi index
// (writer, streamed writer, reader), the planning of range reads and their device path (bgzf_gather_list + inflate +
// bgzf_verify_extract) for data in device memory or in a file.  The walk on the device (zwz_bgzf_walk.hip) behind
// zwz_bgzf_index_dev / zwz_bgzf_gzi_dev, and chunks by virtual offset: their spans walked, on the device or from a file's headers, the
// members walked made an index, the chunks made ranges, and those handed to the same planning and device path.
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "zwz_api_internal.h"
#include "zwz_bgzf.h"
#include "zwz_bgzf_walk.h"
#include "zwz_filejob.h"

using namespace zwz;

namespace {

constexpr uint64_t kMemberMax = (uint64_t)ZWZ_CHUNK_SIZE + kBgzfHeader + kBgzfTrailer - 6u;   // the deflate slot's bytes, reframed
constexpr uint32_t kFileSliceBlocks = 256;          // members per slice of the file functions: 16.7 MB of raw bytes

// Walks the members of gz[0, n).  Strict (partial = false): anything that is not a whole member is ZWZ_E_FORMAT.  partial: stops
// (ZWZ_OK) before a member that does not end inside the buffer -- the file reader's slice boundary.  Also stops after `limit` members.
// on_member(k, offset, isize) sees every member walked; *count counts them; *consumed = the end of the last one.  `at` is the buffer's
// offset in the file and k0 the number of members in front of it, for messages.
template <class F>
int bgzf_walk_each(const uint8_t* gz, uint64_t n, uint64_t at, uint64_t k0, bool partial, uint64_t limit, F&& on_member, uint64_t* count,
                   uint64_t* raw, uint64_t* consumed) {
    uint64_t o = 0, k = 0, total = 0;
    auto fail = [&](const char* what, uint64_t v) {
        if (v == ~0ull) set_error("bgzf: member %llu at byte offset %llu: %s", (unsigned long long)(k0 + k), (unsigned long long)(at + o), what);
        else set_error("bgzf: member %llu at byte offset %llu: %s %llu", (unsigned long long)(k0 + k), (unsigned long long)(at + o), what, (unsigned long long)v);
        *count = k; *raw = total; *consumed = o;
        return ZWZ_E_FORMAT;
    };
    while (o < n && k < limit) {
        const uint64_t avail = n - o;
        const uint8_t* m = gz + o;
        if (m[0] != 0x1f || (avail > 1 && m[1] != 0x8b) || (avail > 2 && m[2] != 8))
            return fail(k0 + k ? "trailing bytes that are not a gzip member" : "not gzip (bad magic or method)", ~0ull);
        if (avail < 12) { if (partial) break; return fail("truncated member header", ~0ull); }
        const uint32_t flg = m[3];
        if (!(flg & 4u)) return fail("no extra field: a plain gzip member, not BGZF", ~0ull);
        if (flg & ~5u) return fail("unsupported gzip header flags", flg);
        const uint32_t xlen = le16_at(m + 10);
        if (avail < 12ull + xlen) { if (partial) break; return fail("extra field runs past the end of the input", ~0ull); }
        uint32_t bsize = 0;
        for (uint32_t x = 0; x < xlen;) {
            if (xlen - x < 4) return fail("malformed extra field", ~0ull);
            const uint8_t* f = m + 12 + x;
            const uint32_t slen = le16_at(f + 2);
            if (4u + slen > xlen - x) return fail("malformed extra field", ~0ull);
            if (f[0] == 'B' && f[1] == 'C' && slen == 2) bsize = le16_at(f + 4) + 1u;
            x += 4 + slen;
        }
        if (!bsize) return fail("no BC subfield: not BGZF", ~0ull);
        if (bsize < 12u + xlen + kBgzfTrailer) return fail("BSIZE smaller than its header and trailer:", bsize);
        if (bsize > avail) { if (partial) break; return fail("BSIZE runs past the end of the input:", bsize); }
        const uint32_t isize = le32_at(m + bsize - 4);
        if (isize > kBgzfMaxIsize) return fail("ISIZE above 65535:", isize);
        on_member(k, o, isize);
        total += isize;
        k++;
        o += bsize;
    }
    *count = k; *raw = total; *consumed = o;
    return ZWZ_OK;
}

// offs[] (may be null) receives up to cap member offsets
int bgzf_walk(const uint8_t* gz, uint64_t n, uint64_t at, bool partial, uint64_t limit, uint64_t* offs, uint64_t cap, uint64_t* count,
              uint64_t* raw, uint64_t* consumed) {
    return bgzf_walk_each(gz, n, at, 0, partial, limit, [&](uint64_t k, uint64_t o, uint32_t) { if (offs && k < cap) offs[k] = o; }, count, raw,
                          consumed);
}

struct BgzfView {
    uint8_t *slots_a, *slots_b;                       // deflate output / gathered bodies; decoded blocks
    uint64_t *off, *moff, *base;
    uint32_t *len, *olen, *st, *crc, *isize, *err;
};

BgzfView bgzf_layout(Carver& w, size_t m) {
    BgzfView v;
    v.slots_a = w.take<uint8_t>(m * kBgzfSlot);
    v.slots_b = w.take<uint8_t>(m * kBgzfSlot, 256);  // (wg_copy reads up to 3 bytes past a decoded block)
    v.off = w.take<uint64_t>(m); v.moff = w.take<uint64_t>(m);
    v.len = w.take<uint32_t>(m); v.olen = w.take<uint32_t>(m); v.st = w.take<uint32_t>(m); v.crc = w.take<uint32_t>(m); v.isize = w.take<uint32_t>(m);
    v.base = w.take<uint64_t>(2); v.err = reinterpret_cast<uint32_t*>(v.base + 1);
    return v;
}

BgzfView bgzf_view(zwz_ctx* c) {
    Carver w(c->buf[kBufBgzf].p);
    return bgzf_layout(w, c->buf[kBufBgzf].count);
}

int ensure_bgzf(zwz_ctx* c, uint32_t m) {
    if (int rc = ensure_crc_tables(c)) return rc;
    return c->buf[kBufBgzf].reserve(c, m, layout_bytes([&](Carver& w) { bgzf_layout(w, m); }));
}

// The device part of compression, d_out_len = total bytes written (with or without the EOF member).  Arguments checked by the caller.
int compress_launch(zwz_ctx* c, const uint8_t* d_in, uint64_t n, uint8_t* d_out, uint64_t* d_out_len, int eof) {
    const uint64_t nblocks = (n + kBgzfBlock - 1) / kBgzfBlock;
    const uint32_t M = (uint32_t)(nblocks < c->max_batch ? (nblocks ? nblocks : 1) : c->max_batch);
    if (int rc = ensure_bgzf(c, M)) return rc;
    const BgzfView v = bgzf_view(c);
    const CrcTables* tab = c->buf[kBufCrcTables].as<const CrcTables>();
    HIPCHK(hipMemsetAsync(v.base, 0, 16, c->stream));
    for (uint64_t first = 0; first < nblocks; first += M) {
        const uint32_t m = (uint32_t)(nblocks - first < M ? nblocks - first : M);
        HIPCHK(launch_bgzf_layout(v.off, v.len, first, m, n, c->stream));
        HIPCHK(launch_crc32_blocks(tab, d_in, v.off, v.len, m, v.crc, c->cu_count, c->stream));
        if (int rc = zwz_deflate_batch_dev(c, d_in, v.off, v.len, m, v.slots_a, kBgzfSlot, v.olen)) return rc;
        HIPCHK(launch_bgzf_scan(v.olen, m, kBgzfHeader + kBgzfTrailer - 6u, ZWZ_CHUNK_SIZE - 1u, v.moff, v.base, v.err, c->stream));
        HIPCHK(launch_bgzf_pack(v.slots_a, v.olen, v.crc, v.len, v.moff, m, d_out, c->stream));
    }
    HIPCHK(launch_bgzf_finish(d_out, v.base, v.err, d_out_len, eof, c->stream));
    return ZWZ_OK;
}

int decompress_launch(zwz_ctx* c, const uint8_t* d_gz, uint64_t gz_len, const uint64_t* d_moff, uint32_t n, uint8_t* d_out, uint64_t* d_out_len,
                      uint32_t* d_status) {
    const uint32_t M = n < c->max_batch ? (n ? n : 1u) : c->max_batch;
    if (int rc = ensure_bgzf(c, M)) return rc;
    const BgzfView v = bgzf_view(c);
    const CrcTables* tab = c->buf[kBufCrcTables].as<const CrcTables>();
    HIPCHK(hipMemsetAsync(v.base, 0, 16, c->stream));
    for (uint32_t first = 0; first < n; first += M) {
        const uint32_t m = n - first < M ? n - first : M;
        HIPCHK(launch_bgzf_gather(d_gz, gz_len, d_moff, n, first, m, v.slots_a, v.off, v.len, v.crc, v.isize, d_status, c->stream));
        if (int rc = zwz_inflate_batch_dev(c, v.slots_a, v.off, v.len, m, v.slots_b, kBgzfSlot, v.olen, v.st)) return rc;
        HIPCHK(launch_bgzf_scan(v.isize, m, 0, kBgzfMaxIsize, v.moff, v.base, v.err, c->stream));
        HIPCHK(launch_bgzf_verify_compact(tab, v.slots_b, v.olen, v.st, v.crc, v.isize, v.moff, m, d_out, d_status + first, c->cu_count, c->stream));
    }
    HIPCHK(launch_bgzf_finish(d_out, v.base, v.err, d_out_len, 0, c->stream));
    return ZWZ_OK;
}

const char* member_status_text(uint32_t st) {
    switch (st) {
        case ZWZ_INF_NEED_INPUT: return "deflate body ends early";
        case ZWZ_INF_DATA_ERROR: return "invalid deflate body";
        case ZWZ_INF_OVERFLOW: return "deflate body decodes past 65535 bytes";
        case ZWZ_BGZF_BAD_MEMBER: return "member does not parse";
        case ZWZ_BGZF_ISIZE_MISMATCH: return "ISIZE mismatch";
        case ZWZ_BGZF_CRC_MISMATCH: return "CRC-32 mismatch";
        default: return "unknown member status";
    }
}

// First failing member of a decoded slice -> ZWZ_E_CHECKSUM / ZWZ_E_FORMAT with its place in zwz_last_error(); else ZWZ_OK.
int check_status(const uint32_t* st, uint32_t n, const uint64_t* offs, uint64_t at, uint64_t first_member) {
    for (uint32_t i = 0; i < n; i++) {
        if (!st[i]) continue;
        set_error("bgzf: member %llu at byte offset %llu: %s", (unsigned long long)(first_member + i), (unsigned long long)(at + offs[i]),
                  member_status_text(st[i]));
        return st[i] == ZWZ_BGZF_CRC_MISMATCH || st[i] == ZWZ_BGZF_ISIZE_MISMATCH ? ZWZ_E_CHECKSUM : ZWZ_E_FORMAT;
    }
    return ZWZ_OK;
}

// ---- .gzi index and range reads ----------------------------------------------------------------------------------------------------

constexpr size_t kWalkBuf = 4u << 20;               // bytes of file a streamed walk holds (a member is at most 65 536 bytes)
constexpr size_t kRangeOutSlice = 16u << 20;        // decoded bytes of one slice of the file range reader (>= one member)

inline void put64(uint8_t* p, uint64_t v) { for (int i = 0; i < 8; i++) p[i] = (uint8_t)(v >> (8 * i)); }

// The writer's rule: one entry (compressed offset, decoded offset) per member after the first, in file order, except a last member
// that decodes to nothing (the EOF member).  An entry is held back until the next member shows it is not the last.
struct GziBuilder {
    uint64_t raw = 0, members = 0, entries = 0;
    bool held = false, held_empty = false;
    uint64_t hc = 0, hu = 0;
    std::vector<uint8_t> buf;                       // serialised entries not yet flushed
    void emit() { uint8_t e[16]; put64(e, hc); put64(e + 8, hu); buf.insert(buf.end(), e, e + 16); entries++; held = false; }
    void member(uint64_t coff, uint32_t isize) {
        if (held) emit();
        if (members++) { held = true; held_empty = isize == 0; hc = coff; hu = raw; }
        raw += isize;
    }
    void finish() { if (held && !held_empty) emit(); held = false; }
};

// Walks the members of an open file from its start with kWalkBuf bytes of memory: on_member(offset, isize) for each, until the end of
// the file or until stop() returns true (asked after every buffer).
template <class F, class S>
int walk_file(FILE* in, F&& on_member, S&& stop) {
    std::vector<uint8_t> buf(kWalkBuf);
    size_t have = 0;
    bool eof = false;
    uint64_t at = 0, k0 = 0;
    for (;;) {
        if (!eof) {
            bool io_err = false;
            const size_t got = read_full(in, buf.data() + have, kWalkBuf - have, &io_err);
            if (io_err) { set_error("read error"); return ZWZ_E_IO; }
            eof = have + got < kWalkBuf;
            have += got;
        }
        if (!have) return ZWZ_OK;
        uint64_t count = 0, raw = 0, used = 0;
        if (int rc = bgzf_walk_each(buf.data(), have, at, k0, !eof, ~0ull, [&](uint64_t, uint64_t o, uint32_t isize) { on_member(at + o, isize); },
                                    &count, &raw, &used))
            return rc;
        if (!count) { set_error("bgzf: cannot split the input at byte offset %llu", (unsigned long long)at); return ZWZ_E_FORMAT; }
        memmove(buf.data(), buf.data() + used, have - used);
        have -= used;
        at += used;
        k0 += count;
        if (stop()) return ZWZ_OK;
    }
}

// A parsed .gzi: entry 0 is the implied (0, 0); coff strictly increasing, uoff not decreasing.
struct GziIndex { std::vector<uint64_t> coff, uoff; };

int parse_gzi(const uint8_t* g, uint64_t n, GziIndex* ix) {
    if (n < 8 || !g) { set_error("gzi: %llu bytes, shorter than its 8-byte entry count", (unsigned long long)n); return ZWZ_E_FORMAT; }
    const uint64_t count = le64_at(g);
    if ((n - 8) % 16 || (n - 8) / 16 != count) {
        set_error("gzi: %llu bytes do not hold the %llu entries its count gives", (unsigned long long)n, (unsigned long long)count);
        return ZWZ_E_FORMAT;
    }
    ix->coff.assign(1, 0);
    ix->uoff.assign(1, 0);
    ix->coff.reserve(count + 1);
    ix->uoff.reserve(count + 1);
    for (uint64_t i = 0; i < count; i++) {
        const uint64_t c = le64_at(g + 8 + 16 * i), u = le64_at(g + 16 + 16 * i);
        if (c <= ix->coff.back()) {
            set_error("gzi: entry %llu: compressed offset %llu does not follow %llu", (unsigned long long)(i + 1), (unsigned long long)c,
                      (unsigned long long)ix->coff.back());
            return ZWZ_E_FORMAT;
        }
        if (u < ix->uoff.back()) {
            set_error("gzi: entry %llu: decoded offset %llu below the previous %llu", (unsigned long long)(i + 1), (unsigned long long)u,
                      (unsigned long long)ix->uoff.back());
            return ZWZ_E_FORMAT;
        }
        ix->coff.push_back(c);
        ix->uoff.push_back(u);
    }
    return ZWZ_OK;
}

// The pieces of k ranges against an index, in compressed sparse rows over the touched members (index entries holding at least one
// requested byte, ascending).  Within a member the pieces of at least kWavePieceMax bytes come first (nlong of them).
struct RangePlan {
    std::vector<uint32_t> member;                   // touched index entries
    std::vector<uint32_t> expect;                   // decoded length the index implies (kNoExpect: the last entry)
    std::vector<uint32_t> row, nlong;               // member t's pieces: [row[t], row[t + 1]), the first nlong[t] long
    std::vector<RangePiece> piece;                  // dst = place in the concatenated output
    std::vector<uint32_t> prange;                   // the range each piece belongs to
    uint64_t total = 0;                             // output bytes
};

int range_past_end(uint32_t r, uint64_t a, uint64_t len) {
    set_error("bgzf: range %u (offset %llu, length %llu) runs past the end of the decoded data", r, (unsigned long long)a, (unsigned long long)len);
    return ZWZ_E_INVALID;
}

int plan_ranges(const GziIndex& ix, const uint64_t* ranges, uint32_t k, RangePlan* P) {
    struct Raw { uint32_t j, r, off, len; uint64_t dst; };
    const uint64_t* uo = ix.uoff.data();
    const size_t N = ix.uoff.size(), last = N - 1;
    std::vector<Raw> raw;
    raw.reserve(k);
    uint64_t dst = 0;
    auto add = [&](size_t j, uint32_t r, uint64_t lo, uint64_t hi) {
        // (pieces of an entry whose span exceeds what a member can hold are clamped to a place no block reaches: the kernel does not copy them)
        const uint64_t off = lo - uo[j], len = hi - lo;
        raw.push_back({(uint32_t)j, r, (uint32_t)std::min<uint64_t>(off, kBgzfSlot), (uint32_t)std::min<uint64_t>(len, kBgzfSlot), dst});
    };
    for (uint32_t r = 0; r < k; r++) {
        const uint64_t a = ranges[2 * r], len = ranges[2 * r + 1];
        if (len > ~0ull - a) {
            set_error("bgzf: range %u (offset %llu, length %llu): offset + length overflows", r, (unsigned long long)a, (unsigned long long)len);
            return ZWZ_E_INVALID;
        }
        const uint64_t b = a + len;
        if (N == 0) { if (b) return range_past_end(r, a, len); continue; }
        // the last entry's member holds at most kBgzfMaxIsize bytes: a range beyond that is past the end without looking further
        if (b > uo[last] && b - uo[last] > kBgzfMaxIsize) return range_past_end(r, a, len);
        if (!len) {
            if (a > uo[last]) add(last, r, a, a);       // the device checks a against the last member's length
            continue;
        }
        const size_t j0 = std::upper_bound(ix.uoff.begin(), ix.uoff.end(), a) - ix.uoff.begin() - 1;
        const size_t j1 = std::upper_bound(ix.uoff.begin() + j0, ix.uoff.end(), b - 1) - ix.uoff.begin() - 1;
        for (size_t j = j0; j <= j1; j++) {
            const uint64_t lo = std::max(a, uo[j]), hi = j < last ? std::min(b, uo[j + 1]) : b;
            if (hi > lo) { add(j, r, lo, hi); dst += hi - lo; }
        }
        if (raw.size() > 0xfffffff0ull) { set_error("bgzf: more than 2^32 - 16 pieces"); return ZWZ_E_INVALID; }
    }
    P->total = dst;
    // counting sort by entry: long pieces from the front of a member's rows, short ones behind them
    std::vector<uint32_t> cnt(N + 1, 0), cntl(N, 0);
    for (const Raw& q : raw) { cnt[q.j]++; if (q.len >= kWavePieceMax) cntl[q.j]++; }
    P->member.clear(); P->expect.clear(); P->row.assign(1, 0); P->nlong.clear();
    std::vector<uint32_t> cur_long(N), cur_short(N);
    for (size_t j = 0; j < N; j++) {
        if (!cnt[j]) continue;
        P->member.push_back((uint32_t)j);
        P->expect.push_back(j < last ? (uint32_t)std::min<uint64_t>(uo[j + 1] - uo[j], kBgzfSlot) : kNoExpect);
        cur_long[j] = P->row.back();
        cur_short[j] = P->row.back() + cntl[j];
        P->nlong.push_back(cntl[j]);
        P->row.push_back(P->row.back() + cnt[j]);
    }
    P->piece.resize(raw.size());
    P->prange.resize(raw.size());
    for (const Raw& q : raw) {
        const uint32_t at = q.len >= kWavePieceMax ? cur_long[q.j]++ : cur_short[q.j]++;
        P->piece[at] = {q.dst, q.off, q.len};
        P->prange[at] = q.r;
    }
    return ZWZ_OK;
}

// One slice of a plan: touched members [t0, t1) and pieces [p0, p1) of theirs (all of them, or a part of one member's).
struct Slice { uint32_t t0, t1, p0, p1; };

// moff, mend (u64); expect, nlong, status, bad, row (u32; row has m + 1); pieces
inline size_t slice_bytes(uint32_t m, uint32_t np) { return round_up(16 * (size_t)m + 20 * (size_t)m + 4, 16) + 16 * (size_t)np; }

struct SliceView { uint64_t *moff, *mend; uint32_t *expect, *nlong, *status, *bad, *row; RangePiece* piece; };
SliceView slice_view(uint8_t* p, uint32_t m) {
    SliceView v;
    v.moff = reinterpret_cast<uint64_t*>(p); v.mend = v.moff + m;
    v.expect = reinterpret_cast<uint32_t*>(v.mend + m); v.nlong = v.expect + m; v.status = v.nlong + m; v.bad = v.status + m; v.row = v.bad + m;
    v.piece = reinterpret_cast<RangePiece*>(p + round_up(36 * (size_t)m + 4, 16));
    return v;
}

// (whole MiB: the file reader asks per slice, and must not reallocate for every slice a little larger than the last)
int ensure_rr(zwz_ctx* c, size_t bytes) {
    const size_t cap = round_up(bytes, (size_t)1 << 20);
    if (int rc = c->buf[kBufRangeHost].reserve(c, 0, cap)) return rc;
    return c->buf[kBufRangeDev].reserve(c, 0, cap);
}

// Packs slice S at h (pinned; its device copy at d) and queues it: one upload, bgzf_gather_list, inflate, bgzf_verify_extract, and the
// status and bad-piece words back into h.  moff / mend: where touched member t starts and how far it may be read in d_gz.  compact:
// the slice's pieces go to d_out one after the other (their output offsets stay in the plan) instead of to their place in the output.
int queue_slice(zwz_ctx* c, const RangePlan& P, const Slice& S, const uint64_t* moff, const uint64_t* mend, uint8_t* h, uint8_t* d,
                const uint8_t* d_gz, uint64_t gz_len, uint8_t* d_out, bool compact) {
    const uint32_t m = S.t1 - S.t0, np = S.p1 - S.p0;
    const SliceView hv = slice_view(h, m), dv = slice_view(d, m);
    uint64_t o = 0;
    hv.row[0] = 0;
    for (uint32_t i = 0; i < m; i++) {
        const uint32_t t = S.t0 + i;
        const uint32_t rs = std::max(P.row[t], S.p0), re = std::min(P.row[t + 1], S.p1);
        const uint32_t ls = std::min(std::max(P.row[t] + P.nlong[t], rs), re);
        hv.moff[i] = moff[t]; hv.mend[i] = mend ? mend[t] : gz_len;
        hv.expect[i] = P.expect[t]; hv.nlong[i] = ls - rs; hv.status[i] = 0; hv.bad[i] = ~0u;
        hv.row[i + 1] = re - S.p0;
    }
    for (uint32_t p = 0; p < np; p++) {
        hv.piece[p] = P.piece[S.p0 + p];
        if (compact) { hv.piece[p].dst = o; o += hv.piece[p].len; }
    }
    const BgzfView v = bgzf_view(c);
    const CrcTables* tab = c->buf[kBufCrcTables].as<const CrcTables>();
    HIPCHK(hipMemcpyAsync(d, h, slice_bytes(m, np), hipMemcpyHostToDevice, c->stream));
    HIPCHK(launch_bgzf_gather_list(d_gz, gz_len, dv.moff, dv.mend, m, v.slots_a, v.off, v.len, v.crc, v.isize, dv.status, c->stream));
    if (int rc = zwz_inflate_batch_dev(c, v.slots_a, v.off, v.len, m, v.slots_b, kBgzfSlot, v.olen, v.st)) return rc;
    HIPCHK(launch_bgzf_verify_extract(tab, v.slots_b, v.olen, v.st, v.crc, v.isize, dv.expect, dv.row, dv.nlong, dv.piece, m, d_out, dv.status, dv.bad,
                                      c->cu_count, c->stream));
    HIPCHK(hipMemcpyAsync(hv.status, dv.status, 8 * (size_t)m, hipMemcpyDeviceToHost, c->stream));
    return ZWZ_OK;
}

// After the slice ran: the first touched member that failed (as check_status reports it), else the first range past the end.
int slice_verdict(const RangePlan& P, const GziIndex& ix, const Slice& S, const uint8_t* h, const uint64_t* ranges) {
    const uint32_t m = S.t1 - S.t0;
    const SliceView hv = slice_view(const_cast<uint8_t*>(h), m);
    for (uint32_t i = 0; i < m; i++) {
        const uint32_t j = P.member[S.t0 + i], st = hv.status[i];
        if (st == kBgzfIndexMismatch) {
            set_error("bgzf: member %u at byte offset %llu: decoded length differs from the .gzi index", j, (unsigned long long)ix.coff[j]);
            return ZWZ_E_FORMAT;
        }
        if (st) {
            const uint64_t off = ix.coff[j];
            return check_status(&st, 1, &off, 0, j);
        }
        if (hv.bad[i] != ~0u) {
            const uint32_t r = P.prange[S.p0 + hv.bad[i]];
            return range_past_end(r, ranges[2 * r], ranges[2 * r + 1]);
        }
    }
    return ZWZ_OK;
}

int read_file_bytes(const char* path, std::vector<uint8_t>* out) {
    FILE* f = fopen(path, "rb");
    if (!f) { set_error("cannot open %s", path); return ZWZ_E_IO; }
    out->clear();
    uint8_t tmp[1 << 16];
    size_t k;
    while ((k = fread(tmp, 1, sizeof tmp, f)) > 0) out->insert(out->end(), tmp, tmp + k);
    const bool bad = ferror(f);
    fclose(f);
    if (bad) { set_error("read error on %s", path); return ZWZ_E_IO; }
    return ZWZ_OK;
}

// The device path of a plan over data in device memory: slices of at most max_batch touched members, queued one behind the other.
int run_plan_dev(zwz_ctx* c, const GziIndex& ix, const RangePlan& P, const uint64_t* ranges, const uint8_t* d_gz, uint64_t gz_len, uint8_t* d_out) {
    const uint32_t T = (uint32_t)P.member.size();
    if (!T) return ZWZ_OK;
    HIPCHK(hipSetDevice(c->device));
    const uint32_t M = T < c->max_batch ? T : c->max_batch;
    if (int rc = ensure_bgzf(c, M)) return rc;
    // every slice packs into its own part of the plan buffers: the host fills slice s + 1 while the device runs slice s
    std::vector<Slice> slices;
    std::vector<size_t> at;
    size_t bytes = 0;
    for (uint32_t t0 = 0; t0 < T; t0 += M) {
        const uint32_t t1 = T - t0 < M ? T : t0 + M;
        slices.push_back({t0, t1, P.row[t0], P.row[t1]});
        at.push_back(bytes);
        bytes += round_up(slice_bytes(t1 - t0, P.row[t1] - P.row[t0]), 16);
    }
    if (int rc = ensure_rr(c, bytes)) return rc;
    std::vector<uint64_t> moff(T);
    for (uint32_t t = 0; t < T; t++) moff[t] = ix.coff[P.member[t]];
    uint8_t* h = c->buf[kBufRangeHost].as<uint8_t>();
    uint8_t* d = c->buf[kBufRangeDev].as<uint8_t>();
    for (size_t s = 0; s < slices.size(); s++)
        if (int rc = queue_slice(c, P, slices[s], moff.data(), nullptr, h + at[s], d + at[s], d_gz, gz_len, d_out, false)) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));
    for (size_t s = 0; s < slices.size(); s++)
        if (int rc = slice_verdict(P, ix, slices[s], h + at[s], ranges)) return rc;
    return ZWZ_OK;
}

// The device path of a plan over a file: its touched members read with one pread per run of consecutive index entries.
int run_plan_file(zwz_ctx* c, const char* src, const GziIndex& ix, const RangePlan& P, const uint64_t* ranges, uint8_t* out) {
    const uint32_t T = (uint32_t)P.member.size();
    if (!T) return ZWZ_OK;
    HIPCHK(hipSetDevice(c->device));
    FileJob job;
    job.fd = open(src, O_RDONLY);
    if (job.fd < 0) { set_error("cannot open %s", src); return ZWZ_E_IO; }
    struct stat stt {};
    if (fstat(job.fd, &stt) != 0) { set_error("cannot stat %s", src); return ZWZ_E_IO; }
    const uint64_t fsize = (uint64_t)stt.st_size;
    // member t's bytes in the file: [coff, end), end = the next entry's offset (at most a member's 65 536 bytes further), or the file's end
    const size_t last = ix.coff.size() - 1;
    std::vector<uint64_t> fend(T);
    for (uint32_t t = 0; t < T; t++) {
        const size_t j = P.member[t];
        const uint64_t s0 = ix.coff[j];
        uint64_t e = std::min<uint64_t>(s0 + kBgzfSlot, fsize);
        if (j < last) e = std::min(e, ix.coff[j + 1]);
        fend[t] = s0 >= fsize ? s0 : e;                     // (an entry past the file's end: nothing to read, the member does not parse)
    }
    const uint32_t S = c->max_batch < kFileSliceBlocks ? c->max_batch : kFileSliceBlocks;
    const size_t B = (size_t)S * kBgzfSlot;
    if (int rc = job.alloc({B + 16, kRangeOutSlice + 16}, {B + 16, kRangeOutSlice + 16})) return rc;    // packed members, decoded pieces
    if (int rc = ensure_bgzf(c, S)) return rc;
    uint8_t* hin = static_cast<uint8_t*>(job.h[0]);
    uint8_t* hout = static_cast<uint8_t*>(job.h[1]);
    std::vector<uint64_t> moff(T), mend(T);
    uint32_t t = 0, p = 0;
    while (t < T) {
        // the slice: whole members while they fit S and kRangeOutSlice, or a part of one member's pieces that alone exceed kRangeOutSlice
        // (every piece is at most 65 536 bytes: a part holds at least one).  Its first member may continue one cut before.
        Slice sl{t, t, p, p};
        uint64_t obytes = 0;
        while (sl.t1 < T && sl.t1 - sl.t0 < S) {
            const uint32_t q0 = sl.t1 == t ? p : P.row[sl.t1];
            uint64_t mb = 0;
            for (uint32_t q = q0; q < P.row[sl.t1 + 1]; q++) mb += P.piece[q].len;
            if (obytes + mb <= kRangeOutSlice) { obytes += mb; sl.t1++; sl.p1 = P.row[sl.t1]; continue; }
            if (sl.t1 == sl.t0) {
                uint32_t q = q0;
                while (q < P.row[sl.t1 + 1] && obytes + P.piece[q].len <= kRangeOutSlice) obytes += P.piece[q++].len;
                sl.t1++;
                sl.p1 = q;
            }
            break;
        }
        // read the slice's members: one pread per run of consecutive entries
        uint64_t packed = 0;
        for (uint32_t i = sl.t0; i < sl.t1;) {
            uint32_t e = i + 1;
            while (e < sl.t1 && P.member[e] == P.member[e - 1] + 1 && fend[e - 1] == ix.coff[P.member[e]]) e++;
            const uint64_t start = ix.coff[P.member[i]], len = fend[e - 1] - start;
            size_t got = 0;
            while (got < len) {
                const ssize_t r = pread(job.fd, hin + packed + got, len - got, (off_t)(start + got));
                if (r < 0) { set_error("read error on %s", src); return ZWZ_E_IO; }
                if (r == 0) break;
                got += (size_t)r;
            }
            for (uint32_t q = i; q < e; q++) {
                moff[q] = packed + (ix.coff[P.member[q]] - start);
                mend[q] = std::min(packed + (fend[q] - start), packed + got);
            }
            packed += got;
            i = e;
        }
        uint8_t* d_in = static_cast<uint8_t*>(job.d[0]);
        uint8_t* d_dec = static_cast<uint8_t*>(job.d[1]);
        const uint32_t m = sl.t1 - sl.t0, np = sl.p1 - sl.p0;
        if (int rc = ensure_rr(c, slice_bytes(m, np))) return rc;
        HIPCHK(hipMemcpyAsync(d_in, hin, packed, hipMemcpyHostToDevice, c->stream));
        if (int rc = queue_slice(c, P, sl, moff.data(), mend.data(), c->buf[kBufRangeHost].as<uint8_t>(), c->buf[kBufRangeDev].as<uint8_t>(), d_in, packed,
                                 d_dec, true))
            return rc;
        if (obytes) HIPCHK(hipMemcpyAsync(hout, d_dec, obytes, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        if (int rc = slice_verdict(P, ix, sl, c->buf[kBufRangeHost].as<const uint8_t>(), ranges)) return rc;
        uint64_t o = 0;
        for (uint32_t q = sl.p0; q < sl.p1; q++) { memcpy(out + P.piece[q].dst, hout + o, P.piece[q].len); o += P.piece[q].len; }
        p = sl.p1;
        t = p < P.row[sl.t1] ? sl.t1 - 1 : sl.t1;         // a member cut in parts: its next part opens the next slice
    }
    return ZWZ_OK;
}

// ---- the member walk on the device, and chunks by virtual offset -----------------------------------------------------------------------

// A failure of the walk (bgzf_core.h) in bgzf_walk_each's words: member number k, byte offset o
int walk_failure(uint32_t kind, uint64_t k, uint64_t o, uint32_t value) {
    static const char* const text[kBgzfNumKinds] = {
        "", "", "truncated member header", "no extra field: a plain gzip member, not BGZF", "unsupported gzip header flags",
        "extra field runs past the end of the input", "malformed extra field", "no BC subfield: not BGZF",
        "BSIZE smaller than its header and trailer:", "BSIZE runs past the end of the input:", "ISIZE above 65535:",
        "the member chain steps over the offset it has to hit: BSIZE"};
    const char* what = kind == kBgzfMagic ? (k ? "trailing bytes that are not a gzip member" : "not gzip (bad magic or method)")
                     : kind < kBgzfNumKinds ? text[kind] : "the walk lost the member chain";
    const bool with_value = kind == kBgzfFlags || kind == kBgzfBsizeSmall || kind == kBgzfBsizePast || kind == kBgzfIsize || kind == kBgzfStepOver;
    if (!with_value) set_error("bgzf: member %llu at byte offset %llu: %s", (unsigned long long)k, (unsigned long long)o, what);
    else set_error("bgzf: member %llu at byte offset %llu: %s %llu", (unsigned long long)k, (unsigned long long)o, what, (unsigned long long)value);
    return ZWZ_E_FORMAT;
}

// The whole buffer as one span: the strict walk.  *r = its result; the members stay on the device (W).
int walk_whole_dev(zwz_ctx* c, const uint8_t* d_gz, uint64_t gz_len, BgzfWalk* W, BgzfSpanResult* r) {
    HIPCHK(hipSetDevice(c->device));
    const BgzfSpan sp{0, gz_len, 0, 0};
    if (int rc = bgzf_walk_spans(c, d_gz, gz_len, &sp, 1, W)) return rc;
    *r = W->res[0];
    return ZWZ_OK;
}

// Member slots [first, first + count) of a walk, brought to the host
int walk_members_host(zwz_ctx* c, const BgzfWalk& W, uint64_t first, uint64_t count, uint64_t* off, uint32_t* isize) {
    if (!count) return ZWZ_OK;
    HIPCHK(hipMemcpyAsync(off, W.d_moff + first, 8 * count, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(isize, W.d_misize + first, 4 * count, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return ZWZ_OK;
}

// k chunks (vbeg, vend) against a stream of gz_len bytes: what can be refused without looking at the stream, and the merged spans of
// their compressed offsets, ascending and apart, each chunk's in span_of.  A span has `limit` where a chunk needs the member AT its
// end: it ends inside that member, or lies in it altogether.
struct ChunkSpans { std::vector<BgzfSpan> spans; std::vector<uint32_t> span_of; };

int chunk_refuse(uint32_t i, const uint64_t* chunks, const char* why) {
    set_error("bgzf: chunk %u (%llu, %llu): %s", i, (unsigned long long)chunks[2 * i], (unsigned long long)chunks[2 * i + 1], why);
    return ZWZ_E_INVALID;
}

int chunk_spans(const uint64_t* chunks, uint32_t k, uint64_t gz_len, ChunkSpans* S) {
    std::vector<uint32_t> order(k);
    for (uint32_t i = 0; i < k; i++) {
        const uint64_t vb = chunks[2 * i], ve = chunks[2 * i + 1];
        if (vb > ve) return chunk_refuse(i, chunks, "begins behind its end");
        if ((vb >> 16) >= gz_len) return chunk_refuse(i, chunks, "begins at or past the end of the stream");
        if ((ve >> 16) > gz_len) return chunk_refuse(i, chunks, "ends past the end of the stream");
        if ((ve >> 16) == gz_len && (ve & 0xffffu)) return chunk_refuse(i, chunks, "ends inside a member that would start at the end of the stream");
        order[i] = i;
    }
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return chunks[2 * a] >> 16 < chunks[2 * b] >> 16; });
    S->spans.clear();
    S->span_of.assign(k, 0);
    for (uint32_t q = 0; q < k; q++) {
        const uint32_t i = order[q];
        const uint64_t cb = chunks[2 * i] >> 16, ce = chunks[2 * i + 1] >> 16;
        const uint32_t limit = ce < gz_len && ((chunks[2 * i + 1] & 0xffffu) || ce == cb) ? 1u : 0u;
        if (S->spans.empty() || cb > S->spans.back().stop) S->spans.push_back(BgzfSpan{cb, ce, limit, 0});
        else {
            BgzfSpan& sp = S->spans.back();
            if (ce > sp.stop) { sp.stop = ce; sp.limit = limit; }
            else if (ce == sp.stop) sp.limit |= limit;
        }
        S->span_of[i] = (uint32_t)S->spans.size() - 1u;
    }
    return ZWZ_OK;
}

// The first failing span of a walk: a chain that steps over its stop is the request's fault (the first chunk that ends there is
// named), everything else the stream's.
int chunk_walk_verdict(const ChunkSpans& S, const BgzfSpanResult* res, const uint64_t* chunks, uint32_t k) {
    for (size_t s = 0; s < S.spans.size(); s++) {
        const BgzfSpanResult& r = res[s];
        if (r.kind == kBgzfOk) continue;
        if (r.kind != kBgzfStepOver) return walk_failure(r.kind, r.count, r.fail_off, r.value);
        for (uint32_t i = 0; i < k; i++)
            if (S.span_of[i] == s && chunks[2 * i + 1] >> 16 == S.spans[s].stop) {
                set_error("bgzf: chunk %u (%llu, %llu): the member chain steps over its end: the member at byte offset %llu has BSIZE %u", i,
                          (unsigned long long)chunks[2 * i], (unsigned long long)chunks[2 * i + 1], (unsigned long long)r.fail_off, r.value);
                return ZWZ_E_INVALID;
            }
        return walk_failure(r.kind, r.count, r.fail_off, r.value);
    }
    return ZWZ_OK;
}

// The members walked (all spans, in order) as an index -- uoff the running sum of ISIZE -- and the chunks as (offset, length) ranges
// in its decoded coordinates.  span_end[s] = the index of the first member behind span s.
int chunk_ranges(const ChunkSpans& S, const std::vector<size_t>& span_end, const GziIndex& ix, const std::vector<uint32_t>& isize, uint64_t total,
                 const uint64_t* chunks, uint32_t k, std::vector<uint64_t>* ranges, uint64_t* sizes) {
    ranges->resize(2 * (size_t)k);
    auto member_at = [&](uint64_t coff, size_t lo, size_t hi) {
        const size_t j = std::lower_bound(ix.coff.begin() + lo, ix.coff.begin() + hi, coff) - ix.coff.begin();
        return j < hi && ix.coff[j] == coff ? j : (size_t)-1;
    };
    for (uint32_t i = 0; i < k; i++) {
        const uint64_t vb = chunks[2 * i], ve = chunks[2 * i + 1];
        const uint32_t s = S.span_of[i];
        const size_t lo = s ? span_end[s - 1] : 0, hi = span_end[s];
        const size_t jb = member_at(vb >> 16, lo, hi);
        if (jb == (size_t)-1) {
            set_error("bgzf: chunk %u (%llu, %llu): byte offset %llu is no member of the chain that starts at byte offset %llu", i, (unsigned long long)vb,
                      (unsigned long long)ve, (unsigned long long)(vb >> 16), (unsigned long long)S.spans[s].head);
            return ZWZ_E_FORMAT;
        }
        if ((vb & 0xffffu) > isize[jb]) return chunk_refuse(i, chunks, "begins past the end of its block (the offset inside the block is above ISIZE)");
        const uint64_t pb = ix.uoff[jb] + (vb & 0xffffu);
        uint64_t pe;
        const size_t je = member_at(ve >> 16, lo, hi);
        if (je != (size_t)-1) {
            if ((ve & 0xffffu) > isize[je]) return chunk_refuse(i, chunks, "ends past the end of its block (the offset inside the block is above ISIZE)");
            pe = ix.uoff[je] + (ve & 0xffffu);
        } else if (ve >> 16 == S.spans[s].stop) {
            pe = hi < ix.uoff.size() ? ix.uoff[hi] : total;         // the span's chain ends there
        } else {
            return chunk_refuse(i, chunks, "the member chain steps over its end");
        }
        (*ranges)[2 * i] = pb;
        (*ranges)[2 * i + 1] = sizes[i] = pe - pb;
    }
    return ZWZ_OK;
}

// Everything in front of the decode for a stream in device memory: refusals, the walk, the index, the ranges, the sizes
struct ChunkJob { GziIndex ix; std::vector<uint64_t> ranges; };

int chunk_prepare_dev(zwz_ctx* c, const uint8_t* d_gz, uint64_t gz_len, const uint64_t* chunks, uint32_t k, uint64_t* sizes, ChunkJob* J) {
    ChunkSpans S;
    if (int rc = chunk_spans(chunks, k, gz_len, &S)) return rc;
    J->ix.coff.clear(); J->ix.uoff.clear(); J->ranges.clear();
    if (!k) return ZWZ_OK;
    HIPCHK(hipSetDevice(c->device));
    BgzfWalk W;
    if (int rc = bgzf_walk_spans(c, d_gz, gz_len, S.spans.data(), (uint32_t)S.spans.size(), &W)) return rc;
    if (int rc = chunk_walk_verdict(S, W.res.data(), chunks, k)) return rc;
    std::vector<uint64_t> off(W.slots);
    std::vector<uint32_t> isz(W.slots);
    if (int rc = walk_members_host(c, W, 0, W.slots, off.data(), isz.data())) return rc;
    std::vector<size_t> span_end(S.spans.size());
    std::vector<uint32_t> isize;
    uint64_t total = 0;
    for (size_t s = 0; s < S.spans.size(); s++) {
        const BgzfSpanResult& r = W.res[s];
        for (uint64_t j = r.first; j < r.first + r.count; j++) {
            J->ix.coff.push_back(off[j]); J->ix.uoff.push_back(total); isize.push_back(isz[j]);
            total += isz[j];
        }
        span_end[s] = J->ix.coff.size();
    }
    return chunk_ranges(S, span_end, J->ix, isize, total, chunks, k, &J->ranges, sizes);
}

// The host walk of one span of a file: the chain from head, which must hit stop (limit: the member there is walked too).  Of every
// member only the header (32 bytes, more where the extra field is longer) and the ISIZE field are read, with pread: nothing in front
// of head, nothing behind the member at stop, and one member's header in memory.
struct FileHeaders {
    int fd = -1;
    uint64_t fsize = 0;
    std::vector<uint8_t> buf;                            // a member's header at its place, ISIZE at its: what bgzf_member_parse looks at
    int fill(uint64_t at, size_t from, size_t to) {      // file bytes [at + from, at + to) -> buf[from, to)
        while (from < to) {
            const ssize_t r = pread(fd, buf.data() + from, to - from, (off_t)(at + from));
            if (r < 0) { set_error("read error"); return ZWZ_E_IO; }
            if (r == 0) break;                               // (the file shrank under the walk: what is left in buf is zeros or stale, and parses or fails as such)
            from += (size_t)r;
        }
        return ZWZ_OK;
    }
    // the member at file offset `at`
    int parse(uint64_t at, BgzfMember* m) {
        constexpr size_t kFirst = 32;
        if (buf.empty()) buf.resize(kBgzfSlot + 16);
        const uint64_t avail = std::min<uint64_t>(fsize - at, kBgzfSlot + 16);     // (a member is at most 65 536 bytes)
        size_t have = (size_t)std::min<uint64_t>(avail, kFirst);
        if (int rc = fill(at, 0, have)) return rc;
        if (have >= 12) {
            const size_t header = (size_t)std::min<uint64_t>(avail, 12u + le16_at(buf.data() + 10));
            if (header > have) { if (int rc = fill(at, have, header)) return rc; have = header; }
        }
        *m = bgzf_member_parse(buf.data(), avail);
        if (m->kind != kBgzfOk && m->kind != kBgzfIsize) return ZWZ_OK;
        // BSIZE holds: now the ISIZE field, which the first parse read as whatever the buffer held
        if (m->bsize > have) if (int rc = fill(at, std::max<size_t>(have, m->bsize - 4u), m->bsize)) return rc;
        *m = bgzf_member_parse(buf.data(), avail);
        return ZWZ_OK;
    }
};

template <class F>
int walk_file_span(FileHeaders& fh, const BgzfSpan& sp, BgzfSpanResult* r, F&& on_member) {
    *r = BgzfSpanResult{0, 0, 0, 0, kBgzfOk, 0, 0};
    uint64_t cur = sp.head, last_off = 0;
    uint32_t last_bsize = 0;
    for (;;) {
        if (cur > sp.stop) { r->kind = kBgzfStepOver; r->value = last_bsize; r->fail_off = last_off; r->count--; return ZWZ_OK; }
        if (cur == sp.stop && (!sp.limit || cur >= fh.fsize)) return ZWZ_OK;
        BgzfMember m;
        if (int rc = fh.parse(cur, &m)) return rc;
        if (m.kind != kBgzfOk) { r->kind = m.kind; r->value = m.value; r->fail_off = cur; return ZWZ_OK; }
        on_member(cur, m.isize);
        r->count++; r->sum += m.isize;
        if (cur == sp.stop) return ZWZ_OK;
        last_bsize = m.bsize; last_off = cur;
        cur += m.bsize;
    }
}

int chunk_prepare_file(const char* src, const uint64_t* chunks, uint32_t k, uint64_t* sizes, ChunkJob* J) {
    J->ix.coff.clear(); J->ix.uoff.clear(); J->ranges.clear();
    FileHeaders fw;
    fw.fd = open(src, O_RDONLY);
    if (fw.fd < 0) { set_error("cannot open %s", src); return ZWZ_E_IO; }
    struct stat stt {};
    if (fstat(fw.fd, &stt) != 0) { close(fw.fd); set_error("cannot stat %s", src); return ZWZ_E_IO; }
    fw.fsize = (uint64_t)stt.st_size;
    ChunkSpans S;
    if (int rc = chunk_spans(chunks, k, fw.fsize, &S)) { close(fw.fd); return rc; }
    std::vector<BgzfSpanResult> res(S.spans.size());
    std::vector<size_t> span_end(S.spans.size());
    std::vector<uint32_t> isize;
    uint64_t total = 0;
    for (size_t s = 0; s < S.spans.size(); s++) {
        const int rc = walk_file_span(fw, S.spans[s], &res[s], [&](uint64_t o, uint32_t isz) {
            J->ix.coff.push_back(o); J->ix.uoff.push_back(total); isize.push_back(isz);
            total += isz;
        });
        if (rc) { close(fw.fd); return rc; }
        if (res[s].kind == kBgzfStepOver) { J->ix.coff.pop_back(); J->ix.uoff.pop_back(); total -= isize.back(); isize.pop_back(); }
        span_end[s] = J->ix.coff.size();
    }
    close(fw.fd);
    if (int rc = chunk_walk_verdict(S, res.data(), chunks, k)) return rc;
    return chunk_ranges(S, span_end, J->ix, isize, total, chunks, k, &J->ranges, sizes);
}

// sum of sizes against a capacity (the sizes are set either way)
int chunk_room(const uint64_t* sizes, uint32_t k, uint64_t cap, const char* who) {
    uint64_t total = 0;
    for (uint32_t i = 0; i < k; i++) total += sizes[i];
    if (total <= cap) return ZWZ_OK;
    set_error("%s: the chunks decode to %llu bytes, room for %llu", who, (unsigned long long)total, (unsigned long long)cap);
    return ZWZ_E_INVALID;
}

}  // namespace

extern "C" {

uint64_t zwz_bgzf_bound(uint64_t n) { return (n + kBgzfBlock - 1) / kBgzfBlock * kMemberMax + kBgzfEofBytes; }

int zwz_bgzf_compress_dev(zwz_ctx* c, const uint8_t* d_in, uint64_t n, uint8_t* d_out, uint64_t out_cap, uint64_t* d_out_len) {
    if (!c || !d_out || !d_out_len || (n && !d_in) || ((uintptr_t)d_in & 15u)) return ZWZ_E_INVALID;
    if (out_cap < zwz_bgzf_bound(n)) { set_error("zwz_bgzf_compress_dev: out_cap %llu below zwz_bgzf_bound(%llu)", (unsigned long long)out_cap, (unsigned long long)n); return ZWZ_E_INVALID; }
    HIPCHK(hipSetDevice(c->device));
    return compress_launch(c, d_in, n, d_out, d_out_len, 1);
}

int zwz_bgzf_index(const uint8_t* gz, uint64_t n, uint64_t* member_off, uint32_t cap, uint32_t* n_members, uint64_t* raw_len) {
    if ((n && !gz) || !n_members || !raw_len) return ZWZ_E_INVALID;
    uint64_t count = 0, raw = 0, used = 0;
    const int rc = bgzf_walk(gz, n, 0, false, ~0ull, member_off, member_off ? cap : 0, &count, &raw, &used);
    if (count > 0xffffffffull) { set_error("bgzf: more than 2^32 - 1 members"); return ZWZ_E_INVALID; }
    *n_members = (uint32_t)count;
    *raw_len = raw;
    if (rc) return rc;
    if (member_off && count > cap) { set_error("zwz_bgzf_index: %llu members, room for %u", (unsigned long long)count, cap); return ZWZ_E_INVALID; }
    return ZWZ_OK;
}

int zwz_bgzf_decompress_dev(zwz_ctx* c, const uint8_t* d_gz, uint64_t gz_len, const uint64_t* d_member_off, uint32_t n_members, uint8_t* d_out,
                            uint64_t* d_out_len, uint32_t* d_status) {
    if (!c || !d_out_len || (n_members && (!d_gz || !d_member_off || !d_out || !d_status)) || ((uintptr_t)d_gz & 15u)) return ZWZ_E_INVALID;
    HIPCHK(hipSetDevice(c->device));
    return decompress_launch(c, d_gz, gz_len, d_member_off, n_members, d_out, d_out_len, d_status);
}

// run_slices' loop (zwz_filejob.h) over slices of whole blocks: the members of a slice, and the EOF member behind the last.
int zwz_bgzf_compress_file(zwz_ctx* c, const char* src, const char* dst) {
    if (!c || !src || !dst) return ZWZ_E_INVALID;
    HIPCHK(hipSetDevice(c->device));
    FileJob job;
    if (int rc = job.open(src, dst)) return rc;
    const uint32_t blocks = c->max_batch < kFileSliceBlocks ? c->max_batch : kFileSliceBlocks;
    const size_t S = (size_t)blocks * kBgzfBlock, O = zwz_bgzf_bound(S);
    if (int rc = job.alloc({S + 16, S + 16, O, O, 64}, {S + 16, O, 64})) return rc;
    const int rc = run_slices(c, job, S,
        [&](size_t n, SliceResult* d_res, SliceResult* h_res) {
            if (int rc = compress_launch(c, job.dp(0), n, job.dp(1), &d_res->out_len, 0)) return rc;
            HIPCHK(hipMemcpyAsync(&h_res->out_len, &d_res->out_len, 8, hipMemcpyDeviceToHost, c->stream));
            return (int)ZWZ_OK;
        },
        [&](size_t, const SliceResult& r) {
            if (r.out_len > O) { set_error("bgzf: a member body reached the deflate slot's length"); return (int)ZWZ_E_FORMAT; }
            return (int)ZWZ_OK;
        });
    if (rc) return rc;
    if (fwrite(kBgzfEof, 1, kBgzfEofBytes, job.out) != kBgzfEofBytes) { set_error("write error on %s", job.part.c_str()); return ZWZ_E_IO; }
    return job.commit(dst);
}

// Slices of at most kFileSliceBlocks whole members: the walk stops before a member the buffer does not hold in full, and those bytes
// open the next buffer, which the reader then fills up.
int zwz_bgzf_decompress_file(zwz_ctx* c, const char* src, const char* dst) {
    if (!c || !src || !dst) return ZWZ_E_INVALID;
    HIPCHK(hipSetDevice(c->device));
    FileJob job;
    if (int rc = job.open(src, dst)) return rc;
    const uint32_t blocks = c->max_batch < kFileSliceBlocks ? c->max_batch : kFileSliceBlocks;
    const size_t B = (size_t)blocks * kBgzfSlot, R = (size_t)blocks * kBgzfMaxIsize;   // a member is at most 65536 bytes
    const size_t small = (size_t)blocks * (8 + 4) + 64;
    if (int rc = job.alloc({B, B, R + 16, R + 16, small}, {B + 16, R + 16, small})) return rc;
    uint8_t* d_gz = static_cast<uint8_t*>(job.d[0]); uint8_t* d_out = static_cast<uint8_t*>(job.d[1]);
    uint64_t* d_len = static_cast<uint64_t*>(job.d[2]); uint64_t* d_moff = d_len + 1; uint32_t* d_st = reinterpret_cast<uint32_t*>(d_moff + blocks);
    uint64_t* h_moff = static_cast<uint64_t*>(job.h[4]); uint32_t* h_st = reinterpret_cast<uint32_t*>(h_moff + blocks);
    size_t have = 0;
    job.start_read(static_cast<uint8_t*>(job.h[0]), B);
    if (int rc = job.finish_read(&have)) return rc;
    bool eof = have < B;
    uint64_t at = 0, member0 = 0;
    for (int b = 0;; b ^= 1) {
        uint8_t* hin = static_cast<uint8_t*>(job.h[b]);
        uint8_t* hout = static_cast<uint8_t*>(job.h[2 + b]);
        uint64_t count = 0, raw = 0, used = 0;
        if (int rc = bgzf_walk(hin, have, at, !eof, blocks, h_moff, blocks, &count, &raw, &used)) { job.join(); return rc; }
        if (!count) {
            if (!have) break;
            // nothing whole in a full buffer cannot happen (a member fits it); at the end of the file: the strict walk names the damage
            uint64_t k2, r2, u2;
            const int rc = bgzf_walk(hin, have, at, false, ~0ull, nullptr, 0, &k2, &r2, &u2);
            job.join();
            if (rc) return rc;
            set_error("bgzf: cannot split the input at byte offset %llu", (unsigned long long)at);
            return ZWZ_E_FORMAT;
        }
        HIPJOB(hipMemcpyAsync(d_gz, hin, used, hipMemcpyHostToDevice, c->stream));
        HIPJOB(hipMemcpyAsync(d_moff, h_moff, count * 8, hipMemcpyHostToDevice, c->stream));
        if (int rc = decompress_launch(c, d_gz, used, d_moff, (uint32_t)count, d_out, d_len, d_st)) { job.join(); return rc; }
        HIPJOB(hipMemcpyAsync(hout, d_out, raw, hipMemcpyDeviceToHost, c->stream));
        HIPJOB(hipMemcpyAsync(h_st, d_st, count * 4, hipMemcpyDeviceToHost, c->stream));
        // the rest of this buffer opens the next one, which the reader fills while the GPU works
        const size_t carry = have - used;
        uint8_t* next = static_cast<uint8_t*>(job.h[b ^ 1]);
        memcpy(next, hin + used, carry);
        if (!eof) job.start_read(next + carry, B - carry);
        HIPJOB(hipStreamSynchronize(c->stream));
        if (int rc = check_status(h_st, (uint32_t)count, h_moff, at, member0)) { job.join(); return rc; }
        if (int rc = job.finish_write()) { job.join(); return rc; }
        job.start_write(hout, raw);
        size_t got = 0;
        if (!eof) { if (int rc = job.finish_read(&got)) { job.join(); return rc; } eof = carry + got < B; }
        have = carry + got;
        at += used;
        member0 += count;
    }
    return job.commit(dst);
}

int zwz_bgzf_gzi(const uint8_t* gz, uint64_t n, uint8_t* gzi, uint64_t cap, uint64_t* gzi_len) {
    if ((n && !gz) || !gzi_len) return ZWZ_E_INVALID;
    *gzi_len = 0;
    GziBuilder b;
    uint64_t count = 0, raw = 0, used = 0;
    if (int rc = bgzf_walk_each(gz, n, 0, 0, false, ~0ull, [&](uint64_t, uint64_t o, uint32_t isize) { b.member(o, isize); }, &count, &raw, &used))
        return rc;
    b.finish();
    *gzi_len = 8 + b.buf.size();
    if (!gzi) return ZWZ_OK;
    if (cap < *gzi_len) { set_error("zwz_bgzf_gzi: %llu bytes, room for %llu", (unsigned long long)*gzi_len, (unsigned long long)cap); return ZWZ_E_INVALID; }
    put64(gzi, b.entries);
    if (!b.buf.empty()) memcpy(gzi + 8, b.buf.data(), b.buf.size());
    return ZWZ_OK;
}

int zwz_bgzf_gzi_file(const char* src, const char* dst_gzi) {
    if (!src || !dst_gzi) return ZWZ_E_INVALID;
    FileJob job;
    if (int rc = job.open(src, dst_gzi)) return rc;
    GziBuilder b;
    bool werr = fwrite("\0\0\0\0\0\0\0\0", 1, 8, job.out) != 8;          // the count, rewritten at the end
    auto flush = [&] { if (!b.buf.empty() && fwrite(b.buf.data(), 1, b.buf.size(), job.out) != b.buf.size()) werr = true; b.buf.clear(); };
    const int rc = walk_file(job.in, [&](uint64_t o, uint32_t isize) { b.member(o, isize); if (b.buf.size() >= (1u << 20)) flush(); },
                             [] { return false; });
    if (rc) return rc;
    b.finish();
    flush();
    uint8_t cnt[8];
    put64(cnt, b.entries);
    if (werr || fseek(job.out, 0, SEEK_SET) != 0 || fwrite(cnt, 1, 8, job.out) != 8) { set_error("write error on %s", job.part.c_str()); return ZWZ_E_IO; }
    return job.commit(dst_gzi);
}

int zwz_bgzf_read_ranges_dev(zwz_ctx* c, const uint8_t* d_gz, uint64_t gz_len, const uint8_t* gzi, uint64_t gzi_len, const uint64_t* ranges, uint32_t k,
                             uint8_t* d_out) {
    if (!c || (k && !ranges) || (gzi_len && !gzi) || (gz_len && !d_gz) || ((uintptr_t)d_gz & 15u)) return ZWZ_E_INVALID;
    GziIndex ix;
    if (int rc = parse_gzi(gzi, gzi_len, &ix)) return rc;
    RangePlan P;
    if (int rc = plan_ranges(ix, ranges, k, &P)) return rc;
    if (P.total && !d_out) return ZWZ_E_INVALID;
    return run_plan_dev(c, ix, P, ranges, d_gz, gz_len, d_out);
}

// Touched members are read with one pread per run of consecutive index entries, into pinned staging of at most kFileSliceBlocks
// members; each slice of members (and at most kRangeOutSlice decoded bytes) runs through the device path and its pieces are copied
// to their places in out.
int zwz_bgzf_read_ranges_file(zwz_ctx* c, const char* src, const char* gzi_path, const uint64_t* ranges, uint32_t k, uint8_t* out) {
    if (!c || !src || (k && !ranges)) return ZWZ_E_INVALID;
    GziIndex ix;
    if (gzi_path) {
        std::vector<uint8_t> g;
        if (int rc = read_file_bytes(gzi_path, &g)) return rc;
        if (int rc = parse_gzi(g.data(), g.size(), &ix)) return rc;
    } else {
        // the index of the members up to the last requested byte, from a walk of the headers
        uint64_t need = 0;
        for (uint32_t r = 0; r < k; r++) need = std::max(need, ranges[2 * r] + std::min<uint64_t>(ranges[2 * r + 1], ~0ull - ranges[2 * r]));
        FILE* f = fopen(src, "rb");
        if (!f) { set_error("cannot open %s", src); return ZWZ_E_IO; }
        uint64_t raw = 0;
        const int rc = walk_file(f, [&](uint64_t o, uint32_t isize) { ix.coff.push_back(o); ix.uoff.push_back(raw); raw += isize; },
                                 [&] { return raw > need; });
        fclose(f);
        if (rc) return rc;
    }
    RangePlan P;
    if (int rc = plan_ranges(ix, ranges, k, &P)) return rc;
    if (P.total && !out) return ZWZ_E_INVALID;
    return run_plan_file(c, src, ix, P, ranges, out);
}

int zwz_bgzf_index_dev(zwz_ctx* c, const uint8_t* d_gz, uint64_t gz_len, uint64_t* d_member_off, uint32_t cap, uint32_t* n_members, uint64_t* raw_len) {
    if (!c || (gz_len && !d_gz) || !n_members || !raw_len || ((uintptr_t)d_gz & 15u)) return ZWZ_E_INVALID;
    BgzfWalk W;
    BgzfSpanResult r;
    if (int rc = walk_whole_dev(c, d_gz, gz_len, &W, &r)) return rc;
    *n_members = r.count;
    *raw_len = r.sum;
    const uint32_t give = d_member_off ? std::min(cap, r.count) : 0u;
    if (give) {
        HIPCHK(hipMemcpyAsync(d_member_off, W.d_moff + r.first, 8 * (size_t)give, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    if (r.kind != kBgzfOk) return walk_failure(r.kind, r.count, r.fail_off, r.value);
    if (d_member_off && r.count > cap) { set_error("zwz_bgzf_index: %llu members, room for %u", (unsigned long long)r.count, cap); return ZWZ_E_INVALID; }
    return ZWZ_OK;
}

int zwz_bgzf_gzi_dev(zwz_ctx* c, const uint8_t* d_gz, uint64_t gz_len, uint8_t* gzi, uint64_t cap, uint64_t* gzi_len) {
    if (!c || (gz_len && !d_gz) || !gzi_len || ((uintptr_t)d_gz & 15u)) return ZWZ_E_INVALID;
    *gzi_len = 0;
    BgzfWalk W;
    BgzfSpanResult r;
    if (int rc = walk_whole_dev(c, d_gz, gz_len, &W, &r)) return rc;
    if (r.kind != kBgzfOk) return walk_failure(r.kind, r.count, r.fail_off, r.value);
    std::vector<uint64_t> off(r.count);
    std::vector<uint32_t> isz(r.count);
    if (int rc = walk_members_host(c, W, r.first, r.count, off.data(), isz.data())) return rc;
    GziBuilder b;
    for (uint32_t j = 0; j < r.count; j++) b.member(off[j], isz[j]);
    b.finish();
    *gzi_len = 8 + b.buf.size();
    if (!gzi) return ZWZ_OK;
    if (cap < *gzi_len) { set_error("zwz_bgzf_gzi: %llu bytes, room for %llu", (unsigned long long)*gzi_len, (unsigned long long)cap); return ZWZ_E_INVALID; }
    put64(gzi, b.entries);
    if (!b.buf.empty()) memcpy(gzi + 8, b.buf.data(), b.buf.size());
    return ZWZ_OK;
}

int zwz_bgzf_voffsets(const uint8_t* gzi, uint64_t gzi_len, const uint64_t* offsets, uint32_t k, uint64_t* voffsets) {
    if ((k && (!offsets || !voffsets)) || (gzi_len && !gzi)) return ZWZ_E_INVALID;
    GziIndex ix;
    if (int rc = parse_gzi(gzi, gzi_len, &ix)) return rc;
    for (uint32_t i = 0; i < k; i++) {
        const uint64_t a = offsets[i];
        const size_t j = std::upper_bound(ix.uoff.begin(), ix.uoff.end(), a) - ix.uoff.begin() - 1;
        const uint64_t within = a - ix.uoff[j];
        if (ix.coff[j] >= kBgzfVoffMaxCoff) {
            set_error("bgzf: offset %u (%llu): its member starts at byte offset %llu, at or above 2^48", i, (unsigned long long)a, (unsigned long long)ix.coff[j]);
            return ZWZ_E_INVALID;
        }
        if (within >= 65536u) {
            set_error("bgzf: offset %u (%llu) lies %llu bytes past the index entry below it: more than a block holds", i, (unsigned long long)a,
                      (unsigned long long)within);
            return ZWZ_E_INVALID;
        }
        voffsets[i] = bgzf_voffset(ix.coff[j], (uint32_t)within);
    }
    return ZWZ_OK;
}

int zwz_bgzf_chunk_sizes_dev(zwz_ctx* c, const uint8_t* d_gz, uint64_t gz_len, const uint64_t* chunks, uint32_t k, uint64_t* sizes) {
    if (!c || (k && (!chunks || !sizes)) || (gz_len && !d_gz) || ((uintptr_t)d_gz & 15u)) return ZWZ_E_INVALID;
    ChunkJob J;
    return chunk_prepare_dev(c, d_gz, gz_len, chunks, k, sizes, &J);
}

int zwz_bgzf_read_chunks_dev(zwz_ctx* c, const uint8_t* d_gz, uint64_t gz_len, const uint64_t* chunks, uint32_t k, uint8_t* d_out, uint64_t out_cap,
                             uint64_t* sizes) {
    if (!c || (k && (!chunks || !sizes)) || (gz_len && !d_gz) || ((uintptr_t)d_gz & 15u)) return ZWZ_E_INVALID;
    ChunkJob J;
    if (int rc = chunk_prepare_dev(c, d_gz, gz_len, chunks, k, sizes, &J)) return rc;
    if (int rc = chunk_room(sizes, k, out_cap, "zwz_bgzf_read_chunks_dev")) return rc;
    if (!k) return ZWZ_OK;
    RangePlan P;
    if (int rc = plan_ranges(J.ix, J.ranges.data(), k, &P)) return rc;
    if (P.total && !d_out) return ZWZ_E_INVALID;
    return run_plan_dev(c, J.ix, P, J.ranges.data(), d_gz, gz_len, d_out);
}

int zwz_bgzf_chunk_sizes_file(const char* src, const uint64_t* chunks, uint32_t k, uint64_t* sizes) {
    if (!src || (k && (!chunks || !sizes))) return ZWZ_E_INVALID;
    ChunkJob J;
    return chunk_prepare_file(src, chunks, k, sizes, &J);
}

int zwz_bgzf_read_chunks_file(zwz_ctx* c, const char* src, const uint64_t* chunks, uint32_t k, uint8_t* out, uint64_t out_cap, uint64_t* sizes) {
    if (!c || !src || (k && (!chunks || !sizes))) return ZWZ_E_INVALID;
    ChunkJob J;
    if (int rc = chunk_prepare_file(src, chunks, k, sizes, &J)) return rc;
    if (int rc = chunk_room(sizes, k, out_cap, "zwz_bgzf_read_chunks_file")) return rc;
    if (!k) return ZWZ_OK;
    RangePlan P;
    if (int rc = plan_ranges(J.ix, J.ranges.data(), k, &P)) return rc;
    if (P.total && !out) return ZWZ_E_INVALID;
    return run_plan_file(c, src, J.ix, P, J.ranges.data(), out);
}

}  // extern "C"
