// zwz_index.cpp -- the seek index for ordinary DEFLATE streams of include/zwz.h: zwz_inflate_streams_index_dev (one decode that also
// writes the index), zwz_inflate_indexed_batch_dev (streams decoded whole, a wave per indexed segment, all of them in one launch; 
// zwz_inflate_indexed_dev is a batch of one) and zwz_inflate_read_ranges_batch_dev (only the segments a batch of ranges touches, across
// streams; zwz_inflate_read_ranges_dev is its one-stream form), and their file forms: zwz_inflate_index_file, zwz_inflate_read_ranges_file (a pread of
// the touched segments only) and zwz_inflate_stream_file_indexed (slices of consecutive index entries, zwz_filejob.h's writer).
// index_core.h has the layout, the checks and the planning; the kernels are
// inflate_kernel's marking and indexed-segment forms (zwz_kernels.hip) and zwz_index.hip.
#include <algorithm>
#include <atomic>
#include <cstring>
#include <thread>
#include <vector>

#include "dstream_core.h"
#include "zwz_api_internal.h"
#include <fcntl.h>
#include <sys/stat.h>
#include <string>

#include "zwz_bgzf.h"
#include "zwz_filejob.h"
#include "zwz_index.h"

using namespace zwz;

namespace {

constexpr uint64_t kIdxWorkspaceBytes = 256ull << 20;     // scratch slots of one slice of a range read (a longer segment is a slice of its own)
constexpr uint64_t kIdxSegMaxOut = 0xffff0000ull;         // origin + hist + count of one segment stay 32-bit positions

// The arrays of one call.  The first `upload` bytes are filled on the host (the pinned twin has the same layout) and copied; the
// `flag_bytes` from `bad` on, the verdict words, are cleared.
struct CallArrays {
    uint64_t *in_off, *in_len; uint4 *seg, *seg2; IndexMove* mv;
    uint64_t* slot_off; uint32_t *row, *nlong; RangePiece* pieces; IndexStream* rec;
    size_t upload;
    uint4* order; uint32_t *bad, *flag; size_t flag_bytes; uint64_t* piece_off; uint32_t *piece_len, *piece_val;
};
// ns segments, np pieces of ranges, nc checksum pieces, nr streams of a whole decode, nb words a segment wave reports through
CallArrays call_layout(Carver& w, size_t ns, size_t np, size_t nc, size_t nr, size_t nb) {
    CallArrays A;
    A.in_off = w.take<uint64_t>(ns); A.in_len = w.take<uint64_t>(ns); A.seg = w.take<uint4>(ns); A.seg2 = w.take<uint4>(ns); A.mv = w.take<IndexMove>(ns);
    A.slot_off = w.take<uint64_t>(ns); A.row = w.take<uint32_t>(ns + 1); A.nlong = w.take<uint32_t>(ns); A.pieces = w.take<RangePiece>(np);
    A.rec = w.take<IndexStream>(nr);
    A.upload = w.used;
    A.order = w.take<uint4>(ns);
    const size_t flags = w.used;
    A.bad = w.take<uint32_t>(nb + 1); A.flag = w.take<uint32_t>(nr + 1);
    A.flag_bytes = w.used - flags;
    A.piece_off = w.take<uint64_t>(nc); A.piece_len = w.take<uint32_t>(nc); A.piece_val = w.take<uint32_t>(nc);
    return A;
}

struct Parsed { IndexView v; std::vector<uint64_t> woff; };      // woff[k]: where entry k's window starts in the index

// The streams and the indexes of one call: stream i is in_len[i] bytes at d_in + in_off[i], its index idx_len[i] bytes at idx +
// idx_off[i] and, with d_idx, at d_idx + idx_off[i] (host arrays of n).  named: a batch call, whose messages say which stream.
struct Batch {
    const uint8_t* d_in; const uint64_t *in_off, *in_len; uint32_t n;
    const uint8_t* idx; const uint64_t *idx_off, *idx_len; const uint8_t* d_idx;
    bool named;
};
const uint64_t kZero = 0;            // the offsets of a call of one stream

constexpr uint64_t kParseAloneBytes = 1u << 20;     // indexes of fewer bytes in all are checked by the calling thread
constexpr unsigned kParseThreads = 16;

// The indexes of the streams of `want` (null: of all) checked and parsed, on up to 16 threads: index_parse reads every byte for the index CRC.
int parse_indexes(const Batch& B, const std::vector<uint8_t>* want, std::vector<Parsed>* P, const char* who) {
    P->resize(B.n);
    std::vector<uint32_t> todo, fault(B.n, kIdxOk);
    uint64_t bytes = 0;
    for (uint32_t i = 0; i < B.n; i++) if (!want || (*want)[i]) { todo.push_back(i); bytes += B.idx_len[i]; }
    auto one = [&](uint32_t i) {
        Parsed& q = (*P)[i];
        fault[i] = index_parse(B.idx + B.idx_off[i], B.idx_len[i], &q.v);
        if (fault[i] != kIdxOk) return;
        q.woff.resize(q.v.count);
        uint64_t at = q.v.win_off;
        for (uint32_t k = 0; k < q.v.count; k++) { q.woff[k] = at; at += q.v.entry(k).hist; }
    };
    const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    const unsigned nt = bytes < kParseAloneBytes ? 1u : (unsigned)std::min<size_t>(todo.size(), std::min(hw, kParseThreads));
    if (nt <= 1) for (uint32_t i : todo) one(i);
    else {
        std::atomic<size_t> next{0};
        auto work = [&] { for (size_t t; (t = next.fetch_add(1)) < todo.size();) one(todo[t]); };
        std::vector<std::thread> pool;
        for (unsigned t = 1; t < nt; t++) pool.emplace_back(work);
        work();
        for (std::thread& t : pool) t.join();
    }
    for (uint32_t i : todo)
        if (fault[i] != kIdxOk) {
            if (B.named) set_error("%s: stream %u: the index is malformed: %s", who, i, index_fault_name(fault[i]));
            else set_error("%s: the index is malformed: %s", who, index_fault_name(fault[i]));
            return ZWZ_E_FORMAT;
        }
    return ZWZ_OK;
}

int parse_index(const uint8_t* idx, uint64_t idx_len, std::vector<Parsed>* P, const char* who) {
    return parse_indexes(Batch{nullptr, &kZero, nullptr, 1, idx, &kZero, &idx_len, nullptr, false}, nullptr, P, who);
}

// Whether segment k is within the kernel's 32-bit positions
bool segment_fits(const IndexView& v, uint32_t k) {
    const IndexEntry e = v.entry(k);
    const uint64_t count = v.seg_end_off(k) - e.off, base = (e.bit >> 3) & ~15ull, len = ((v.seg_end_bit(k) + 7u) >> 3) - base;
    return len < kStreamMaxIn && count + e.hist + 16u <= kIdxSegMaxOut;
}

// Segment k's records at slot j of the call's arrays.  a: the address in the call's output buffer of the byte hist in front of the
// segment's first; in_at: where its stream starts in the call's input (remap: where its own input does); win_at: where its index starts
// in the index buffer; word: which word of `bad` it reports through; stream: whose flag its window sets.
void fill_segment(const Parsed& P, uint32_t k, uint64_t a, size_t j, CallArrays& H, uint32_t* n_moves, uint64_t in_at, const uint64_t* remap, uint64_t win_at,
                  uint32_t word, uint32_t stream) {
    const IndexView& v = P.v;
    const IndexEntry e = v.entry(k);
    const uint64_t end_bit = v.seg_end_bit(k), count = v.seg_end_off(k) - e.off;
    const uint64_t base = (e.bit >> 3) & ~15ull, len = ((end_bit + 7u) >> 3) - base;
    H.in_off[j] = remap ? *remap : in_at + base; H.in_len[j] = len;
    H.seg[j] = make_uint4((uint32_t)((e.bit >> 3) & 15u) | (uint32_t)(e.bit & 7u) << 4 | (k + 1u == v.count ? 128u : 0u), word, (uint32_t)count, e.hist);
    H.seg2[j] = make_uint4((uint32_t)a, (uint32_t)(a >> 32), (uint32_t)(end_bit - base * 8u), 0u);
    if (e.hist) H.mv[(*n_moves)++] = IndexMove{win_at + P.woff[k], a, e.hist, stream};
}

// Both layouts of a call: the device arrays D and their pinned twin H (waits for the stream: an earlier call's copies may still read H)
int reserve_call(zwz_ctx* c, size_t ns, size_t np, size_t nc, size_t nr, size_t nb, CallArrays* D, CallArrays* H) {
    const size_t bytes = layout_bytes([&](Carver& w) { call_layout(w, ns, np, nc, nr, nb); });
    if (int rc = c->buf[kBufIndex0].reserve(c, 0, bytes)) return rc;
    if (int rc = c->buf[kBufIndexHost].reserve(c, 0, bytes)) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));
    Carver wd(c->buf[kBufIndex0].p), wh(c->buf[kBufIndexHost].p);
    *D = call_layout(wd, ns, np, nc, nr, nb); *H = call_layout(wh, ns, np, nc, nr, nb);
    return ZWZ_OK;
}

// Whole decodes: every stream of B into d_out + out_off[i], the segments of all of them in one launch, their windows placed and
// compared, their checksum pieces summed and their verdicts given by one launch each (zwz_index.hip).
int indexed_core(zwz_ctx* c, const Batch& B, uint8_t* d_out, const uint64_t* out_off, const uint64_t* out_cap, uint64_t* d_out_len, uint32_t* d_status,
                 uint32_t* d_segments, const char* who) {
    const uint32_t n = B.n;
    std::vector<Parsed> P;
    if (int rc = parse_indexes(B, nullptr, &P, who)) return rc;
    // d_out + out_off[i] may be any byte: the waves' positions count from `al`, the 16-byte boundary at or in front of d_out, and a
    // stream's first checksum piece is its bytes up to the next one
    const uint32_t shift = (uint32_t)((uintptr_t)d_out & 15u);
    uint8_t* al = d_out - shift;
    // the verdicts that need no GPU work, and what the others take
    std::vector<IndexStream> R(n);
    uint64_t ns = 0, ng = 0, na = 0;
    for (uint32_t i = 0; i < n; i++) {
        const IndexView& v = P[i].v;
        IndexStream& r = R[i];
        r = IndexStream{B.in_off[i], B.in_len[i], (v.end_bit + 7u) >> 3, out_off[i], 0, index_head_bytes((uint32_t)((shift + out_off[i]) & 15u), v.decoded_len),
                        v.wrap, v.check, 0, 0, 0, 0, 0};
        const uint64_t nc = index_piece_count(v.wrap, r.head, v.decoded_len);
        if (out_cap[i] < v.decoded_len) r.refused = kInfOverflow;
        else if (B.in_len[i] != v.stream_len) r.refused = kStrIndex;
        else if (nc > 0xffffffffull) r.refused = kStrTooLarge;
        else for (uint32_t k = 0; k < v.count && !r.refused; k++) if (!segment_fits(v, k)) r.refused = kStrTooLarge;
        if (r.refused) continue;
        r.total = v.decoded_len; r.nseg = v.count; r.pieces = (uint32_t)nc;
        ns += v.count; (v.wrap == kWrapGzip ? ng : na) += nc;
    }
    if (ns > 0xffffffffull || ng + na > 0xffffffffull) { set_error("%s: more than 2^32 - 1 segments or checksum pieces in one call", who); return ZWZ_E_INVALID; }
    CallArrays D, H;
    if (int rc = reserve_call(c, (size_t)ns, 0, (size_t)(ng + na), n, n, &D, &H)) return rc;
    uint32_t n_moves = 0, j = 0, at_g = 0, at_a = (uint32_t)ng;           // (the CRC-32 pieces first, then the Adler-32 ones)
    uint64_t idx_end = 0;
    for (uint32_t i = 0; i < n; i++) {
        IndexStream& r = R[i];
        if (!r.refused) {
            uint32_t& at = r.wrap == kWrapGzip ? at_g : at_a;
            r.piece0 = at; at += r.pieces;
            for (uint32_t k = 0; k < r.nseg; k++, j++) {
                const IndexEntry e = P[i].v.entry(k);
                fill_segment(P[i], k, shift + out_off[i] + e.off - e.hist, j, H, &n_moves, B.in_off[i], nullptr, B.idx_off[i], i, i);
            }
            idx_end = std::max(idx_end, B.idx_off[i] + B.idx_len[i]);
        }
        H.rec[i] = r;
    }
    hipStream_t st = c->stream;
    const uint8_t* d_idx = B.d_idx;
    if (!d_idx) {
        if (int rc = c->buf[kBufIndex1].reserve(c, 0, (size_t)idx_end + 16)) return rc;
        uint8_t* up = c->buf[kBufIndex1].as<uint8_t>();
        for (uint32_t i = 0; i < n; i++)
            if (!R[i].refused) HIPCHK(hipMemcpyAsync(up + B.idx_off[i], B.idx + B.idx_off[i], (size_t)B.idx_len[i], hipMemcpyHostToDevice, st));
        d_idx = up;
    }
    if (ng) if (int rc = ensure_crc_tables(c)) return rc;
    HIPCHK(hipMemcpyAsync(D.in_off, H.in_off, H.upload, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(D.bad, 0, D.flag_bytes, st));
    HIPCHK(launch_index_place(d_idx, al, D.mv, n_moves, st));
    HIPCHK(launch_inflate_indexed(InflateIndexedArgs{B.d_in, D.in_off, D.in_len, (uint32_t)ns, al, D.order, D.seg, D.seg2, D.bad, c->inflate_serial_header}, st));
    HIPCHK(launch_index_compare(d_idx, al, D.mv, n_moves, D.flag, st));
    const IndexBatch f{B.d_in, d_out, D.rec, n, D.piece_off, D.piece_len, D.piece_val, (uint32_t)(ng + na), (uint32_t)ng, D.bad, D.flag, d_out_len, d_status, d_segments};
    HIPCHK(launch_index_batch_finish(c->buf[kBufCrcTables].as<const CrcTables>(), f, c->cu_count, st));
    return ZWZ_OK;
}

}  // namespace

extern "C" uint64_t zwz_inflate_index_bound(uint64_t decoded_cap, uint32_t span) {
    if (span == 0) span = kIdxSpanDefault;
    return index_span_ok(span) ? index_bound(decoded_cap, span) : 0u;
}

extern "C" int zwz_inflate_streams_index_dev(zwz_ctx* c, int wrap, const uint8_t* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len, uint32_t n,
                                             uint8_t* d_out, const uint64_t* d_out_off, const uint64_t* d_out_cap, uint64_t* d_out_len, uint32_t* d_status,
                                             uint32_t span, uint8_t* d_idx, const uint64_t* d_idx_off, const uint64_t* d_idx_cap, uint64_t* d_idx_len) {
    if (!c || wrap < ZWZ_WRAP_RAW || wrap > ZWZ_WRAP_GZIP) return ZWZ_E_INVALID;
    if (span == 0) span = c->index_span_bytes;
    if (!index_span_ok(span)) return ZWZ_E_INVALID;
    if (n && (!d_in || !d_in_off || !d_in_len || !d_out || !d_out_off || !d_out_cap || !d_out_len || !d_status || !d_idx || !d_idx_off || !d_idx_cap || !d_idx_len))
        return ZWZ_E_INVALID;
    if (((uintptr_t)d_in & 15u) || ((uintptr_t)d_out & 15u) || ((uintptr_t)d_idx & 15u)) return ZWZ_E_INVALID;
    if (n == 0) return ZWZ_OK;
    HIPCHK(hipSetDevice(c->device));
    if (int rc = ensure_inf_order(c, n)) return rc;
    if (int rc = c->buf[kBufStreamRec].reserve(c, n, (size_t)n * sizeof(uint4))) return rc;
    if (int rc = ensure_crc_tables(c)) return rc;                 // (the index CRC, whatever the wrapper)
    uint4* rec = c->buf[kBufStreamRec].as<uint4>();
    const CrcTables* tab = c->buf[kBufCrcTables].as<const CrcTables>();
    InflateMarkArgs a{{d_in, d_in_off, d_in_len, n, d_out, d_out_off, d_out_cap, d_out_len, d_status, c->buf[kBufInfOrder].as<uint4>(), rec, (uint32_t)wrap,
                       c->inflate_serial_header}, d_idx, d_idx_off, d_idx_cap, d_idx_len, span};
    HIPCHK(launch_inflate_mark(a, c->stream));
    HIPCHK(launch_stream_check(tab, d_out, d_out_off, rec, n, (uint32_t)wrap, d_status, c->cu_count, c->stream));
    HIPCHK(launch_index_windows(tab, IndexBuild{d_out, d_out_off, d_in_len, d_status, n, (uint32_t)wrap, span, d_idx, d_idx_off, d_idx_len}, c->stream));
    return ZWZ_OK;
}

// (a batch of one: its stream, its index and its output at offset 0)
extern "C" int zwz_inflate_indexed_dev(zwz_ctx* c, const uint8_t* d_in, uint64_t in_len, const uint8_t* idx, uint64_t idx_len, const uint8_t* d_idx,
                                       uint8_t* d_out, uint64_t out_cap, uint64_t* d_out_len, uint32_t* d_status, uint32_t* d_segments) {
    if (!c || !d_in || !idx || !d_out || !d_out_len || !d_status) return ZWZ_E_INVALID;
    if (((uintptr_t)d_in & 15u) || ((uintptr_t)d_idx & 15u)) return ZWZ_E_INVALID;
    HIPCHK(hipSetDevice(c->device));
    return indexed_core(c, Batch{d_in, &kZero, &in_len, 1, idx, &kZero, &idx_len, d_idx, false}, d_out, &kZero, &out_cap, d_out_len, d_status, d_segments,
                        "zwz_inflate_indexed_dev");
}

namespace {

// The alignment rules of a batch call's host arrays
bool batch_aligned(const Batch& B) {
    if (((uintptr_t)B.d_in & 15u) || ((uintptr_t)B.d_idx & 15u)) return false;
    for (uint32_t i = 0; i < B.n; i++) if ((B.in_off[i] & 15u) || (B.idx_off[i] & 15u)) return false;
    return true;
}

}  // namespace

extern "C" int zwz_inflate_indexed_batch_dev(zwz_ctx* c, const uint8_t* d_in, const uint64_t* in_off, const uint64_t* in_len, uint32_t n, const uint8_t* idx,
                                             const uint64_t* idx_off, const uint64_t* idx_len, const uint8_t* d_idx, uint8_t* d_out, const uint64_t* out_off,
                                             const uint64_t* out_cap, uint64_t* d_out_len, uint32_t* d_status, uint32_t* d_segments) {
    if (!c) return ZWZ_E_INVALID;
    if (n == 0) return ZWZ_OK;
    if (!d_in || !in_off || !in_len || !idx || !idx_off || !idx_len || !d_out || !out_off || !out_cap || !d_out_len || !d_status) return ZWZ_E_INVALID;
    const Batch B{d_in, in_off, in_len, n, idx, idx_off, idx_len, d_idx, true};
    if (!batch_aligned(B)) return ZWZ_E_INVALID;
    HIPCHK(hipSetDevice(c->device));
    return indexed_core(c, B, d_out, out_off, out_cap, d_out_len, d_status, d_segments, "zwz_inflate_indexed_batch_dev");
}

namespace {

IndexBatchPlan one_stream_plan(IndexPlan&& p) {
    IndexBatchPlan b;
    b.stream.assign(p.segs.size(), 0u);
    b.segs = std::move(p.segs); b.row = std::move(p.row); b.pieces = std::move(p.pieces); b.total = p.total;
    return b;
}

int plan_ranges(const IndexView& v, const uint64_t* ranges, uint32_t k, IndexPlan* plan, const char* who) {
    const int64_t bad_range = index_plan(v, ranges, k, plan);
    if (bad_range >= 0) {
        set_error("%s: range %lld (offset %llu, length %llu) lies past the decoded length %llu", who, (long long)bad_range,
                  (unsigned long long)ranges[2 * bad_range], (unsigned long long)ranges[2 * bad_range + 1], (unsigned long long)v.decoded_len);
        return ZWZ_E_INVALID;
    }
    return ZWZ_OK;
}

// The touched segments of a plan, of whichever streams, decoded into scratch slots, slice by slice, and their pieces dealt to d_out.
// remap: where touched segment i's input starts in B.d_in (a multiple of 16) when that holds only what was read of a file; null: B.d_in
// holds the streams.  Returns synchronised.
int ranges_core(zwz_ctx* c, const Batch& B, const std::vector<Parsed>& P, const IndexBatchPlan& plan, const std::vector<uint64_t>* remap, uint8_t* d_out,
                const char* who) {
    hipStream_t st = c->stream;
    const size_t nt = plan.segs.size();
    for (size_t t = 0; t < nt; t++)
        if (!segment_fits(P[plan.stream[t]].v, plan.segs[t])) {
            if (B.named) set_error("%s: stream %u, segment %u is beyond the limits of one wave", who, plan.stream[t], plan.segs[t]);
            else set_error("%s: segment %u is beyond the limits of one wave", who, plan.segs[t]);
            return ZWZ_E_FORMAT;
        }
    for (size_t s0 = 0; s0 < nt;) {
        // a slice of touched segments whose slots fit the workspace bound
        size_t s1 = s0;
        uint64_t bytes = 0;
        std::vector<uint64_t> slot;
        while (s1 < nt) {
            const IndexView& v = P[plan.stream[s1]].v;
            const IndexEntry e = v.entry(plan.segs[s1]);
            const uint64_t need = round_up((size_t)(e.hist + (v.seg_end_off(plan.segs[s1]) - e.off)), 16) + 16;
            if (s1 > s0 && bytes + need > kIdxWorkspaceBytes) break;
            slot.push_back(bytes); bytes += need; s1++;
        }
        const size_t ns = s1 - s0, np = plan.row[s1] - plan.row[s0];
        CallArrays D, H;
        if (int rc = reserve_call(c, ns, np, 0, 0, ns, &D, &H)) return rc;
        if (int rc = c->buf[kBufIndex1].reserve(c, 0, (size_t)bytes + 16)) return rc;
        uint8_t* slots = c->buf[kBufIndex1].as<uint8_t>();
        uint32_t n_moves = 0;
        for (size_t j = 0; j < ns; j++) {
            const uint32_t si = plan.stream[s0 + j], sk = plan.segs[s0 + j];
            fill_segment(P[si], sk, slot[j], j, H, &n_moves, B.in_off[si], remap ? &(*remap)[s0 + j] : nullptr, B.idx_off[si], (uint32_t)j, 0u);
            H.slot_off[j] = slot[j] + P[si].v.entry(sk).hist;
            // the row's pieces, the long ones first
            const uint32_t r0 = plan.row[s0 + j], r1 = plan.row[s0 + j + 1], b = r0 - plan.row[s0];
            uint32_t at = b, nl = 0;
            for (int pass = 0; pass < 2; pass++)
                for (uint32_t p = r0; p < r1; p++) {
                    const IndexPiece& q = plan.pieces[p];
                    if ((q.len >= kWavePieceMax) == (pass == 0)) { H.pieces[at++] = RangePiece{q.dst, q.off, q.len}; nl += pass == 0; }
                }
            H.row[j] = b; H.nlong[j] = nl;
        }
        H.row[ns] = (uint32_t)np;
        HIPCHK(hipMemcpyAsync(D.in_off, H.in_off, H.upload, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemsetAsync(D.bad, 0, D.flag_bytes, st));
        if (B.d_idx) HIPCHK(launch_index_place(B.d_idx, slots, D.mv, n_moves, st));
        else for (uint32_t i = 0; i < n_moves; i++) HIPCHK(hipMemcpyAsync(slots + H.mv[i].dst, B.idx + H.mv[i].src, H.mv[i].len, hipMemcpyHostToDevice, st));   // the windows this slice needs
        HIPCHK(launch_inflate_indexed(InflateIndexedArgs{B.d_in, D.in_off, D.in_len, (uint32_t)ns, slots, D.order, D.seg, D.seg2, D.bad, c->inflate_serial_header}, st));
        HIPCHK(launch_index_extract(slots, D.slot_off, D.row, D.nlong, D.pieces, (uint32_t)ns, D.bad, d_out, c->cu_count, st));
        std::vector<uint32_t> bad(ns);
        HIPCHK(hipMemcpyAsync(bad.data(), D.bad, ns * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        for (size_t j = 0; j < ns; j++)
            if (bad[j]) {
                const uint32_t si = plan.stream[s0 + j], sk = plan.segs[s0 + j];
                const unsigned long long off = P[si].v.entry(sk).off;
                if (B.named) set_error("%s: stream %u, segment %u (decoded offset %llu) does not decode as indexed", who, si, sk, off);
                else set_error("%s: segment %u (decoded offset %llu) does not decode as indexed", who, sk, off);
                return ZWZ_E_FORMAT;
            }
        s0 = s1;
    }
    return ZWZ_OK;
}

// The compressed bytes of the touched segments of a plan out of a file: one pread per run of consecutive index entries, the runs one
// after the other in `buf` (each from a multiple of 16, zeros behind the last); remap[i] = where touched segment i's input starts.
int pread_touched(int fd, const char* src, const IndexView& v, const IndexPlan& plan, std::vector<uint8_t>* buf, std::vector<uint64_t>* remap) {
    buf->clear(); remap->clear();
    const size_t nt = plan.segs.size();
    for (size_t i = 0; i < nt;) {
        size_t j = i;
        while (j + 1 < nt && plan.segs[j + 1] == plan.segs[j] + 1u) j++;
        const uint64_t first = (v.entry(plan.segs[i]).bit >> 3) & ~15ull, last = (v.seg_end_bit(plan.segs[j]) + 7u) >> 3;
        const size_t at = buf->size();
        buf->resize(at + round_up((size_t)(last - first), 16) + 16, 0);
        for (uint64_t got = 0; got < last - first;) {
            const ssize_t r = pread(fd, buf->data() + at + got, (size_t)(last - first - got), (off_t)(first + got));
            if (r <= 0) { set_error("read error on %s at offset %llu", src, (unsigned long long)(first + got)); return ZWZ_E_IO; }
            got += (uint64_t)r;
        }
        for (size_t t = i; t <= j; t++) remap->push_back(at + (((v.entry(plan.segs[t]).bit >> 3) & ~15ull) - first));
        i = j + 1;
    }
    return ZWZ_OK;
}

int read_whole_file(const char* path, std::vector<uint8_t>* out, size_t slack) {
    FILE* f = fopen(path, "rb");
    if (!f) { set_error("cannot open %s", path); return ZWZ_E_IO; }
    fseeko(f, 0, SEEK_END);
    const off_t n = ftello(f);
    fseeko(f, 0, SEEK_SET);
    out->assign((size_t)n + slack, 0);
    bool err = false;
    const size_t got = read_full(f, out->data(), (size_t)n, &err);
    fclose(f);
    if (err || got != (size_t)n) { set_error("read error on %s", path); return ZWZ_E_IO; }
    out->resize((size_t)n + slack);
    return ZWZ_OK;
}

struct DevMem {          // device memory of one file call
    void* p = nullptr;
    ~DevMem() { if (p) (void)hipFree(p); }
    int get(size_t n) { if (p) { (void)hipFree(p); p = nullptr; } HIPCHK(hipMalloc(&p, n ? n : 16)); return ZWZ_OK; }
    template <class T = uint8_t> T* as() const { return static_cast<T*>(p); }
};

}  // namespace

extern "C" int zwz_inflate_read_ranges_dev(zwz_ctx* c, const uint8_t* d_in, uint64_t in_len, const uint8_t* idx, uint64_t idx_len, const uint8_t* d_idx,
                                           const uint64_t* ranges, uint32_t k, uint8_t* d_out) {
    if (!c || !d_in || !idx || (k && (!ranges || !d_out))) return ZWZ_E_INVALID;
    if (((uintptr_t)d_in & 15u) || ((uintptr_t)d_idx & 15u)) return ZWZ_E_INVALID;
    HIPCHK(hipSetDevice(c->device));
    std::vector<Parsed> P;
    if (int rc = parse_index(idx, idx_len, &P, "zwz_inflate_read_ranges_dev")) return rc;
    const IndexView& v = P[0].v;
    if (in_len != v.stream_len) { set_error("zwz_inflate_read_ranges_dev: the stream has %llu bytes, the index was made for %llu", (unsigned long long)in_len, (unsigned long long)v.stream_len); return ZWZ_E_FORMAT; }
    IndexPlan plan;
    if (int rc = plan_ranges(v, ranges, k, &plan, "zwz_inflate_read_ranges_dev")) return rc;
    return ranges_core(c, Batch{d_in, &kZero, &in_len, 1, idx, &kZero, &idx_len, d_idx, false}, P, one_stream_plan(std::move(plan)), nullptr, d_out,
                       "zwz_inflate_read_ranges_dev");
}

extern "C" int zwz_inflate_read_ranges_batch_dev(zwz_ctx* c, const uint8_t* d_in, const uint64_t* in_off, const uint64_t* in_len, uint32_t n, const uint8_t* idx,
                                                 const uint64_t* idx_off, const uint64_t* idx_len, const uint8_t* d_idx, const uint64_t* ranges, uint32_t k,
                                                 uint8_t* d_out) {
    const char* who = "zwz_inflate_read_ranges_batch_dev";
    if (!c || (n && (!d_in || !in_off || !in_len || !idx || !idx_off || !idx_len)) || (k && (!ranges || !d_out))) return ZWZ_E_INVALID;
    const Batch B{d_in, in_off, in_len, n, idx, idx_off, idx_len, d_idx, true};
    if (!batch_aligned(B)) return ZWZ_E_INVALID;
    HIPCHK(hipSetDevice(c->device));
    std::vector<uint8_t> named;
    const int64_t stray = index_batch_named(ranges, k, n, &named);
    if (stray >= 0) {
        set_error("%s: range %lld names stream %llu of a batch of %u", who, (long long)stray, (unsigned long long)ranges[3 * stray], n);
        return ZWZ_E_INVALID;
    }
    std::vector<Parsed> P;
    if (int rc = parse_indexes(B, &named, &P, who)) return rc;
    std::vector<IndexView> views(n);
    for (uint32_t i = 0; i < n; i++) {
        if (!named[i]) continue;
        views[i] = P[i].v;
        if (in_len[i] != views[i].stream_len) {
            set_error("%s: stream %u has %llu bytes, the index was made for %llu", who, i, (unsigned long long)in_len[i], (unsigned long long)views[i].stream_len);
            return ZWZ_E_FORMAT;
        }
    }
    IndexBatchPlan plan;
    const int64_t bad_range = index_plan_batch(views.data(), ranges, k, &plan);
    if (bad_range >= 0) {
        set_error("%s: range %lld (stream %llu, offset %llu, length %llu) lies past the decoded length %llu", who, (long long)bad_range,
                  (unsigned long long)ranges[3 * bad_range], (unsigned long long)ranges[3 * bad_range + 1], (unsigned long long)ranges[3 * bad_range + 2],
                  (unsigned long long)views[ranges[3 * bad_range]].decoded_len);
        return ZWZ_E_INVALID;
    }
    return ranges_core(c, B, P, plan, nullptr, d_out, who);
}

extern "C" int zwz_inflate_index_info(const uint8_t* idx, uint64_t idx_len, int* wrap, uint64_t* stream_len, uint64_t* decoded_len, uint32_t* count) {
    if (!idx) return ZWZ_E_INVALID;
    IndexView v;
    const uint32_t f = index_parse(idx, idx_len, &v);
    if (f != kIdxOk) { set_error("zwz_inflate_index_info: the index is malformed: %s", index_fault_name(f)); return ZWZ_E_FORMAT; }
    if (wrap) *wrap = (int)v.wrap;
    if (stream_len) *stream_len = v.stream_len;
    if (decoded_len) *decoded_len = v.decoded_len;
    if (count) *count = v.count;
    return ZWZ_OK;
}

// zwz_filejob.h: the whole file through one launch
int zwz::inflate_whole_file(zwz_ctx* c, int wrap, const char* who, const char* src, const uint8_t* in, uint64_t n, std::vector<uint8_t>* out, std::vector<uint8_t>* idx) {
    DevMem d_in, d_out, d_idx, d_par;
    if (int rc = d_in.get(round_up((size_t)n + 16, 16))) return rc;
    if (int rc = d_par.get(80)) return rc;
    HIPCHK(hipMemcpy(d_in.p, in, round_up((size_t)n + 16, 16), hipMemcpyHostToDevice));
    const uint32_t span = c->index_span_bytes;
    uint64_t cap = std::max<uint64_t>(8 * n, 1u << 20), h_par[10];
    uint64_t* q = d_par.as<uint64_t>();
    for (;;) {
        cap = std::min<uint64_t>(cap, kStreamMaxOut - 16);
        const uint64_t bound = idx ? index_bound(cap, span) : 0u;
        if (int rc = d_out.get((size_t)cap + 16)) return rc;
        if (idx) if (int rc = d_idx.get((size_t)bound)) return rc;
        const uint64_t par[10] = {0, n, 0, cap, 0, bound, 0, 0, 0, 0};      // in_off, in_len, out_off, out_cap, idx_off, idx_cap, out_len, idx_len, status
        HIPCHK(hipMemcpy(d_par.p, par, sizeof par, hipMemcpyHostToDevice));
        uint32_t* d_status = reinterpret_cast<uint32_t*>(q + 8);
        if (int rc = idx ? zwz_inflate_streams_index_dev(c, wrap, d_in.as<uint8_t>(), q, q + 1, 1, d_out.as<uint8_t>(), q + 2, q + 3, q + 6, d_status, span,
                                                         d_idx.as<uint8_t>(), q + 4, q + 5, q + 7)
                         : zwz_inflate_streams_dev(c, wrap, d_in.as<uint8_t>(), q, q + 1, 1, d_out.as<uint8_t>(), q + 2, q + 3, q + 6, d_status)) return rc;
        HIPCHK(hipStreamSynchronize(c->stream));
        HIPCHK(hipMemcpy(h_par, d_par.p, sizeof h_par, hipMemcpyDeviceToHost));
        const uint32_t status = (uint32_t)h_par[8];
        if (status == kInfOverflow && cap < kStreamMaxOut - 16) { cap *= 2; continue; }
        if (status == kInfOverflow) return kGoLegs;
        if (status == kStrChecksum || status == kStrLength) { set_error("%s: %s: %s mismatch", who, src, status == kStrLength ? "length" : "checksum"); return ZWZ_E_CHECKSUM; }
        if (status != kInfEnd) { set_error("%s: %s: stream status %u after %llu decoded bytes", who, src, status, (unsigned long long)h_par[6]); return ZWZ_E_FORMAT; }
        break;
    }
    if (out) { out->resize((size_t)h_par[6]); if (!out->empty()) HIPCHK(hipMemcpy(out->data(), d_out.p, out->size(), hipMemcpyDeviceToHost)); }
    if (idx) { idx->resize((size_t)h_par[7]); if (!idx->empty()) HIPCHK(hipMemcpy(idx->data(), d_idx.p, idx->size(), hipMemcpyDeviceToHost)); }
    return ZWZ_OK;
}

// A file of 2^29 bytes or more, or one whose decoded bytes one launch cannot hold, goes through the file loop in legs (zwz_legs_file.cpp).
extern "C" int zwz_inflate_index_file(zwz_ctx* c, int wrap, const char* src, const char* dst_idx) {
    if (!c || !src || !dst_idx || wrap < ZWZ_WRAP_RAW || wrap > ZWZ_WRAP_GZIP) return ZWZ_E_INVALID;
    HIPCHK(hipSetDevice(c->device));
    struct stat sb;
    if (stat(src, &sb) != 0) { set_error("cannot open %s", src); return ZWZ_E_IO; }
    if ((uint64_t)sb.st_size >= kStreamMaxIn) return zwz_inflate_legs_file(c, wrap, src, nullptr, dst_idx, nullptr);
    std::vector<uint8_t> in, idx;
    if (int rc = read_whole_file(src, &in, 32)) return rc;
    const int rc = inflate_whole_file(c, wrap, "zwz_inflate_index_file", src, in.data(), in.size() - 32, nullptr, &idx);
    if (rc) return rc == kGoLegs ? zwz_inflate_legs_file(c, wrap, src, nullptr, dst_idx, nullptr) : rc;
    if (idx.empty()) { set_error("zwz_inflate_index_file: %s decodes, but no index is made for a gzip file of several members", src); return ZWZ_E_FORMAT; }
    return commit_with_index_bytes(dst_idx, nullptr, idx.data(), idx.size(), [] { return (int)ZWZ_OK; }, "cannot write %s", false);
}

namespace {

struct SrcFile {         // the compressed file of a range call, by descriptor
    int fd = -1;
    ~SrcFile() { if (fd >= 0) close(fd); }
    int open_checked(const char* src, uint64_t want_len, const char* who) {
        fd = open(src, O_RDONLY);
        if (fd < 0) { set_error("cannot open %s", src); return ZWZ_E_IO; }
        const off_t n = lseek(fd, 0, SEEK_END);
        if ((uint64_t)n != want_len) { set_error("%s: %s has %llu bytes, the index was made for %llu", who, src, (unsigned long long)n, (unsigned long long)want_len); return ZWZ_E_FORMAT; }
        return ZWZ_OK;
    }
};

// The touched segments of `plan` out of the file and through ranges_core into d_out
int ranges_from_file(zwz_ctx* c, const SrcFile& f, const char* src, const std::vector<Parsed>& P, IndexPlan&& plan, const uint8_t* idx, uint64_t idx_len,
                     DevMem& d_in, uint8_t* d_out, const char* who) {
    std::vector<uint8_t> buf;
    std::vector<uint64_t> remap;
    if (int rc = pread_touched(f.fd, src, P[0].v, plan, &buf, &remap)) return rc;
    if (int rc = d_in.get(buf.size() + 16)) return rc;
    if (!buf.empty()) HIPCHK(hipMemcpy(d_in.p, buf.data(), buf.size(), hipMemcpyHostToDevice));
    const uint64_t in_len = buf.size();
    return ranges_core(c, Batch{d_in.as<uint8_t>(), &kZero, &in_len, 1, idx, &kZero, &idx_len, nullptr, false}, P, one_stream_plan(std::move(plan)), &remap, d_out, who);
}

}  // namespace

extern "C" int zwz_inflate_read_ranges_file(zwz_ctx* c, const char* src, const char* idx_path, const uint64_t* ranges, uint32_t k, uint8_t* out) {
    if (!c || !src || !idx_path || (k && (!ranges || !out))) return ZWZ_E_INVALID;
    HIPCHK(hipSetDevice(c->device));
    std::vector<uint8_t> idx;
    if (int rc = read_whole_file(idx_path, &idx, 0)) return rc;
    std::vector<Parsed> P;
    if (int rc = parse_index(idx.data(), idx.size(), &P, "zwz_inflate_read_ranges_file")) return rc;
    IndexPlan plan;
    if (int rc = plan_ranges(P[0].v, ranges, k, &plan, "zwz_inflate_read_ranges_file")) return rc;
    SrcFile f;
    if (int rc = f.open_checked(src, P[0].v.stream_len, "zwz_inflate_read_ranges_file")) return rc;
    DevMem d_in, d_out;
    const uint64_t total = plan.total;
    if (int rc = d_out.get((size_t)total + 16)) return rc;
    if (int rc = ranges_from_file(c, f, src, P, std::move(plan), idx.data(), idx.size(), d_in, d_out.as<uint8_t>(), "zwz_inflate_read_ranges_file")) return rc;
    if (total) HIPCHK(hipMemcpy(out, d_out.p, (size_t)total, hipMemcpyDeviceToHost));
    return ZWZ_OK;
}

// Slices of consecutive index entries: each slice's compressed bytes are read (pread), its segments decoded a wave each, its bytes
// written by the writer thread while the next slice runs; the checksum is joined from the slices' pieces and checked against the index's
// and the file's own trailer at the end.
extern "C" int zwz_inflate_stream_file_indexed(zwz_ctx* c, const char* src, const char* idx_path, const char* dst) {
    if (!c || !src || !idx_path || !dst) return ZWZ_E_INVALID;
    HIPCHK(hipSetDevice(c->device));
    const char* who = "zwz_inflate_stream_file_indexed";
    std::vector<uint8_t> idx;
    if (int rc = read_whole_file(idx_path, &idx, 0)) return rc;
    std::vector<Parsed> P;
    if (int rc = parse_index(idx.data(), idx.size(), &P, who)) return rc;
    const IndexView& v = P[0].v;
    SrcFile f;
    if (int rc = f.open_checked(src, v.stream_len, who)) return rc;
    FileJob job;
    if (int rc = job.open(src, dst)) return rc;
    // a slice: entries whose decoded bytes fit the output staging (one entry at least)
    uint64_t O = std::min<uint64_t>(std::max<uint64_t>(4ull * c->split_slice_bytes, 65536), std::max<uint64_t>(v.decoded_len, 16));
    for (uint32_t k = 0; k < v.count; k++) O = std::max<uint64_t>(O, v.seg_end_off(k) - v.entry(k).off);
    const size_t np = (size_t)(O / kPieceBytes + 2);
    if (int rc = job.alloc({0, 0, (size_t)O, (size_t)O, 0}, {0, (size_t)O + 16, 0})) return rc;
    DevMem d_in, d_pieces;
    if (int rc = d_pieces.get(np * 16 + 768)) return rc;
    uint64_t* p_off = d_pieces.as<uint64_t>();
    uint32_t* p_len = reinterpret_cast<uint32_t*>(d_pieces.as<uint8_t>() + round_up(np * 8, 256));
    uint32_t* p_val = reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(p_len) + round_up(np * 4, 256));
    if (v.wrap == kWrapGzip) if (int rc = ensure_crc_tables(c)) return rc;
    std::vector<uint32_t> h_len(np), h_val(np);
    uint32_t check = dstream_check_init(v.wrap);
    int b = 0;
    for (uint32_t k0 = 0; k0 < v.count;) {
        uint32_t k1 = k0 + 1;
        while (k1 < v.count && v.seg_end_off(k1) - v.entry(k0).off <= O) k1++;
        const uint64_t r[2] = {v.entry(k0).off, v.seg_end_off(k1 - 1) - v.entry(k0).off};
        k0 = k1;
        if (!r[1]) continue;
        IndexPlan plan;
        if (int rc = plan_ranges(v, r, 1, &plan, who)) return rc;
        if (int rc = ranges_from_file(c, f, src, P, std::move(plan), idx.data(), idx.size(), d_in, job.dp(1), who)) { job.join(); return rc; }
        const uint32_t pieces = v.wrap == kWrapRaw ? 0u : (uint32_t)((r[1] + kPieceBytes - 1) / kPieceBytes);
        IndexPieces fin{};
        fin.out = job.dp(1); fin.total = r[1]; fin.wrap = v.wrap; fin.piece_off = p_off; fin.piece_len = p_len; fin.piece_val = p_val;
        fin.pieces = pieces;
        fin.head = (uint32_t)std::min<uint64_t>(kPieceBytes, r[1]);        // (an aligned buffer: the first piece is a whole one)
        HIPJOB(launch_index_piece_sums(c->buf[kBufCrcTables].as<const CrcTables>(), fin, c->cu_count, c->stream));
        if (int rc = job.finish_write()) return rc;                      // (two writes back: this buffer is free)
        uint8_t* hout = job.hp(2 + b);
        HIPJOB(hipMemcpyAsync(hout, job.d[1], (size_t)r[1], hipMemcpyDeviceToHost, c->stream));
        if (pieces) {
            HIPJOB(hipMemcpyAsync(h_len.data(), p_len, pieces * 4u, hipMemcpyDeviceToHost, c->stream));
            HIPJOB(hipMemcpyAsync(h_val.data(), p_val, pieces * 4u, hipMemcpyDeviceToHost, c->stream));
        }
        HIPJOB(hipStreamSynchronize(c->stream));
        for (uint32_t j = 0; j < pieces; j++)
            check = v.wrap == kWrapZlib ? AdlerSum::join(check, h_val[j], AdlerSum::pof(h_len[j])) : CrcSum::join(check, h_val[j], CrcSum::pof(h_len[j]));
        job.start_write(hout, (size_t)r[1]);
        b ^= 1;
    }
    if (int rc = job.finish_write()) return rc;
    if (v.wrap != kWrapRaw) {
        uint8_t tr[8] = {};
        const size_t want = v.wrap == kWrapZlib ? 4 : 8;
        if (pread(f.fd, tr, want, (off_t)((v.end_bit + 7u) >> 3)) != (ssize_t)want) { set_error("%s: %s ends inside its trailer", who, src); return ZWZ_E_FORMAT; }
        const uint32_t stored = v.wrap == kWrapZlib ? be32_at(tr) : le32_at(tr);
        if (stored != check || v.check != check) { set_error("%s: %s: checksum mismatch", who, src); return ZWZ_E_CHECKSUM; }
        if (v.wrap == kWrapGzip && le32_at(tr + 4) != (uint32_t)v.decoded_len) { set_error("%s: %s: length mismatch", who, src); return ZWZ_E_CHECKSUM; }
    }
    return job.commit(dst);
}

