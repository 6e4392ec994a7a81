// zwz_split.cpp -- zwz_inflate_split_streams_dev of include/zwz.h: the host driver of the split decode (split_core.h).  The launch
// sizes depend on what the scan and the chains give, so the call waits for the context's stream three times: for the batch's sizes,
// for the candidates per stream, and for the chains' verdicts.  Streams that do not split go through zwz_inflate_streams_dev as they
// are; the splitting ones are handed to it with a length of zero and get their results behind it.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "dstream_core.h"
#include "index_core.h"
#include "zwz_api_internal.h"
#include "zwz_bgzf.h"
#include "zwz_filejob.h"
#include "zwz_split.h"

using namespace zwz;

namespace {

constexpr uint64_t kSplitMaxKept = 8u << 20;        // kept candidates of one call: the workspace is (levels + 20) words each

// The three device workspaces of a call, each carved for that call's sizes: which is known only once the step before has run.
// Per stream (body, tile_first, cfirst, kbase, dbase, pbase, res, bad, the lengths handed to the fallback) and per scan tile (count, offset)
struct StreamArrays { uint32_t *tile_first, *kbase, *dbase, *pbase, *bad, *chk, *icount; uint64_t* fb_len; uint4 *res, *res2; };
StreamArrays streams_layout(Carver& w, size_t n, size_t tiles, SplitStreams& S) {
    StreamArrays A;
    S.body = w.take<uint32_t>(n + 1);
    S.tile_first = A.tile_first = w.take<uint32_t>(n + 1);
    S.kbase = A.kbase = w.take<uint32_t>(n + 1);
    A.dbase = w.take<uint32_t>(n + 1);
    A.pbase = w.take<uint32_t>(n + 1);
    A.bad = w.take<uint32_t>(n + 1);
    S.cfirst = w.take<uint64_t>(n + 1);
    A.fb_len = w.take<uint64_t>(n + 1);
    A.res = w.take<uint4>(n);
    A.res2 = w.take<uint4>(n);
    A.chk = w.take<uint32_t>(n + 1);
    A.icount = w.take<uint32_t>(n + 1);
    S.tile_cnt = w.take<uint32_t>(tiles);
    S.tile_off = w.take<uint64_t>(tiles);
    S.base = w.take<uint64_t>(2);
    return A;
}

// Per kept candidate; returns the launch order's scratch
uint4* cands_layout(Carver& w, size_t m, uint32_t levels, SplitCands& C) {
    C.pos = w.take<uint32_t>(m); C.mark = w.take<uint32_t>(m); C.ostart = w.take<uint32_t>(m); C.rank = w.take<uint32_t>(m);
    C.jump = w.take<uint32_t>((size_t)levels * m);
    C.in_off = w.take<uint64_t>(m); C.in_len = w.take<uint64_t>(m);
    C.seg = w.take<uint4>(m); C.meas = w.take<uint4>(m);
    return w.take<uint4>(m);
}

// Per chain segment to decode (nd) and per checksum piece (np)
void decode_layout(Carver& w, size_t nd, size_t np, SplitDecode& D, SplitPieces& P) {
    D.in_off = w.take<uint64_t>(nd); D.in_len = w.take<uint64_t>(nd); D.seg = w.take<uint4>(nd);
    P.off = w.take<uint64_t>(np); P.len = w.take<uint32_t>(np); P.val = w.take<uint32_t>(np);
}

// Reserves workspace `id` for what `layout` takes and carves it
template <class F>
int carve_ws(zwz_ctx* c, BufId id, F&& layout) {
    if (int rc = c->buf[id].reserve(c, 0, layout_bytes(layout))) return rc;
    Carver w(c->buf[id].p);
    layout(w);
    return ZWZ_OK;
}

// One slice of a file (zwz_inflate_stream_file): the stream is raw DEFLATE data that starts at a known block start p0 and need not end
// in the slice.  Decoded is the longest prefix of the chain that ends cleanly inside the slice and fits the output staging; nothing
// falls back.  Results (after the call, which then returns synchronised): segments decoded, their bytes, where the prefix ends in
// the slice, how its last segment ended, the checksum of the bytes.
// points (may be null): the prefix's segment starts, pairs (offset in the slice, decoded bytes of the slice in front), in chain order;
// low3: a final block's end bit within its byte (split_core.h: split_final_end_bit)
struct SlicePart { uint32_t p0; uint32_t nseg, total, end, kind, chk; std::vector<uint64_t>* points = nullptr; uint32_t low3 = 0; };

// zwz_inflate_split_streams_index_dev's further arguments (device arrays): the streams that split get the index of their flush points,
// the others the marking form's instead of the plain stream form
struct IndexOut { uint32_t span; uint8_t* idx; const uint64_t *idx_off, *idx_cap; uint64_t* idx_len; };

int split_call(zwz_ctx* c, int wrap, const uint8_t* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len,
               uint32_t n, uint8_t* d_out, const uint64_t* d_out_off, const uint64_t* d_out_cap,
               uint64_t* d_out_len, uint32_t* d_status, uint32_t* d_segments, SlicePart* part, const IndexOut* ix = nullptr) {
    hipStream_t st = c->stream;
    auto fall_back = [&](const uint64_t* lens) {
        if (part) return (int)ZWZ_OK;
        if (ix) return zwz_inflate_streams_index_dev(c, wrap, d_in, d_in_off, lens, n, d_out, d_out_off, d_out_cap, d_out_len, d_status, ix->span, ix->idx,
                                                     ix->idx_off, ix->idx_cap, ix->idx_len);
        return zwz_inflate_streams_dev(c, wrap, d_in, d_in_off, lens, n, d_out, d_out_off, d_out_cap, d_out_len, d_status);
    };
    const uint32_t min_bytes = part ? 1u : c->split_min_bytes;
    if (part) { part->nseg = 0; part->total = 0; part->end = part->p0; part->kind = kSegBad; part->chk = 0; }

    // 1. the sizes: which streams are scanned at all, and their tiles
    std::vector<uint64_t> h_len(n), h_cap(n);
    HIPCHK(hipMemcpyAsync(h_len.data(), d_in_len, n * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(h_cap.data(), d_out_cap, n * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (d_segments) HIPCHK(hipMemsetAsync(d_segments, 0, n * sizeof(uint32_t), st));
    if (int rc = c->buf[kBufSplitHost].reserve(c, n, (size_t)(n + 1) * 24)) return rc;
    uint64_t* fb_len = c->buf[kBufSplitHost].as<uint64_t>();
    uint32_t* tile_first = reinterpret_cast<uint32_t*>(fb_len + n + 1);
    uint32_t *kbase = tile_first + n + 1, *dbase = kbase + n + 1, *pbase = dbase + n + 1;
    uint64_t tiles = 0;
    for (uint32_t i = 0; i < n; i++) {
        tile_first[i] = (uint32_t)tiles;
        if (h_len[i] < kStreamMaxIn && h_cap[i] < kStreamMaxOut && h_len[i] >= min_bytes && h_len[i]) tiles += (h_len[i] + kSplitTile - 1) / kSplitTile;
        if (tiles > 0x7fffffffull) return fall_back(d_in_len);          // (2^43 bytes of input in one call)
    }
    tile_first[n] = (uint32_t)tiles;
    if (!tiles) return fall_back(d_in_len);

    SplitStreams S{};
    S.in = d_in; S.in_off = d_in_off; S.in_len = d_in_len; S.out_cap = d_out_cap; S.n = n; S.wrap = (uint32_t)wrap; S.n_tiles = (uint32_t)tiles;
    StreamArrays A{};
    if (int rc = carve_ws(c, kBufSplit0, [&](Carver& w) { A = streams_layout(w, n, tiles, S); })) return rc;
    HIPCHK(hipMemcpyAsync(A.tile_first, tile_first, (n + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(A.bad, 0, n * sizeof(uint32_t), st));
    if (part) HIPCHK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(S.body), (int)part->p0, 1, st));      // (the body starts where the last slice's chain ended)
    else HIPCHK(launch_split_head(S, min_bytes, st));
    HIPCHK(launch_split_count(S, st));

    // 2. the candidates per stream: which streams are measured
    std::vector<uint64_t> cfirst(n + 1);
    HIPCHK(hipMemcpyAsync(cfirst.data(), S.cfirst, (n + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    uint64_t kept = 0;
    uint32_t longest = 0;
    for (uint32_t i = 0; i < n; i++) {
        kbase[i] = (uint32_t)kept;
        const uint64_t cnt = cfirst[i + 1] - cfirst[i];
        if (cnt >= (part ? 1u : 2u) && cnt <= c->split_max_candidates && kept + cnt <= kSplitMaxKept) { kept += cnt; longest = std::max(longest, (uint32_t)cnt); }
    }
    kbase[n] = (uint32_t)kept;
    if (!kept) return fall_back(d_in_len);
    const uint32_t m = (uint32_t)kept, levels = split_levels(longest);
    SplitCands C{};
    C.m = m;
    uint4* d_order = nullptr;
    if (int rc = carve_ws(c, kBufSplit1, [&](Carver& w) { d_order = cands_layout(w, m, levels, C); })) return rc;
    HIPCHK(hipMemcpyAsync(A.kbase, kbase, (n + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIPCHK(launch_split_write(S, C, c->split_budget, st));
    {
        InflateSplitArgs a{d_in, C.in_off, C.in_len, m, nullptr, nullptr, d_order, C.seg, C.meas, nullptr, 1u, c->inflate_serial_header};
        HIPCHK(launch_inflate_split(a, st));
    }
    HIPCHK(launch_split_resolve(S, C, levels, A.res, part ? 1u : 0u, part ? h_cap[0] : 0, A.res2, st));

    // 3. the chains' verdicts: the segments to decode, the checksum pieces, and who falls back
    std::vector<uint4> res(n);
    HIPCHK(hipMemcpyAsync(res.data(), A.res, n * sizeof(uint4), hipMemcpyDeviceToHost, st));
    uint4 res2{};
    if (part) HIPCHK(hipMemcpyAsync(&res2, A.res2, sizeof(uint4), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (uint32_t i = 0; i < n; i++) fb_len[i] = h_len[i];
    uint64_t nd = 0, np = 0;
    uint32_t n_fall = 0;
    for (uint32_t i = 0; i < n; i++) {
        dbase[i] = (uint32_t)nd; pbase[i] = (uint32_t)np;
        if (res[i].x) { nd += res[i].y; if (wrap != ZWZ_WRAP_RAW) np += ((uint64_t)res[i].z + kPieceBytes - 1) / kPieceBytes; fb_len[i] = 0; }
        else n_fall++;
    }
    dbase[n] = (uint32_t)nd; pbase[n] = (uint32_t)np;
    if (!nd) return fall_back(d_in_len);
    // The stream path runs over the whole batch with the splitting streams' lengths set to zero: a wave each that ends at once and
    // writes status 1 and length 0 for them.  Their real results are written by split_finish_kernel further down.  Both are queued on
    // the context's stream in this order, and the call's correctness depends on that: the later write wins.
    if (n_fall && !part) {
        HIPCHK(hipMemcpyAsync(A.fb_len, fb_len, n * sizeof(uint64_t), hipMemcpyHostToDevice, st));
        const int rc = fall_back(A.fb_len);
        if (rc) return rc;
    }
    if (wrap == ZWZ_WRAP_GZIP || ix) if (int rc = ensure_crc_tables(c)) return rc;      // (the index CRC, whatever the wrapper)
    SplitDecode D{};
    D.res = A.res; D.dbase = A.dbase;
    SplitPieces P{};
    P.pbase = A.pbase; P.p = (uint32_t)np;
    if (int rc = carve_ws(c, kBufSplit2, [&](Carver& w) { decode_layout(w, nd, np, D, P); })) return rc;
    HIPCHK(hipMemcpyAsync(A.dbase, dbase, (n + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(A.pbase, pbase, (n + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIPCHK(launch_split_emit(S, C, D, st));
    std::vector<uint64_t> p_off;
    std::vector<uint4> p_seg;
    if (part && part->points) {                       // (the records are dense by rank: the prefix is the first res[0].y of them)
        p_off.resize(nd); p_seg.resize(nd);
        HIPCHK(hipMemcpyAsync(p_off.data(), D.in_off, nd * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(p_seg.data(), D.seg, nd * sizeof(uint4), hipMemcpyDeviceToHost, st));
    }
    SplitIndex X{};
    if (ix) {
        X = SplitIndex{ix->idx, ix->idx_off, ix->idx_cap, ix->idx_len, A.icount, ix->span};
        HIPCHK(launch_split_index(S, D, X, st));
    }
    {
        InflateSplitArgs a{d_in, D.in_off, D.in_len, (uint32_t)nd, d_out, d_out_off, d_order, D.seg, nullptr, A.bad, 0u, c->inflate_serial_header};
        HIPCHK(launch_inflate_split(a, st));
    }
    HIPCHK(launch_split_finish(S, D, P, c->buf[kBufCrcTables].as<const CrcTables>(), d_out, d_out_off, A.bad, d_out_len, d_status, d_segments,
                               part ? A.chk : nullptr, c->cu_count, st));
    if (ix) HIPCHK(launch_split_seal(S, D, X, A.res2, c->buf[kBufCrcTables].as<const CrcTables>(), d_status, c->cu_count, st));
    if (part) {
        HIPCHK(hipMemcpyAsync(&part->chk, A.chk, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        uint32_t bad = 0;
        HIPCHK(hipMemcpyAsync(&bad, A.bad, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (bad) { set_error("split inflate: a segment did not decode as it was measured"); return ZWZ_E_FORMAT; }
        part->nseg = res[0].y; part->total = res[0].z; part->end = res2.x; part->kind = res2.y; part->low3 = res2.z;
        if (part->points) {
            part->points->clear();
            for (uint64_t j = 0; j < nd; j++) { part->points->push_back(p_off[j] + p_seg[j].x); part->points->push_back(p_seg[j].z); }
        }
    }
    return ZWZ_OK;
}

}  // namespace

extern "C" int zwz_inflate_split_streams_dev(zwz_ctx* c, int wrap, const uint8_t* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len,
                                             uint32_t n, uint8_t* d_out, const uint64_t* d_out_off, const uint64_t* d_out_cap,
                                             uint64_t* d_out_len, uint32_t* d_status, uint32_t* d_segments) {
    if (!c || wrap < ZWZ_WRAP_RAW || wrap > ZWZ_WRAP_GZIP) return ZWZ_E_INVALID;
    if (n && (!d_in || !d_in_off || !d_in_len || !d_out || !d_out_off || !d_out_cap || !d_out_len || !d_status)) return ZWZ_E_INVALID;
    if (((uintptr_t)d_in & 15u) || ((uintptr_t)d_out & 15u)) return ZWZ_E_INVALID;
    if (n == 0) return ZWZ_OK;
    HIPCHK(hipSetDevice(c->device));
    return split_call(c, wrap, d_in, d_in_off, d_in_len, n, d_out, d_out_off, d_out_cap, d_out_len, d_status, d_segments, nullptr);
}

extern "C" int zwz_inflate_split_streams_index_dev(zwz_ctx* c, int wrap, const uint8_t* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len,
                                                   uint32_t n, uint8_t* d_out, const uint64_t* d_out_off, const uint64_t* d_out_cap,
                                                   uint64_t* d_out_len, uint32_t* d_status, uint32_t* d_segments, uint32_t span, uint8_t* d_idx,
                                                   const uint64_t* d_idx_off, const uint64_t* d_idx_cap, uint64_t* d_idx_len) {
    if (!c || wrap < ZWZ_WRAP_RAW || wrap > ZWZ_WRAP_GZIP) return ZWZ_E_INVALID;
    if (span == 0) span = c->index_span_bytes;
    if (!index_span_ok(span)) return ZWZ_E_INVALID;
    if (n && (!d_in || !d_in_off || !d_in_len || !d_out || !d_out_off || !d_out_cap || !d_out_len || !d_status || !d_idx || !d_idx_off || !d_idx_cap || !d_idx_len))
        return ZWZ_E_INVALID;
    if (((uintptr_t)d_in & 15u) || ((uintptr_t)d_out & 15u) || ((uintptr_t)d_idx & 15u)) return ZWZ_E_INVALID;
    if (n == 0) return ZWZ_OK;
    HIPCHK(hipSetDevice(c->device));
    const IndexOut ix{span, d_idx, d_idx_off, d_idx_cap, d_idx_len};
    return split_call(c, wrap, d_in, d_in_off, d_in_len, n, d_out, d_out_off, d_out_cap, d_out_len, d_status, d_segments, nullptr, &ix);
}

// One file of any size.  The device holds a slice of the compressed file at a time; split_call decodes the chain segments that end
// inside it and fit the output staging, the host writes them (a writer thread, two pinned buffers), joins their checksum onto the
// file's and goes on with a slice that starts at the chain's position, rounded down to 16: the bytes behind it are kept, the rest is
// read.  A chain that makes no progress in a whole slice is broken: before any byte was written the file goes through the one-stream
// path if it fits its limits, later it is ZWZ_E_FORMAT.
// With dst_idx (zwz_inflate_split_index_file) the index of the flush points as well: every slice hands back the starts of the segments
// it decoded, the host applies index_core.h's rule to them with the last point's offset carried from slice to slice, and seals the
// header once the trailer is known; dst may then be null.  A file that does not split goes to zwz_inflate_legs_file with dst_idx.
namespace {

int inflate_stream_file_core(zwz_ctx* c, int wrap_, const char* src, const char* dst, const char* dst_idx) {
    if (!c || !src || (!dst && !dst_idx) || wrap_ < ZWZ_WRAP_RAW || wrap_ > ZWZ_WRAP_GZIP) return ZWZ_E_INVALID;
    const uint32_t wrap = (uint32_t)wrap_;
    HIPCHK(hipSetDevice(c->device));
    FileJob job;
    if (dst) { if (int rc = job.open(src, dst)) return rc; }
    else { job.in = fopen(src, "rb"); if (!job.in) { set_error("cannot open %s", src); return ZWZ_E_IO; } }
    std::vector<uint64_t> points;                     // of one slice
    std::vector<uint8_t> ents(kIdxHeader);            // the index as it grows: the header's place, then the entries
    uint64_t prev_off = 0, end_bit = 0;
    bool first_point = true;
    const size_t S = c->split_slice_bytes, O = std::max<size_t>(4 * S, 4u << 20);
    if (int rc = job.alloc({S + 32, 0, O, O, 64}, {S + 32, O + 16, 64})) return rc;      // (one input buffer: the next slice depends on this one's end)
    uint8_t* hin = static_cast<uint8_t*>(job.h[0]);
    uint8_t* d_in = static_cast<uint8_t*>(job.d[0]); uint8_t* d_out = static_cast<uint8_t*>(job.d[1]);
    uint64_t* d_par = static_cast<uint64_t*>(job.d[2]);           // in_off, in_len, out_off, out_cap, out_len, (status, segments)
    uint64_t* h_par = static_cast<uint64_t*>(job.h[4]);
    bool io_err = false;
    uint64_t base = 0;                    // file offset of hin[0], a multiple of 16
    size_t have = read_full(job.in, hin, S, &io_err);
    if (io_err) { set_error("read error on %s", src); return ZWZ_E_IO; }
    bool eof = have < S;
    uint32_t p0 = 0;
    bool chain_ok = true;
    {
        uint32_t nz = 0;
        while (nz < have && hin[nz] == 0) nz++;
        chain_ok = have && stream_begin(wrap, hin, (uint32_t)have, wrap == kWrapGzip ? (nz ? (uint32_t)have : 0u) : (uint32_t)have, &p0) == kInfRunning && p0 < have;
    }
    uint32_t check = dstream_check_init(wrap);
    uint64_t total = 0, at = p0;          // decoded bytes written; file offset of the chain's position
    uint32_t kind = kSegBad;
    int b = 0;
    while (chain_ok) {
        memset(hin + have, 0, 32);
        h_par[0] = 0; h_par[1] = have; h_par[2] = 0; h_par[3] = O;
        HIPJOB(hipMemcpyAsync(d_in, hin, round_up(have + 16, 16), hipMemcpyHostToDevice, c->stream));
        HIPJOB(hipMemcpyAsync(d_par, h_par, 32, hipMemcpyHostToDevice, c->stream));
        SlicePart part{};
        if (dst_idx) part.points = &points;
        part.p0 = (uint32_t)(at - base);
        if (int rc = split_call(c, wrap_, d_in, d_par, d_par + 1, 1, d_out, d_par + 2, d_par + 3, d_par + 4, reinterpret_cast<uint32_t*>(d_par + 5), nullptr, &part)) { job.join(); return rc; }
        if (!part.nseg) { chain_ok = false; break; }             // no segment ends inside a whole slice (or its input does)
        if (dst_idx && !total && part.nseg == 1 && part.kind == kSegFinal) { chain_ok = false; break; }   // one piece in all: no flush point, the index is the one-wave decode's
        if (dst) {
            uint8_t* hout = static_cast<uint8_t*>(job.h[2 + b]);
            if (int rc = job.finish_write()) return rc;               // (two writes back: this buffer is free)
            HIPJOB(hipMemcpyAsync(hout, d_out, part.total, hipMemcpyDeviceToHost, c->stream));
            HIPJOB(hipStreamSynchronize(c->stream));
            job.start_write(hout, part.total);
            b ^= 1;
        }
        if (dst_idx) {
            // the prefix's points: offsets in the file and in the output; whether bytes follow a point is known only at the end
            for (uint32_t j = 0; j < part.nseg; j++) {
                const uint64_t p = base + points[2 * (size_t)j], o = total + points[2 * (size_t)j + 1];
                if (first_point || index_flush_due(prev_off, o, ~0ull, c->index_span_bytes)) {
                    ents.resize(ents.size() + kIdxEntry);
                    index_flush_entry(ents.data() + ents.size() - kIdxEntry, 8u * p, o);
                }
                first_point = false; prev_off = o;
            }
            if (part.kind == kSegFinal) end_bit = split_final_end_bit(base + part.end, part.low3);
        }
        if (wrap == kWrapZlib) check = AdlerSum::join(check, part.chk, AdlerSum::pof(part.total));
        else if (wrap == kWrapGzip) check = CrcSum::join(check, part.chk, CrcSum::pof(part.total));
        total += part.total;
        at = base + part.end;
        kind = part.kind;
        if (kind == kSegFinal) break;
        // the next slice: from the chain's position rounded down to 16
        const uint64_t nbase = at & ~15ull;
        const size_t keep = (size_t)(base + have - nbase);
        if (keep == have && eof) { chain_ok = false; break; }     // (cannot happen: a segment was decoded)
        memmove(hin, hin + (nbase - base), keep);
        base = nbase; have = keep;
        if (!eof) {
            const size_t got = read_full(job.in, hin + keep, S - keep, &io_err);
            if (io_err) { job.join(); set_error("read error on %s", src); return ZWZ_E_IO; }
            have += got;
            eof = got < S - keep;
        } else if (at >= base + have) { chain_ok = false; break; }   // the file ends at a flush point: no final block
    }
    if (int rc = job.finish_write()) return rc;
    fseeko(job.in, 0, SEEK_END);
    const uint64_t size = (uint64_t)ftello(job.in);
    // the whole file in legs through staging windows (zwz_legs_file.cpp), where the paths below end: at the one-wave rate; what was written is dropped
    auto in_legs = [&]() -> int {
        job.join();
        for (void*& p : job.h) if (p) { (void)hipHostFree(p); p = nullptr; }
        for (void*& p : job.d) if (p) { (void)hipFree(p); p = nullptr; }
        if (job.out) { fclose(job.out); job.out = nullptr; unlink(job.part.c_str()); }
        return zwz_inflate_legs_file(c, wrap_, src, dst, dst_idx, nullptr);
    };
    // the whole file as one stream through one launch (inflate_whole_file); what was written is dropped
    auto one_stream = [&]() -> int {
        job.join();
        if (fflush(job.out) != 0 || ftruncate(fileno(job.out), 0) != 0 || fseeko(job.out, 0, SEEK_SET) != 0) { set_error("write error on %s", job.part.c_str()); return ZWZ_E_IO; }
        for (int i = 0; i < 4; i++) { if (job.h[i]) { (void)hipHostFree(job.h[i]); job.h[i] = nullptr; } if (i < 2 && job.d[i]) { (void)hipFree(job.d[i]); job.d[i] = nullptr; } }
        std::vector<uint8_t> whole((size_t)size + 32, 0), outv;
        fseeko(job.in, 0, SEEK_SET);
        if (read_full(job.in, whole.data(), (size_t)size, &io_err) != size || io_err) { set_error("read error on %s", src); return ZWZ_E_IO; }
        if (int rc = inflate_whole_file(c, wrap_, "zwz_inflate_stream_file", src, whole.data(), size, &outv, nullptr)) return rc;
        if (!outv.empty() && fwrite(outv.data(), 1, outv.size(), job.out) != outv.size()) { set_error("write error on %s", job.part.c_str()); return ZWZ_E_IO; }
        return job.commit(dst);
    };
    if (!chain_ok || kind != kSegFinal) {
        // the chain broke at `at`
        if (total) { set_error("zwz_inflate_stream_file: %s: no block ends cleanly from compressed offset %llu on", src, (unsigned long long)at); return ZWZ_E_FORMAT; }
        // nothing written yet
        if (size >= kStreamMaxIn || dst_idx) return in_legs();
        const int rc = one_stream();
        return rc == kGoLegs ? in_legs() : rc;
    }
    // the trailer behind the final block, and for gzip nothing but zero bytes behind it
    if (wrap != kWrapRaw) {
        uint8_t tr[8];
        const size_t want = wrap == kWrapZlib ? 4 : 8;
        fseeko(job.in, (off_t)at, SEEK_SET);
        if (read_full(job.in, tr, want, &io_err) != want) { set_error("zwz_inflate_stream_file: %s ends inside its trailer at compressed offset %llu", src, (unsigned long long)at); return ZWZ_E_FORMAT; }
        const uint32_t stored = wrap == kWrapZlib ? be32_at(tr) : le32_at(tr);
        if (stored != check) { set_error("zwz_inflate_stream_file: %s: checksum mismatch", src); return ZWZ_E_CHECKSUM; }
        if (wrap == kWrapGzip) {
            if (le32_at(tr + 4) != (uint32_t)total) { set_error("zwz_inflate_stream_file: %s: length mismatch", src); return ZWZ_E_CHECKSUM; }
            uint8_t buf[4096];
            for (size_t k; (k = fread(buf, 1, sizeof buf, job.in)) > 0;)
                for (size_t i = 0; i < k; i++)
                    if (buf[i]) {
                        // another member, or garbage: both paths read the one and name the other, from the file's first byte
                        if (size >= kStreamMaxIn || dst_idx) return in_legs();
                        const int rc = one_stream();
                        return rc == kGoLegs ? in_legs() : rc;
                    }
        }
    }
    if (!dst_idx) return job.commit(dst);
    // entries at the decoded length have no byte behind them (the empty final block, markers in a row at the end)
    while (ents.size() > kIdxHeader + kIdxEntry && le64_of(ents.data() + ents.size() - kIdxEntry + 8) >= total) ents.resize(ents.size() - kIdxEntry);
    const uint64_t count = (ents.size() - kIdxHeader) / kIdxEntry;
    if (count > 0xffffffffull) { set_error("zwz_inflate_split_index_file: more than 2^32 - 1 index entries"); return ZWZ_E_INVALID; }
    ents.resize((size_t)index_flush_bytes(count));
    index_flush_seal(ents.data(), wrap, c->index_span_bytes, size, total, (uint32_t)count, end_bit, wrap == kWrapRaw ? 0u : check);
    return commit_with_index_bytes(dst_idx, dst, ents.data(), ents.size(), [&] { return dst ? job.commit(dst) : (int)ZWZ_OK; });
}

}  // namespace

extern "C" int zwz_inflate_stream_file(zwz_ctx* c, int wrap, const char* src, const char* dst) {
    if (!dst) return ZWZ_E_INVALID;
    return inflate_stream_file_core(c, wrap, src, dst, nullptr);
}

extern "C" int zwz_inflate_split_index_file(zwz_ctx* c, int wrap, const char* src, const char* dst, const char* dst_idx) {
    if (!dst_idx) return ZWZ_E_INVALID;
    return inflate_stream_file_core(c, wrap, src, dst, dst_idx);
}
