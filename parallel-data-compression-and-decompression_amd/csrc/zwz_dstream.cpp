// zwz_dstream.cpp -- zwz_deflate_streams_dev / zwz_deflate_stream_file of include/zwz.h: the host driver around the codec.  Per slice
// of at most max_batch pieces: dstream_layout + crc32_blocks (gzip) + zwz_deflate_batch_dev + dstream_size + the scan +
// dstream_combine + dstream_pack, all on the context's stream; what runs from slice to slice (the scan's base, every stream's first
// scan value and checksum) stays in device memory, so the host never waits between slices.  The dependent calls
// (zwz_deflate_dep_streams_dev, zwz_deflate_dep_stream_file) are the same driver with the other PieceForm of dstream_core.h: the piece's
// own Adler-32 under zlib, the codec entered behind the dictionary, and windows with the index's entries are all that differs.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "dstream_core.h"
#include "index_core.h"
#include "zwz_api_internal.h"
#include "zwz_bgzf.h"
#include "zwz_dstream.h"
#include "zwz_filejob.h"

using namespace zwz;

namespace {

constexpr uint32_t kFileSlicePieces = 256;          // pieces per slice of zwz_deflate_stream_file: 16.7 MB of input

struct PiecesView { DstreamPieces P; uint64_t* base; uint32_t* err; uint64_t* rbase; };     // rbase: the rank scan's base (index)
PiecesView pieces_layout(Carver& w, size_t m) {
    PiecesView v;
    v.P.slots = w.take<uint8_t>(m * ZWZ_DEV_STRIDE, 256);     // (wg_copy reads up to 3 bytes past a slot's bytes)
    v.P.off = w.take<uint64_t>(m); v.P.x = w.take<uint64_t>(m);
    v.P.len = w.take<uint32_t>(m); v.P.olen = w.take<uint32_t>(m); v.P.crc = w.take<uint32_t>(m); v.P.sidx = w.take<uint32_t>(m);
    v.P.slen = w.take<uint32_t>(m); v.P.hbit = w.take<uint32_t>(m); v.P.ebit = w.take<uint32_t>(m);
    v.P.due = w.take<uint32_t>(m); v.P.rank = w.take<uint64_t>(m);
    v.base = w.take<uint64_t>(3); v.err = reinterpret_cast<uint32_t*>(v.base + 1); v.rbase = v.base + 2;
    v.P.skip = w.take<uint32_t>(m); v.P.poff = w.take<uint64_t>(m); v.P.plen = w.take<uint32_t>(m);
    return v;
}

PiecesView pieces_view(zwz_ctx* c) {
    Carver w(c->buf[kBufPieces].p);
    return pieces_layout(w, c->buf[kBufPieces].count);
}

// in_off, in_len, out_off, out_cap (n each), pfirst (n + 1), with an index idx_off and idx_cap (n each) -- copied from the host -- then
// xs, rs, cnt (n each) and chk (n)
size_t streams_host_bytes(uint32_t n, bool index = true) { return ((index ? 7 : 5) * (size_t)n + 1) * 8; }
size_t streams_dev_bytes(uint32_t n) { return streams_host_bytes(n) + 3 * (size_t)n * 8 + (size_t)n * 4 + 64; }

int ensure_dstream(zwz_ctx* c, uint32_t pieces, uint32_t streams, bool crc) {
    if (crc) if (int rc = ensure_crc_tables(c)) return rc;
    if (!c->ds_copied) HIPCHK(hipEventCreateWithFlags(&c->ds_copied, hipEventDisableTiming));
    if (int rc = c->buf[kBufPieces].reserve(c, pieces, layout_bytes([&](Carver& w) { pieces_layout(w, pieces); }))) return rc;
    if (int rc = c->buf[kBufStreamsDev].reserve(c, streams, streams_dev_bytes(streams))) return rc;
    return c->buf[kBufStreamsHost].reserve(c, streams, streams_host_bytes(streams));
}

// One call of the device part: n streams of d_in (host arrays in_off, in_len) into d_out (host arrays out_off, out_cap), lengths and
// statuses into device memory.
struct DstreamCall {
    uint32_t wrap;
    const uint8_t* d_in; const uint64_t *in_off, *in_len; uint32_t n;
    uint8_t* d_out; const uint64_t *out_off, *out_cap; uint64_t* d_out_len; uint32_t* d_status;
    // partial: every stream's pieces alone, and its checksum left in *d_chk (the file function's slices)
    bool partial = false;
    // ix: the index as well, idx_off and idx_cap host arrays of n; sealed by the call unless partial, when *d_cnt is where the stream's
    // count of entries will stand
    const DstreamIndex* ix = nullptr; const uint64_t *idx_off = nullptr, *idx_cap = nullptr;
    // form: independent pieces, or dependent ones (dstream_core.h) -- each compressed behind the kDepDictBytes of input in front of it;
    // lead: the dictionary bytes that lie in front of in_off[i] for every stream's first piece (the dependent file function's later
    // slices), else 0; win_base: where a partial call's index windows go (zwz_dstream.h)
    PieceForm form = kPiecesAlone; uint32_t lead = 0; uint64_t win_base = 0;
    const uint32_t** d_chk = nullptr; const uint64_t** d_cnt = nullptr;
};

// The device part, arguments checked by the caller.  Returns with everything queued on the context's stream.
int dstream_launch(zwz_ctx* c, const DstreamCall& k) {
    const uint32_t n = k.n, wrap = k.wrap;
    const PieceForm F = k.form;
    // pieces are counted in 64 bits: the only limit is that they, and the output they need, can be counted at all
    const uint64_t piece = F.piece;
    std::vector<uint64_t> pfirst((size_t)n + 1);
    pfirst[0] = 0;
    for (uint32_t i = 0; i < n; i++) {
        if (k.in_len[i] > ~0ull - piece || (k.in_len[i] + piece - 1) / piece > (~0ull >> 18) - pfirst[i]) {
            set_error("%s: the streams up to stream %u have more than 2^46 pieces", F.dict ? "zwz_deflate_dep_streams_dev" : "zwz_deflate_streams_dev", i);
            return ZWZ_E_INVALID;
        }
        pfirst[i + 1] = pfirst[i] + (k.in_len[i] + piece - 1) / piece;
    }
    const uint64_t G = pfirst[n];
    const uint32_t M = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(G, 1), c->max_batch);
    if (int rc = ensure_dstream(c, M, n, wrap == kWrapGzip || (k.ix && !k.partial))) return rc;     // (the index CRC, whatever the wrapper)
    // the pinned arrays may still be the source of the previous call's copy
    HIPCHK(hipEventSynchronize(c->ds_copied));
    uint64_t* h = c->buf[kBufStreamsHost].as<uint64_t>();
    memcpy(h, k.in_off, (size_t)n * 8); memcpy(h + n, k.in_len, (size_t)n * 8);
    memcpy(h + 2 * (size_t)n, k.out_off, (size_t)n * 8); memcpy(h + 3 * (size_t)n, k.out_cap, (size_t)n * 8);
    memcpy(h + 4 * (size_t)n, pfirst.data(), ((size_t)n + 1) * 8);
    if (k.ix) { memcpy(h + 5 * (size_t)n + 1, k.idx_off, (size_t)n * 8); memcpy(h + 6 * (size_t)n + 1, k.idx_cap, (size_t)n * 8); }
    uint64_t* d = c->buf[kBufStreamsDev].as<uint64_t>();
    HIPCHK(hipMemcpyAsync(d, h, streams_host_bytes(n, k.ix != nullptr), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipEventRecord(c->ds_copied, c->stream));
    DstreamStreams S;
    S.in_off = d; S.in_len = d + n; S.out_off = d + 2 * (size_t)n; S.out_cap = d + 3 * (size_t)n; S.pfirst = d + 4 * (size_t)n;
    S.idx_off = d + 5 * (size_t)n + 1; S.idx_cap = d + 6 * (size_t)n + 1;
    S.xs = d + 7 * (size_t)n + 1; S.rs = S.xs + n; S.cnt = S.rs + n; S.chk = reinterpret_cast<uint32_t*>(S.cnt + n); S.n = n;
    if (k.d_chk) *k.d_chk = S.chk;
    if (k.d_cnt) *k.d_cnt = S.cnt;
    const DstreamOut O{k.d_out, k.d_out_len, k.d_status, wrap, k.partial ? 1u : 0u, zlib_flg_of(c->level, c->strategy), gzip_xfl_of(c->strategy)};
    const PiecesView v = pieces_view(c);
    const CrcTables* tab = c->buf[kBufCrcTables].as<const CrcTables>();
    HIPCHK(hipMemsetAsync(v.base, 0, 24, c->stream));
    HIPCHK(launch_dstream_begin(S, O, c->stream));
    uint32_t s0 = 0;                                  // the stream of the slice's first piece
    for (uint64_t g0 = 0; g0 < G; g0 += M) {
        const uint32_t m = (uint32_t)std::min<uint64_t>(G - g0, M);
        while (pfirst[s0 + 1] <= g0) s0++;
        uint32_t s1 = s0;                             // the stream of its last
        while (pfirst[s1 + 1] < g0 + m) s1++;
        // the chunk of a piece is [dictionary | piece], read where it lies in the caller's input; the checksum is the piece's alone
        HIPCHK(launch_dstream_layout(S, v.P, F, k.lead, g0, m, c->stream));
        if (wrap == kWrapGzip) HIPCHK(launch_crc32_blocks(tab, k.d_in, v.P.poff, v.P.plen, m, v.P.crc, c->cu_count, c->stream));
        else if (wrap == kWrapZlib && F.dict) HIPCHK(launch_dstream_adler(k.d_in, v.P, m, c->cu_count, c->stream));
        // (without a dictionary the codec is entered with no skip array at all, not one of zeros: its kernels are the batch call's)
        if (int rc = F.dict ? deflate_batch_dev_skip(c, k.d_in, v.P.off, v.P.len, v.P.skip, m, v.P.slots, ZWZ_DEV_STRIDE, v.P.olen)
                            : zwz_deflate_batch_dev(c, k.d_in, v.P.off, v.P.len, m, v.P.slots, ZWZ_DEV_STRIDE, v.P.olen)) return rc;
        DeflateArgs a;                                // the slice's block records are still in the codec's workspace
        carve_workspace(c, a);
        HIPCHK(launch_dstream_size(a.info, a.blocks, a.plans, v.P, m, v.err, c->stream));
        HIPCHK(launch_bgzf_scan(v.P.slen, m, 0, ~0u, v.P.x, v.base, v.err + 1, c->stream));
        HIPCHK(launch_dstream_combine(S, v.P, F, g0, m, s0, s1 - s0 + 1, wrap, c->stream));
        HIPCHK(launch_dstream_pack(S, v.P, g0, m, O, v.err, c->stream));
        if (k.ix) {
            HIPCHK(launch_dstream_due(S, v.P, F, g0, m, *k.ix, c->stream));
            HIPCHK(launch_bgzf_scan(v.P.due, m, 0, ~0u, v.P.rank, v.rbase, v.err + 1, c->stream));
            HIPCHK(launch_dstream_index(k.d_in, S, v.P, F, g0, m, O, *k.ix, k.win_base, c->stream));
        }
        s0 = s1;
    }
    if (k.ix && !k.partial) HIPCHK(launch_dstream_index_seal(tab, S, F, O, *k.ix, c->cu_count, c->stream));
    return ZWZ_OK;
}

// What the dependent calls refuse beyond the independent ones' checks
int dep_strategy_ok(zwz_ctx* c, const char* who) {
    if (c->strategy == kStrategyDefault) return ZWZ_OK;
    set_error("%s: dependent pieces need the default strategy (the context's is %u): under Z_HUFFMAN_ONLY and Z_RLE there is nothing "
              "to gain from the bytes in front of a piece -- use the independent call", who, c->strategy);
    return ZWZ_E_INVALID;
}

// The four _dev entry points: the checks, in `who`'s name, and the launch.  span: null without an index, else the caller's (0: the
// context's), with d_idx and d_idx_len.
int dstream_dev(zwz_ctx* c, const char* who, int wrap, DstreamCall k, const uint32_t* span_ = nullptr, uint8_t* d_idx = nullptr, uint64_t* d_idx_len = nullptr) {
    if (!c || wrap < ZWZ_WRAP_RAW || wrap > ZWZ_WRAP_GZIP) return ZWZ_E_INVALID;
    const uint32_t span = span_ ? (*span_ ? *span_ : c->index_span_bytes) : kIdxSpanDefault;
    if (!index_span_ok(span)) return ZWZ_E_INVALID;
    if (k.n && (!k.d_in || !k.in_off || !k.in_len || !k.d_out || !k.out_off || !k.out_cap || !k.d_out_len || !k.d_status)) return ZWZ_E_INVALID;
    if (k.n && span_ && (!d_idx || !k.idx_off || !k.idx_cap || !d_idx_len)) return ZWZ_E_INVALID;
    if (((uintptr_t)k.d_in & 15u) || ((uintptr_t)k.d_out & 15u) || ((uintptr_t)d_idx & 15u)) return ZWZ_E_INVALID;
    for (uint32_t i = 0; i < k.n; i++)
        if ((k.in_off[i] & 15u) || (k.out_off[i] & 15u) || (span_ && (k.idx_off[i] & 15u))) { set_error("%s: stream %u: offsets must be multiples of 16", who, i); return ZWZ_E_INVALID; }
    if (k.form.dict) if (int rc = dep_strategy_ok(c, who)) return rc;
    if (k.n == 0) return ZWZ_OK;
    HIPCHK(hipSetDevice(c->device));
    k.wrap = (uint32_t)wrap;
    const DstreamIndex X{d_idx, d_idx_len, span, 0, 0};
    if (span_) k.ix = &X;
    return dstream_launch(c, k);
}

}  // namespace

uint64_t zwz_deflate_stream_bound(uint64_t n, int wrap) { return dstream_bound(n, (uint32_t)wrap); }

int zwz_deflate_streams_dev(zwz_ctx* c, int wrap, const uint8_t* d_in, const uint64_t* in_off, const uint64_t* in_len, uint32_t n, uint8_t* d_out,
                            const uint64_t* out_off, const uint64_t* out_cap, uint64_t* d_out_len, uint32_t* d_status) {
    return dstream_dev(c, "zwz_deflate_streams_dev", wrap, DstreamCall{0, d_in, in_off, in_len, n, d_out, out_off, out_cap, d_out_len, d_status});
}

uint64_t zwz_deflate_stream_index_bound(uint64_t n, uint32_t span) {
    if (span == 0) span = kIdxSpanDefault;
    return index_span_ok(span) ? index_flush_bound(n, span) : 0u;
}

int zwz_deflate_streams_index_dev(zwz_ctx* c, int wrap, const uint8_t* d_in, const uint64_t* in_off, const uint64_t* in_len, uint32_t n, uint8_t* d_out,
                                  const uint64_t* out_off, const uint64_t* out_cap, uint64_t* d_out_len, uint32_t* d_status, uint32_t span, uint8_t* d_idx,
                                  const uint64_t* idx_off, const uint64_t* idx_cap, uint64_t* d_idx_len) {
    DstreamCall k{0, d_in, in_off, in_len, n, d_out, out_off, out_cap, d_out_len, d_status};
    k.idx_off = idx_off; k.idx_cap = idx_cap;
    return dstream_dev(c, "zwz_deflate_streams_index_dev", wrap, k, &span, d_idx, d_idx_len);
}

uint64_t zwz_deflate_dep_stream_bound(uint64_t n, int wrap) { return dep_stream_bound(n, (uint32_t)wrap); }

int zwz_deflate_dep_streams_dev(zwz_ctx* c, int wrap, const uint8_t* d_in, const uint64_t* in_off, const uint64_t* in_len, uint32_t n, uint8_t* d_out,
                                const uint64_t* out_off, const uint64_t* out_cap, uint64_t* d_out_len, uint32_t* d_status) {
    DstreamCall k{0, d_in, in_off, in_len, n, d_out, out_off, out_cap, d_out_len, d_status};
    k.form = kPiecesDep;
    return dstream_dev(c, "zwz_deflate_dep_streams_dev", wrap, k);
}

uint64_t zwz_deflate_dep_stream_index_bound(uint64_t n, uint32_t span) {
    if (span == 0) span = kIdxSpanDefault;
    return index_span_ok(span) ? index_dep_bound(n, span) : 0u;
}

int zwz_deflate_dep_streams_index_dev(zwz_ctx* c, int wrap, const uint8_t* d_in, const uint64_t* in_off, const uint64_t* in_len, uint32_t n, uint8_t* d_out,
                                      const uint64_t* out_off, const uint64_t* out_cap, uint64_t* d_out_len, uint32_t* d_status, uint32_t span, uint8_t* d_idx,
                                      const uint64_t* idx_off, const uint64_t* idx_cap, uint64_t* d_idx_len) {
    DstreamCall k{0, d_in, in_off, in_len, n, d_out, out_off, out_cap, d_out_len, d_status};
    k.idx_off = idx_off; k.idx_cap = idx_cap; k.form = kPiecesDep;
    return dstream_dev(c, "zwz_deflate_dep_streams_index_dev", wrap, k, &span, d_idx, d_idx_len);
}

// One slice of kFileSlicePieces whole pieces at a time: its pieces alone (partial), and its own checksum, which the host joins onto
// the file's by the slice's length.  The header goes in front of the first slice and 03 00 + trailer behind the last.
// With dst_idx the index as well (index_core.h: the index at full-flush points), at the context's "index_span_bytes": the entries of
// each slice come from the same kernels, which are told the decoded bytes and the stream bytes in front of the slice; the host appends
// them and seals the header once the trailer is known.  The small buffers then hold, behind the slice's results, its count of
// entries and, from byte 64, the entries themselves.
namespace {

// dep: dependent pieces (zwz_deflate_dep_stream_file).  A slice's input then runs through a second device buffer that keeps the last
// kDepDictBytes of the slice before in front of it, so that the slice's first piece finds its dictionary where every other piece does;
// with an index, the slice's windows come back behind its entries (the host knows how many: index_dep_step) and are appended to the
// file's, which go behind all entries when the index is sealed.
struct DevBytes { uint8_t* p = nullptr; ~DevBytes() { if (p) (void)hipFree(p); } };

int deflate_stream_file_core(zwz_ctx* c, int wrap_, const char* src, const char* dst, const char* dst_idx, PieceForm F) {
    if (!c || !src || !dst || wrap_ < ZWZ_WRAP_RAW || wrap_ > ZWZ_WRAP_GZIP) return ZWZ_E_INVALID;
    const bool dep = F.dict != 0u;
    if (dep) if (int rc = dep_strategy_ok(c, dst_idx ? "zwz_deflate_dep_stream_file_index" : "zwz_deflate_dep_stream_file")) return rc;
    const uint32_t wrap = (uint32_t)wrap_;
    HIPCHK(hipSetDevice(c->device));
    FileJob job;
    if (int rc = job.open(src, dst)) return rc;
    const uint32_t file_pieces = dep ? 2u * kFileSlicePieces : kFileSlicePieces;       // (the same 16.7 MB of input)
    const uint32_t pieces = c->max_batch < file_pieces ? c->max_batch : file_pieces;
    const size_t S = (size_t)pieces * F.piece;
    const size_t O = round_up((size_t)pieces * (dep ? dep_piece_bound(kDepPieceBytes, kDepDictBytes) : piece_bound(kPieceBytes)), 16);
    const uint64_t win_base = index_flush_bytes(pieces);                                // dep: where a slice's windows come back
    const uint64_t ent_cap = !dst_idx ? 0u : dep ? win_base + (uint64_t)pieces * kDepDictBytes : index_flush_bytes(pieces);      // (the header's 64 bytes are the results' place)
    const size_t small = dst_idx ? (size_t)ent_cap : 64;
    if (int rc = job.alloc({S + 16, S + 16, O, O, small}, {S + 16, O, small})) return rc;
    DevBytes work;                                  // dep: [the dictionary | the slice]
    if (dep) HIPCHK(hipMalloc(reinterpret_cast<void**>(&work.p), kDepDictBytes + S + 16));
    std::vector<uint8_t> wins;                      // dep: the index's windows as they grow
    const uint64_t step = index_dep_step(c->index_span_bytes);
    uint64_t slice_cnt = 0;                         // dep: the entries the slice in flight must report
    std::vector<uint8_t> ents(kIdxHeader);          // the index as it grows: the header's place, then the entries
    uint64_t pos = dstream_header_bytes(wrap);      // stream bytes in front of the next slice
    uint8_t frame[kGzipHeaderBytes + 2 + 8];
    const uint32_t hdr = dstream_header_bytes(wrap);
    for (uint32_t i = 0; i < hdr; i++) frame[i] = (uint8_t)dstream_header_byte(wrap, i, zlib_flg_of(c->level, c->strategy), gzip_xfl_of(c->strategy));
    if (hdr && fwrite(frame, 1, hdr, job.out) != hdr) { set_error("write error on %s", job.part.c_str()); return ZWZ_E_IO; }
    uint32_t check = dstream_check_init(wrap);
    uint64_t total_in = 0;
    const int rc = run_slices(c, job, S,
        [&](size_t n, SliceResult* d_res, SliceResult* h_res) {
            const uint64_t zero = 0, dict = F.dict, len = n, cap = O;
            const uint32_t* d_chk = nullptr;
            const DstreamIndex X{job.dp(2), nullptr, c->index_span_bytes, total_in, pos};
            const uint64_t* d_cnt = nullptr;
            // the slice's input: where it was copied to, or (dep) behind its dictionary in `work`
            DstreamCall k{wrap, dep ? work.p : job.dp(0), &dict, &len, 1, job.dp(1), &zero, &cap, &d_res->out_len, &d_res->status};
            k.partial = true; k.d_chk = &d_chk; k.d_cnt = &d_cnt;
            if (dst_idx) { k.ix = &X; k.idx_off = &zero; k.idx_cap = &ent_cap; }
            k.form = F; k.lead = total_in ? F.dict : 0u; k.win_base = win_base;
            if (dep) {
                const uint64_t k0 = total_in / kDepPieceBytes, k1 = k0 + (n + kDepPieceBytes - 1) / kDepPieceBytes;
                slice_cnt = (k1 + step - 1) / step - (k0 + step - 1) / step;          // pieces k0 .. k1 - 1 whose number is a multiple of step
                HIPCHK(hipMemcpyAsync(work.p + dict, job.dp(0), n, hipMemcpyDeviceToDevice, c->stream));
            }
            if (int rc = dstream_launch(c, k)) return rc;
            if (dep && n == S) HIPCHK(hipMemcpyAsync(work.p, work.p + n, dict, hipMemcpyDeviceToDevice, c->stream));      // the next slice's dictionary (S >= 2 dict: no overlap)
            HIPCHK(hipMemcpyAsync(h_res, d_res, 12, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipMemcpyAsync(&h_res->check, d_chk, 4, hipMemcpyDeviceToHost, c->stream));
            if (dst_idx) {
                uint8_t* h = reinterpret_cast<uint8_t*>(h_res);
                HIPCHK(hipMemcpyAsync(h + 16, d_cnt, 8, hipMemcpyDeviceToHost, c->stream));
                HIPCHK(hipMemcpyAsync(h + kIdxHeader, job.dp(2) + kIdxHeader, (size_t)index_flush_bytes(pieces) - kIdxHeader, hipMemcpyDeviceToHost, c->stream));
                const uint64_t nwin = dep ? slice_cnt - (total_in ? 0u : 1u) : 0u;       // (the file's first entry has no window)
                if (nwin) HIPCHK(hipMemcpyAsync(h + win_base, job.dp(2) + win_base, (size_t)(nwin * kDepDictBytes), hipMemcpyDeviceToHost, c->stream));
            }
            return (int)ZWZ_OK;
        },
        [&](size_t n, const SliceResult& r) {
            if (r.status || r.out_len > O) { set_error("deflate stream: a slice needs %llu bytes, above its bound", (unsigned long long)r.out_len); return (int)ZWZ_E_FORMAT; }
            if (wrap == kWrapZlib) check = AdlerSum::join(check, r.check, AdlerSum::pof(n));
            else if (wrap == kWrapGzip) check = CrcSum::join(check, r.check, CrcSum::pof(n));
            total_in += n; pos += r.out_len;
            if (dst_idx) {
                const uint8_t* h = reinterpret_cast<const uint8_t*>(&r);
                const uint64_t cnt = le64_of(h + 16);
                if (cnt > pieces || (dep && cnt != slice_cnt)) { set_error("deflate stream: a slice of %u pieces reports %llu index entries", pieces, (unsigned long long)cnt); return (int)ZWZ_E_FORMAT; }
                ents.insert(ents.end(), h + kIdxHeader, h + kIdxHeader + cnt * kIdxEntry);
                if (dep) wins.insert(wins.end(), h + win_base, h + win_base + (cnt - (total_in == n ? 1u : 0u)) * kDepDictBytes);
            }
            return (int)ZWZ_OK;
        });
    if (rc) return rc;
    const uint32_t tail = 2u + dstream_trailer_bytes(wrap);
    for (uint32_t i = 0; i < tail; i++) frame[i] = (uint8_t)dstream_tail_byte(wrap, i, check, total_in);
    if (fwrite(frame, 1, tail, job.out) != tail) { set_error("write error on %s", job.part.c_str()); return ZWZ_E_IO; }
    if (!dst_idx) return job.commit(dst);
    // the index: an empty input has its one entry from here; written as .part, and renamed only behind the stream
    if (!total_in) { ents.resize(kIdxHeader + kIdxEntry); index_flush_entry(ents.data() + kIdxHeader, 8u * hdr, 0); }
    const uint64_t count = (ents.size() - kIdxHeader) / kIdxEntry;
    if (count > 0xffffffffull) { set_error("deflate stream: more than 2^32 - 1 index entries"); return ZWZ_E_INVALID; }
    if (dep && (count != index_dep_count(total_in, c->index_span_bytes) || wins.size() != (count - 1u) * kDepDictBytes)) { set_error("deflate stream: the index's entries and windows do not add up"); return ZWZ_E_FORMAT; }
    // the windows (dep) behind the entries, zero padding behind them (index_dep_bytes without windows is index_flush_bytes)
    ents.insert(ents.end(), wins.begin(), wins.end());
    ents.resize((size_t)((kIdxHeader + count * kIdxEntry + wins.size() + 15u) & ~15ull), 0);
    index_seal(ents.data(), ents.size(), wrap, c->index_span_bytes, pos + tail, total_in, (uint32_t)count, index_flush_end_bit(pos), wrap == kWrapRaw ? 0u : check);
    return commit_with_index_bytes(dst_idx, dst, ents.data(), ents.size(), [&] { return job.commit(dst); });
}

}  // namespace

int zwz_deflate_stream_file(zwz_ctx* c, int wrap, const char* src, const char* dst) { return deflate_stream_file_core(c, wrap, src, dst, nullptr, kPiecesAlone); }

int zwz_deflate_stream_file_index(zwz_ctx* c, int wrap, const char* src, const char* dst, const char* dst_idx) {
    if (!dst_idx) return ZWZ_E_INVALID;
    return deflate_stream_file_core(c, wrap, src, dst, dst_idx, kPiecesAlone);
}

int zwz_deflate_dep_stream_file(zwz_ctx* c, int wrap, const char* src, const char* dst) { return deflate_stream_file_core(c, wrap, src, dst, nullptr, kPiecesDep); }

int zwz_deflate_dep_stream_file_index(zwz_ctx* c, int wrap, const char* src, const char* dst, const char* dst_idx) {
    if (!dst_idx) return ZWZ_E_INVALID;
    return deflate_stream_file_core(c, wrap, src, dst, dst_idx, kPiecesDep);
}
