// zwz_dstream.cpp -- zwz_deflate_streams_dev / zwz_deflate_stream_file of include/zwz.h: the host driver around the codec.  Per slice
// of at most max_batch pieces: dstream_layout + crc32_blocks (gzip) + zwz_deflate_batch_dev + dstream_size + the scan +
// dstream_combine + dstream_pack, all on the context's stream; what runs from slice to slice (the scan's base, every stream's first
// scan value and checksum) stays in device memory, so the host never waits between slices.
#include <algorithm>
#include <cstring>
#include <vector>

#include "dstream_core.h"
#include "zwz_api_internal.h"
#include "zwz_bgzf.h"
#include "zwz_dstream.h"
#include "zwz_filejob.h"

using namespace zwz;

#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return hip_fail(e_, #x); } while (0)

namespace {

constexpr uint32_t kFileSlicePieces = 256;          // pieces per slice of zwz_deflate_stream_file: 16.7 MB of input

inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }
size_t pieces_bytes(uint32_t m) { return up256((size_t)m * ZWZ_DEV_STRIDE + 256) + 2 * up256((size_t)m * 8) + 7 * up256((size_t)m * 4) + 256; }

struct PiecesView { DstreamPieces P; uint64_t* base; uint32_t* err; };
PiecesView pieces_view(zwz_ctx* c) {
    const size_t m = c->ds_cap;
    uint8_t* p = static_cast<uint8_t*>(c->ds_ws);
    auto take = [&](size_t bytes) { uint8_t* r = p; p += up256(bytes); return r; };
    auto u32s = [&]() { return reinterpret_cast<uint32_t*>(take(m * 4)); };
    PiecesView v;
    v.P.slots = take(m * ZWZ_DEV_STRIDE + 256);       // (wg_copy reads up to 3 bytes past a slot's bytes)
    v.P.off = reinterpret_cast<uint64_t*>(take(m * 8)); v.P.x = reinterpret_cast<uint64_t*>(take(m * 8));
    v.P.len = u32s(); v.P.olen = u32s(); v.P.crc = u32s(); v.P.sidx = u32s(); v.P.slen = u32s(); v.P.hbit = u32s(); v.P.ebit = u32s();
    v.base = reinterpret_cast<uint64_t*>(take(16)); v.err = reinterpret_cast<uint32_t*>(v.base + 1);
    return v;
}

// in_off, in_len, out_off, out_cap (n each), pfirst (n + 1) -- copied from the host -- then xs (n) and chk (n)
size_t streams_host_bytes(uint32_t n) { return (5 * (size_t)n + 1) * 8; }
size_t streams_dev_bytes(uint32_t n) { return streams_host_bytes(n) + (size_t)n * 8 + (size_t)n * 4 + 64; }

int ensure_dstream(zwz_ctx* c, uint32_t pieces, uint32_t streams, bool crc) {
    if (crc && !c->crc_tables) {
        HIPCHK(hipMalloc(&c->crc_tables, sizeof(CrcTables)));
        HIPCHK(launch_crc_tables(static_cast<CrcTables*>(c->crc_tables), c->stream));
    }
    if (!c->ds_copied) HIPCHK(hipEventCreateWithFlags(&c->ds_copied, hipEventDisableTiming));
    if (pieces > c->ds_cap || streams > c->ds_streams) HIPCHK(hipStreamSynchronize(c->stream));
    if (pieces > c->ds_cap) {
        if (c->ds_ws) { (void)hipFree(c->ds_ws); c->ds_ws = nullptr; c->ds_cap = 0; }
        HIPCHK(hipMalloc(&c->ds_ws, pieces_bytes(pieces)));
        c->ds_cap = pieces;
    }
    if (streams > c->ds_streams) {
        if (c->ds_dev) { (void)hipFree(c->ds_dev); c->ds_dev = nullptr; }
        if (c->ds_host) { (void)hipHostFree(c->ds_host); c->ds_host = nullptr; }
        c->ds_streams = 0;
        HIPCHK(hipMalloc(&c->ds_dev, streams_dev_bytes(streams)));
        HIPCHK(hipHostMalloc(&c->ds_host, streams_host_bytes(streams), hipHostMallocDefault));
        c->ds_streams = streams;
    }
    return ZWZ_OK;
}

// The device part, arguments checked by the caller.  partial: every stream's pieces alone, and its checksum left in *d_chk (the file
// function's slices).  Returns with everything queued on the context's stream.
int dstream_launch(zwz_ctx* c, uint32_t wrap, const uint8_t* d_in, const uint64_t* in_off, const uint64_t* in_len, uint32_t n, uint8_t* d_out,
                   const uint64_t* out_off, const uint64_t* out_cap, uint64_t* d_out_len, uint32_t* d_status, bool partial, const uint32_t** d_chk) {
    // pieces are counted in 64 bits: the only limit is that they, and the output they need, can be counted at all
    std::vector<uint64_t> pfirst((size_t)n + 1);
    pfirst[0] = 0;
    for (uint32_t i = 0; i < n; i++) {
        if (in_len[i] > ~0ull - kPieceBytes || (in_len[i] + kPieceBytes - 1) / kPieceBytes > (~0ull >> 18) - pfirst[i]) {
            set_error("zwz_deflate_streams_dev: the streams up to stream %u have more than 2^46 pieces", i);
            return ZWZ_E_INVALID;
        }
        pfirst[i + 1] = pfirst[i] + (in_len[i] + kPieceBytes - 1) / kPieceBytes;
    }
    const uint64_t G = pfirst[n];
    const uint32_t M = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(G, 1), c->max_batch);
    if (int rc = ensure_dstream(c, M, n, wrap == kWrapGzip)) return rc;
    // the pinned arrays may still be the source of the previous call's copy
    HIPCHK(hipEventSynchronize(c->ds_copied));
    uint64_t* h = static_cast<uint64_t*>(c->ds_host);
    memcpy(h, in_off, (size_t)n * 8); memcpy(h + n, in_len, (size_t)n * 8);
    memcpy(h + 2 * (size_t)n, out_off, (size_t)n * 8); memcpy(h + 3 * (size_t)n, out_cap, (size_t)n * 8);
    memcpy(h + 4 * (size_t)n, pfirst.data(), ((size_t)n + 1) * 8);
    uint64_t* d = static_cast<uint64_t*>(c->ds_dev);
    HIPCHK(hipMemcpyAsync(d, h, streams_host_bytes(n), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipEventRecord(c->ds_copied, c->stream));
    DstreamStreams S;
    S.in_off = d; S.in_len = d + n; S.out_off = d + 2 * (size_t)n; S.out_cap = d + 3 * (size_t)n; S.pfirst = d + 4 * (size_t)n;
    S.xs = d + 5 * (size_t)n + 1; S.chk = reinterpret_cast<uint32_t*>(S.xs + n); S.n = n;
    if (d_chk) *d_chk = S.chk;
    const DstreamOut O{d_out, d_out_len, d_status, wrap, partial ? 1u : 0u};
    const PiecesView v = pieces_view(c);
    const CrcTables* tab = static_cast<const CrcTables*>(c->crc_tables);
    HIPCHK(hipMemsetAsync(v.base, 0, 16, c->stream));
    HIPCHK(launch_dstream_begin(S, O, c->stream));
    uint32_t s0 = 0;                                  // the stream of the slice's first piece
    for (uint64_t g0 = 0; g0 < G; g0 += M) {
        const uint32_t m = (uint32_t)std::min<uint64_t>(G - g0, M);
        while (pfirst[s0 + 1] <= g0) s0++;
        uint32_t s1 = s0;                             // the stream of its last
        while (pfirst[s1 + 1] < g0 + m) s1++;
        HIPCHK(launch_dstream_layout(S, v.P, g0, m, c->stream));
        if (wrap == kWrapGzip) HIPCHK(launch_crc32_blocks(tab, d_in, v.P.off, v.P.len, m, v.P.crc, c->cu_count, c->stream));
        if (int rc = zwz_deflate_batch_dev(c, d_in, v.P.off, v.P.len, m, v.P.slots, ZWZ_DEV_STRIDE, v.P.olen)) return rc;
        DeflateArgs a;                                // the slice's block records are still in the codec's workspace
        carve_workspace(c, a);
        HIPCHK(launch_dstream_size(a.info, a.blocks, a.plans, v.P, m, v.err, c->stream));
        HIPCHK(launch_bgzf_scan(v.P.slen, m, 0, ~0u, v.P.x, v.base, v.err + 1, c->stream));
        HIPCHK(launch_dstream_combine(S, v.P, g0, m, s0, s1 - s0 + 1, wrap, c->stream));
        HIPCHK(launch_dstream_pack(S, v.P, g0, m, O, v.err, c->stream));
        s0 = s1;
    }
    return ZWZ_OK;
}

}  // namespace

uint64_t zwz_deflate_stream_bound(uint64_t n, int wrap) { return dstream_bound(n, (uint32_t)wrap); }

int zwz_deflate_streams_dev(zwz_ctx* c, int wrap, const uint8_t* d_in, const uint64_t* in_off, const uint64_t* in_len, uint32_t n, uint8_t* d_out,
                            const uint64_t* out_off, const uint64_t* out_cap, uint64_t* d_out_len, uint32_t* d_status) {
    if (!c || wrap < ZWZ_WRAP_RAW || wrap > ZWZ_WRAP_GZIP) return ZWZ_E_INVALID;
    if (n && (!d_in || !in_off || !in_len || !d_out || !out_off || !out_cap || !d_out_len || !d_status)) return ZWZ_E_INVALID;
    if (((uintptr_t)d_in & 15u) || ((uintptr_t)d_out & 15u)) return ZWZ_E_INVALID;
    for (uint32_t i = 0; i < n; i++)
        if ((in_off[i] & 15u) || (out_off[i] & 15u)) { set_error("zwz_deflate_streams_dev: stream %u: offsets must be multiples of 16", i); return ZWZ_E_INVALID; }
    if (n == 0) return ZWZ_OK;
    HIPCHK(hipSetDevice(c->device));
    return dstream_launch(c, (uint32_t)wrap, d_in, in_off, in_len, n, d_out, out_off, out_cap, d_out_len, d_status, false, nullptr);
}

// One slice of kFileSlicePieces whole pieces at a time: its pieces alone (partial), and its own checksum, which the host joins onto
// the file's by the slice's length.  The header goes in front of the first slice and 03 00 + trailer behind the last.
int zwz_deflate_stream_file(zwz_ctx* c, int wrap_, const char* src, const char* dst) {
    if (!c || !src || !dst || wrap_ < ZWZ_WRAP_RAW || wrap_ > ZWZ_WRAP_GZIP) return ZWZ_E_INVALID;
    const uint32_t wrap = (uint32_t)wrap_;
    HIPCHK(hipSetDevice(c->device));
    FileJob job;
    if (int rc = job.open(src, dst)) return rc;
    const uint32_t pieces = c->max_batch < kFileSlicePieces ? c->max_batch : kFileSlicePieces;
    const size_t S = (size_t)pieces * kPieceBytes, O = ((size_t)pieces * piece_bound(kPieceBytes) + 15) & ~(size_t)15;
    for (int i = 0; i < 2; i++) HIPCHK(hipHostMalloc(&job.h[i], S + 16, hipHostMallocDefault));
    for (int i = 2; i < 4; i++) HIPCHK(hipHostMalloc(&job.h[i], O, hipHostMallocDefault));
    HIPCHK(hipHostMalloc(&job.h[4], 64, hipHostMallocDefault));
    HIPCHK(hipMalloc(&job.d[0], S + 16));
    HIPCHK(hipMalloc(&job.d[1], O));
    HIPCHK(hipMalloc(&job.d[2], 64));
    uint8_t* d_in = static_cast<uint8_t*>(job.d[0]); uint8_t* d_out = static_cast<uint8_t*>(job.d[1]);
    uint64_t* d_len = static_cast<uint64_t*>(job.d[2]); uint32_t* d_st = reinterpret_cast<uint32_t*>(d_len + 1);
    uint64_t* h_len = static_cast<uint64_t*>(job.h[4]); uint32_t* h_st = reinterpret_cast<uint32_t*>(h_len + 1); uint32_t* h_chk = h_st + 1;
    uint8_t frame[kGzipHeaderBytes + 2 + 8];
    const uint32_t hdr = dstream_header_bytes(wrap);
    for (uint32_t i = 0; i < hdr; i++) frame[i] = (uint8_t)dstream_header_byte(wrap, i);
    if (hdr && fwrite(frame, 1, hdr, job.out) != hdr) { set_error("write error on %s", job.part.c_str()); return ZWZ_E_IO; }
    uint32_t check = dstream_check_init(wrap);
    uint64_t total_in = 0;
    size_t n = 0;
    job.start_read(static_cast<uint8_t*>(job.h[0]), S);
    if (int rc = job.finish_read(&n)) return rc;
    for (int b = 0; n; b ^= 1) {
        uint8_t* hin = static_cast<uint8_t*>(job.h[b]);
        uint8_t* hout = static_cast<uint8_t*>(job.h[2 + b]);
        const uint64_t zero = 0, len = n, cap = O;
        const uint32_t* d_chk = nullptr;
        HIPJOB(hipMemcpyAsync(d_in, hin, n, hipMemcpyHostToDevice, c->stream));
        if (int rc = dstream_launch(c, wrap, d_in, &zero, &len, 1, d_out, &zero, &cap, d_len, d_st, true, &d_chk)) { job.join(); return rc; }
        HIPJOB(hipMemcpyAsync(h_len, d_len, 12, hipMemcpyDeviceToHost, c->stream));
        HIPJOB(hipMemcpyAsync(h_chk, d_chk, 4, hipMemcpyDeviceToHost, c->stream));
        if (n == S) job.start_read(static_cast<uint8_t*>(job.h[b ^ 1]), S);     // (a short slice is the last one)
        HIPJOB(hipStreamSynchronize(c->stream));
        const uint64_t out_len = *h_len;
        if (*h_st || out_len > O) { job.join(); set_error("deflate stream: a slice needs %llu bytes, above its bound", (unsigned long long)out_len); return ZWZ_E_FORMAT; }
        if (wrap == kWrapZlib) check = AdlerSum::join(check, *h_chk, AdlerSum::pof(n));
        else if (wrap == kWrapGzip) check = CrcSum::join(check, *h_chk, CrcSum::pof(n));
        total_in += n;
        HIPJOB(hipMemcpyAsync(hout, d_out, out_len, hipMemcpyDeviceToHost, c->stream));
        HIPJOB(hipStreamSynchronize(c->stream));
        if (int rc = job.finish_write()) { job.join(); return rc; }
        job.start_write(hout, out_len);
        size_t next = 0;
        if (n == S) { if (int rc = job.finish_read(&next)) { job.join(); return rc; } }
        n = next;
    }
    if (int rc = job.finish_write()) return rc;
    const uint32_t tail = 2u + dstream_trailer_bytes(wrap);
    for (uint32_t i = 0; i < tail; i++) frame[i] = (uint8_t)dstream_tail_byte(wrap, i, check, total_in);
    if (fwrite(frame, 1, tail, job.out) != tail) { set_error("write error on %s", job.part.c_str()); return ZWZ_E_IO; }
    return job.commit(dst);
}
