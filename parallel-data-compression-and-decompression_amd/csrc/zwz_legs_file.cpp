// zwz_legs_file.cpp -- zwz_inflate_legs_file of include/zwz.h: one file holding one raw, zlib or gzip stream of ANY length decoded, and indexed,
// in legs that pass through staging windows of bounded size.  The loop and its rules are legfile_core.h's (shared with
// the CPU restatement, tests/emu_legfile); this file is where the windows live: one pinned buffer and one device window for the compressed
// bytes, one device window for the decoded ones, two pinned buffers behind it that the writer thread empties while the next leg runs, and a
// spool file for the index's windows.  It makes no stream faster: a stream runs at the one-wave rate.
// Every wait is a join of a thread that only does file I/O, or a stream synchronisation (zwz_filejob.h's rule).
#include <sys/stat.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "dstream_core.h"
#include "zwz_filejob.h"
#include "zwz_index.h"

using namespace zwz;

namespace {

constexpr size_t kPackBytes = 4u << 20;          // the windows of committed entries leave the device this many bytes at a time (+ one window)
constexpr size_t kSpoolChunk = 1u << 20;         // the spool is appended to the index through a buffer of this size

// A grow-only allocation of one call, counted
struct Mem {
    void* p = nullptr; size_t n = 0; bool pinned = false;
    template <class T = uint8_t> T* as() const { return static_cast<T*>(p); }
};

// The per-file state of one call: files, buffers, the writer thread.  Everything is released, and every file that is not a finished
// result removed, whatever the outcome.
struct LegFileJob {
    zwz_ctx* c = nullptr;
    const char* src = nullptr;
    uint32_t wrap = 0, span = 0;
    FILE *in = nullptr, *out = nullptr, *spool = nullptr;
    std::string out_part, spool_path;
    Mem h_in{nullptr, 0, true}, h_commit[2] = {{nullptr, 0, true}, {nullptr, 0, true}}, h_pack{nullptr, 0, true}, h_small{nullptr, 0, true}, h_pieces{nullptr, 0, true};
    Mem d_in, d_out, d_carry, d_ent, d_pack, d_small, d_pieces;
    uint64_t live = 0, peak = 0;
    uint64_t base = 0; size_t have = 0;          // file offset of h_in[0]; the bytes of the file that stand in h_in
    uint64_t out_len = 0;                        // the output window's bytes (what a gather may read)
    int b = 0;
    std::thread writer; bool write_err = false;
    std::vector<IndexMove> moves;

    ~LegFileJob() {
        if (writer.joinable()) writer.join();
        if (c) (void)hipStreamSynchronize(c->stream);
        for (Mem* m : {&h_in, &h_commit[0], &h_commit[1], &h_pack, &h_small, &h_pieces}) if (m->p) (void)hipHostFree(m->p);
        for (Mem* m : {&d_in, &d_out, &d_carry, &d_ent, &d_pack, &d_small, &d_pieces}) if (m->p) (void)hipFree(m->p);
        if (in) fclose(in);
        if (out) { fclose(out); unlink(out_part.c_str()); }
        if (spool) { fclose(spool); unlink(spool_path.c_str()); }
    }
    // At least `need` bytes; the first `keep` bytes survive a pinned buffer's growth.  (The caller has waited for whatever used the old one.)
    int grow(Mem& m, size_t need, size_t keep = 0) {
        if (m.n >= need) return ZWZ_OK;
        void* q = nullptr;
        if (m.pinned) HIPCHK(hipHostMalloc(&q, need, hipHostMallocDefault)); else HIPCHK(hipMalloc(&q, need));
        if (m.p) { if (keep) memcpy(q, m.p, keep); if (m.pinned) (void)hipHostFree(m.p); else (void)hipFree(m.p); }
        live += need - m.n; peak = std::max(peak, live);
        m.p = q; m.n = need;
        return ZWZ_OK;
    }
    int finish_write() {
        if (writer.joinable()) writer.join();
        if (write_err) { set_error("write error on %s", out_part.c_str()); return ZWZ_E_IO; }
        return ZWZ_OK;
    }

    // the small arrays of a leg, the same layout pinned and on the device
    struct Small { LegState* leg; LegPlan* legw; LegStage* legf; uint4* order; uint64_t *zero, *idx_cap, *out_len, *idx_len; uint32_t* status; };
    static Small small_layout(Carver& w) {
        Small s;
        s.leg = w.take<LegState>(1); s.legw = w.take<LegPlan>(1); s.legf = w.take<LegStage>(1); s.order = w.take<uint4>(1);
        s.zero = w.take<uint64_t>(1); s.idx_cap = w.take<uint64_t>(1); s.out_len = w.take<uint64_t>(1); s.idx_len = w.take<uint64_t>(1); s.status = w.take<uint32_t>(1);
        return s;
    }

    // ---- legfile_loop's io -----------------------------------------------------------------------------------------------------------
    int input(const LegPlan& w) {
        const size_t need = (size_t)legfile_in_bytes(w);
        size_t keep = 0;
        if (w.in_base >= base && w.in_base <= base + have) keep = (size_t)(base + have - w.in_base);
        if (keep) memmove(h_in.as(), h_in.as() + (w.in_base - base), keep);
        else if (fseeko(in, (off_t)w.in_base, SEEK_SET) != 0) { set_error("read error on %s", src); return ZWZ_E_IO; }
        base = w.in_base; have = keep;
        if (int rc = grow(h_in, std::max(need, have), have)) return rc;
        if (int rc = grow(d_in, need)) return rc;
        if (have < w.in_len) {
            bool io_err = false;
            const size_t want = w.in_len - have, got = read_full(in, h_in.as() + have, want, &io_err);
            if (io_err || got != want) { set_error("read error on %s", src); return ZWZ_E_IO; }
            have += got;
        }
        HIPCHK(hipMemcpyAsync(d_in.p, h_in.p, w.in_len, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemsetAsync(d_in.as() + w.in_len, 0, need - w.in_len, c->stream));
        return ZWZ_OK;
    }
    int output(const LegPlan& w, uint64_t from, uint32_t n, uint32_t slots) {
        if (n) {
            if (int rc = grow(d_carry, kIdxWindow + 16)) return rc;
            HIPCHK(hipMemcpyAsync(d_carry.p, d_out.as() + from, n, hipMemcpyDeviceToDevice, c->stream));
        }
        if (d_out.n < legfile_out_bytes(w)) HIPCHK(hipStreamSynchronize(c->stream));
        if (int rc = grow(d_out, (size_t)legfile_out_bytes(w))) return rc;
        if (n) HIPCHK(hipMemcpyAsync(d_out.p, d_carry.p, n, hipMemcpyDeviceToDevice, c->stream));
        out_len = w.out_len;
        return grow(d_ent, kIdxHeader + (size_t)slots * kIdxEntry);
    }
    int leg(LegState* s, const LegPlan& w, const LegStage& g) {
        Carver wh(h_small.p), wd(d_small.p);
        const Small H = small_layout(wh), D = small_layout(wd);
        *H.leg = *s; *H.legw = w; *H.legf = g; *H.order = make_uint4(0, 0, w.in_len, 0);
        *H.zero = 0; *H.idx_cap = kLegFileIdxCap;
        HIPCHK(hipMemcpyAsync(d_small.p, h_small.p, wh.used, hipMemcpyHostToDevice, c->stream));
        HIPCHK(launch_inflate_legs(InflateLegArgs{d_in.as(), D.order, 1, d_out.as(), D.zero, D.out_len, D.status, spool ? d_ent.as() : nullptr, D.zero, D.idx_cap, D.idx_len, span,
                                                  D.legw, D.leg, wrap, c->inflate_serial_header, D.legf}, c->stream));
        HIPCHK(hipMemcpyAsync(H.leg, D.leg, sizeof(LegState), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        *s = *H.leg;
        return ZWZ_OK;
    }
    template <class Sum>
    int sum(uint64_t at, uint64_t n, LegSum* sm) {
        if (!n) return ZWZ_OK;
        IndexPieces f{};
        f.out = d_out.as() + at; f.total = n; f.wrap = wrap; f.head = index_head_bytes((uint32_t)(at & 15u), n);      // (the window's first byte is 16-byte aligned)
        f.pieces = (uint32_t)index_piece_count(wrap, f.head, n);
        const size_t arr = round_up((size_t)f.pieces * 8, 256);
        if (int rc = grow(d_pieces, 3 * arr)) return rc;
        if (int rc = grow(h_pieces, 2 * arr)) return rc;
        f.piece_off = d_pieces.as<uint64_t>(); f.piece_len = reinterpret_cast<uint32_t*>(d_pieces.as() + arr); f.piece_val = reinterpret_cast<uint32_t*>(d_pieces.as() + 2 * arr);
        uint32_t* len = h_pieces.as<uint32_t>();
        uint32_t* val = reinterpret_cast<uint32_t*>(h_pieces.as() + arr);
        HIPCHK(launch_index_piece_sums(c->buf[kBufCrcTables].as<const CrcTables>(), f, c->cu_count, c->stream));
        HIPCHK(hipMemcpyAsync(len, f.piece_len, (size_t)f.pieces * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(val, f.piece_val, (size_t)f.pieces * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        for (uint32_t j = 0; j < f.pieces; j++) legfile_sum_add<Sum>(*sm, val[j], len[j]);
        return ZWZ_OK;
    }
    int bytes(uint64_t at, uint64_t n) {
        if (!out) return ZWZ_OK;
        if (int rc = finish_write()) return rc;                        // (the write from two legs back used this buffer; the last one has ended too)
        // (doubled while it grows, so that commits of slowly rising lengths do not allocate one each; never beyond the window)
        if (h_commit[b].n < n) if (int rc = grow(h_commit[b], std::max<size_t>((size_t)n, std::min<size_t>(2 * h_commit[b].n, (size_t)out_len)))) return rc;
        uint8_t* p = h_commit[b].as();
        HIPCHK(hipMemcpyAsync(p, d_out.as() + at, (size_t)n, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        FILE* f = out;
        writer = std::thread([this, f, p, n] { if (fwrite(p, 1, (size_t)n, f) != n) write_err = true; });
        b ^= 1;
        return ZWZ_OK;
    }
    int entries(uint32_t slot, uint32_t k, uint64_t out_base, LegIndexParts* parts) {
        const size_t at = parts->entries.size();
        parts->entries.resize(at + (size_t)k * kIdxEntry);
        HIPCHK(hipMemcpy(parts->entries.data() + at, d_ent.as() + kIdxHeader + (size_t)slot * kIdxEntry, (size_t)k * kIdxEntry, hipMemcpyDeviceToHost));
        if (int rc = grow(d_pack, kPackBytes + kIdxWindow)) return rc;
        if (int rc = grow(h_pack, kPackBytes + kIdxWindow)) return rc;
        for (uint32_t i = 0; i < k;) {
            moves.clear();
            uint64_t fill = 0;
            for (; i < k && fill < kPackBytes; i++) {
                const uint8_t* e = parts->entries.data() + at + (size_t)i * kIdxEntry;
                const uint64_t off = le64_of(e + 8);
                const uint32_t hist = le32_at(e + 16);
                if (hist > kIdxWindow || off < out_base + hist || off - out_base > out_len) { set_error("zwz_inflate_legs_file: an index entry's window lies outside the leg's staging"); return ZWZ_E_FORMAT; }
                moves.push_back(IndexMove{off - hist - out_base, fill, hist, 0});
                fill += hist;
            }
            if (!fill) continue;
            if (int rc = grow(d_pieces, round_up(moves.size() * sizeof(IndexMove), 256))) return rc;
            HIPCHK(hipMemcpy(d_pieces.p, moves.data(), moves.size() * sizeof(IndexMove), hipMemcpyHostToDevice));
            HIPCHK(launch_index_gather(d_out.as(), out_len, d_pack.as(), d_pack.n, d_pieces.as<const IndexMove>(), (uint32_t)moves.size(), c->stream));
            HIPCHK(hipMemcpyAsync(h_pack.p, d_pack.p, (size_t)fill, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
            if (fwrite(h_pack.p, 1, (size_t)fill, spool) != fill) { set_error("write error on %s", spool_path.c_str()); return ZWZ_E_IO; }
            parts->windows(h_pack.as(), fill);
        }
        return ZWZ_OK;
    }
};

// header, entries, the spooled windows, zero padding -> f, the index's .part (commit_with_index's body)
bool write_index(FILE* f, LegFileJob& job, const LegIndexParts& parts, uint64_t stream_len, const LegState& s) {
    uint8_t head[kIdxHeader];
    const uint8_t zeros[16] = {};
    parts.header(head, job.wrap, job.span, stream_len, s);
    bool ok = fwrite(head, 1, kIdxHeader, f) == kIdxHeader && fwrite(parts.entries.data(), 1, parts.entries.size(), f) == parts.entries.size();
    std::vector<uint8_t> buf(kSpoolChunk);
    ok = ok && fflush(job.spool) == 0 && fseeko(job.spool, 0, SEEK_SET) == 0;
    for (uint64_t left = parts.win_bytes; ok && left;) {
        const size_t k = (size_t)std::min<uint64_t>(left, buf.size());
        ok = fread(buf.data(), 1, k, job.spool) == k && fwrite(buf.data(), 1, k, f) == k;
        left -= k;
    }
    return ok && fwrite(zeros, 1, parts.pad(), f) == parts.pad();
}

}  // namespace

extern "C" int zwz_inflate_legs_file(zwz_ctx* c, int wrap, const char* src, const char* dst, const char* dst_idx, uint64_t* stats) {
    if (!c || !src || (!dst && !dst_idx) || wrap < ZWZ_WRAP_RAW || wrap > ZWZ_WRAP_GZIP) return ZWZ_E_INVALID;
    uint64_t st[kLfStats] = {};
    if (stats) std::copy(st, st + kLfStats, stats);
    HIPCHK(hipSetDevice(c->device));
    if (int rc = ensure_crc_tables(c)) return rc;
    LegFileJob job;
    job.c = c; job.src = src; job.wrap = (uint32_t)wrap; job.span = c->index_span_bytes;
    job.in = fopen(src, "rb");
    if (!job.in) { set_error("cannot open %s", src); return ZWZ_E_IO; }
    fseeko(job.in, 0, SEEK_END);
    const uint64_t size = (uint64_t)ftello(job.in);
    fseeko(job.in, 0, SEEK_SET);
    if (dst) {
        job.out_part = std::string(dst) + ".part";
        job.out = fopen(job.out_part.c_str(), "wb");
        if (!job.out) { set_error("cannot create %s", job.out_part.c_str()); return ZWZ_E_IO; }
    }
    if (dst_idx) {
        job.spool_path = std::string(dst_idx) + ".part.windows";
        job.spool = fopen(job.spool_path.c_str(), "w+b");
        if (!job.spool) { set_error("cannot create %s", job.spool_path.c_str()); return ZWZ_E_IO; }
    }
    const size_t small = layout_bytes([](Carver& w) { LegFileJob::small_layout(w); });
    if (int rc = job.grow(job.h_small, small)) return rc;
    if (int rc = job.grow(job.d_small, small)) return rc;
    LegIndexParts parts;
    LegFileEnd end{};
    const int rc = legfile_loop(job, job.wrap, size, job.span, dst_idx != nullptr, c->leg_file_bytes, c->leg_file_out_bytes, kLegMaxIn, kLegMaxOut, &parts, &end, st);
    st[kLfBytes] = job.peak;
    if (stats) std::copy(st, st + kLfStats, stats);
    if (rc > 0) { set_error("zwz_inflate_legs_file: %s: a checksum was read outside the leg that made its bytes final", src); return ZWZ_E_FORMAT; }
    if (rc) return rc;
    if (int r = job.finish_write()) return r;
    const LegState& s = end.s;
    if (end.too_large) {
        set_error("zwz_inflate_legs_file: %s: stream status %u (ZWZ_STREAM_TOO_LARGE): one stretch between restart points is beyond a window's limit; the last restart point is at "
                  "compressed offset %llu, %llu decoded bytes", src, (unsigned)kStrTooLarge, (unsigned long long)(s.bit >> 3), (unsigned long long)s.out);
        return ZWZ_E_FORMAT;
    }
    if (end.status == kStrChecksum || end.status == kStrLength) { set_error("zwz_inflate_legs_file: %s: %s mismatch", src, end.status == kStrLength ? "length" : "checksum"); return ZWZ_E_CHECKSUM; }
    if (end.status != kInfEnd) {
        set_error("zwz_inflate_legs_file: %s: stream status %u after %llu decoded bytes, at compressed offset %llu", src, end.status, (unsigned long long)s.end_out,
                  (unsigned long long)(leg_stop_bit(s) >> 3));
        return ZWZ_E_FORMAT;
    }
    if (dst_idx) {
        if (s.mk_full) { set_error("zwz_inflate_legs_file: %s decodes, but its index would take 2^32 bytes or more at this span: none is made", src); return ZWZ_E_FORMAT; }
        if (s.mk_second || !s.mk_have_end || !s.mk_count) { set_error("zwz_inflate_index_file: %s decodes, but no index is made for a gzip file of several members", src); return ZWZ_E_FORMAT; }
        if (parts.count() != s.mk_count || kIdxHeader + parts.entries.size() + parts.win_bytes != s.mk_bytes) { set_error("zwz_inflate_legs_file: %s: the committed index parts do not add up", src); return ZWZ_E_FORMAT; }
    }
    auto commit = [&]() -> int {
        if (!dst) return ZWZ_OK;
        FILE* f = job.out;
        job.out = nullptr;
        if (fclose(f) != 0 || rename(job.out_part.c_str(), dst) != 0) { unlink(job.out_part.c_str()); set_error("cannot write %s", dst); return ZWZ_E_IO; }
        return ZWZ_OK;
    };
    if (!dst_idx) return commit();
    return commit_with_index(dst_idx, dst, [&](FILE* f) { return write_index(f, job, parts, size, s); }, commit, "cannot write %s");
}
