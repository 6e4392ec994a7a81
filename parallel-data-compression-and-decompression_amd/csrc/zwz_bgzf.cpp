// zwz_bgzf.cpp -- BGZF entry points of include/zwz.h: the host walk of member headers, the device drivers around the codec
// (crc32_blocks + zwz_deflate_batch_dev + bgzf_scan + bgzf_pack; bgzf_gather + inflate + bgzf_scan + bgzf_verify_compact), and
// whole-file streaming through pinned staging with reading, the GPU and writing overlapped.
#include <unistd.h>

#include <cstdio>
#include <cstring>
#include <string>
#include <thread>

#include "zwz_api_internal.h"
#include "zwz_bgzf.h"

using namespace zwz;

#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return hip_fail(e_, #x); } while (0)

namespace {

constexpr uint64_t kMemberMax = (uint64_t)ZWZ_CHUNK_SIZE + kBgzfHeader + kBgzfTrailer - 6u;   // the deflate slot's bytes, reframed
constexpr uint32_t kFileSliceBlocks = 256;          // members per slice of the file functions: 16.7 MB of raw bytes

inline uint32_t le16(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
inline uint32_t le32(const uint8_t* p) { return le16(p) | le16(p + 2) << 16; }

// Walks the members of gz[0, n).  Strict (partial = false): anything that is not a whole member is ZWZ_E_FORMAT.  partial: stops
// (ZWZ_OK) before a member that does not end inside the buffer -- the file reader's slice boundary.  Also stops after `limit` members.
// offs[] (may be null) receives up to cap offsets; *count counts every member walked; *consumed = the end of the last one.
// `at` is the buffer's offset in the file, for messages.
int bgzf_walk(const uint8_t* gz, uint64_t n, uint64_t at, bool partial, uint64_t limit, uint64_t* offs, uint64_t cap, uint64_t* count,
              uint64_t* raw, uint64_t* consumed) {
    uint64_t o = 0, k = 0, total = 0;
    auto fail = [&](const char* what, uint64_t v) {
        if (v == ~0ull) set_error("bgzf: member %llu at byte offset %llu: %s", (unsigned long long)k, (unsigned long long)(at + o), what);
        else set_error("bgzf: member %llu at byte offset %llu: %s %llu", (unsigned long long)k, (unsigned long long)(at + o), what, (unsigned long long)v);
        *count = k; *raw = total; *consumed = o;
        return ZWZ_E_FORMAT;
    };
    while (o < n && k < limit) {
        const uint64_t avail = n - o;
        const uint8_t* m = gz + o;
        if (m[0] != 0x1f || (avail > 1 && m[1] != 0x8b) || (avail > 2 && m[2] != 8))
            return fail(k ? "trailing bytes that are not a gzip member" : "not gzip (bad magic or method)", ~0ull);
        if (avail < 12) { if (partial) break; return fail("truncated member header", ~0ull); }
        const uint32_t flg = m[3];
        if (!(flg & 4u)) return fail("no extra field: a plain gzip member, not BGZF", ~0ull);
        if (flg & ~5u) return fail("unsupported gzip header flags", flg);
        const uint32_t xlen = le16(m + 10);
        if (avail < 12ull + xlen) { if (partial) break; return fail("extra field runs past the end of the input", ~0ull); }
        uint32_t bsize = 0;
        for (uint32_t x = 0; x < xlen;) {
            if (xlen - x < 4) return fail("malformed extra field", ~0ull);
            const uint8_t* f = m + 12 + x;
            const uint32_t slen = le16(f + 2);
            if (4u + slen > xlen - x) return fail("malformed extra field", ~0ull);
            if (f[0] == 'B' && f[1] == 'C' && slen == 2) bsize = le16(f + 4) + 1u;
            x += 4 + slen;
        }
        if (!bsize) return fail("no BC subfield: not BGZF", ~0ull);
        if (bsize < 12u + xlen + kBgzfTrailer) return fail("BSIZE smaller than its header and trailer:", bsize);
        if (bsize > avail) { if (partial) break; return fail("BSIZE runs past the end of the input:", bsize); }
        const uint32_t isize = le32(m + bsize - 4);
        if (isize > kBgzfMaxIsize) return fail("ISIZE above 65535:", isize);
        if (offs && k < cap) offs[k] = o;
        total += isize;
        k++;
        o += bsize;
    }
    *count = k; *raw = total; *consumed = o;
    return ZWZ_OK;
}

struct BgzfView {
    uint8_t *slots_a, *slots_b;                       // deflate output / gathered bodies; decoded blocks
    uint64_t *off, *moff, *base;
    uint32_t *len, *olen, *st, *crc, *isize, *err;
};

size_t bgzf_bytes(uint32_t m) { return 2 * (size_t)m * kBgzfSlot + (size_t)m * (2 * 8 + 5 * 4) + 4096; }

BgzfView bgzf_view(zwz_ctx* c) {
    const size_t m = c->bgzf_cap;
    uint8_t* p = static_cast<uint8_t*>(c->bgzf_ws);
    auto take = [&](size_t bytes) { uint8_t* r = p; p += (bytes + 255) & ~(size_t)255; return r; };
    BgzfView v;
    v.slots_a = take(m * kBgzfSlot);
    v.slots_b = take(m * kBgzfSlot + 256);            // (wg_copy reads up to 3 bytes past a decoded block)
    v.off = reinterpret_cast<uint64_t*>(take(m * 8)); v.moff = reinterpret_cast<uint64_t*>(take(m * 8));
    v.len = reinterpret_cast<uint32_t*>(take(m * 4)); v.olen = reinterpret_cast<uint32_t*>(take(m * 4));
    v.st = reinterpret_cast<uint32_t*>(take(m * 4)); v.crc = reinterpret_cast<uint32_t*>(take(m * 4));
    v.isize = reinterpret_cast<uint32_t*>(take(m * 4));
    v.base = reinterpret_cast<uint64_t*>(take(16)); v.err = reinterpret_cast<uint32_t*>(v.base + 1);
    return v;
}

int ensure_bgzf(zwz_ctx* c, uint32_t m) {
    if (!c->crc_tables) {
        HIPCHK(hipMalloc(&c->crc_tables, sizeof(CrcTables)));
        HIPCHK(launch_crc_tables(static_cast<CrcTables*>(c->crc_tables), c->stream));
    }
    if (m > c->bgzf_cap) {
        HIPCHK(hipStreamSynchronize(c->stream));
        if (c->bgzf_ws) { (void)hipFree(c->bgzf_ws); c->bgzf_ws = nullptr; c->bgzf_cap = 0; }
        HIPCHK(hipMalloc(&c->bgzf_ws, bgzf_bytes(m)));
        c->bgzf_cap = m;
    }
    return ZWZ_OK;
}

// The device part of compression, d_out_len = total bytes written (with or without the EOF member).  Arguments checked by the caller.
int compress_launch(zwz_ctx* c, const uint8_t* d_in, uint64_t n, uint8_t* d_out, uint64_t* d_out_len, int eof) {
    const uint64_t nblocks = (n + kBgzfBlock - 1) / kBgzfBlock;
    const uint32_t M = (uint32_t)(nblocks < c->max_batch ? (nblocks ? nblocks : 1) : c->max_batch);
    if (int rc = ensure_bgzf(c, M)) return rc;
    const BgzfView v = bgzf_view(c);
    const CrcTables* tab = static_cast<const CrcTables*>(c->crc_tables);
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
    const CrcTables* tab = static_cast<const CrcTables*>(c->crc_tables);
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

size_t read_full(FILE* f, uint8_t* p, size_t n, bool* io_err) {
    size_t got = 0;
    while (got < n) {
        const size_t k = fread(p + got, 1, n - got, f);
        if (k == 0) { if (ferror(f)) *io_err = true; break; }
        got += k;
    }
    return got;
}

// Buffers and threads of one file call; everything is released (threads joined first) whatever the outcome.
struct FileJob {
    FILE *in = nullptr, *out = nullptr;
    std::string part;
    void* h[5] = {};                 // pinned: two input buffers, two output buffers, small values
    void* d[4] = {};
    std::thread reader, writer;
    size_t read_got = 0; bool read_err = false; bool write_err = false;
    void join() { if (reader.joinable()) reader.join(); if (writer.joinable()) writer.join(); }
    ~FileJob() {
        join();
        for (void* p : h) if (p) (void)hipHostFree(p);
        for (void* p : d) if (p) (void)hipFree(p);
        if (in) fclose(in);
        if (out) { fclose(out); unlink(part.c_str()); }
    }
    int open(const char* src, const char* dst) {
        in = fopen(src, "rb");
        if (!in) { set_error("cannot open %s", src); return ZWZ_E_IO; }
        part = std::string(dst) + ".part";
        out = fopen(part.c_str(), "wb");
        if (!out) { set_error("cannot create %s", part.c_str()); return ZWZ_E_IO; }
        return ZWZ_OK;
    }
    void start_read(uint8_t* p, size_t n) { read_got = 0; read_err = false; reader = std::thread([this, p, n] { read_got = read_full(in, p, n, &read_err); }); }
    void start_write(const uint8_t* p, size_t n) { writer = std::thread([this, p, n] { if (n && fwrite(p, 1, n, out) != n) write_err = true; }); }
    int finish_read(size_t* got) {
        if (reader.joinable()) reader.join();
        if (read_err) { set_error("read error"); return ZWZ_E_IO; }
        *got = read_got;
        return ZWZ_OK;
    }
    int finish_write() {
        if (writer.joinable()) writer.join();
        if (write_err) { set_error("write error on %s", part.c_str()); return ZWZ_E_IO; }
        return ZWZ_OK;
    }
    int commit(const char* dst) {
        if (int rc = finish_write()) return rc;
        FILE* f = out;
        out = nullptr;
        if (fclose(f) != 0 || rename(part.c_str(), dst) != 0) { unlink(part.c_str()); set_error("cannot write %s", dst); return ZWZ_E_IO; }
        return ZWZ_OK;
    }
};

#define HIPJOB(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { job.join(); return hip_fail(e_, #x); } } while (0)

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

// Slice s: its input was read into hin[s & 1] while slice s - 1 ran; it runs while slice s + 1 is read into the other buffer and
// slice s - 1's output is written from hout[(s - 1) & 1].  Every wait is a join of a thread that only does file I/O, or a stream
// synchronisation that returns on a HIP error: no wait depends on another thread reaching a point.
int zwz_bgzf_compress_file(zwz_ctx* c, const char* src, const char* dst) {
    if (!c || !src || !dst) return ZWZ_E_INVALID;
    HIPCHK(hipSetDevice(c->device));
    FileJob job;
    if (int rc = job.open(src, dst)) return rc;
    const uint32_t blocks = c->max_batch < kFileSliceBlocks ? c->max_batch : kFileSliceBlocks;
    const size_t S = (size_t)blocks * kBgzfBlock, O = zwz_bgzf_bound(S);
    for (int i = 0; i < 2; i++) HIPCHK(hipHostMalloc(&job.h[i], S + 16, hipHostMallocDefault));
    for (int i = 2; i < 4; i++) HIPCHK(hipHostMalloc(&job.h[i], O, hipHostMallocDefault));
    HIPCHK(hipHostMalloc(&job.h[4], 64, hipHostMallocDefault));
    HIPCHK(hipMalloc(&job.d[0], S + 16));
    HIPCHK(hipMalloc(&job.d[1], O));
    HIPCHK(hipMalloc(&job.d[2], 64));
    uint8_t* d_in = static_cast<uint8_t*>(job.d[0]); uint8_t* d_out = static_cast<uint8_t*>(job.d[1]);
    uint64_t* d_len = static_cast<uint64_t*>(job.d[2]); uint64_t* h_len = static_cast<uint64_t*>(job.h[4]);
    size_t n = 0;
    job.start_read(static_cast<uint8_t*>(job.h[0]), S);
    if (int rc = job.finish_read(&n)) return rc;
    for (int b = 0; n; b ^= 1) {
        uint8_t* hin = static_cast<uint8_t*>(job.h[b]);
        uint8_t* hout = static_cast<uint8_t*>(job.h[2 + b]);
        HIPJOB(hipMemcpyAsync(d_in, hin, n, hipMemcpyHostToDevice, c->stream));
        if (int rc = compress_launch(c, d_in, n, d_out, d_len, 0)) { job.join(); return rc; }
        HIPJOB(hipMemcpyAsync(h_len, d_len, 8, hipMemcpyDeviceToHost, c->stream));
        if (n == S) job.start_read(static_cast<uint8_t*>(job.h[b ^ 1]), S);     // (a short slice is the last one)
        HIPJOB(hipStreamSynchronize(c->stream));
        const uint64_t len = *h_len;
        if (len > O) { job.join(); set_error("bgzf: a member body reached the deflate slot's length"); return ZWZ_E_FORMAT; }
        HIPJOB(hipMemcpyAsync(hout, d_out, len, hipMemcpyDeviceToHost, c->stream));
        HIPJOB(hipStreamSynchronize(c->stream));
        if (int rc = job.finish_write()) { job.join(); return rc; }
        job.start_write(hout, len);
        size_t next = 0;
        if (n == S) { if (int rc = job.finish_read(&next)) { job.join(); return rc; } }
        n = next;
    }
    if (int rc = job.finish_write()) return rc;
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
    for (int i = 0; i < 2; i++) HIPCHK(hipHostMalloc(&job.h[i], B, hipHostMallocDefault));
    for (int i = 2; i < 4; i++) HIPCHK(hipHostMalloc(&job.h[i], R + 16, hipHostMallocDefault));
    HIPCHK(hipHostMalloc(&job.h[4], (size_t)blocks * (8 + 4) + 64, hipHostMallocDefault));
    HIPCHK(hipMalloc(&job.d[0], B + 16));
    HIPCHK(hipMalloc(&job.d[1], R + 16));
    HIPCHK(hipMalloc(&job.d[2], (size_t)blocks * (8 + 4) + 64));
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

}  // extern "C"
