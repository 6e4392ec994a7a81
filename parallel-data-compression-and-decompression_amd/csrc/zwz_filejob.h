// zwz_filejob.h -- what the whole-file entry points share (zwz_bgzf.cpp, zwz_dstream.cpp, zwz_split.cpp): the open files, the pinned
// double buffers and the reader and writer threads of one call, the slice loop of the two compressing ones, the commit of an output
// that an index goes with, and the decode of a whole file by one launch.  Host code.
#pragma once
#include <unistd.h>

#include <cstdio>
#include <initializer_list>
#include <string>
#include <thread>
#include <vector>

#include "zwz_api_internal.h"

namespace zwz {

inline size_t read_full(FILE* f, uint8_t* p, size_t n, bool* io_err) {
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
    int fd = -1;                     // (the range reader's input: pread)
    std::string part;
    void* h[5] = {};                 // pinned: two input buffers, two output buffers, small values
    void* d[3] = {};                 // input, output, small values
    std::thread reader, writer;
    size_t read_got = 0; bool read_err = false; bool write_err = false;
    void join() { if (reader.joinable()) reader.join(); if (writer.joinable()) writer.join(); }
    ~FileJob() {
        join();
        for (void* p : h) if (p) (void)hipHostFree(p);
        for (void* p : d) if (p) (void)hipFree(p);
        if (in) fclose(in);
        if (fd >= 0) close(fd);
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
    // The buffers of the call: h[i] of h_bytes[i] bytes, d[i] of d_bytes[i] (0: none).  Returns the first error.
    int alloc(std::initializer_list<size_t> h_bytes, std::initializer_list<size_t> d_bytes) {
        void** q = h;
        for (size_t n : h_bytes) { if (n) HIPCHK(hipHostMalloc(q, n, hipHostMallocDefault)); q++; }
        q = d;
        for (size_t n : d_bytes) { if (n) HIPCHK(hipMalloc(q, n)); q++; }
        return ZWZ_OK;
    }
    template <class T = uint8_t> T* hp(int i) const { return static_cast<T*>(h[i]); }
    template <class T = uint8_t> T* dp(int i) const { return static_cast<T*>(d[i]); }
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

// An index goes with this output.  <dst_idx>.part is created and body(f) writes it (false: a write failed); commit() puts the data file
// `dst` in place (null: there is none, and commit() returns ZWZ_OK); the index is renamed last.  Whatever fails, no index, no .part of
// it and no data file is left: a failed commit() has removed its own .part, and dst is unlinked if the last rename fails.
// write_fail, names_part: a failed write's message, and whether it names the .part or the index.
template <class Body, class Commit>
int commit_with_index(const char* dst_idx, const char* dst, Body&& body, Commit&& commit, const char* write_fail = "write error on %s", bool names_part = true) {
    const std::string ipart = std::string(dst_idx) + ".part";
    FILE* f = fopen(ipart.c_str(), "wb");
    if (!f) { set_error("cannot create %s", ipart.c_str()); return ZWZ_E_IO; }
    const bool wrote = body(f);
    if ((fclose(f) != 0) | !wrote) { unlink(ipart.c_str()); set_error(write_fail, names_part ? ipart.c_str() : dst_idx); return ZWZ_E_IO; }
    if (int rc = commit()) { unlink(ipart.c_str()); return rc; }
    if (rename(ipart.c_str(), dst_idx) != 0) { unlink(ipart.c_str()); if (dst) unlink(dst); set_error("cannot write %s", dst_idx); return ZWZ_E_IO; }
    return ZWZ_OK;
}
// The index is the n bytes at p
template <class Commit>
int commit_with_index_bytes(const char* dst_idx, const char* dst, const uint8_t* p, size_t n, Commit&& commit, const char* write_fail = "write error on %s", bool names_part = true) {
    return commit_with_index(dst_idx, dst, [&](FILE* f) { return fwrite(p, 1, n, f) == n; }, commit, write_fail, names_part);
}

// A whole file of n < kStreamMaxIn bytes as ONE stream through one launch -- zwz_inflate_streams_dev, with idx
// zwz_inflate_streams_index_dev at the context's span -- its output capacity doubled until the decoded bytes fit.  in: the file's bytes
// and 32 zero bytes behind them; out, idx (either may be null): the decoded bytes, the index (empty: the launch made none).  A stream
// that does not end well is an error in `who`'s name (zwz_index.cpp).  kGoLegs: the decoded bytes do not fit the launch's largest
// capacity, and the file goes through zwz_inflate_legs_file.
constexpr int kGoLegs = 1;
int inflate_whole_file(zwz_ctx* c, int wrap, const char* who, const char* src, const uint8_t* in, uint64_t n, std::vector<uint8_t>* out, std::vector<uint8_t>* idx);

#define HIPJOB(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { job.join(); return hip_fail(e_, #x); } } while (0)

// What a compressed slice hands back through h[4] / d[2]: the bytes it wrote, its status (0: fine) and its checksum where it has one
struct SliceResult { uint64_t out_len; uint32_t status, check; };

// The loop of zwz_bgzf_compress_file and zwz_deflate_stream_file over slices of S input bytes, buffers as FileJob::alloc({S.., S.., O, O,
// small}, {S.., O, small}) gave them.  Slice s: its input was read into h[s & 1] while slice s - 1 ran; it runs while slice s + 1 is
// read into the other buffer and slice s - 1's output is written from h[2 + ((s - 1) & 1)].  Every wait is a join of a thread that
// only does file I/O, or a stream synchronisation that returns on a HIP error: no wait depends on another thread reaching a point.
//   queue(n, d_res, h_res)  the slice's n bytes are on their way to d[0]: queue its work on the context's stream, output to d[1], and
//                           the copy of its results into *h_res
//   back(n, res)            the results have arrived: judge them (anything but ZWZ_OK ends the call)
// Returns with the last write joined and checked.
template <class Q, class B>
int run_slices(zwz_ctx* c, FileJob& job, size_t S, Q&& queue, B&& back) {
    SliceResult* res = job.hp<SliceResult>(4);
    *res = SliceResult{};
    size_t n = 0;
    job.start_read(job.hp(0), S);
    if (int rc = job.finish_read(&n)) return rc;
    for (int b = 0; n; b ^= 1) {
        uint8_t* hout = job.hp(2 + b);
        HIPJOB(hipMemcpyAsync(job.d[0], job.h[b], n, hipMemcpyHostToDevice, c->stream));
        if (int rc = queue(n, job.dp<SliceResult>(2), res)) { job.join(); return rc; }
        if (n == S) job.start_read(job.hp(b ^ 1), S);     // (a short slice is the last one)
        HIPJOB(hipStreamSynchronize(c->stream));
        if (int rc = back(n, *res)) { job.join(); return rc; }
        const uint64_t len = res->out_len;
        HIPJOB(hipMemcpyAsync(hout, job.d[1], len, hipMemcpyDeviceToHost, c->stream));
        HIPJOB(hipStreamSynchronize(c->stream));
        if (int rc = job.finish_write()) { job.join(); return rc; }
        job.start_write(hout, len);
        size_t next = 0;
        if (n == S) { if (int rc = job.finish_read(&next)) { job.join(); return rc; } }
        n = next;
    }
    return job.finish_write();
}

}  // namespace zwz
