// zwz_filejob.h -- what the whole-file entry points share (zwz_bgzf.cpp, zwz_dstream.cpp): the open files, the pinned double buffers
// and the reader and writer threads of one call.  Host code; include after zwz_api_internal.h.
#pragma once
#include <unistd.h>

#include <cstdio>
#include <string>
#include <thread>

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


}  // namespace zwz
