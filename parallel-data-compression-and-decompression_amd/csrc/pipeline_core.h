// pipeline_core.h -- the parts of the directory pipeline (zwz_pipeline.cpp) that need no GPU: plain C++, so that
// tests/emu_pipeline/pipeline_emu.cpp can pin them with g++ alone.
#pragma once
#include <algorithm>
#include <cerrno>
#include <cstdint>
#include <sys/uio.h>

namespace zwz {

// Chunks per staging slice.  A slice costs 2 x 64 KiB of pinned host memory per chunk, twice (double buffering), and pinning is
// slow (0.2 s for 4096-chunk slices, a quarter of a 2 GB job); 2048 chunks still give every CU eight chunks a launch.
constexpr uint32_t kSliceChunks = 2048;

// Slice size for a job of `chunks` chunks: at most the context's batch and kSliceChunks, and small enough that a job of a few
// chunks still runs as two slices.  In 64 bits: `chunks` may be 2^32 - 1.
inline uint32_t slice_cap(uint32_t max_batch, uint64_t chunks) {
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint64_t>(max_batch, kSliceChunks), (chunks + 1) / 2 + 1));
}

// The pieces iov[0, n) to `off` and onwards through write(pieces, count, offset) -> bytes taken or -1 with errno (pwritev's
// contract), at most max_pieces a call: empty pieces are skipped, EINTR is retried, a short write is continued behind its last
// byte (the iovec is advanced in place).  Returns whether everything was written.
template <class Write>
bool write_pieces(Write&& write, struct iovec* iov, size_t n, uint64_t off, size_t max_pieces) {
    size_t k = 0;
    while (k < n) {
        if (iov[k].iov_len == 0) { k++; continue; }
        const ssize_t w = write(iov + k, (int)std::min(max_pieces, n - k), off);
        if (w < 0 && errno == EINTR) continue;
        if (w <= 0) return false;
        off += (uint64_t)w;
        size_t left = (size_t)w;
        while (left) {
            if (left >= iov[k].iov_len) { left -= iov[k].iov_len; k++; }
            else { iov[k].iov_base = static_cast<char*>(iov[k].iov_base) + left; iov[k].iov_len -= left; left = 0; }
        }
    }
    return true;
}

// 16 digest bytes -> 32 lower-case hex characters (no terminator)
inline void digest_hex(const uint8_t* digest, char* hex) {
    static const char* dig = "0123456789abcdef";
    for (int i = 0; i < 16; i++) { hex[2 * i] = dig[digest[i] >> 4]; hex[2 * i + 1] = dig[digest[i] & 15]; }
}

}  // namespace zwz
