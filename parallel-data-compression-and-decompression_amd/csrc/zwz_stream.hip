// zwz_stream.hip -- stream_check_kernel: the checksum half of zwz_inflate_streams_dev.  inflate_kernel's stream form decodes every
// stream and leaves, per stream, the length of output its checksum covers, the expected checksum and a provisional status
// (stream_core.h: StreamRecord); persistent workgroups here compute the Adler-32 (zlib) or CRC-32 (gzip, every member whose CRC field
// was read, as one range) of that output and write the final status.
#include "../../include/zwz.h"
#include "crc_wg.h"
#include "stream_core.h"
#include "zwz_kernels.h"

namespace zwz {

namespace {

// adler32(p[0, L)) by the whole workgroup (stream_core.h's sums): lane t takes vectors t, t + T, t + 2T, ..., four loads in flight;
// the sums of the lanes are added and the tail of L % 16 bytes is added by every lane.  The result is valid in every lane.
__device__ uint32_t adler_range_wg(uint32_t* part /* 2 words a wave */, const uint8_t* p, uint32_t L) {
    constexpr uint32_t T = kBgzfThreads;
    const uint32_t t = threadIdx.x, V = L / 16u;
    const uint4* pv = reinterpret_cast<const uint4*>(p);
    uint32_t s0 = 0, s1 = 0, v = t;
    for (; v + 3u * T < V; v += 4u * T) {
        uint4 w[4];
#pragma unroll
        for (uint32_t u = 0; u < 4; u++) w[u] = pv[v + u * T];
#pragma unroll
        for (uint32_t u = 0; u < 4; u++) adler_vec16(16u * (v + u * T), w[u].x, w[u].y, w[u].z, w[u].w, s0, s1);
    }
    for (; v < V; v += T) { const uint4 w = pv[v]; adler_vec16(16u * v, w.x, w.y, w.z, w.w, s0, s1); }
#pragma unroll
    for (uint32_t d = 32; d; d >>= 1) { s0 += __shfl_xor(s0, d, 64); s1 += __shfl_xor(s1, d, 64); }   // < 64 * 65521
    if ((t & 63u) == 0) { part[2u * (t >> 6)] = s0 % kAdlerMod; part[2u * (t >> 6) + 1u] = s1 % kAdlerMod; }
    __syncthreads();
    s0 = 0; s1 = 0;
#pragma unroll
    for (uint32_t w = 0; w < T / 64u; w++) { s0 += part[2u * w]; s1 += part[2u * w + 1u]; }
    s0 %= kAdlerMod; s1 %= kAdlerMod;
    adler_bytes(16u * V, p + (size_t)V * 16u, L & 15u, s0, s1);
    __syncthreads();                               // (part is reused by the next stream)
    return adler_finish(s0, s1, L);
}

__global__ void __launch_bounds__(kBgzfThreads) stream_check_kernel(const CrcTables* tab, const uint8_t* out, const uint64_t* out_off,
                                                                    const uint4* rec, uint32_t n, uint32_t wrap, uint32_t* status) {
    __shared__ CrcLds s;
    __shared__ uint32_t s_part[2 * kBgzfThreads / 64];
    if (wrap == kWrapGzip) crc_load_tables(s, tab);
    for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
        const uint4 r = rec[i];
        uint32_t actual = 0;
        if (r.z) {                                 // (workgroup-uniform)
            const uint8_t* p = out + out_off[i];
            actual = wrap == kWrapGzip ? crc_block_wg(s, p, r.x) : adler_range_wg(s_part, p, r.x);
        }
        if (threadIdx.x == 0) status[i] = stream_verdict(StreamRecord{r.x, r.y, r.z, r.w}, actual);
    }
}

}  // namespace

hipError_t launch_stream_check(const CrcTables* tab, const uint8_t* out, const uint64_t* out_off, const uint4* rec, uint32_t n,
                               uint32_t wrap, uint32_t* status, uint32_t cu_count, hipStream_t s) {
    if (n == 0 || wrap == kWrapRaw) return hipSuccess;       // raw: no checksum, the provisional status is final
    const uint32_t g = (cu_count ? cu_count : 256u) * 4u;
    stream_check_kernel<<<n < g ? n : g, kBgzfThreads, 0, s>>>(tab, out, out_off, rec, n, wrap, status);
    return hipGetLastError();
}

}  // namespace zwz
