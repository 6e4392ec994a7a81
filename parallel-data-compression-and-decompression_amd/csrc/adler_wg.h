// adler_wg.h -- Adler-32 of a byte range by one workgroup of kBgzfThreads lanes (stream_core.h's sums), shared by the stream check
// (zwz_stream.hip) and the piece checksums of the split decode (zwz_split.hip).  Device only.
#pragma once
#include "stream_core.h"
#include "zwz_bgzf.h"
#include "zwz_device.h"

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

}  // namespace
}  // namespace zwz
