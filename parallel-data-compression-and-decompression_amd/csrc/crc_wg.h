// crc_wg.h -- CRC-32 of a byte range by one workgroup of kBgzfThreads lanes from LDS tables (crc_core.h's schedule), shared by the
// BGZF kernels (zwz_bgzf.hip) and the stream check (zwz_stream.hip).  Device only.
#pragma once
#include "crc_core.h"
#include "zwz_bgzf.h"
#include "zwz_device.h"

namespace zwz {
namespace {

// Tables of one workgroup: 16 KiB slicing + 4 KiB multiplier + 1 KiB lane shifts, copied from device memory once per workgroup.
struct __align__(16) CrcLds { uint32_t vec[16 * 256]; uint32_t mul[4 * 256]; uint32_t lane[kBgzfThreads]; uint32_t part[kBgzfThreads / 64]; };

__device__ __forceinline__ void crc_load_tables(CrcLds& s, const CrcTables* t) {
    copy_vec16(reinterpret_cast<uint4*>(s.vec), reinterpret_cast<const uint4*>(t->vec), (16 * 256 + 4 * 256 + kBgzfThreads) / 4);
    __syncthreads();
}

// crc32(p[0, L)) by the whole workgroup (kBgzfThreads lanes, crc_core.h's schedule); the result is valid in every lane.  p 16-byte
// aligned; no byte at or past p + L is read.  Any L below 2^32: a BGZF block, or a whole decoded stream (every index below stays
// under 2^28 vectors).
__device__ uint32_t crc_block_wg(CrcLds& s, const uint8_t* p, uint32_t L) {
    const uint32_t t = threadIdx.x, V = L / 16u, slots = crc_lane_slots(L, kBgzfThreads), pad = slots * kBgzfThreads - V;
    const uint4* pv = reinterpret_cast<const uint4*>(p);
    uint32_t acc = 0;
    uint32_t k = 0;
    // slots whose vector lies wholly in front of the block (the zero padding) leave acc at 0: start at the first real one
    if (pad > t) k = (pad - t + kBgzfThreads - 1u) / kBgzfThreads;
    for (; k + 4 <= slots; k += 4) {               // four loads in flight a lane
        uint4 w[4];
#pragma unroll
        for (uint32_t u = 0; u < 4; u++) w[u] = pv[(k + u) * kBgzfThreads + t - pad];
#pragma unroll
        for (uint32_t u = 0; u < 4; u++) {
            if ((k + u) * kBgzfThreads + t == pad) w[u].x ^= 0xffffffffu;      // vector 0: the initial register
            acc = crc_mul_tab(s.mul, acc) ^ crc_vec16(s.vec, w[u].x, w[u].y, w[u].z, w[u].w);
        }
    }
    for (; k < slots; k++) {
        uint4 w = pv[k * kBgzfThreads + t - pad];
        if (k * kBgzfThreads + t == pad) w.x ^= 0xffffffffu;
        acc = crc_mul_tab(s.mul, acc) ^ crc_vec16(s.vec, w.x, w.y, w.z, w.w);
    }
    uint32_t raw = crc_mulmod(acc, s.lane[t]);
#pragma unroll
    for (uint32_t d = 32; d; d >>= 1) raw ^= __shfl_xor(raw, d, 64);
    if ((t & 63u) == 0) s.part[t >> 6] = raw;
    __syncthreads();
    raw = 0;
#pragma unroll
    for (uint32_t w = 0; w < kBgzfThreads / 64; w++) raw ^= s.part[w];
    raw = crc_raw_bytes(V ? raw : 0xffffffffu, p + (size_t)V * 16u, L & 15u) ^ 0xffffffffu;   // the tail, then the final complement
    __syncthreads();                               // (s.part is reused by the next block)
    return raw;
}

}  // namespace
}  // namespace zwz
