// copy_wg.h -- byte copies between arbitrarily aligned global addresses by a wave or a workgroup (device code only): BGZF's packing and
// extraction (zwz_bgzf.hip) and the stream packer (zwz_dstream.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace zwz {

// Copies len bytes src -> dst with `lanes` lanes, this one being `lane`.  Every whole 16-byte aligned vector of dst is one store, its
// bytes gathered from four or five aligned source dwords with v_alignbyte (the source's misalignment against dst is the same for
// every vector); the partly covered vectors at both ends go byte by byte.  Reads up to 3 bytes past src + len: callers keep those
// readable.
static __device__ void lanes_copy(uint8_t* dst, const uint8_t* src, uint32_t len, uint32_t lane, uint32_t lanes) {
    if (!len) return;
    const uintptr_t d0 = reinterpret_cast<uintptr_t>(dst), d1 = d0 + len, v0 = d0 & ~(uintptr_t)15;
    const uint32_t nv = (uint32_t)((((d1 + 15) & ~(uintptr_t)15) - v0) >> 4);
    const uintptr_t delta = reinterpret_cast<uintptr_t>(src) - d0;        // (modular) source address of dst byte a: a + delta
    const uint32_t r = (uint32_t)(delta & 3u);
    for (uint32_t j = lane; j < nv; j += lanes) {
        const uintptr_t D = v0 + ((uintptr_t)j << 4);
        if (D >= d0 && D + 16 <= d1) {
            const uint32_t* w = reinterpret_cast<const uint32_t*>((D + delta) & ~(uintptr_t)3);
            uint4 o;
            if (r == 0) { o.x = w[0]; o.y = w[1]; o.z = w[2]; o.w = w[3]; }
            else {
                const uint32_t a = w[0], b = w[1], c = w[2], d = w[3], e = w[4];
                o.x = __builtin_amdgcn_alignbyte(b, a, r); o.y = __builtin_amdgcn_alignbyte(c, b, r);
                o.z = __builtin_amdgcn_alignbyte(d, c, r); o.w = __builtin_amdgcn_alignbyte(e, d, r);
            }
            *reinterpret_cast<uint4*>(D) = o;
        } else {
            for (uint32_t b = 0; b < 16; b++) {
                const uintptr_t a = D + b;
                if (a >= d0 && a < d1) *reinterpret_cast<uint8_t*>(a) = *reinterpret_cast<const uint8_t*>(a + delta);
            }
        }
    }
}

// The workgroup's copy (every lane of the block)
static __device__ __forceinline__ void wg_copy(uint8_t* dst, const uint8_t* src, uint32_t len) { lanes_copy(dst, src, len, threadIdx.x, blockDim.x); }

}  // namespace zwz
