// index_seal_wg.h -- the last step of every kernel that finishes a seek index (zwz_dstream.hip, zwz_split.hip, zwz_index.hip): the index
// CRC by one workgroup of kBgzfThreads lanes and the header of index_core.h.  Device only.
#pragma once
#include "crc_wg.h"
#include "index_core.h"

namespace zwz {
namespace {

// The CRC-32 of q[64, len), valid in every lane.  Entries, windows and padding are in place, written by this workgroup or by kernels
// before it: the fence and the barrier make this workgroup's own stores visible to all its lanes first.
__device__ uint32_t index_crc_wg(CrcLds& lds, const uint8_t* q, uint32_t len) {
    __threadfence();
    __syncthreads();
    return crc_block_wg(lds, q + kIdxHeader, len - kIdxHeader);
}

// The whole seal of the index of `len` padded bytes at q (16-byte aligned): its CRC, then thread 0 stores the header (f.crc is set here)
__device__ void index_seal_wg(CrcLds& lds, uint8_t* q, uint32_t len, IndexHeader f) {
    f.crc = index_crc_wg(lds, q, len);
    if (threadIdx.x == 0) index_header_words(reinterpret_cast<uint32_t*>(q), f);
}

}  // namespace
}  // namespace zwz
