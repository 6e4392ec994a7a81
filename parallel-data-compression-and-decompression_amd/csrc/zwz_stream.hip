// zwz_stream.hip -- stream_check_kernel: the checksum half of zwz_inflate_streams_dev.  inflate_kernel's stream form decodes every
// stream and leaves, per stream, the length of output its checksum covers, the expected checksum and a provisional status
// (stream_core.h: StreamRecord); persistent workgroups here compute the Adler-32 (zlib) or CRC-32 (gzip, every member whose CRC field
// was read, as one range) of that output and write the final status.
#include "../../include/zwz.h"
#include "adler_wg.h"
#include "crc_wg.h"
#include "stream_core.h"
#include "zwz_kernels.h"

namespace zwz {

namespace {

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
