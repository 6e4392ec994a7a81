// zwz_zip.hip -- the device half of zwz_zip_dev and zwz_unzip_dev on gfx950.  The codec is untouched: entries are compressed by
// zwz_deflate_streams_dev and decoded by zwz_inflate_split_streams_dev; the kernels here place them.  Writing: two 64-bit scans give
// every local header and central record its offset (zip_scan), one workgroup per tile of kZipTile bytes moves the compressed data to
// its place behind its header (zip_pack), one wave per entry writes its central record (zip_directory).  Reading: one workgroup per tile
// moves an entry's data to aligned staging, or a stored entry's straight to its output (zip_gather); the decoded bytes are cut into
// tiles for crc32_blocks_kernel (zip_crc_layout) and one wave per entry joins its tiles' CRCs and gives the verdict (zip_verdict).
// Work is dealt by tile everywhere: one huge entry among many small ones is thousands of workgroups, not one.
#include "../../include/zwz.h"
#include "copy_wg.h"
#include "dstream_core.h"
#include "zip_core.h"
#include "zwz_device.h"
#include "zwz_zip.h"

namespace zwz {

namespace {

constexpr uint32_t kZipScanThreads = 1024;

__device__ __forceinline__ uint64_t shfl_up64(uint64_t v, uint32_t d) {
    const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, d, 64), hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), d, 64);
    return (uint64_t)hi << 32 | lo;
}

// Exclusive 64-bit scan of f(0) .. f(n - 1) into off[] by one workgroup; returns the total (to every thread).
template <class F>
__device__ uint64_t wg_scan64(uint32_t n, uint64_t* off, uint64_t* wsum, F&& f) {
    const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
    uint64_t carry = 0;
    for (uint32_t i0 = 0; i0 < n; i0 += kZipScanThreads) {
        const uint32_t i = i0 + t;
        const uint64_t y = i < n ? f(i) : 0ull;
        uint64_t incl = y;
#pragma unroll
        for (uint32_t d = 1; d < 64u; d <<= 1) { const uint64_t o = shfl_up64(incl, d); if (lane >= d) incl += o; }
        if (lane == 63u) wsum[w] = incl;
        __syncthreads();
        uint64_t before = 0, total = 0;
        for (uint32_t j = 0; j < kZipScanThreads / 64u; j++) { const uint64_t s = wsum[j]; before += j < w ? s : 0ull; total += s; }
        if (i < n) off[i] = carry + before + incl - y;
        carry += total;
        __syncthreads();
    }
    return carry;
}

// The record of entry i as both of its headers are written from it
__device__ ZipRec zip_rec(const ZipWrite& W, uint32_t i) {
    const ZipIn e = W.in[i];
    ZipRec r;
    const uint64_t g = W.glen[i];
    r.csize = g - (kGzipHeaderBytes + 8u);
    const uint8_t* tr = W.stage + e.soff + g - 8u;                 // the gzip trailer: CRC-32, ISIZE
    r.crc = zip_get32(tr);
    r.usize = e.usize;
    r.offset = W.hoff[i];
    r.attr = e.attr; r.name_len = e.name_len; r.flags = (uint16_t)e.flags;
    r.time = (uint16_t)e.time_date; r.date = (uint16_t)(e.time_date >> 16);
    r.force64 = W.force64;
    return r;
}

// One workgroup: both scans one after the other (a central record's size depends on its header's offset), then the totals.
__global__ void __launch_bounds__(kZipScanThreads) zip_scan_kernel(ZipWrite W) {
    __shared__ uint64_t wsum[kZipScanThreads / 64u];
    __shared__ uint32_t bad;
    if (threadIdx.x == 0) bad = 0;
    __syncthreads();
    // 1. local header + data: every entry's header offset
    const uint64_t cd_off = wg_scan64(W.n, W.hoff, wsum, [&](uint32_t i) -> uint64_t {
        if (W.gst[i] != 0 || W.glen[i] < kGzipHeaderBytes + 8u + 2u) { bad = 1; return 0ull; }
        const uint64_t csize = W.glen[i] - (kGzipHeaderBytes + 8u), usize = W.in[i].usize;
        const bool big = W.force64 || csize >= kZipSat32 || usize >= kZipSat32;
        return zip_local_bytes(W.in[i].name_len, big) + csize;
    });
    // 2. the central records, which know their header offsets now
    const uint64_t cd_size = wg_scan64(W.n, W.coff, wsum, [&](uint32_t i) -> uint64_t {
        const uint64_t csize = W.glen[i] - (kGzipHeaderBytes + 8u), usize = W.in[i].usize;
        const bool big = W.force64 || csize >= kZipSat32 || usize >= kZipSat32;
        return zip_central_bytes(W.in[i].name_len, big, W.force64 || W.hoff[i] >= kZipSat32);
    });
    if (threadIdx.x == 0) {
        const uint64_t need = W.partial ? cd_off : cd_off + cd_size + zip_end_bytes(zip_end64(W.n, cd_size, cd_off, W.force64 != 0));
        ZipTotals t;
        t.cd_off = cd_off; t.cd_size = cd_size; t.need = need; t.ok = !bad && need <= W.out_cap; t.pad = 0;
        *W.tot = t;
        *W.out_len = need;
        *W.status = bad ? (uint32_t)ZWZ_INF_DATA_ERROR : need > W.out_cap ? (uint32_t)ZWZ_INF_OVERFLOW : 0u;
    }
}

// The entry of tile b: the last one whose first tile is not behind it
template <class T, class F>
__device__ uint32_t tile_entry(uint32_t n, T b, F&& first) {
    uint32_t lo = 0, hi = n;                       // first(lo) <= b < first(hi)
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (first(mid) <= b) lo = mid; else hi = mid;
    }
    return lo;
}

// One workgroup per tile.  An entry's first tile also writes its local header.  The tiles are counted from the bound of the
// compressed size (the launch cannot wait for the real one), so an entry's last tiles may have nothing to do.
__global__ void __launch_bounds__(256) zip_pack_kernel(ZipWrite W) {
    if (!W.tot->ok) return;
    const uint64_t b = blockIdx.x;
    const uint32_t t = threadIdx.x;
    const uint32_t e = tile_entry(W.n, b, [&](uint32_t i) { return W.in[i].tfirst; });
    const uint64_t k = b - W.in[e].tfirst;
    const ZipRec r = zip_rec(W, e);
    const uint32_t hdr = zip_local_bytes(r.name_len, zip_big(r));
    uint8_t* dst = W.out + r.offset;
    if (k == 0) {
        if (t == 0) zip_write_local(dst, r);
        const uint8_t* name = W.names + W.in[e].name_off;
        for (uint32_t j = t; j < r.name_len; j += 256u) dst[kZipLocalFixed + j] = name[j];
    }
    const uint64_t at = k * kZipTile;
    if (at >= r.csize) return;
    const uint32_t len = (uint32_t)min<uint64_t>(kZipTile, r.csize - at);
    wg_copy(dst + hdr + at, W.stage + W.in[e].soff + kGzipHeaderBytes + at, len);      // (reads at most 3 bytes past: the stream's trailer)
}

// One wave per entry: its central record.  The first wave also writes the end records.
__global__ void __launch_bounds__(256) zip_directory_kernel(ZipWrite W) {
    const ZipTotals T = *W.tot;
    if (!T.ok) return;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = lane_id();
    if (wave == 0 && lane == 0) zip_write_end(W.out + T.cd_off + T.cd_size, W.n, T.cd_size, T.cd_off, W.force64 != 0);
    if (wave >= W.n) return;
    const ZipRec r = zip_rec(W, wave);
    uint8_t* dst = W.out + T.cd_off + W.coff[wave];
    if (lane == 0) zip_write_central(dst, r);
    const uint8_t* name = W.names + W.in[wave].name_off;
    for (uint32_t j = lane; j < r.name_len; j += 64u) dst[kZipCentralFixed + j] = name[j];
}

// One workgroup per tile of an entry's data in the archive.  lanes_copy reads whole aligned dwords of its source: at most up to the
// archive's length rounded up to 4, which the caller keeps readable (up to 16).
__global__ void __launch_bounds__(256) zip_gather_kernel(ZipRead R) {
    const uint32_t b = blockIdx.x;
    const uint32_t e = tile_entry(R.n, b, [&](uint32_t i) { return R.in[i].tfirst; });
    const UnzIn u = R.in[e];
    const uint64_t at = (uint64_t)(b - u.tfirst) * kZipTile;
    if (u.kind == kUnzSkip || at >= u.len) return;
    const uint32_t len = (uint32_t)min<uint64_t>(kZipTile, u.len - at);
    uint8_t* dst = (u.kind == kUnzStored ? R.out : R.stage) + u.dst + at;
    wg_copy(dst, R.zip + u.src + at, len);
}

// CRC tile t: bytes of its entry's output range (16-byte aligned: out_off and kZipTile are multiples of 16)
__global__ void __launch_bounds__(256) zip_crc_layout_kernel(ZipRead R, uint32_t ctiles) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ctiles) return;
    const uint32_t e = tile_entry(R.n, t, [&](uint32_t i) { return R.in[i].ctfirst; });
    const UnzIn u = R.in[e];
    const uint64_t at = (uint64_t)(t - u.ctfirst) * kZipTile;
    R.toff[t] = u.out_off + at;
    R.tlen[t] = (uint32_t)min<uint64_t>(kZipTile, u.usize - at);
}

// One wave per entry: the CRC-32 of its tiles joined in dstream_combine_kernel's schedule -- lane l joins K = ceil(full / 64)
// consecutive full tiles, the 64 values are folded pairwise at distances 1, 2, 4, ..., the last (short) tile is joined by its own
// length -- then the verdict, in the order UNSUPPORTED / BAD_ENTRY (the host's), inflate's 1 / 2, SIZE_MISMATCH, CRC_MISMATCH.
__global__ void __launch_bounds__(256) zip_verdict_kernel(ZipRead R) {
    const uint32_t e = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = lane_id();
    if (e >= R.n) return;
    const UnzIn u = R.in[e];
    if (u.pre || u.kind == kUnzSkip) {
        if (lane == 0) { R.status[e] = u.pre; R.out_len[e] = 0; }
        return;
    }
    const uint32_t p0 = u.ctfirst, cnt = R.in[e + 1].ctfirst - p0;
    uint32_t acc = CrcSum::identity();
    if (cnt) {
        const uint32_t full = cnt - 1u;
        if (full) {
            const uint32_t p1 = CrcSum::pof(kZipTile), K = (full + kSumRow - 1u) / kSumRow, pad = K * kSumRow - full;
            uint32_t x = CrcSum::identity();
            for (uint32_t j = 0; j < K; j++) {
                const uint32_t v = lane * K + j;
                if (v >= pad) x = CrcSum::join(x, R.tcrc[p0 + v - pad], p1);
            }
            uint32_t pd = sum_ptimes<CrcSum>(p1, K);
#pragma unroll
            for (uint32_t k = 0; k < 6; k++) {
                const uint32_t d = 1u << k, y = (uint32_t)__shfl_down((int)x, d, 64);
                if ((lane & (2u * d - 1u)) == 0) x = CrcSum::join(x, y, pd);
                pd = CrcSum::pjoin(pd, pd);
            }
            acc = (uint32_t)__shfl((int)x, 0, 64);
        }
        acc = CrcSum::join(acc, R.tcrc[p0 + full], CrcSum::pof(R.tlen[p0 + full]));
    }
    if (lane != 0) return;
    uint32_t st = 0;
    if (u.kind == kUnzDeflated) {
        const uint32_t is = R.ist[e];
        if (is == (uint32_t)ZWZ_INF_NEED_INPUT || is == (uint32_t)ZWZ_INF_DATA_ERROR) st = is;
        else if (is == (uint32_t)ZWZ_INF_OVERFLOW || (is == 0 && R.out_len[e] != u.usize)) st = (uint32_t)ZWZ_ZIP_SIZE_MISMATCH;
        else if (is) st = is;
    } else {
        R.out_len[e] = u.usize;
    }
    if (!st && acc != u.crc) st = (uint32_t)ZWZ_ZIP_CRC_MISMATCH;
    R.status[e] = st;
}

}  // namespace

hipError_t launch_zip_scan(const ZipWrite& W, hipStream_t s) {
    zip_scan_kernel<<<1, kZipScanThreads, 0, s>>>(W);
    return hipGetLastError();
}

hipError_t launch_zip_pack(const ZipWrite& W, uint32_t tiles, hipStream_t s) {
    if (!tiles) return hipSuccess;
    zip_pack_kernel<<<tiles, 256, 0, s>>>(W);
    return hipGetLastError();
}

hipError_t launch_zip_directory(const ZipWrite& W, hipStream_t s) {
    zip_directory_kernel<<<(max(W.n, 1u) + 3u) / 4u, 256, 0, s>>>(W);
    return hipGetLastError();
}

hipError_t launch_zip_gather(const ZipRead& R, uint32_t tiles, hipStream_t s) {
    if (!tiles) return hipSuccess;
    zip_gather_kernel<<<tiles, 256, 0, s>>>(R);
    return hipGetLastError();
}

hipError_t launch_zip_crc_layout(const ZipRead& R, uint32_t ctiles, hipStream_t s) {
    if (!ctiles) return hipSuccess;
    zip_crc_layout_kernel<<<(ctiles + 255u) / 256u, 256, 0, s>>>(R, ctiles);
    return hipGetLastError();
}

hipError_t launch_zip_verdict(const ZipRead& R, hipStream_t s) {
    if (!R.n) return hipSuccess;
    zip_verdict_kernel<<<(R.n + 3u) / 4u, 256, 0, s>>>(R);
    return hipGetLastError();
}

}  // namespace zwz
