// zwz_bgzf.hip -- BGZF framing on gfx950: CRC-32 of every block, member packing, and on the way back body gathering and
// check + compaction of the decoded blocks.  The codec itself is untouched: members are made from zwz_deflate_batch_dev's
// slots and decoded by inflate_kernel (a raw body behind a 78 9c header is a zlib stream whose Adler-32 inflate never reads).
//
// Every kernel here moves bytes once; the CRC is table-driven from LDS (crc_core.h) so that it runs at a fraction of the
// load rate rather than one bit a step.
#include "../../include/zwz.h"
#include "crc_core.h"
#include "copy_wg.h"
#include "crc_wg.h"
#include "zwz_bgzf.h"
#include "zwz_device.h"

namespace zwz {

const uint8_t kBgzfEof[kBgzfEofBytes] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0, 0x1b, 0, 0x03, 0, 0, 0, 0, 0, 0, 0, 0, 0};

namespace {

__constant__ uint8_t c_eof[kBgzfEofBytes] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0, 0x1b, 0, 0x03, 0, 0, 0, 0, 0, 0, 0, 0, 0};

__global__ void __launch_bounds__(kBgzfThreads) crc_tables_kernel(CrcTables* t) {
    const uint32_t b = threadIdx.x;
    if (b < 256) crc_fill_column(t->vec, t->mul, b, crc_xpow8n(16ull * kBgzfThreads));
    t->lane[b] = crc_xpow8n(16ull * (kBgzfThreads - 1u - b));
}

__global__ void bgzf_layout_kernel(uint64_t* off, uint32_t* len, uint64_t first, uint32_t m, uint64_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const uint64_t o = (first + i) * kBgzfBlock;
    off[i] = o;
    len[i] = (uint32_t)min<uint64_t>(kBgzfBlock, n - o);
}

__global__ void __launch_bounds__(kBgzfThreads) crc32_blocks_kernel(const CrcTables* t, const uint8_t* in, const uint64_t* off, const uint32_t* len,
                                                                    uint32_t m, uint32_t* crc) {
    __shared__ CrcLds s;
    crc_load_tables(s, t);
    for (uint32_t i = blockIdx.x; i < m; i += gridDim.x) {
        const uint32_t c = crc_block_wg(s, in + off[i], len[i]);
        if (threadIdx.x == 0) crc[i] = c;
    }
}

constexpr uint32_t kScanThreads = 1024;

__global__ void __launch_bounds__(kScanThreads) bgzf_scan_kernel(const uint32_t* v, uint32_t m, uint32_t add, uint32_t limit, uint64_t* off,
                                                                 uint64_t* base, uint32_t* err) {
    __shared__ uint32_t wsum[kScanThreads / 64];
    __shared__ uint32_t bad;
    const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
    if (t == 0) bad = 0;
    uint64_t carry = *base;
    __syncthreads();
    for (uint32_t i0 = 0; i0 < m; i0 += kScanThreads) {
        const uint32_t i = i0 + t;
        const uint32_t x = i < m ? v[i] : 0u;
        if (i < m && x > limit) bad = 1;
        const uint32_t y = i < m ? x + add : 0u;   // (<= 1024 * 65556: no 32-bit overflow within a round)
        const uint32_t incl = wave_scan_incl(y);
        if (lane == 63) wsum[w] = incl;
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (uint32_t j = 0; j < kScanThreads / 64; j++) { const uint32_t s = wsum[j]; before += j < w ? s : 0u; total += s; }
        if (i < m) off[i] = carry + before + incl - y;
        carry += total;
        __syncthreads();                           // (wsum is rewritten by the next round)
    }
    if (t == 0) { *base = carry; if (bad) *err = 1; }
}

__device__ __forceinline__ void put_le32(uint8_t* p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }
__device__ __forceinline__ uint32_t get_le16(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
__device__ __forceinline__ uint32_t get_le32(const uint8_t* p) { return get_le16(p) | get_le16(p + 2) << 16; }

__global__ void __launch_bounds__(256) bgzf_pack_kernel(const uint8_t* slots, const uint32_t* olen, const uint32_t* crc, const uint32_t* isize,
                                                        const uint64_t* moff, uint8_t* out) {
    const uint32_t i = blockIdx.x, t = threadIdx.x;
    const uint32_t L = olen[i], body = L >= 6u ? L - 6u : 0u, bsize = kBgzfHeader + body + kBgzfTrailer;
    uint8_t* dst = out + moff[i];
    if (t < kBgzfHeader) {
        uint8_t b;
        switch (t) {
            case 0: b = 0x1f; break; case 1: b = 0x8b; break; case 2: b = 0x08; break; case 3: b = 0x04; break;
            case 9: b = 0xff; break; case 10: b = 0x06; break; case 12: b = 'B'; break; case 13: b = 'C'; break; case 14: b = 0x02; break;
            case 16: b = (uint8_t)(bsize - 1u); break; case 17: b = (uint8_t)((bsize - 1u) >> 8); break;
            default: b = 0;
        }
        dst[t] = b;
    } else if (t == 32) {
        put_le32(dst + kBgzfHeader + body, crc[i]);
        put_le32(dst + kBgzfHeader + body + 4, isize[i]);
    }
    wg_copy(dst + kBgzfHeader, slots + (size_t)i * ZWZ_DEV_STRIDE + 2, body);
}

__global__ void bgzf_finish_kernel(uint8_t* out, const uint64_t* base, const uint32_t* err, uint64_t* out_len, int eof) {
    const uint64_t b = *base;
    if (eof && threadIdx.x < kBgzfEofBytes) out[b + threadIdx.x] = c_eof[threadIdx.x];
    if (threadIdx.x == 0) *out_len = *err ? ~0ull : b + (eof ? kBgzfEofBytes : 0u);
}

__global__ void __launch_bounds__(256) bgzf_gather_kernel(const uint8_t* gz, uint64_t gz_len, const uint64_t* member_off, uint32_t n_members, uint32_t first,
                                                          uint8_t* slots, uint64_t* in_off, uint32_t* in_len, uint32_t* crc, uint32_t* isize,
                                                          uint32_t* status) {
    __shared__ uint32_t body_start, body_len, ok;
    const uint32_t i = blockIdx.x, g = first + i;
    const uint64_t o = member_off[g], e = g + 1 < n_members ? member_off[g + 1] : gz_len;
    uint8_t* slot = slots + (size_t)i * kBgzfSlot;
    if (threadIdx.x == 0) {
        // zwz_bgzf_index has checked every member on the host; this only keeps a wrong offset list from reading out of bounds
        uint32_t good = o + 12 <= e && e <= gz_len && e - o <= 65536;
        const uint32_t xlen = good ? get_le16(gz + o + 10) : 0u;
        good = good && o + 12 + xlen + kBgzfTrailer <= e;
        body_start = 12 + xlen;
        body_len = good ? (uint32_t)(e - o) - 12u - xlen - kBgzfTrailer : 0u;
        ok = good;
        slot[0] = 0x78; slot[1] = 0x9c;
        in_off[i] = (uint64_t)i * kBgzfSlot;
        in_len[i] = 2 + body_len;
        crc[i] = good ? get_le32(gz + e - 8) : 0u;
        isize[i] = good ? min(get_le32(gz + e - 4), kBgzfMaxIsize) : 0u;
        status[g] = good ? 0u : (uint32_t)ZWZ_BGZF_BAD_MEMBER;
    }
    __syncthreads();
    if (ok) wg_copy(slot + 2, gz + o + body_start, body_len);
}

__global__ void __launch_bounds__(kBgzfThreads) bgzf_verify_compact_kernel(const CrcTables* tab, const uint8_t* slots, const uint32_t* olen,
                                                                           const uint32_t* inf_status, const uint32_t* crc, const uint32_t* isize,
                                                                           const uint64_t* ooff, uint32_t m, uint8_t* out, uint32_t* status) {
    __shared__ CrcLds s;
    crc_load_tables(s, tab);
    for (uint32_t i = blockIdx.x; i < m; i += gridDim.x) {
        const uint8_t* slot = slots + (size_t)i * kBgzfSlot;
        const uint32_t L = olen[i], want = isize[i];
        const uint32_t c = crc_block_wg(s, slot, L);
        if (threadIdx.x == 0 && status[i] == 0) {
            const uint32_t st = inf_status[i];
            status[i] = st != ZWZ_INF_END ? st : L != want ? (uint32_t)ZWZ_BGZF_ISIZE_MISMATCH : c != crc[i] ? (uint32_t)ZWZ_BGZF_CRC_MISMATCH : 0u;
        }
        wg_copy(out + ooff[i], slot, min(L, want));
    }
}

// Range reads (zwz_bgzf_read_ranges_*): touched member i starts at gz + moff[i] and may use bytes up to min(mend[i], gz_len) (mend null:
// gz_len).  Its header is parsed here as the host walk parses it -- magic, flags, XLEN, the BC subfield -- so the end comes from BSIZE,
// never from the index; then the body goes behind 78 9c into slot i as bgzf_gather_kernel does.
__global__ void __launch_bounds__(256) bgzf_gather_list_kernel(const uint8_t* gz, uint64_t gz_len, const uint64_t* moff, const uint64_t* mend,
                                                               uint8_t* slots, uint64_t* in_off, uint32_t* in_len, uint32_t* crc, uint32_t* isize,
                                                               uint32_t* status) {
    __shared__ uint32_t body_start, body_len, ok;
    const uint32_t i = blockIdx.x;
    const uint64_t o = moff[i], lim = mend ? min(mend[i], gz_len) : gz_len;
    uint8_t* slot = slots + (size_t)i * kBgzfSlot;
    if (threadIdx.x == 0) {
        const uint8_t* p = gz + o;
        uint32_t xlen = 0, bsize = 0;
        bool good = o < lim && lim - o >= 12 && p[0] == 0x1f && p[1] == 0x8b && p[2] == 8 && (p[3] & 4u) && !(p[3] & ~5u);
        if (good) { xlen = get_le16(p + 10); good = lim - o >= 12ull + xlen; }
        for (uint32_t x = 0; good && x < xlen;) {
            const uint8_t* f = p + 12 + x;
            const uint32_t slen = xlen - x < 4 ? 0u : get_le16(f + 2);
            if (xlen - x < 4 || 4u + slen > xlen - x) { good = false; break; }
            if (f[0] == 'B' && f[1] == 'C' && slen == 2) bsize = get_le16(f + 4) + 1u;
            x += 4 + slen;
        }
        good = good && bsize >= 12u + xlen + kBgzfTrailer && bsize <= lim - o;
        const uint32_t isz = good ? get_le32(p + bsize - 4) : 0u;
        good = good && isz <= kBgzfMaxIsize;
        body_start = 12 + xlen;
        body_len = good ? bsize - 12u - xlen - kBgzfTrailer : 0u;
        ok = good;
        slot[0] = 0x78; slot[1] = 0x9c;
        in_off[i] = (uint64_t)i * kBgzfSlot;
        in_len[i] = 2 + body_len;
        crc[i] = good ? get_le32(p + bsize - 8) : 0u;
        isize[i] = good ? isz : 0u;
        status[i] = good ? 0u : (uint32_t)ZWZ_BGZF_BAD_MEMBER;
    }
    __syncthreads();
    if (ok) wg_copy(slot + 2, gz + o + body_start, body_len);
}

// Check of decoded slot i (inflate status, ISIZE, CRC-32, and the length the index implies: expect[i] unless kNoExpect) into status[i],
// then its pieces row[i] .. row[i + 1] - 1 to out.  The first nlong[i] of them are at least kWavePieceMax bytes and go with the
// whole workgroup; each of the rest goes with one wave, the four waves taking turns.  A piece past the decoded length is not copied:
// the smallest such piece index goes to bad_piece[i] (initialised to ~0 by the caller).
__global__ void __launch_bounds__(kBgzfThreads) bgzf_verify_extract_kernel(const CrcTables* tab, const uint8_t* slots, const uint32_t* olen,
                                                                           const uint32_t* inf_status, const uint32_t* crc, const uint32_t* isize,
                                                                           const uint32_t* expect, const uint32_t* row, const uint32_t* nlong,
                                                                           const RangePiece* pieces, uint32_t m, uint8_t* out, uint32_t* status,
                                                                           uint32_t* bad_piece) {
    __shared__ CrcLds s;
    crc_load_tables(s, tab);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t i = blockIdx.x; i < m; i += gridDim.x) {
        const uint8_t* slot = slots + (size_t)i * kBgzfSlot;
        const uint32_t L = min(olen[i], kBgzfMaxIsize);
        const uint32_t c = crc_block_wg(s, slot, L);
        if (threadIdx.x == 0 && status[i] == 0) {
            const uint32_t st = inf_status[i], e = expect[i];
            status[i] = st != ZWZ_INF_END ? st : L != isize[i] ? (uint32_t)ZWZ_BGZF_ISIZE_MISMATCH : c != crc[i] ? (uint32_t)ZWZ_BGZF_CRC_MISMATCH
                      : e != kNoExpect && L != e ? kBgzfIndexMismatch : 0u;
        }
        const uint32_t p0 = row[i], pl = p0 + nlong[i], p1 = row[i + 1];
        for (uint32_t p = p0; p < pl; p++) {
            const RangePiece q = pieces[p];
            if ((uint64_t)q.off + q.len > L) { if (threadIdx.x == 0) atomicMin(&bad_piece[i], p); continue; }
            wg_copy(out + q.dst, slot + q.off, q.len);
        }
        for (uint32_t p = pl + wave; p < p1; p += kBgzfThreads / 64) {
            const RangePiece q = pieces[p];
            if ((uint64_t)q.off + q.len > L) { if (lane == 0) atomicMin(&bad_piece[i], p); continue; }
            lanes_copy(out + q.dst, slot + q.off, q.len, lane, 64);
        }
    }
}

uint32_t persistent_grid(uint32_t m, uint32_t cu_count) {
    const uint32_t g = (cu_count ? cu_count : 256u) * 4u;     // four 21-KiB table copies a CU
    return m < g ? m : g;
}

}  // namespace

hipError_t launch_crc_tables(CrcTables* t, hipStream_t s) {
    crc_tables_kernel<<<1, kBgzfThreads, 0, s>>>(t);
    return hipGetLastError();
}

hipError_t launch_bgzf_layout(uint64_t* off, uint32_t* len, uint64_t first, uint32_t m, uint64_t n, hipStream_t s) {
    if (!m) return hipSuccess;
    bgzf_layout_kernel<<<(m + 255) / 256, 256, 0, s>>>(off, len, first, m, n);
    return hipGetLastError();
}

hipError_t launch_crc32_blocks(const CrcTables* t, const uint8_t* in, const uint64_t* off, const uint32_t* len, uint32_t m, uint32_t* crc,
                               uint32_t cu_count, hipStream_t s) {
    if (!m) return hipSuccess;
    crc32_blocks_kernel<<<persistent_grid(m, cu_count), kBgzfThreads, 0, s>>>(t, in, off, len, m, crc);
    return hipGetLastError();
}

hipError_t launch_bgzf_scan(const uint32_t* v, uint32_t m, uint32_t add, uint32_t limit, uint64_t* off, uint64_t* base, uint32_t* err, hipStream_t s) {
    if (!m) return hipSuccess;
    bgzf_scan_kernel<<<1, kScanThreads, 0, s>>>(v, m, add, limit, off, base, err);
    return hipGetLastError();
}

hipError_t launch_bgzf_pack(const uint8_t* slots, const uint32_t* olen, const uint32_t* crc, const uint32_t* isize, const uint64_t* moff,
                            uint32_t m, uint8_t* out, hipStream_t s) {
    if (!m) return hipSuccess;
    bgzf_pack_kernel<<<m, 256, 0, s>>>(slots, olen, crc, isize, moff, out);
    return hipGetLastError();
}

hipError_t launch_bgzf_finish(uint8_t* out, const uint64_t* base, const uint32_t* err, uint64_t* out_len, int eof, hipStream_t s) {
    bgzf_finish_kernel<<<1, 64, 0, s>>>(out, base, err, out_len, eof);
    return hipGetLastError();
}

hipError_t launch_bgzf_gather(const uint8_t* gz, uint64_t gz_len, const uint64_t* member_off, uint32_t n_members, uint32_t first, uint32_t m,
                              uint8_t* slots, uint64_t* in_off, uint32_t* in_len, uint32_t* crc, uint32_t* isize, uint32_t* status, hipStream_t s) {
    if (!m) return hipSuccess;
    bgzf_gather_kernel<<<m, 256, 0, s>>>(gz, gz_len, member_off, n_members, first, slots, in_off, in_len, crc, isize, status);
    return hipGetLastError();
}

hipError_t launch_bgzf_verify_compact(const CrcTables* t, const uint8_t* slots, const uint32_t* olen, const uint32_t* inf_status, const uint32_t* crc,
                                      const uint32_t* isize, const uint64_t* ooff, uint32_t m, uint8_t* out, uint32_t* status, uint32_t cu_count,
                                      hipStream_t s) {
    if (!m) return hipSuccess;
    bgzf_verify_compact_kernel<<<persistent_grid(m, cu_count), kBgzfThreads, 0, s>>>(t, slots, olen, inf_status, crc, isize, ooff, m, out, status);
    return hipGetLastError();
}

hipError_t launch_bgzf_gather_list(const uint8_t* gz, uint64_t gz_len, const uint64_t* moff, const uint64_t* mend, uint32_t m, uint8_t* slots,
                                   uint64_t* in_off, uint32_t* in_len, uint32_t* crc, uint32_t* isize, uint32_t* status, hipStream_t s) {
    if (!m) return hipSuccess;
    bgzf_gather_list_kernel<<<m, 256, 0, s>>>(gz, gz_len, moff, mend, slots, in_off, in_len, crc, isize, status);
    return hipGetLastError();
}

hipError_t launch_bgzf_verify_extract(const CrcTables* t, const uint8_t* slots, const uint32_t* olen, const uint32_t* inf_status, const uint32_t* crc,
                                      const uint32_t* isize, const uint32_t* expect, const uint32_t* row, const uint32_t* nlong, const RangePiece* pieces,
                                      uint32_t m, uint8_t* out, uint32_t* status, uint32_t* bad_piece, uint32_t cu_count, hipStream_t s) {
    if (!m) return hipSuccess;
    bgzf_verify_extract_kernel<<<persistent_grid(m, cu_count), kBgzfThreads, 0, s>>>(t, slots, olen, inf_status, crc, isize, expect, row, nlong, pieces,
                                                                                     m, out, status, bad_piece);
    return hipGetLastError();
}

}  // namespace zwz
