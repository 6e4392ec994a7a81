// zwz_index.hip -- the device half of the seek index around inflate_kernel's marking and indexed-segment forms (index_core.h has the
// layout and the method): the windows out of a decoded stream into its index with the header and the index CRC (windows), the windows
// of a call to where its segment waves expect them (place), whether they were the stream's bytes (compare), the checksum of a
// batch of whole-stream decodes from fixed pieces joined with dstream_core.h's sums and every stream's verdict (batch finish), and the
// pieces of a batch of ranges out of the decoded segments (extract).
#include "../../include/zwz.h"
#include "adler_wg.h"
#include "copy_wg.h"
#include "dstream_core.h"
#include "index_seal_wg.h"
#include "zwz_device.h"
#include "zwz_index.h"

namespace zwz {

namespace {

__device__ __forceinline__ uint64_t ld64(const uint8_t* p) { return *reinterpret_cast<const uint64_t*>(p); }      // (8-byte aligned fields)
__device__ __forceinline__ uint32_t ld32(const uint8_t* p) { return *reinterpret_cast<const uint32_t*>(p); }

// One workgroup per stream.  The marking form has left the entries, and in the header the decoded length, the count, the end bit and
// the stored checksum; idx_len[i] is the index's padded length, 0 if none can be made.
__global__ void __launch_bounds__(kBgzfThreads) index_windows_kernel(const CrcTables* tab, IndexBuild b) {
    __shared__ CrcLds s;
    crc_load_tables(s, tab);
    const uint32_t t = threadIdx.x;
    for (uint32_t i = blockIdx.x; i < b.n; i += gridDim.x) {
        const uint64_t len = b.idx_len[i];
        if (len == 0 || len > 0xffffffffull || b.status[i] != 0u) {          // (workgroup-uniform)
            if (t == 0) b.idx_len[i] = 0;
            continue;
        }
        uint8_t* p = b.idx + b.idx_off[i];
        const uint32_t count = ld32(p + 32);
        const uint8_t* ent = p + kIdxHeader;
        uint8_t* win = p + kIdxHeader + (size_t)count * kIdxEntry;
        const uint8_t* src = b.out + b.out_off[i];
        uint64_t at = 0;
        for (uint32_t k = 0; k < count; k++) {
            const uint64_t off = ld64(ent + (size_t)k * kIdxEntry + 8);
            const uint32_t h = ld32(ent + (size_t)k * kIdxEntry + 16);
            wg_copy(win + at, src + off - h, h);
            at += h;
        }
        for (uint64_t z = kIdxHeader + (uint64_t)count * kIdxEntry + at + t; z < len; z += kBgzfThreads) p[z] = 0;
        const uint32_t crc = index_crc_wg(s, p, (uint32_t)len);
        if (t == 0) {                                                         // (the words the marking form has not left: index_header_words' others)
            uint32_t* h = reinterpret_cast<uint32_t*>(p);
            h[0] = kIdxMagicLo; h[1] = kIdxMagicHi;
            h[2] = b.wrap; h[3] = b.span;
            const uint64_t n = b.in_len[i];
            h[4] = (uint32_t)n; h[5] = (uint32_t)(n >> 32);
            h[9] = 0; h[13] = crc; h[14] = 0; h[15] = 0;
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256) index_place_kernel(const uint8_t* idx, uint8_t* out, const IndexMove* mv, uint32_t m) {
    for (uint32_t i = blockIdx.x; i < m; i += gridDim.x) { const IndexMove q = mv[i]; wg_copy(out + q.dst, idx + q.src, q.len); }
}

// The file loop's commit (zwz_legs_file.cpp): the windows of a leg's committed entries out of its output staging, packed back to back.
// A workgroup per window; a move that does not lie inside both buffers is not made (the host planned it: cannot happen).
__global__ void __launch_bounds__(256) index_gather_kernel(const uint8_t* stage, uint64_t stage_len, uint8_t* packed, uint64_t packed_cap, const IndexMove* mv, uint32_t m) {
    for (uint32_t i = blockIdx.x; i < m; i += gridDim.x) {
        const IndexMove q = mv[i];                                             // (workgroup-uniform)
        if (q.src > stage_len || q.len > stage_len - q.src || q.dst > packed_cap || q.len > packed_cap - q.dst) continue;
        wg_copy(packed + q.dst, stage + q.src, q.len);
    }
}

__global__ void __launch_bounds__(256) index_compare_kernel(const uint8_t* idx, const uint8_t* out, const IndexMove* mv, uint32_t m, uint32_t* flag) {
    for (uint32_t i = blockIdx.x; i < m; i += gridDim.x) {
        const IndexMove q = mv[i];
        uint32_t differs = 0;
        for (uint32_t j = threadIdx.x; j < q.len; j += 256u) differs |= (uint32_t)(out[q.dst + j] != idx[q.src + j]);
        if (differs) atomicOr(flag + q.stream, 1u);
    }
}

static_assert(kIdxPieceBytes == kPieceBytes, "index_core.h's piece layout is dstream_core.h's piece");

__global__ void __launch_bounds__(256) index_pieces_kernel(IndexPieces f) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= f.pieces) return;
    f.piece_off[j] = index_piece_start(f.head, j);
    f.piece_len[j] = index_piece_bytes(f.head, f.total, j);
}

// A workgroup per stream, a thread per piece: where in `out` the stream's pieces lie
__global__ void __launch_bounds__(256) index_batch_pieces_kernel(const IndexStream* rec, uint32_t n, uint64_t* piece_off, uint32_t* piece_len) {
    for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
        const IndexStream r = rec[i];                                          // (workgroup-uniform)
        for (uint32_t j = threadIdx.x; j < r.pieces; j += 256u) {
            piece_off[r.piece0 + j] = r.out_off + index_piece_start(r.head, j);
            piece_len[r.piece0 + j] = index_piece_bytes(r.head, r.total, j);
        }
    }
}

__global__ void __launch_bounds__(kBgzfThreads) index_adler_kernel(const uint8_t* out, const uint64_t* piece_off, const uint32_t* piece_len, uint32_t* piece_val,
                                                                   uint32_t pieces) {
    __shared__ uint32_t s_part[2 * kBgzfThreads / 64];
    for (uint32_t j = blockIdx.x; j < pieces; j += gridDim.x) {
        const uint32_t a = adler_range_wg(s_part, out + piece_off[j], piece_len[j]);
        if (threadIdx.x == 0) piece_val[j] = a;
    }
}

// Lane l joins its share of `cnt` consecutive pieces, then every lane the 64 shares: the checksum of the pieces' bytes (wave-uniform)
template <class Sum>
__device__ uint32_t index_join_pieces(const uint32_t* piece_len, const uint32_t* piece_val, uint32_t cnt, uint32_t lane) {
    const uint32_t K = (cnt + 63u) / 64u, p1 = Sum::pof(kPieceBytes);
    uint32_t x = Sum::identity(), acc = Sum::identity();
    uint64_t bytes = 0;
    for (uint32_t j = lane * K; j < min(cnt, (lane + 1u) * K); j++) {
        const uint32_t len = piece_len[j];
        x = Sum::join(x, piece_val[j], len == kPieceBytes ? p1 : Sum::pof(len));
        bytes += len;
    }
    const uint32_t pl = Sum::pof(bytes);
    for (uint32_t l = 0; l < 64u; l++) acc = Sum::join(acc, (uint32_t)__shfl((int)x, (int)l, 64), (uint32_t)__shfl((int)pl, (int)l, 64));
    return acc;
}

// One wave per stream: the join of its pieces, then the verdict and the stream's three result words.
__global__ void __launch_bounds__(64) index_batch_finish_kernel(IndexBatch b) {
    const uint32_t lane = lane_id();
    for (uint32_t i = blockIdx.x; i < b.n; i += gridDim.x) {
        const IndexStream r = b.rec[i];                                        // (wave-uniform, as every branch on it below)
        uint32_t st = r.refused;
        uint64_t total = r.total;
        if (st) total = 0;
        else if (b.bad[i]) st = kStrIndex;
        else if (b.flag[i]) st = kStrChecksum;
        else if (r.wrap != kWrapRaw) {
            const uint32_t acc = r.wrap == kWrapGzip ? index_join_pieces<CrcSum>(b.piece_len + r.piece0, b.piece_val + r.piece0, r.pieces, lane)
                                                     : index_join_pieces<AdlerSum>(b.piece_len + r.piece0, b.piece_val + r.piece0, r.pieces, lane);
            // the stream's own trailer: Adler-32 big-endian (zlib); CRC-32 and ISIZE little-endian (gzip)
            const uint32_t want = r.wrap == kWrapZlib ? 4u : 8u;
            bool ok = acc == r.expect && r.trailer + want <= r.in_len;
            if (ok) {
                const uint8_t* q = b.in + r.in_off + r.trailer;
                ok = r.wrap == kWrapZlib ? be32_at(q) == acc : le32_at(q) == acc && le32_at(q + 4) == (uint32_t)r.total;
            }
            if (!ok) st = kStrChecksum;
        }
        if (lane == 0) {
            b.out_len[i] = total;
            b.status[i] = st;
            if (b.segments) b.segments[i] = r.refused ? 0u : r.nseg;
        }
    }
}

// The decode in legs (zwz_legs.cpp), one wave per stream: the join of the pieces of its checked output against the checksum its
// trailers gave; a mismatch beats the provisional status (stream_core.h: stream_verdict).  nseg: whether any checksum was read.
__global__ void __launch_bounds__(64) legs_finish_kernel(const IndexStream* rec, uint32_t n, const uint32_t* piece_len, const uint32_t* piece_val, uint32_t* status) {
    const uint32_t lane = lane_id();
    for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
        const IndexStream r = rec[i];                                          // (wave-uniform)
        if (r.refused || !r.nseg) continue;
        const uint32_t acc = r.wrap == kWrapGzip ? index_join_pieces<CrcSum>(piece_len + r.piece0, piece_val + r.piece0, r.pieces, lane)
                                                 : index_join_pieces<AdlerSum>(piece_len + r.piece0, piece_val + r.piece0, r.pieces, lane);
        if (lane == 0 && acc != r.expect) status[i] = kStrChecksum;
    }
}

// bgzf_verify_extract's dealing of the pieces: long ones by the workgroup, short ones a wave each
__global__ void __launch_bounds__(kBgzfThreads) index_extract_kernel(const uint8_t* slots, const uint64_t* slot_off, const uint32_t* row, const uint32_t* nlong,
                                                                     const RangePiece* pieces, uint32_t m, const uint32_t* bad, uint8_t* out) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t i = blockIdx.x; i < m; i += gridDim.x) {
        if (bad[i]) continue;
        const uint8_t* slot = slots + slot_off[i];
        const uint32_t p0 = row[i], pl = p0 + nlong[i], p1 = row[i + 1];
        for (uint32_t p = p0; p < pl; p++) { const RangePiece q = pieces[p]; wg_copy(out + q.dst, slot + q.off, q.len); }
        for (uint32_t p = pl + wave; p < p1; p += kBgzfThreads / 64) { const RangePiece q = pieces[p]; lanes_copy(out + q.dst, slot + q.off, q.len, lane, 64); }
    }
}

uint32_t grid_for(uint32_t m, uint32_t cu_count, uint32_t per_cu) {
    const uint32_t g = (cu_count ? cu_count : 256u) * per_cu;
    return m < g ? m : g;
}

}  // namespace

hipError_t launch_index_windows(const CrcTables* tab, const IndexBuild& b, hipStream_t s) {
    if (!b.n) return hipSuccess;
    index_windows_kernel<<<b.n, kBgzfThreads, 0, s>>>(tab, b);
    return hipGetLastError();
}

hipError_t launch_index_place(const uint8_t* idx, uint8_t* out, const IndexMove* mv, uint32_t m, hipStream_t s) {
    if (!m) return hipSuccess;
    index_place_kernel<<<m < 65536u ? m : 65536u, 256, 0, s>>>(idx, out, mv, m);
    return hipGetLastError();
}

hipError_t launch_index_gather(const uint8_t* stage, uint64_t stage_len, uint8_t* packed, uint64_t packed_cap, const IndexMove* mv, uint32_t m, hipStream_t s) {
    if (!m) return hipSuccess;
    index_gather_kernel<<<m < 65536u ? m : 65536u, 256, 0, s>>>(stage, stage_len, packed, packed_cap, mv, m);
    return hipGetLastError();
}

hipError_t launch_index_compare(const uint8_t* idx, const uint8_t* out, const IndexMove* mv, uint32_t m, uint32_t* flag, hipStream_t s) {
    if (!m) return hipSuccess;
    index_compare_kernel<<<m < 65536u ? m : 65536u, 256, 0, s>>>(idx, out, mv, m, flag);
    return hipGetLastError();
}

hipError_t launch_index_piece_sums(const CrcTables* tab, const IndexPieces& f, uint32_t cu_count, hipStream_t s) {
    if (f.wrap == kWrapRaw || !f.pieces) return hipSuccess;
    index_pieces_kernel<<<(f.pieces + 255u) / 256u, 256, 0, s>>>(f);
    if (f.wrap == kWrapGzip) return launch_crc32_blocks(tab, f.out, f.piece_off, f.piece_len, f.pieces, f.piece_val, cu_count, s);
    index_adler_kernel<<<grid_for(f.pieces, cu_count, 8u), kBgzfThreads, 0, s>>>(f.out, f.piece_off, f.piece_len, f.piece_val, f.pieces);
    return hipGetLastError();
}

hipError_t launch_index_batch_finish(const CrcTables* tab, const IndexBatch& b, uint32_t cu_count, hipStream_t s) {
    if (!b.n) return hipSuccess;
    if (b.pieces) {
        index_batch_pieces_kernel<<<grid_for(b.n, cu_count, 8u), 256, 0, s>>>(b.rec, b.n, b.piece_off, b.piece_len);
        const uint32_t g = b.gzip_pieces, a = b.pieces - g;
        if (g) { const hipError_t e = launch_crc32_blocks(tab, b.out, b.piece_off, b.piece_len, g, b.piece_val, cu_count, s); if (e != hipSuccess) return e; }
        if (a) index_adler_kernel<<<grid_for(a, cu_count, 8u), kBgzfThreads, 0, s>>>(b.out, b.piece_off + g, b.piece_len + g, b.piece_val + g, a);
    }
    index_batch_finish_kernel<<<grid_for(b.n, cu_count, 16u), 64, 0, s>>>(b);
    return hipGetLastError();
}

hipError_t launch_legs_check(const CrcTables* tab, const LegsCheck& b, uint32_t cu_count, hipStream_t s) {
    if (!b.n || b.wrap == kWrapRaw) return hipSuccess;       // raw: no checksum, the provisional status is final
    if (b.pieces) {
        index_batch_pieces_kernel<<<grid_for(b.n, cu_count, 8u), 256, 0, s>>>(b.rec, b.n, b.piece_off, b.piece_len);
        if (b.wrap == kWrapGzip) { const hipError_t e = launch_crc32_blocks(tab, b.out, b.piece_off, b.piece_len, b.pieces, b.piece_val, cu_count, s); if (e != hipSuccess) return e; }
        else index_adler_kernel<<<grid_for(b.pieces, cu_count, 8u), kBgzfThreads, 0, s>>>(b.out, b.piece_off, b.piece_len, b.piece_val, b.pieces);
    }
    legs_finish_kernel<<<grid_for(b.n, cu_count, 16u), 64, 0, s>>>(b.rec, b.n, b.piece_len, b.piece_val, b.status);
    return hipGetLastError();
}

hipError_t launch_index_extract(const uint8_t* slots, const uint64_t* slot_off, const uint32_t* row, const uint32_t* nlong, const RangePiece* pieces,
                                uint32_t m, const uint32_t* bad, uint8_t* out, uint32_t cu_count, hipStream_t s) {
    if (!m) return hipSuccess;
    index_extract_kernel<<<grid_for(m, cu_count, 4u), kBgzfThreads, 0, s>>>(slots, slot_off, row, nlong, pieces, m, bad, out);
    return hipGetLastError();
}

}  // namespace zwz
