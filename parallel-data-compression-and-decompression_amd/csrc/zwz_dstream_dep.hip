// zwz_dstream_dep.hip -- the device half of zwz_deflate_dep_streams_dev and zwz_deflate_dep_streams_index_dev on gfx950: streams of
// dependent pieces (dstream_core.h).  A piece of kDepPieceBytes and the kDepDictBytes of input in front of it are
// one chunk of the codec, which enters it behind the dictionary (zwz_kernels.h: DeflateArgs::skip).  The kernels here restate
// zwz_dstream.hip's layout, combine, due and seal for that geometry and add the piece's own Adler-32 and the index entries with their
// windows; size, the scans and pack are zwz_dstream.hip's as they are.  A file of its own, so that the independent form's kernels are
// compiled as they were.
#include "../../include/zwz.h"
#include "adler_wg.h"
#include "copy_wg.h"
#include "crc_wg.h"
#include "dstream_core.h"
#include "index_core.h"
#include "zwz_device.h"
#include "zwz_dstream.h"

namespace zwz {

namespace {

// dstream_layout_kernel for pieces of kDepPieceBytes: the codec's chunk starts dep_skip bytes in front of the piece, in the caller's own input
__global__ void __launch_bounds__(256) dstream_dep_layout_kernel(DstreamStreams S, DstreamPieces P, DstreamDep Q, uint64_t g0, uint32_t m, uint32_t lead) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= m) return;
    const uint64_t g = g0 + p;
    uint32_t lo = 0, hi = S.n;                     // pfirst[lo] <= g < pfirst[hi]
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (S.pfirst[mid] <= g) lo = mid; else hi = mid;
    }
    const uint64_t k = g - S.pfirst[lo], at = k * kDepPieceBytes, left = S.in_len[lo] - at;
    const uint32_t skip = dep_skip(k, lead), len = (uint32_t)min<uint64_t>(left, kDepPieceBytes);
    Q.poff[p] = S.in_off[lo] + at; Q.plen[p] = len; Q.skip[p] = skip;
    P.off[p] = S.in_off[lo] + at - skip;
    P.len[p] = skip + len;
    P.sidx[p] = lo;
}

// Under zlib: the Adler-32 of every piece's own bytes, a workgroup a piece at a time
__global__ void __launch_bounds__(kBgzfThreads) dstream_dep_adler_kernel(const uint8_t* __restrict__ in, DstreamPieces P, DstreamDep Q, uint32_t m) {
    __shared__ uint32_t part[2 * (kBgzfThreads / 64)];
    for (uint32_t p = blockIdx.x; p < m; p += gridDim.x) {
        const uint32_t a = adler_range_wg(part, in + Q.poff[p], Q.plen[p]);       // (the piece starts on a multiple of 16, as the chunk does)
        if (threadIdx.x == 0) P.crc[p] = a;
    }
}

// dstream_combine_kernel's schedule for pieces of kDepPieceBytes; the values are in P.crc under either wrapper
template <class Sum>
__global__ void __launch_bounds__(256) dstream_dep_combine_kernel(DstreamStreams S, DstreamPieces P, DstreamDep Q, uint64_t g0, uint32_t m, uint32_t s0, uint32_t ns) {
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = lane_id();
    if (wave >= ns) return;
    const uint32_t s = s0 + wave;
    const uint64_t lo = max(S.pfirst[s], g0), hi = min(S.pfirst[s + 1], g0 + m);
    if (hi <= lo) return;
    const uint32_t p0 = (uint32_t)(lo - g0), cnt = (uint32_t)(hi - lo), full = cnt - 1u;
    uint32_t acc = S.chk[s];
    if (full) {
        const uint32_t p1 = Sum::pof(kDepPieceBytes), K = (full + kSumRow - 1u) / kSumRow, pad = K * kSumRow - full;
        uint32_t x = Sum::identity();
        for (uint32_t j = 0; j < K; j++) {
            const uint32_t v = lane * K + j;
            if (v >= pad) x = Sum::join(x, P.crc[p0 + v - pad], p1);
        }
        uint32_t pd = sum_ptimes<Sum>(p1, K);
#pragma unroll
        for (uint32_t k = 0; k < 6; k++) {
            const uint32_t d = 1u << k, y = (uint32_t)__shfl_down((int)x, d, 64);
            if ((lane & (2u * d - 1u)) == 0) x = Sum::join(x, y, pd);
            pd = Sum::pjoin(pd, pd);
        }
        x = (uint32_t)__shfl((int)x, 0, 64);
        acc = Sum::join(acc, x, sum_ptimes<Sum>(p1, full));
    }
    acc = Sum::join(acc, P.crc[p0 + full], Sum::pof(Q.plen[p0 + full]));
    if (lane == 0) S.chk[s] = acc;
}

// dstream_due_kernel with the points kDepPieceBytes apart
__global__ void __launch_bounds__(256) dstream_dep_due_kernel(DstreamStreams S, DstreamPieces P, uint64_t g0, uint32_t m, DstreamIndex X) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= m) return;
    const uint32_t s = P.sidx[p];
    const uint64_t off = X.off_base + (g0 + p - S.pfirst[s]) * kDepPieceBytes;
    P.due[p] = off == 0u || index_flush_due(off - kDepPieceBytes, off, X.off_base + S.in_len[s], X.span) ? 1u : 0u;
}

// A workgroup per piece, behind the rank scan and behind pack.  Thread 0 does dstream_index_kernel's work -- the entry's hist is the
// piece's dictionary -- and the workgroup copies the window, the input in front of the piece (the chunk's head), to its place:
// window w of the index belongs to entry w + 1 (entry 0, at offset 0, has none).  A whole call knows the number of entries, and so
// where the windows start and whether the index fits, before it writes any (index_dep_count); a partial call's windows go to
// win_base, in the order of its entries.
__global__ void __launch_bounds__(256) dstream_dep_index_kernel(const uint8_t* __restrict__ in, DstreamStreams S, DstreamPieces P, DstreamDep Q, uint64_t g0,
                                                                DstreamOut O, DstreamIndex X, uint64_t win_base) {
    const uint32_t p = blockIdx.x, t = threadIdx.x;
    const uint32_t s = P.sidx[p], due = P.due[p];
    const uint64_t g = g0 + p, pf = S.pfirst[s];
    const uint64_t xs = pf >= g0 ? P.x[pf - g0] : S.xs[s], rs = pf >= g0 ? P.rank[pf - g0] : S.rs[s];
    const uint64_t r = P.rank[p] - rs;
    if (t == 0) {
        if (g == pf) S.rs[s] = P.rank[p];           // (read by this stream's pieces in later slices only)
        if (g + 1 == S.pfirst[s + 1]) S.cnt[s] = r + due;
    }
    if (!due) return;
    const uint32_t hist = Q.skip[p];
    uint64_t win_at;                                // of the stream's index space: where this entry's window goes (meaningless without one)
    if (O.partial) {
        if (index_flush_bytes(r + 1u) > win_base) return;
        win_at = win_base + (r - (X.off_base == 0u ? 1u : 0u)) * kDepDictBytes;
    } else {
        const uint64_t count = index_dep_count(S.in_len[s], X.span);
        if (r >= count || index_dep_bytes(count) > S.idx_cap[s]) return;
        win_at = kIdxHeader + count * kIdxEntry + (r - 1u) * kDepDictBytes;
    }
    if (hist && win_at + hist > S.idx_cap[s]) return;
    uint8_t* q = X.idx + S.idx_off[s];
    if (t == 0) {
        const uint32_t hdr = O.partial ? 0u : dstream_header_bytes(O.wrap);
        uint64_t* e = reinterpret_cast<uint64_t*>(q + kIdxHeader + r * kIdxEntry);
        e[0] = 8u * (X.pos_base + hdr + (P.x[p] - xs));
        e[1] = X.off_base + (g - pf) * kDepPieceBytes;
        e[2] = hist;
    }
    if (hist) wg_copy(q + win_at, in + P.off[p], hist);
}

// dstream_index_seal_kernel for an index with windows: they lie behind the entries, the padding behind them
__global__ void __launch_bounds__(kBgzfThreads) dstream_dep_index_seal_kernel(const CrcTables* tab, DstreamStreams S, DstreamOut O, DstreamIndex X) {
    __shared__ CrcLds lds;
    crc_load_tables(lds, tab);
    const uint32_t t = threadIdx.x;
    for (uint32_t i = blockIdx.x; i < S.n; i += gridDim.x) {
        const uint64_t count = S.in_len[i] ? S.cnt[i] : 1u, len = index_dep_bytes(count);      // (workgroup-uniform, as the branch below)
        if (O.status[i] != 0u || count > 0xffffffffull || len > 0xffffffffull || len > S.idx_cap[i] || count != index_dep_count(S.in_len[i], X.span)) {
            if (t == 0) X.idx_len[i] = 0;
            continue;
        }
        uint8_t* q = X.idx + S.idx_off[i];
        const uint32_t hdr = dstream_header_bytes(O.wrap);
        if (t == 0) {
            uint64_t* e = reinterpret_cast<uint64_t*>(q + kIdxHeader);
            if (!S.in_len[i]) { e[0] = 8u * hdr; e[1] = 0; e[2] = 0; }
            if (count & 1u) *reinterpret_cast<uint64_t*>(q + len - 8u) = 0;       // 24 count is 8 mod 16, a window 0: the padding
        }
        __threadfence();
        __syncthreads();
        const uint32_t crc = crc_block_wg(lds, q + kIdxHeader, (uint32_t)(len - kIdxHeader));
        if (t == 0) {
            const uint64_t total = O.out_len[i], end_bit = index_flush_end_bit(total - dstream_trailer_bytes(O.wrap) - 2u), n = S.in_len[i];
            uint32_t* h = reinterpret_cast<uint32_t*>(q);
            h[0] = 0x495a575au; h[1] = 0x01005844u;                               // "ZWZIDX\0\1"
            h[2] = O.wrap; h[3] = X.span;
            h[4] = (uint32_t)total; h[5] = (uint32_t)(total >> 32); h[6] = (uint32_t)n; h[7] = (uint32_t)(n >> 32);
            h[8] = (uint32_t)count; h[9] = 0; h[10] = (uint32_t)end_bit; h[11] = (uint32_t)(end_bit >> 32);
            h[12] = O.wrap == kWrapRaw ? 0u : S.chk[i]; h[13] = crc; h[14] = 0; h[15] = 0;
            X.idx_len[i] = len;
        }
        __syncthreads();
    }
}

}  // namespace

hipError_t launch_dstream_dep_layout(const DstreamStreams& S, const DstreamPieces& P, const DstreamDep& Q, uint64_t g0, uint32_t m, uint32_t lead, hipStream_t s) {
    if (!m) return hipSuccess;
    dstream_dep_layout_kernel<<<(m + 255u) / 256u, 256, 0, s>>>(S, P, Q, g0, m, lead);
    return hipGetLastError();
}

hipError_t launch_dstream_dep_adler(const uint8_t* in, const DstreamPieces& P, const DstreamDep& Q, uint32_t m, uint32_t cu_count, hipStream_t s) {
    if (!m) return hipSuccess;
    const uint32_t g = (cu_count ? cu_count : 256u) * 8u;
    dstream_dep_adler_kernel<<<m < g ? m : g, kBgzfThreads, 0, s>>>(in, P, Q, m);
    return hipGetLastError();
}

hipError_t launch_dstream_dep_combine(const DstreamStreams& S, const DstreamPieces& P, const DstreamDep& Q, uint64_t g0, uint32_t m, uint32_t s0, uint32_t ns,
                                      uint32_t wrap, hipStream_t s) {
    if (!m || !ns || wrap == kWrapRaw) return hipSuccess;
    const uint32_t grid = (ns + 3u) / 4u;
    if (wrap == kWrapZlib) dstream_dep_combine_kernel<AdlerSum><<<grid, 256, 0, s>>>(S, P, Q, g0, m, s0, ns);
    else dstream_dep_combine_kernel<CrcSum><<<grid, 256, 0, s>>>(S, P, Q, g0, m, s0, ns);
    return hipGetLastError();
}

hipError_t launch_dstream_dep_due(const DstreamStreams& S, const DstreamPieces& P, uint64_t g0, uint32_t m, const DstreamIndex& X, hipStream_t s) {
    if (!m) return hipSuccess;
    dstream_dep_due_kernel<<<(m + 255u) / 256u, 256, 0, s>>>(S, P, g0, m, X);
    return hipGetLastError();
}

hipError_t launch_dstream_dep_index(const uint8_t* in, const DstreamStreams& S, const DstreamPieces& P, const DstreamDep& Q, uint64_t g0, uint32_t m,
                                    const DstreamOut& O, const DstreamIndex& X, uint64_t win_base, hipStream_t s) {
    if (!m) return hipSuccess;
    dstream_dep_index_kernel<<<m, 256, 0, s>>>(in, S, P, Q, g0, O, X, win_base);
    return hipGetLastError();
}

hipError_t launch_dstream_dep_index_seal(const CrcTables* tab, const DstreamStreams& S, const DstreamOut& O, const DstreamIndex& X, uint32_t cu_count,
                                         hipStream_t s) {
    if (!S.n) return hipSuccess;
    const uint32_t g = (cu_count ? cu_count : 256u) * 4u;
    dstream_dep_index_seal_kernel<<<S.n < g ? S.n : g, kBgzfThreads, 0, s>>>(tab, S, O, X);
    return hipGetLastError();
}

}  // namespace zwz
