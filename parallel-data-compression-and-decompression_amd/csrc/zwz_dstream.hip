// zwz_dstream.hip -- the device half of zwz_deflate_streams_dev on gfx950.  The codec is untouched: every piece of at most kPieceBytes
// goes through zwz_deflate_batch_dev into its slot, and the kernels here cut the batch into pieces (layout), find where each piece's
// stream is spliced from the block records the encoder itself was laid out by (size), fold the pieces' checksums into their streams'
// (combine) and move every piece once, with its marker, to its place in its stream (pack).  dstream_core.h has the format and the
// arithmetic; the scan between size and pack is BGZF's (launch_bgzf_scan).  zwz_deflate_streams_index_dev adds the index at the pieces'
// starts (index_core.h: the index at full-flush points): a flag per piece (due), the same scan over the flags, the entries (index)
// and, behind the last slice, every stream's header and index CRC (seal).  Nothing is decoded: a piece's decoded offset is its number
// times the piece length and its first bit is where pack puts it.
// The dependent form (zwz_deflate_dep_streams_dev) runs through the same kernels: they take the PieceForm
// (dstream_core.h), and a piece of kDepPieceBytes with the kDepDictBytes of input in front of it is one chunk of the codec, which enters it
// behind the dictionary (zwz_kernels.h: DeflateArgs::skip).  Two kernels are that form's alone: the Adler-32 of the piece's own bytes
// (the slot's covers the dictionary too) and the index entries with their windows.
#include "../../include/zwz.h"
#include "adler_wg.h"
#include "copy_wg.h"
#include "dstream_core.h"
#include "index_seal_wg.h"
#include "zwz_device.h"
#include "zwz_dstream.h"

namespace zwz {

namespace {

// Streams without input are complete here (header, 03 00, trailer); the others start their running checksum.
__global__ void __launch_bounds__(256) dstream_begin_kernel(DstreamStreams S, DstreamOut O) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= S.n) return;
    const uint32_t init = dstream_check_init(O.wrap);
    S.chk[i] = init;
    S.xs[i] = 0;
    if (S.in_len[i]) return;
    const uint32_t hdr = O.partial ? 0u : dstream_header_bytes(O.wrap), tail = O.partial ? 0u : 2u + dstream_trailer_bytes(O.wrap);
    const bool fits = hdr + tail <= S.out_cap[i];
    if (fits) {
        uint8_t* dst = O.out + S.out_off[i];
        for (uint32_t b = 0; b < hdr; b++) dst[b] = (uint8_t)dstream_header_byte(O.wrap, b, O.zflg, O.xfl);
        for (uint32_t b = 0; b < tail; b++) dst[hdr + b] = (uint8_t)dstream_tail_byte(O.wrap, b, init, 0);
    }
    O.out_len[i] = hdr + tail;
    O.status[i] = fits ? 0u : (uint32_t)ZWZ_INF_OVERFLOW;
}

// Piece g0 + p: its stream is the last one whose first piece is not behind it (streams without pieces share their successor's first).
// The codec's chunk starts `skip` bytes in front of the piece, in the caller's own input: the piece's dictionary (none: the piece itself).
__global__ void __launch_bounds__(256) dstream_layout_kernel(DstreamStreams S, DstreamPieces P, PieceForm F, uint32_t lead, uint64_t g0, uint32_t m) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= m) return;
    const uint64_t g = g0 + p;
    uint32_t lo = 0, hi = S.n;                     // pfirst[lo] <= g < pfirst[hi]
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (S.pfirst[mid] <= g) lo = mid; else hi = mid;
    }
    const uint64_t k = g - S.pfirst[lo], at = k * F.piece, left = S.in_len[lo] - at;
    const uint32_t skip = F.skip(k, lead), len = (uint32_t)min<uint64_t>(left, F.piece);
    P.poff[p] = S.in_off[lo] + at; P.plen[p] = len; P.skip[p] = skip;
    P.off[p] = S.in_off[lo] + at - skip;
    P.len[p] = skip + len;
    P.sidx[p] = lo;
}

// Dependent pieces under zlib: the Adler-32 of every piece's own bytes, a workgroup a piece at a time
__global__ void __launch_bounds__(kBgzfThreads) dstream_adler_kernel(const uint8_t* __restrict__ in, DstreamPieces P, uint32_t m) {
    __shared__ uint32_t part[2 * (kBgzfThreads / 64)];
    for (uint32_t p = blockIdx.x; p < m; p += gridDim.x) {
        const uint32_t a = adler_range_wg(part, in + P.poff[p], P.plen[p]);       // (the piece starts on a multiple of 16, as the chunk does)
        if (threadIdx.x == 0) P.crc[p] = a;
    }
}

// (The records are the ones the slot's stream was written from; should they ever contradict its length, *err is set, the piece gets
// harmless splice points and its stream ends with status ZWZ_INF_DATA_ERROR.)
__global__ void __launch_bounds__(256) dstream_size_kernel(const ChunkInfo* info, const BlockInfo* blocks, const BlockOut* plans, DstreamPieces P,
                                                           uint32_t m, uint32_t* err) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= m) return;
    const BlockInfo* bi = blocks + (size_t)p * kMaxBlocks;
    const BlockOut* bo = plans + (size_t)p * kMaxBlocks;
    const uint32_t nb = min(info[p].n_blocks, kMaxBlocks);
    auto block = [&](uint32_t b, uint32_t& type, uint32_t& hdr_bits, uint32_t& body_bits, uint32_t& stored) {
        type = bo[b].type; hdr_bits = bo[b].hdr_bits; body_bits = bo[b].body_bits; stored = bi[b].end - bi[b].start;
    };
    const SplicePoints sp_ = splice_points(nb, block);
    SplicePoints sp = sp_;
    // A piece whose symbols fill its blocks exactly ends, in the slot's Z_FINISH stream, with an empty block: the finishing flush writes one
    // whatever it holds.  A full flush writes a block only if it holds a symbol, so the piece's share of the stream ends with the block before
    // (dstream_pack_kernel clears what the slot has behind it).  Every piece under Z_HUFFMAN_ONLY of 16 383 k bytes is one.
    if (nb > 1u && bi[nb - 1u].end == bi[nb - 1u].start && bo[nb - 1u].type != kStored) sp = splice_points(nb - 1u, block);
    if (2u + spliced_source_bytes(sp_.end_bit) + 4u != P.olen[p] || sp.hdr_bit >= sp.end_bit) { *err = 1; sp.hdr_bit = 16; sp.end_bit = 16; }
    P.hbit[p] = sp.hdr_bit;
    P.ebit[p] = sp.end_bit;
    P.slen[p] = spliced_bytes(sp.end_bit);
}

// One wave per stream with a piece in the slice: the checksums of its pieces there, in order, joined onto the stream's running value.
// All but the last of them are F.piece bytes long (only a stream's last piece is shorter).  Lane l joins K = ceil(full / 64) consecutive
// ones one after the other -- the short share is lane 0's, padded in front with nothing -- and the 64 lanes' values, each now the
// checksum of K pieces, are folded pairwise at distances 1, 2, 4, ... with the parameter of K, 2K, 4K, ... pieces
// (dstream_core.h: sum_fold_row_host is that fold on the host).  A stream of 8 192 pieces a slice costs 128 + 6 joins deep instead of 8 192.
// The last piece is joined by its own length.  A piece's value is the slot's trailing Adler-32 (kFromSlot: independent pieces under
// zlib) or P.crc: crc32_blocks' under gzip, dstream_adler_kernel's for dependent pieces under zlib.
template <class Sum, bool kFromSlot>
__global__ void __launch_bounds__(256) dstream_combine_kernel(DstreamStreams S, DstreamPieces P, PieceForm F, uint64_t g0, uint32_t m, uint32_t s0, uint32_t ns) {
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = lane_id();
    if (wave >= ns) return;
    const uint32_t s = s0 + wave;
    const uint64_t lo = max(S.pfirst[s], g0), hi = min(S.pfirst[s + 1], g0 + m);
    if (hi <= lo) return;
    const uint32_t p0 = (uint32_t)(lo - g0), cnt = (uint32_t)(hi - lo), full = cnt - 1u;
    auto value = [&](uint32_t p) -> uint32_t {
        if (!kFromSlot) return P.crc[p];
        const uint8_t* a = P.slots + (size_t)p * ZWZ_DEV_STRIDE + P.olen[p] - 4u;        // the slot's Adler-32, big-endian
        return (uint32_t)a[0] << 24 | (uint32_t)a[1] << 16 | (uint32_t)a[2] << 8 | (uint32_t)a[3];
    };
    uint32_t acc = S.chk[s];
    if (full) {
        const uint32_t p1 = Sum::pof(F.piece), K = (full + kSumRow - 1u) / kSumRow, pad = K * kSumRow - full;
        uint32_t x = Sum::identity();
        for (uint32_t j = 0; j < K; j++) {
            const uint32_t v = lane * K + j;
            if (v >= pad) x = Sum::join(x, value(p0 + v - pad), p1);
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
    acc = Sum::join(acc, value(p0 + full), Sum::pof(P.plen[p0 + full]));
    if (lane == 0) S.chk[s] = acc;
}

// One workgroup per piece.  Thread 0 first makes the slot's bytes [2, 2 + slen) the piece's share of the stream -- BFINAL cleared, the
// marker behind the last block (over the slot's Adler-32, which dstream_combine_kernel has read) -- then the workgroup copies them
// to their place.  A stream's first piece also writes the header and its last the tail, the length and the status.  Nothing is
// written that would end behind the stream's capacity.
__global__ void __launch_bounds__(256) dstream_pack_kernel(DstreamStreams S, DstreamPieces P, uint64_t g0, DstreamOut O, const uint32_t* err) {
    const uint32_t p = blockIdx.x, t = threadIdx.x;
    const uint32_t s = P.sidx[p], slen = P.slen[p];
    const uint64_t g = g0 + p, pf = S.pfirst[s];
    uint8_t* slot = P.slots + (size_t)p * ZWZ_DEV_STRIDE;
    if (t == 0) {
        const uint32_t hbit = P.hbit[p], src = spliced_source_bytes(P.ebit[p]);
        slot[hbit >> 3] &= (uint8_t)~(1u << (hbit & 7u));
        if (P.ebit[p] & 7u) slot[P.ebit[p] >> 3] &= (uint8_t)((1u << (P.ebit[p] & 7u)) - 1u);      // (zero already, unless an empty last block was left out)
        if (slen - 4u > src) slot[2u + src] = 0;
        uint8_t* mk = slot + 2u + slen - 4u;
        mk[0] = 0; mk[1] = 0; mk[2] = 0xff; mk[3] = 0xff;
    }
    const bool first = g == pf, last = g + 1 == S.pfirst[s + 1];
    const uint64_t xs = pf >= g0 ? P.x[pf - g0] : S.xs[s];
    const uint32_t hdr = O.partial ? 0u : dstream_header_bytes(O.wrap), tail = O.partial ? 0u : 2u + dstream_trailer_bytes(O.wrap);
    const uint64_t start = hdr + (P.x[p] - xs), end = start + slen, cap = S.out_cap[s];
    uint8_t* dst = O.out + S.out_off[s];
    if (first) {
        if (t == 0) S.xs[s] = P.x[p];              // (read by this stream's pieces in later slices only)
        if (t < hdr && hdr <= cap) dst[t] = (uint8_t)dstream_header_byte(O.wrap, t, O.zflg, O.xfl);
    }
    if (last) {
        const uint64_t total = end + tail;
        if (t == 0) { O.out_len[s] = total; O.status[s] = *err ? (uint32_t)ZWZ_INF_DATA_ERROR : total > cap ? (uint32_t)ZWZ_INF_OVERFLOW : 0u; }
        if (t >= 64u && t - 64u < tail && total <= cap) dst[end + (t - 64u)] = (uint8_t)dstream_tail_byte(O.wrap, t - 64u, S.chk[s], S.in_len[s]);
    }
    __syncthreads();
    if (end <= cap) wg_copy(dst + start, slot + 2, slen);
}

// Piece k of its stream is point k of the rule, at decoded offset k * F.piece behind X.off_base; the point in front of it is the
// piece in front of it, whichever slice that was in.
__global__ void __launch_bounds__(256) dstream_due_kernel(DstreamStreams S, DstreamPieces P, PieceForm F, uint64_t g0, uint32_t m, DstreamIndex X) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= m) return;
    const uint32_t s = P.sidx[p];
    const uint64_t off = X.off_base + (g0 + p - S.pfirst[s]) * F.piece;
    P.due[p] = off == 0u || index_flush_due(off - F.piece, off, X.off_base + S.in_len[s], X.span) ? 1u : 0u;
}

// What the two index kernels share, behind the rank scan and behind pack (S.xs).  A piece's rank within its stream: with `book`, a
// stream's first piece keeps the scan's value for the stream's pieces in later slices, as pack keeps S.xs, and its last piece the
// stream's count.
struct PieceRank { uint32_t s, due; uint64_t r; };
__device__ PieceRank dstream_rank(const DstreamStreams& S, const DstreamPieces& P, uint64_t g0, uint32_t p, bool book) {
    const uint32_t s = P.sidx[p], due = P.due[p];
    const uint64_t g = g0 + p, pf = S.pfirst[s];
    const uint64_t r = P.rank[p] - (pf >= g0 ? P.rank[pf - g0] : S.rs[s]);
    if (book && g == pf) S.rs[s] = P.rank[p];       // (read by this stream's pieces in later slices only)
    if (book && g + 1 == S.pfirst[s + 1]) S.cnt[s] = r + due;
    return PieceRank{s, due, r};
}
// The entry of a due piece, three 8-byte stores where its rank says: its first bit is where pack put it, hist its dictionary's length
__device__ void dstream_entry(const DstreamStreams& S, const DstreamPieces& P, PieceForm F, uint64_t g0, uint32_t p, const PieceRank& k, const DstreamOut& O,
                              const DstreamIndex& X, uint32_t hist) {
    const uint64_t pf = S.pfirst[k.s], xs = pf >= g0 ? P.x[pf - g0] : S.xs[k.s];
    const uint32_t hdr = O.partial ? 0u : dstream_header_bytes(O.wrap);
    uint64_t* e = reinterpret_cast<uint64_t*>(X.idx + S.idx_off[k.s] + kIdxHeader + k.r * kIdxEntry);
    e[0] = 8u * (X.pos_base + hdr + (P.x[p] - xs));
    e[1] = X.off_base + (g0 + p - pf) * F.piece;
    e[2] = hist;
}

// Independent pieces, a thread per piece: no entry is written that would end behind the index's capacity.
__global__ void __launch_bounds__(256) dstream_index_kernel(DstreamStreams S, DstreamPieces P, PieceForm F, uint64_t g0, uint32_t m, DstreamOut O, DstreamIndex X) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= m) return;
    const PieceRank k = dstream_rank(S, P, g0, p, true);
    if (!k.due || index_flush_bytes(k.r + 1u) > S.idx_cap[k.s]) return;
    dstream_entry(S, P, F, g0, p, k, O, X, 0u);
}

// Dependent pieces, a workgroup per piece.  Thread 0 does dstream_index_kernel's work -- the entry's hist is the piece's dictionary --
// and the workgroup copies the window, the input in front of the piece (the chunk's head), to its place: window w of the index belongs to
// entry w + 1 (entry 0, at offset 0, has none).  A whole call knows the number of entries, and so where the windows start and whether
// the index fits, before it writes any (index_dep_count); a partial call's windows go to win_base, in the order of its entries.
__global__ void __launch_bounds__(256) dstream_index_windows_kernel(const uint8_t* __restrict__ in, DstreamStreams S, DstreamPieces P, PieceForm F, uint64_t g0,
                                                                    DstreamOut O, DstreamIndex X, uint64_t win_base) {
    const uint32_t p = blockIdx.x, t = threadIdx.x;
    const PieceRank k = dstream_rank(S, P, g0, p, t == 0);
    if (!k.due) return;
    const uint32_t hist = P.skip[p];
    const uint64_t r = k.r;
    uint64_t win_at;                                // of the stream's index space: where this entry's window goes (meaningless without one)
    if (O.partial) {
        if (index_flush_bytes(r + 1u) > win_base) return;
        win_at = win_base + (r - (X.off_base == 0u ? 1u : 0u)) * F.dict;
    } else {
        const uint64_t count = index_dep_count(S.in_len[k.s], X.span);
        if (r >= count || index_dep_bytes(count) > S.idx_cap[k.s]) return;
        win_at = kIdxHeader + count * kIdxEntry + (r - 1u) * F.dict;
    }
    if (hist && win_at + hist > S.idx_cap[k.s]) return;
    if (t == 0) dstream_entry(S, P, F, g0, p, k, O, X, hist);
    if (hist) wg_copy(X.idx + S.idx_off[k.s] + win_at, in + P.off[p], hist);
}
static_assert(kIdxDepPiece == kDepPieceBytes && kIdxDepDict == kDepDictBytes, "index_core.h's dependent geometry is dstream_core.h's");

// One workgroup per stream, behind the last slice: the entry of a stream without input, the padding, the index CRC and the header.
// The stream's length and status are pack's (or begin's), its stored check value combine's.  With windows (F.dict) they lie behind the
// entries and the padding behind them, and the count must be the one the windows were placed by.
__global__ void __launch_bounds__(kBgzfThreads) dstream_index_seal_kernel(const CrcTables* tab, DstreamStreams S, PieceForm F, DstreamOut O, DstreamIndex X) {
    __shared__ CrcLds lds;
    crc_load_tables(lds, tab);
    const uint32_t t = threadIdx.x;
    for (uint32_t i = blockIdx.x; i < S.n; i += gridDim.x) {
        const uint64_t n = S.in_len[i], count = n ? S.cnt[i] : 1u, len = F.dict ? index_dep_bytes(count) : index_flush_bytes(count);      // (workgroup-uniform, as the branch below)
        if (O.status[i] != 0u || count > 0xffffffffull || len > 0xffffffffull || len > S.idx_cap[i] || (F.dict && count != index_dep_count(n, X.span))) {
            if (t == 0) X.idx_len[i] = 0;
            continue;
        }
        uint8_t* q = X.idx + S.idx_off[i];
        if (t == 0) {
            uint64_t* e = reinterpret_cast<uint64_t*>(q + kIdxHeader);
            if (!n) { e[0] = 8u * dstream_header_bytes(O.wrap); e[1] = 0; e[2] = 0; }
            if (count & 1u) *reinterpret_cast<uint64_t*>(q + len - 8u) = 0;       // 24 count is 8 mod 16, a window 0: the padding
        }
        const uint64_t total = O.out_len[i];
        index_seal_wg(lds, q, (uint32_t)len, IndexHeader{O.wrap, X.span, total, n, (uint32_t)count, index_flush_end_bit(total - dstream_trailer_bytes(O.wrap) - 2u),
                                                         O.wrap == kWrapRaw ? 0u : S.chk[i], 0u});
        if (t == 0) X.idx_len[i] = len;
        __syncthreads();
    }
}

}  // namespace

hipError_t launch_dstream_begin(const DstreamStreams& S, const DstreamOut& O, hipStream_t s) {
    if (!S.n) return hipSuccess;
    dstream_begin_kernel<<<(S.n + 255u) / 256u, 256, 0, s>>>(S, O);
    return hipGetLastError();
}

hipError_t launch_dstream_layout(const DstreamStreams& S, const DstreamPieces& P, PieceForm F, uint32_t lead, uint64_t g0, uint32_t m, hipStream_t s) {
    if (!m) return hipSuccess;
    dstream_layout_kernel<<<(m + 255u) / 256u, 256, 0, s>>>(S, P, F, lead, g0, m);
    return hipGetLastError();
}

hipError_t launch_dstream_adler(const uint8_t* in, const DstreamPieces& P, uint32_t m, uint32_t cu_count, hipStream_t s) {
    if (!m) return hipSuccess;
    const uint32_t g = (cu_count ? cu_count : 256u) * 8u;
    dstream_adler_kernel<<<m < g ? m : g, kBgzfThreads, 0, s>>>(in, P, m);
    return hipGetLastError();
}

hipError_t launch_dstream_size(const ChunkInfo* info, const BlockInfo* blocks, const BlockOut* plans, const DstreamPieces& P, uint32_t m, uint32_t* err,
                               hipStream_t s) {
    if (!m) return hipSuccess;
    dstream_size_kernel<<<(m + 255u) / 256u, 256, 0, s>>>(info, blocks, plans, P, m, err);
    return hipGetLastError();
}

hipError_t launch_dstream_combine(const DstreamStreams& S, const DstreamPieces& P, PieceForm F, uint64_t g0, uint32_t m, uint32_t s0, uint32_t ns, uint32_t wrap,
                                  hipStream_t s) {
    if (!m || !ns || wrap == kWrapRaw) return hipSuccess;
    const uint32_t grid = (ns + 3u) / 4u;
    if (wrap == kWrapGzip) dstream_combine_kernel<CrcSum, false><<<grid, 256, 0, s>>>(S, P, F, g0, m, s0, ns);
    else if (F.dict) dstream_combine_kernel<AdlerSum, false><<<grid, 256, 0, s>>>(S, P, F, g0, m, s0, ns);
    else dstream_combine_kernel<AdlerSum, true><<<grid, 256, 0, s>>>(S, P, F, g0, m, s0, ns);
    return hipGetLastError();
}

hipError_t launch_dstream_pack(const DstreamStreams& S, const DstreamPieces& P, uint64_t g0, uint32_t m, const DstreamOut& O, const uint32_t* err,
                               hipStream_t s) {
    if (!m) return hipSuccess;
    dstream_pack_kernel<<<m, 256, 0, s>>>(S, P, g0, O, err);
    return hipGetLastError();
}

hipError_t launch_dstream_due(const DstreamStreams& S, const DstreamPieces& P, PieceForm F, uint64_t g0, uint32_t m, const DstreamIndex& X, hipStream_t s) {
    if (!m) return hipSuccess;
    dstream_due_kernel<<<(m + 255u) / 256u, 256, 0, s>>>(S, P, F, g0, m, X);
    return hipGetLastError();
}

hipError_t launch_dstream_index(const uint8_t* in, const DstreamStreams& S, const DstreamPieces& P, PieceForm F, uint64_t g0, uint32_t m, const DstreamOut& O,
                                const DstreamIndex& X, uint64_t win_base, hipStream_t s) {
    if (!m) return hipSuccess;
    if (F.dict) dstream_index_windows_kernel<<<m, 256, 0, s>>>(in, S, P, F, g0, O, X, win_base);
    else dstream_index_kernel<<<(m + 255u) / 256u, 256, 0, s>>>(S, P, F, g0, m, O, X);
    return hipGetLastError();
}

hipError_t launch_dstream_index_seal(const CrcTables* tab, const DstreamStreams& S, PieceForm F, const DstreamOut& O, const DstreamIndex& X, uint32_t cu_count,
                                     hipStream_t s) {
    if (!S.n) return hipSuccess;
    const uint32_t g = (cu_count ? cu_count : 256u) * 4u;
    dstream_index_seal_kernel<<<S.n < g ? S.n : g, kBgzfThreads, 0, s>>>(tab, S, F, O, X);
    return hipGetLastError();
}

}  // namespace zwz
