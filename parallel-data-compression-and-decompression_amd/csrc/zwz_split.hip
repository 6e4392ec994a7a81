// zwz_split.hip -- the device half of zwz_inflate_split_streams_dev on gfx950 around inflate_kernel's two split forms (split_core.h has
// the method): where the streams' bodies start (head), their candidates in stream order (count, BGZF's scan, write), the chain of
// every stream by pointer jumping (link, jump, mark, resolve), the records of the segment decode (emit), and the checksum of a
// splitting stream's output from fixed pieces computed in parallel and joined with dstream_core.h's sums (finish).  With an index
// (zwz_inflate_split_streams_index_dev): the entries at the chain's piece starts (index) and the header behind the verdict (seal).
#include "../../include/zwz.h"
#include "adler_wg.h"
#include "crc_wg.h"
#include "dstream_core.h"
#include "index_seal_wg.h"
#include "zwz_bgzf.h"
#include "zwz_device.h"
#include "zwz_split.h"

namespace zwz {

namespace {

constexpr uint32_t kScanThreads = kSplitTile / 16u;      // 256

__global__ void __launch_bounds__(256) split_head_kernel(SplitStreams S, uint32_t min_bytes) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= S.n) return;
    uint32_t body = 0;
    const bool ok = split_eligible(S.wrap, S.in + S.in_off[i], S.in_len[i], S.out_cap[i], min_bytes, &body);
    S.body[i] = ok ? body : kSplitNil;
}

// the last index i < n with first[i] <= x (first[0] <= x < first[n])
__device__ __forceinline__ uint32_t owner_of(const uint32_t* first, uint32_t n, uint32_t x) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (first[mid] <= x) lo = mid; else hi = mid;
    }
    return lo;
}

// One workgroup per tile of kSplitTile input bytes, 16 bytes a lane.  kWrite = false counts the tile's candidates; kWrite = true, behind
// the scan, writes the candidates of the kept streams at their ranks (only tiles that hold one read their input again).
template <bool kWrite>
__global__ void __launch_bounds__(kScanThreads) split_scan_kernel(SplitStreams S, SplitCands C, uint32_t budget) {
    __shared__ uint32_t wsum[kScanThreads / 64];
    const uint32_t tile = blockIdx.x, t = threadIdx.x, lane = t & 63u, w = t >> 6;
    if (kWrite && S.tile_cnt[tile] == 0u) return;
    const uint32_t s = owner_of(S.tile_first, S.n, tile);
    if (kWrite && S.kbase[s + 1] == S.kbase[s]) return;
    const uint32_t body = S.body[s], nin = (uint32_t)S.in_len[s], nin16 = (nin + 15u) & ~15u;
    const uint32_t o = (tile - S.tile_first[s]) * kSplitTile + t * 16u;
    uint32_t mask = 0;
    if (body != kSplitNil && o < nin16) {
        const uint8_t* src = S.in + S.in_off[s];
        const uint4 v = *reinterpret_cast<const uint4*>(src + o);
        const uint32_t wd[5] = {o ? *reinterpret_cast<const uint32_t*>(src + o - 4u) : 0u, v.x, v.y, v.z, v.w};
        mask = split_candidate_mask(wd, o, body, nin);
    }
    const uint32_t c = (uint32_t)__popc(mask), incl = wave_scan_incl(c);
    if (lane == 63u) wsum[w] = incl;
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (uint32_t j = 0; j < kScanThreads / 64; j++) { const uint32_t x = wsum[j]; before += j < w ? x : 0u; total += x; }
    if (!kWrite) { if (t == 0) S.tile_cnt[tile] = total; return; }
    uint32_t idx = S.kbase[s] + (uint32_t)(S.tile_off[tile] - S.cfirst[s]) + before + incl - c;
    const uint64_t soff = S.in_off[s];
    while (mask) {
        const uint32_t p = o + (uint32_t)__builtin_ctz(mask);
        mask &= mask - 1u;
        C.pos[idx] = p;
        C.seg[idx] = make_uint4(p & 15u, s, 0u, p & ~15u);
        C.in_off[idx] = soff + (p & ~15u);
        C.in_len[idx] = split_wave_input(p, nin, budget);
        idx++;
    }
}

__global__ void __launch_bounds__(256) split_ranges_kernel(SplitStreams S) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > S.n) return;
    const uint32_t tf = S.tile_first[i];
    S.cfirst[i] = i < S.n && tf < S.n_tiles ? S.tile_off[tf] : S.base[0];
}

// the chain's first link: from a segment that ends in a flush to the candidate at its end; the heads are the chains' first marks
__global__ void __launch_bounds__(256) split_link_kernel(SplitStreams S, SplitCands C) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= C.m) return;
    const uint4 mz = C.meas[k];
    const uint32_t s = C.seg[k].y;
    C.jump[k] = mz.x == kSegFlush ? split_find(C.pos, S.kbase[s], S.kbase[s + 1], mz.y) : kSplitNil;
    C.mark[k] = k == S.kbase[s] ? 1u : 0u;
}

__global__ void __launch_bounds__(256) split_jump_kernel(SplitCands C, uint32_t level) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= C.m) return;
    const uint32_t* prev = C.jump + (size_t)(level - 1u) * C.m;
    const uint32_t a = prev[k];
    C.jump[(size_t)level * C.m + k] = a == kSplitNil ? kSplitNil : prev[a];
}

// Levels from the highest down: a marked node marks the node 2^level steps on.  After level 0 every node within 2^levels - 1 steps of
// a head is marked.  (A mark set by another lane of the same launch and seen here only sends it on early: every mark is on the chain.)
__global__ void __launch_bounds__(256) split_mark_kernel(SplitCands C, uint32_t level) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= C.m) return;
    if (!__hip_atomic_load(&C.mark[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
    const uint32_t a = C.jump[(size_t)level * C.m + k];
    if (a != kSplitNil) __hip_atomic_store(&C.mark[a], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One workgroup per stream: the chain's segments in order (offsets ascend along a chain, so the marks are in chain order), their ranks
// and the exclusive sum of their counts; the last of them must end the stream, and the trailer must be fine.
constexpr uint32_t kResolveThreads = 256;
// partial (zwz_inflate_stream_file, one slice of a file): the stream need not end here.  The result is the longest prefix of the chain
// whose segments ended at a flush or the final block and whose counts fit pcap; res2 = (where it ends, how its last segment ended).
__global__ void __launch_bounds__(kResolveThreads) split_resolve_kernel(SplitStreams S, SplitCands C, uint4* res, uint32_t partial, uint64_t pcap, uint4* res2) {
    __shared__ uint64_t sh_sum[kResolveThreads];
    __shared__ uint32_t sh_cnt[kResolveThreads];
    __shared__ uint32_t sh_last, sh_nok, sh_lastok;
    __shared__ unsigned long long sh_sumok;
    const uint32_t s = blockIdx.x, t = threadIdx.x;
    const uint32_t k0 = S.kbase[s], k1 = S.kbase[s + 1];
    if (k0 == k1) { if (t == 0) res[s] = make_uint4(0, 0, 0, 0); return; }      // (res2[s] stays unwritten: res[s].x == 0 gates every reader of it)
    if (t == 0) { sh_last = 0; sh_nok = 0; sh_lastok = 0; sh_sumok = 0; }
    uint64_t carry = 0;
    uint32_t ncarry = 0;
    __syncthreads();
    for (uint32_t b = k0; b < k1; b += kResolveThreads) {
        const uint32_t k = b + t;
        const bool on = k < k1 && C.mark[k] != 0u;
        const uint32_t cnt = on ? C.meas[k].z : 0u;
        sh_sum[t] = cnt; sh_cnt[t] = on ? 1u : 0u;
        __syncthreads();
        for (uint32_t d = 1; d < kResolveThreads; d <<= 1) {
            const uint64_t a = t >= d ? sh_sum[t - d] : 0ull;
            const uint32_t ac = t >= d ? sh_cnt[t - d] : 0u;
            __syncthreads();
            sh_sum[t] += a; sh_cnt[t] += ac;
            __syncthreads();
        }
        const uint64_t before = carry + sh_sum[t] - cnt;
        if (on) {
            C.rank[k] = ncarry + sh_cnt[t] - 1u;
            C.ostart[k] = (uint32_t)min<uint64_t>(before, 0xffffffffull);      // (saturates only in a chain whose counts pass the capacity: not decoded)
            atomicMax(&sh_last, k - k0);
            if (partial && C.meas[k].x != kSegBad && before + cnt <= pcap) {     // (a prefix: only a chain's last segment is kSegBad, the sums ascend)
                atomicAdd(&sh_nok, 1u); atomicAdd(&sh_sumok, (unsigned long long)cnt); atomicMax(&sh_lastok, k - k0);
            }
        }
        carry += sh_sum[kResolveThreads - 1u]; ncarry += sh_cnt[kResolveThreads - 1u];
        __syncthreads();
    }
    if (t != 0) return;
    if (partial) {
        const uint4 e = C.meas[k0 + sh_lastok];
        res[s] = sh_nok ? make_uint4(1u, sh_nok, (uint32_t)sh_sumok, 0u) : make_uint4(0, 0, 0, 0);
        res2[s] = make_uint4(e.y, e.x, e.w, 0u);
        return;
    }
    const uint4 end = C.meas[k0 + sh_last];
    const uint32_t nin = (uint32_t)S.in_len[s];
    bool ok = end.x == kSegFinal && ncarry >= 2u && carry <= S.out_cap[s] && carry <= 0xffffffffull;      // (every capacity the call accepts, 2^32 - 1 included: kSplitMeasureCap bounds one segment, not the stream)
    uint32_t expect = 0;
    if (ok) ok = split_trailer_ok(S.wrap, S.in + S.in_off[s], nin, end.y, (uint32_t)carry, &expect);
    res[s] = ok ? make_uint4(1u, ncarry, (uint32_t)carry, expect) : make_uint4(0, 0, 0, 0);
    res2[s] = make_uint4(end.y, end.x, end.w, 0u);
}

__global__ void __launch_bounds__(256) split_emit_kernel(SplitCands C, SplitDecode D) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= C.m || !C.mark[k]) return;
    const uint4 sg = C.seg[k];
    if (!D.res[sg.y].x || C.rank[k] >= D.res[sg.y].y) return;       // (a slice of a file decodes a prefix of its chain)
    const uint32_t idx = D.dbase[sg.y] + C.rank[k];
    const uint4 mz = C.meas[k];
    D.in_off[idx] = C.in_off[k];
    D.in_len[idx] = mz.y - sg.w;                    // up to the byte behind the segment's last block
    D.seg[idx] = make_uint4(sg.x, sg.y, C.ostart[k], mz.z);
}

__global__ void __launch_bounds__(256) split_pieces_kernel(SplitPieces P, const uint4* res, const uint64_t* out_off, uint32_t n) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= P.p) return;
    const uint32_t s = owner_of(P.pbase, n, j);
    const uint64_t at = (uint64_t)(j - P.pbase[s]) * kPieceBytes;
    P.off[j] = out_off[s] + at;
    P.len[j] = (uint32_t)min<uint64_t>(kPieceBytes, res[s].z - at);
}

__global__ void __launch_bounds__(kBgzfThreads) split_adler_kernel(const uint8_t* out, SplitPieces P) {
    __shared__ uint32_t s_part[2 * kBgzfThreads / 64];
    for (uint32_t j = blockIdx.x; j < P.p; j += gridDim.x) {
        const uint32_t a = adler_range_wg(s_part, out + P.off[j], P.len[j]);
        if (threadIdx.x == 0) P.val[j] = a;
    }
}

// One wave per splitting stream: lane l joins its share of consecutive pieces, lane 0 the 64 shares; then the stream's results.
template <class Sum, bool kCheck>
__global__ void __launch_bounds__(256) split_finish_kernel(SplitPieces P, const uint4* res, const uint32_t* bad, uint32_t n, uint64_t* out_len,
                                                           uint32_t* status, uint32_t* segments, uint32_t* chk_out /* not null: no verdict, the checksum itself */) {
    const uint32_t s = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = lane_id();
    if (s >= n) return;
    const uint4 r = res[s];
    if (!r.x) return;
    uint32_t acc = Sum::identity();
    if (kCheck) {
        const uint32_t j0 = P.pbase[s], cnt = P.pbase[s + 1] - j0, K = (cnt + 63u) / 64u;
        const uint32_t p1 = Sum::pof(kPieceBytes);
        uint32_t x = Sum::identity();
        uint64_t bytes = 0;
        for (uint32_t j = lane * K; j < min(cnt, (lane + 1u) * K); j++) {
            const uint32_t len = P.len[j0 + j];
            x = Sum::join(x, P.val[j0 + j], len == kPieceBytes ? p1 : Sum::pof(len));
            bytes += len;
        }
        const uint32_t pl = Sum::pof(bytes);
        for (uint32_t l = 0; l < 64u; l++) acc = Sum::join(acc, (uint32_t)__shfl((int)x, (int)l, 64), (uint32_t)__shfl((int)pl, (int)l, 64));
    }
    if (lane != 0) return;
    out_len[s] = r.z;
    status[s] = bad[s] ? (uint32_t)ZWZ_INF_DATA_ERROR : kCheck && !chk_out && acc != r.w ? (uint32_t)kStrChecksum : 0u;
    if (chk_out) chk_out[s] = acc;
    if (segments) segments[s] = r.y;
}

// One workgroup per splitting stream, over the chain's segments in order -- emit's records, dense by rank: segment j starts at
// point j of the rule, at the stream offset its input and its first byte's place in it give and at the decoded offset resolve summed.
// A tile of 256 points a round: the due flag from the point's offset and the one in front of it, its rank among the due ones from
// the wave's ballot, the waves in front of it (LDS) and the tiles in front of it; an entry is three 8-byte stores, and none is
// written that would end behind the index's capacity.
constexpr uint32_t kIndexThreads = 256;
__global__ void __launch_bounds__(kIndexThreads) split_index_kernel(SplitStreams S, SplitDecode D, SplitIndex X) {
    __shared__ uint32_t wsum[kIndexThreads / 64];
    const uint32_t s = blockIdx.x, t = threadIdx.x, lane = t & 63u, w = t >> 6;
    const uint4 r = D.res[s];
    if (!r.x) return;                                // (workgroup-uniform)
    const uint32_t d0 = D.dbase[s], nseg = r.y;
    const uint64_t in0 = S.in_off[s], cap = X.idx_cap[s];
    uint8_t* ent = X.idx + X.idx_off[s] + kIdxHeader;
    uint32_t carry = 0;
    for (uint32_t b = 0; b < nseg; b += kIndexThreads) {
        const uint32_t j = b + t;
        const bool on = j < nseg;
        const uint4 sg = on ? D.seg[d0 + j] : make_uint4(0, 0, 0, 0);
        const uint32_t prev = on && j ? D.seg[d0 + j - 1u].z : 0u;
        const bool due = on && (j == 0u || index_flush_due(prev, sg.z, r.z, X.span));
        const uint64_t vote = __ballot(due);
        if (lane == 0) wsum[w] = (uint32_t)__popcll(vote);
        __syncthreads();
        uint32_t before = 0, total = 0;
#pragma unroll
        for (uint32_t i = 0; i < kIndexThreads / 64; i++) { const uint32_t x = wsum[i]; before += i < w ? x : 0u; total += x; }
        const uint32_t rank = carry + before + (uint32_t)__popcll(vote & ((1ull << lane) - 1ull));
        if (due && index_flush_bytes((uint64_t)rank + 1u) <= cap) {
            uint64_t* e = reinterpret_cast<uint64_t*>(ent + (size_t)rank * kIdxEntry);
            e[0] = 8u * (D.in_off[d0 + j] - in0 + sg.x);
            e[1] = sg.z;
            e[2] = 0;
        }
        carry += total;
        __syncthreads();                             // (wsum is rewritten by the next round)
    }
    if (t == 0) X.count[s] = carry;
}

// One workgroup per splitting stream, behind the verdict: the padding, the index CRC and the header.  The stored check value is the
// trailer's (resolve read it), the end bit the final segment's (res2).
__global__ void __launch_bounds__(kBgzfThreads) split_seal_kernel(const CrcTables* tab, SplitStreams S, SplitDecode D, SplitIndex X, const uint4* res2,
                                                                  const uint32_t* status) {
    __shared__ CrcLds lds;
    crc_load_tables(lds, tab);
    const uint32_t t = threadIdx.x;
    for (uint32_t s = blockIdx.x; s < S.n; s += gridDim.x) {
        const uint4 r = D.res[s];
        if (!r.x) continue;                          // (workgroup-uniform, as the branch below)
        const uint64_t count = X.count[s], len = index_flush_bytes(count);
        if (status[s] != 0u || len > X.idx_cap[s]) {
            if (t == 0) X.idx_len[s] = 0;
            continue;
        }
        uint8_t* q = X.idx + X.idx_off[s];
        if (t == 0 && (count & 1u)) reinterpret_cast<uint64_t*>(q + kIdxHeader)[3u * count] = 0;      // 24 count is 8 mod 16: the padding
        index_seal_wg(lds, q, (uint32_t)len, IndexHeader{S.wrap, X.span, S.in_len[s], r.z, (uint32_t)count, split_final_end_bit(res2[s].x, res2[s].z),
                                                         S.wrap == kWrapRaw ? 0u : r.w, 0u});
        if (t == 0) X.idx_len[s] = len;
        __syncthreads();
    }
}

inline uint32_t blocks_of(uint32_t n) { return (n + 255u) / 256u; }

}  // namespace

hipError_t launch_split_head(const SplitStreams& S, uint32_t min_bytes, hipStream_t s) {
    split_head_kernel<<<blocks_of(S.n), 256, 0, s>>>(S, min_bytes);
    return hipGetLastError();
}

hipError_t launch_split_count(const SplitStreams& S, hipStream_t s) {
    hipError_t e = hipMemsetAsync(S.base, 0, 16, s);
    if (e != hipSuccess) return e;
    if (S.n_tiles) {
        split_scan_kernel<false><<<S.n_tiles, kScanThreads, 0, s>>>(S, SplitCands{}, 0u);
        e = launch_bgzf_scan(S.tile_cnt, S.n_tiles, 0, ~0u, S.tile_off, S.base, reinterpret_cast<uint32_t*>(S.base + 1), s);
        if (e != hipSuccess) return e;
    }
    split_ranges_kernel<<<blocks_of(S.n + 1u), 256, 0, s>>>(S);
    return hipGetLastError();
}

hipError_t launch_split_write(const SplitStreams& S, const SplitCands& C, uint32_t budget, hipStream_t s) {
    if (!C.m || !S.n_tiles) return hipSuccess;
    split_scan_kernel<true><<<S.n_tiles, kScanThreads, 0, s>>>(S, C, budget);
    return hipGetLastError();
}

hipError_t launch_split_resolve(const SplitStreams& S, const SplitCands& C, uint32_t levels, uint4* res, uint32_t partial, uint64_t pcap, uint4* res2,
                                hipStream_t s) {
    if (C.m) {
        split_link_kernel<<<blocks_of(C.m), 256, 0, s>>>(S, C);
        for (uint32_t d = 1; d < levels; d++) split_jump_kernel<<<blocks_of(C.m), 256, 0, s>>>(C, d);
        for (uint32_t d = levels; d-- > 0;) split_mark_kernel<<<blocks_of(C.m), 256, 0, s>>>(C, d);
    }
    split_resolve_kernel<<<S.n, kResolveThreads, 0, s>>>(S, C, res, partial, pcap, res2);
    return hipGetLastError();
}

hipError_t launch_split_emit(const SplitStreams& S, const SplitCands& C, const SplitDecode& D, hipStream_t s) {
    if (!C.m) return hipSuccess;
    split_emit_kernel<<<blocks_of(C.m), 256, 0, s>>>(C, D);
    return hipGetLastError();
}

hipError_t launch_split_finish(const SplitStreams& S, const SplitDecode& D, const SplitPieces& P, const CrcTables* tab, const uint8_t* out,
                               const uint64_t* out_off, const uint32_t* bad, uint64_t* out_len, uint32_t* status, uint32_t* segments,
                               uint32_t* chk_out, uint32_t cu_count, hipStream_t s) {
    const uint32_t grid = (S.n + 3u) / 4u;
    if (S.wrap == kWrapRaw) {
        split_finish_kernel<AdlerSum, false><<<grid, 256, 0, s>>>(P, D.res, bad, S.n, out_len, status, segments, chk_out);
        return hipGetLastError();
    }
    if (P.p) {
        split_pieces_kernel<<<blocks_of(P.p), 256, 0, s>>>(P, D.res, out_off, S.n);
        if (S.wrap == kWrapGzip) {
            const hipError_t e = launch_crc32_blocks(tab, out, P.off, P.len, P.p, P.val, cu_count, s);
            if (e != hipSuccess) return e;
        } else {
            const uint32_t g = (cu_count ? cu_count : 256u) * 8u;
            split_adler_kernel<<<P.p < g ? P.p : g, kBgzfThreads, 0, s>>>(out, P);
        }
    }
    if (S.wrap == kWrapGzip) split_finish_kernel<CrcSum, true><<<grid, 256, 0, s>>>(P, D.res, bad, S.n, out_len, status, segments, chk_out);
    else split_finish_kernel<AdlerSum, true><<<grid, 256, 0, s>>>(P, D.res, bad, S.n, out_len, status, segments, chk_out);
    return hipGetLastError();
}

hipError_t launch_split_index(const SplitStreams& S, const SplitDecode& D, const SplitIndex& X, hipStream_t s) {
    if (!S.n) return hipSuccess;
    split_index_kernel<<<S.n, kIndexThreads, 0, s>>>(S, D, X);
    return hipGetLastError();
}

hipError_t launch_split_seal(const SplitStreams& S, const SplitDecode& D, const SplitIndex& X, const uint4* res2, const CrcTables* tab, const uint32_t* status,
                             uint32_t cu_count, hipStream_t s) {
    if (!S.n) return hipSuccess;
    const uint32_t g = (cu_count ? cu_count : 256u) * 4u;
    split_seal_kernel<<<S.n < g ? S.n : g, kBgzfThreads, 0, s>>>(tab, S, D, X, res2, status);
    return hipGetLastError();
}

}  // namespace zwz
