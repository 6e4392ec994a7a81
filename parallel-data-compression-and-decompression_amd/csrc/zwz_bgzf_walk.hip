// zwz_bgzf_walk.hip -- the walk of BGZF member chains on gfx950 (bgzf_core.h has the method): the candidates of a batch of spans in
// offset order (count, BGZF's scan, fill), their parse and first link, the chains by pointer jumping (jump, mark), the marked good
// members ranked by two prefix sums (values, BGZF's scan, emit) and the end of every span's chain (resolve).  No kernel follows a
// chain member by member.
#include <algorithm>

#include "zwz_api_internal.h"
#include "zwz_bgzf.h"
#include "zwz_bgzf_walk.h"
#include "zwz_device.h"

namespace zwz {

namespace {

constexpr uint32_t kWalkThreads = kBgzfWalkTile / 16u;      // 256

struct WalkSpans {                                   // per span and per scan tile (kBufWalk0)
    const uint8_t* gz; uint64_t n;
    BgzfSpan* span; uint32_t ns;
    uint32_t* tile_first;                            // ns + 1: the span's first tile; [ns] = n_tiles
    uint32_t n_tiles;
    uint32_t* tile_cnt; uint64_t* tile_off;          // candidates of a tile, and in front of it
    uint32_t* kbase;                                 // ns + 1: the span's first candidate; [ns] = m
    uint32_t* tail;                                  // the last node of the span's chain, or kBgzfNil
    BgzfSpanResult* res;
    uint64_t* base;                                  // [0] candidates, [1] a flag bgzf_scan wants, [2] good chain members, [3] their ISIZE sum
};

struct WalkCands {                                   // per candidate (kBufWalk1)
    uint32_t m, levels;
    uint64_t* pos;
    BgzfMeas* meas;
    uint32_t* jump;                                  // levels * m: the node 2^level links on, or kBgzfNil
    uint32_t* mark;
    uint32_t *vcnt, *visz;                           // m + 1: 1 / ISIZE of a good member on a chain, else 0
    uint64_t *rank, *usum;                           // m + 1: their exclusive sums
    uint64_t* moff; uint32_t* misize;                // m + 2 ns member slots: the resolve step adds at most two members to a span's list
};

// the last index i < n with first[i] <= x (first[0] <= x)
__device__ __forceinline__ uint32_t owner_of(const uint32_t* first, uint32_t n, uint32_t x) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (first[mid] <= x) lo = mid; else hi = mid;
    }
    return lo;
}

// One workgroup per tile of kBgzfWalkTile bytes, 16 bytes a lane.  kWrite = false counts the tile's candidates; kWrite = true, behind
// the scan, writes their offsets at their ranks (only tiles that hold one read their input again).
template <bool kWrite>
__global__ void __launch_bounds__(kWalkThreads) bgzf_walk_scan_kernel(WalkSpans S, WalkCands C) {
    __shared__ uint32_t wsum[kWalkThreads / 64];
    const uint32_t tile = blockIdx.x, t = threadIdx.x, lane = t & 63u, w = t >> 6;
    if (kWrite && S.tile_cnt[tile] == 0u) return;
    const uint32_t s = owner_of(S.tile_first, S.ns, tile);
    const BgzfSpan sp = S.span[s];
    const uint64_t hi = bgzf_span_end(sp, S.n);
    const uint64_t o = bgzf_span_base(sp) + (uint64_t)(tile - S.tile_first[s]) * kBgzfWalkTile + t * 16u;
    uint32_t mask = 0;
    if (o < hi) {
        uint32_t wd[5];
        if (o + 20u <= S.n) {
            const uint4 v = *reinterpret_cast<const uint4*>(S.gz + o);
            wd[0] = v.x; wd[1] = v.y; wd[2] = v.z; wd[3] = v.w;
            wd[4] = *reinterpret_cast<const uint32_t*>(S.gz + o + 16u);
        } else {
            // the buffer's last vectors: byte by byte, nothing read behind its end
#pragma unroll
            for (uint32_t q = 0; q < 5; q++) {
                uint32_t x = 0;
#pragma unroll
                for (uint32_t b = 0; b < 4; b++) {
                    const uint64_t p = o + 4u * q + b;
                    if (p < S.n) x |= (uint32_t)S.gz[p] << (8u * b);
                }
                wd[q] = x;
            }
        }
        mask = bgzf_candidate_mask(wd, o, sp.head, hi, S.n);
    }
    const uint32_t c = (uint32_t)__popc(mask), incl = wave_scan_incl(c);
    if (lane == 63u) wsum[w] = incl;
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (uint32_t j = 0; j < kWalkThreads / 64; j++) { const uint32_t x = wsum[j]; before += j < w ? x : 0u; total += x; }
    if (!kWrite) { if (t == 0) S.tile_cnt[tile] = total; return; }
    uint64_t idx = S.tile_off[tile] + before + incl - c;
    while (mask) {
        C.pos[idx++] = o + (uint32_t)__builtin_ctz(mask);
        mask &= mask - 1u;
    }
}

__global__ void __launch_bounds__(256) bgzf_walk_ranges_kernel(WalkSpans S, uint32_t m) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > S.ns) return;
    const uint32_t tf = S.tile_first[i];
    S.kbase[i] = i < S.ns && tf < S.n_tiles ? (uint32_t)S.tile_off[tf] : m;
    if (i < S.ns) S.tail[i] = kBgzfNil;
}

// the parse of every candidate and the chain's first link; the spans' heads are the chains' first marks
__global__ void __launch_bounds__(256) bgzf_walk_parse_kernel(WalkSpans S, WalkCands C) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= C.m) return;
    const uint32_t s = owner_of(S.kbase, S.ns, k);
    const BgzfSpan sp = S.span[s];
    BgzfMeas mz;
    C.jump[k] = bgzf_parse_link(S.gz, S.n, sp, C.pos, S.kbase[s], S.kbase[s + 1], k, &mz);
    C.meas[k] = mz;
    C.mark[k] = C.pos[k] == sp.head ? 1u : 0u;
}

__global__ void __launch_bounds__(256) bgzf_walk_jump_kernel(WalkCands C, uint32_t level) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= C.m) return;
    const uint32_t* prev = C.jump + (size_t)(level - 1u) * C.m;
    const uint32_t a = prev[k];
    C.jump[(size_t)level * C.m + k] = a == kBgzfNil ? kBgzfNil : prev[a];
}

// Levels from the highest down: a marked node marks the node 2^level links on.  After level 0 every node within 2^levels - 1 links of
// a head is marked.  (A mark set by another lane of the same launch and seen here only sends it on early: every mark is on a chain.)
__global__ void __launch_bounds__(256) bgzf_walk_mark_kernel(WalkCands C, uint32_t level) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= C.m) return;
    if (!__hip_atomic_load(&C.mark[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
    const uint32_t a = C.jump[(size_t)level * C.m + k];
    if (a != kBgzfNil) __hip_atomic_store(&C.mark[a], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// what the two sums add up, and the chains' last nodes (a chain has one node without a link)
__global__ void __launch_bounds__(256) bgzf_walk_values_kernel(WalkSpans S, WalkCands C) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k > C.m) return;
    if (k == C.m) { C.vcnt[k] = 0; C.visz[k] = 0; return; }
    const bool on = C.mark[k] != 0u;
    const BgzfMeas mz = C.meas[k];
    const bool last = C.jump[k] == kBgzfNil;
    // (the chain's last node is the resolve step's: it may step over the stop)
    const bool good = on && !last && mz.kind == kBgzfOk;
    C.vcnt[k] = good ? 1u : 0u;
    C.visz[k] = good ? mz.isize : 0u;
    if (on && last) S.tail[owner_of(S.kbase, S.ns, k)] = k;
}

__global__ void __launch_bounds__(256) bgzf_walk_emit_kernel(WalkSpans S, WalkCands C) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= C.m || !C.vcnt[k]) return;
    const uint64_t slot = C.rank[k] + 2ull * owner_of(S.kbase, S.ns, k);
    C.moff[slot] = C.pos[k];
    C.misize[slot] = C.meas[k].isize;
}

// One lane per span: the end of its chain (bgzf_span_resolve) and the members it adds, the chain's last node and what `limit` asks for
__global__ void __launch_bounds__(256) bgzf_walk_resolve_kernel(WalkSpans S, WalkCands C) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S.ns) return;
    const BgzfSpan sp = S.span[s];
    const uint32_t k0 = S.kbase[s], tail = S.tail[s];
    const bool has_tail = tail != kBgzfNil;
    const uint64_t r0 = C.rank[k0], u0 = C.usum[k0];
    const uint64_t first = r0 + 2ull * s;
    BgzfMeas tm{kBgzfOk, 0, 0, 0};
    uint64_t tpos = 0, rank = 0, sum = 0;
    if (has_tail) { tm = C.meas[tail]; tpos = C.pos[tail]; rank = C.rank[tail] - r0; sum = C.usum[tail] - u0; }
    bool has_extra = false;
    uint64_t xoff = 0;
    uint32_t xisz = 0;
    BgzfSpanResult r = bgzf_span_resolve(S.gz, S.n, sp, tpos, has_tail, tm, (uint32_t)rank, sum, &has_extra, &xoff, &xisz);
    r.first = first;
    uint64_t slot = first + rank;
    if (has_tail && r.count > rank) { C.moff[slot] = tpos; C.misize[slot] = tm.isize; slot++; }
    if (has_extra) { C.moff[slot] = xoff; C.misize[slot] = xisz; }
    S.res[s] = r;
}

inline uint32_t blocks_of(uint32_t n) { return (n + 255u) / 256u; }

WalkSpans spans_layout(Carver& w, uint32_t ns, uint32_t n_tiles) {
    WalkSpans S{};
    S.span = w.take<BgzfSpan>(ns);
    S.tile_first = w.take<uint32_t>((size_t)ns + 1);
    S.tile_cnt = w.take<uint32_t>(n_tiles);
    S.tile_off = w.take<uint64_t>(n_tiles);
    S.kbase = w.take<uint32_t>((size_t)ns + 1);
    S.tail = w.take<uint32_t>(ns);
    S.res = w.take<BgzfSpanResult>(ns);
    S.base = w.take<uint64_t>(4);
    S.ns = ns; S.n_tiles = n_tiles;
    return S;
}

WalkCands cands_layout(Carver& w, uint32_t m, uint32_t levels, uint32_t ns) {
    WalkCands C{};
    C.m = m; C.levels = levels;
    C.pos = w.take<uint64_t>(m);
    C.meas = w.take<BgzfMeas>(m);
    C.jump = w.take<uint32_t>((size_t)levels * m);
    C.mark = w.take<uint32_t>(m);
    C.vcnt = w.take<uint32_t>((size_t)m + 1);
    C.visz = w.take<uint32_t>((size_t)m + 1);
    C.rank = w.take<uint64_t>((size_t)m + 1);
    C.usum = w.take<uint64_t>((size_t)m + 1);
    C.moff = w.take<uint64_t>((size_t)m + 2 * (size_t)ns);
    C.misize = w.take<uint32_t>((size_t)m + 2 * (size_t)ns);
    return C;
}

}  // namespace

int bgzf_walk_spans(zwz_ctx* c, const uint8_t* d_gz, uint64_t n, const BgzfSpan* spans, uint32_t ns, BgzfWalk* out) {
    out->res.clear();
    out->d_moff = nullptr; out->d_misize = nullptr; out->slots = 0; out->candidates = 0;
    if (!ns) return ZWZ_OK;
    uint64_t tiles = 0;
    for (uint32_t s = 0; s < ns; s++) {
        if (spans[s].head > spans[s].stop || spans[s].stop > n || (s && spans[s].head < spans[s - 1].stop)) {
            set_error("bgzf: walk span %u (%llu, %llu) out of order or outside the %llu bytes", s, (unsigned long long)spans[s].head,
                      (unsigned long long)spans[s].stop, (unsigned long long)n);
            return ZWZ_E_INVALID;
        }
        tiles += bgzf_span_tiles(spans[s], n);
    }
    if (tiles > 0x7fffffffull) { set_error("bgzf: more than 2^31 - 1 scan tiles"); return ZWZ_E_INVALID; }
    const uint32_t n_tiles = (uint32_t)tiles;
    if (int rc = c->buf[kBufWalk0].reserve(c, 0, layout_bytes([&](Carver& w) { spans_layout(w, ns, n_tiles); }))) return rc;
    const size_t up = round_up(sizeof(BgzfSpan) * (size_t)ns, 16) + 4 * ((size_t)ns + 1);
    const size_t hbytes = std::max(up, sizeof(BgzfSpanResult) * (size_t)ns) + 64;
    if (int rc = c->buf[kBufWalkHost].reserve(c, 0, round_up(hbytes, 4096))) return rc;
    Carver w0(c->buf[kBufWalk0].p);
    WalkSpans S = spans_layout(w0, ns, n_tiles);
    S.gz = d_gz; S.n = n;
    uint8_t* h = c->buf[kBufWalkHost].as<uint8_t>();
    BgzfSpan* h_span = reinterpret_cast<BgzfSpan*>(h);
    uint32_t* h_first = reinterpret_cast<uint32_t*>(h + round_up(sizeof(BgzfSpan) * (size_t)ns, 16));
    uint32_t tf = 0;
    for (uint32_t s = 0; s < ns; s++) { h_span[s] = spans[s]; h_first[s] = tf; tf += (uint32_t)bgzf_span_tiles(spans[s], n); }
    h_first[ns] = tf;
    hipStream_t st = c->stream;
    HIPCHK(hipMemcpyAsync(S.span, h_span, sizeof(BgzfSpan) * (size_t)ns, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(S.tile_first, h_first, 4 * ((size_t)ns + 1), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(S.base, 0, 32, st));
    uint64_t m64 = 0;
    if (n_tiles) {
        bgzf_walk_scan_kernel<false><<<n_tiles, kWalkThreads, 0, st>>>(S, WalkCands{});
        HIPCHK(hipGetLastError());
        HIPCHK(launch_bgzf_scan(S.tile_cnt, n_tiles, 0, ~0u, S.tile_off, S.base, reinterpret_cast<uint32_t*>(S.base + 1), st));
        HIPCHK(hipMemcpyAsync(h, S.base, 8, hipMemcpyDeviceToHost, st));      // (behind the uploads on the same stream)
        HIPCHK(hipStreamSynchronize(st));
        m64 = *reinterpret_cast<const uint64_t*>(h);
    }
    if (m64 > 0xfffffff0ull) { set_error("bgzf: more than 2^32 - 16 member candidates"); return ZWZ_E_INVALID; }
    const uint32_t m = (uint32_t)m64, levels = split_levels(m);
    if (int rc = c->buf[kBufWalk1].reserve(c, 0, layout_bytes([&](Carver& w) { cands_layout(w, m, levels, ns); }))) return rc;
    Carver w1(c->buf[kBufWalk1].p);
    const WalkCands C = cands_layout(w1, m, levels, ns);
    bgzf_walk_ranges_kernel<<<blocks_of(ns + 1u), 256, 0, st>>>(S, m);
    if (m) {
        bgzf_walk_scan_kernel<true><<<n_tiles, kWalkThreads, 0, st>>>(S, C);
        bgzf_walk_parse_kernel<<<blocks_of(m), 256, 0, st>>>(S, C);
        for (uint32_t d = 1; d < levels; d++) bgzf_walk_jump_kernel<<<blocks_of(m), 256, 0, st>>>(C, d);
        for (uint32_t d = levels; d-- > 0;) bgzf_walk_mark_kernel<<<blocks_of(m), 256, 0, st>>>(C, d);
    }
    bgzf_walk_values_kernel<<<blocks_of(m + 1u), 256, 0, st>>>(S, C);
    HIPCHK(hipGetLastError());
    uint32_t* flag = reinterpret_cast<uint32_t*>(S.base + 1);
    HIPCHK(launch_bgzf_scan(C.vcnt, m + 1u, 0, ~0u, C.rank, S.base + 2, flag, st));
    HIPCHK(launch_bgzf_scan(C.visz, m + 1u, 0, ~0u, C.usum, S.base + 3, flag, st));
    if (m) bgzf_walk_emit_kernel<<<blocks_of(m), 256, 0, st>>>(S, C);
    bgzf_walk_resolve_kernel<<<blocks_of(ns), 256, 0, st>>>(S, C);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h, S.res, sizeof(BgzfSpanResult) * (size_t)ns, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const BgzfSpanResult* hr = reinterpret_cast<const BgzfSpanResult*>(h);
    out->res.assign(hr, hr + ns);
    out->d_moff = C.moff; out->d_misize = C.misize;
    out->slots = hr[ns - 1].first + hr[ns - 1].count;
    out->candidates = m;
    return ZWZ_OK;
}

}  // namespace zwz
