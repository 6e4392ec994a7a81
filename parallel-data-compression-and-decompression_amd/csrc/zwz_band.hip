// zwz_band.hip -- match records of chain-heavy chunks (text: four positions in five have a chain predecessor) without a
// chain walk.  Replaces, for those chunks, what lz_match's walk did with two dependent LDS gathers per candidate
// (consumer()'s longest_match, compression.cpp:119-131); the arithmetic and its proof of equivalence are csrc/lz_band.h.
//
//   lz_dense_list  one wave / chunk     a sample of the chunk's trigrams says "chain-heavy" or not -> two lists
//   lz_sort        one WG / chunk       positions sorted by (hash bucket, position): histogram, scan, and a ranking pass by
//                                       ONE wave -- ds_add_rtn serves same-address lanes in lane order, the property lz_links
//                                       already stands on -- whose results go out as (bucket << 16 | position) words
//   lz_match_band  one WG / chunk       the chunk's bytes in LDS; the sorted array streams through in tiles; per tile:
//                                       eight comparison bytes beside every entry, candidates per entry, then the banded
//                                       first pass (lane = entry, step k = "the entry k places in front": consecutive
//                                       lanes read consecutive LDS words -- no gather, no conflict) and the sharers' pass
// Records and has128 bits come out exactly as lz_match writes them; lz_parse does not know the difference.
#include <hip/hip_runtime.h>

#include "lz_band.h"
#include "zwz_kernels.h"
#include "zwz_device.h"

#ifndef ZWZ_BAND_EXP
#define ZWZ_BAND_EXP 0     // timing experiments only (tools/gpu.sh times band ... <bits>; the records are then not zlib's): 1 = no second pass, 2 = no band loop, 4 = no record stores
#endif

// (ZWZ_BAND_EXP & 16: thread 0 of every workgroup adds the cycles it spent per phase, >> 8, to tickets[16 + phase]; launch_deflate
// prints them when ZWZ_BAND_TIMES is set)
#if ZWZ_BAND_EXP & 16
#define ZWZ_STAMP(ph) do { if (tid == 0) { const uint64_t now_ = __builtin_amdgcn_s_memtime(); atomicAdd(&tickets[16 + (ph)], (uint32_t)((now_ - stamp_) >> 8)); stamp_ = now_; } } while (0)
#else
#define ZWZ_STAMP(ph) do { } while (0)
#endif

namespace zwz {

// ------------------------------------------------------------------------------------------------
// lz_dense_list: a wave per chunk hashes the chunk's first kDenseSample trigrams into two 32 Ki-bit sets (LDS) -- bucket taken, bucket
// taken twice -- and counts the ones that are at least the second resp. the third of their bucket (zwz_kernels.h: sample_is_dense).
// Chain-heavy chunks get kDenseMark in link_stat[], the others 0 (for lz_links to count in); lz_lists turns the marks into the two lists.
constexpr uint32_t kDenseThreads = 256;
__global__ __launch_bounds__(kDenseThreads) void lz_dense_list_kernel(const uint8_t* __restrict__ in, const uint64_t* __restrict__ in_off,
                                                                      const uint32_t* __restrict__ in_len, uint32_t n, uint32_t* __restrict__ link_stat,
                                                                      uint32_t force /* 2: every chunk is chain-heavy */) {
    __shared__ uint32_t s_set[kDenseThreads / 64][2048];
    const uint32_t wave = threadIdx.x >> 6, lane = lane_id();
    uint32_t* set = s_set[wave];
    // persistent: a wave takes chunks wave-id, + all waves, ... (a workgroup per four chunks spent more time being dispatched than working)
    for (uint32_t c = blockIdx.x * (kDenseThreads / 64u) + wave; c < n; c += gridDim.x * (kDenseThreads / 64u)) {
        const uint32_t L = in_len[c];
        bool dense = force == 2u && L != 0u;
        if (!dense && L >= kMinMatch) {
            for (uint32_t i = lane; i < 2048u; i += 64u) set[i] = 0;
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            const uint32_t* d32 = reinterpret_cast<const uint32_t*>(in + in_off[c]);       // 16-byte aligned; readable to L rounded up to 16
            const uint32_t sampled = min(L - (kMinMatch - 1u), kDenseSample), nd = ((L + 15u) & ~15u) >> 2;
            uint32_t repeats = 0, thirds = 0;
            static_assert(kDenseSample == 2048, "eight trips of 256 positions, their loads asked for together");
            uint32_t w0[8], w1[8];                                                      // four positions a lane a trip: a dword and its successor
#pragma unroll
            for (uint32_t t = 0; t < 8; t++) {
                const uint32_t i = 64u * t + lane;
                w0[t] = 256u * t < sampled && i < nd ? d32[i] : 0u; w1[t] = 256u * t < sampled && i + 1u < nd ? d32[i + 1u] : 0u;
            }
#pragma unroll
            for (uint32_t t = 0; t < 8; t++) {
                if (256u * t >= sampled) break;
#pragma unroll
                for (uint32_t j = 0; j < 4; j++) {
                    const uint32_t x = j ? __builtin_amdgcn_alignbyte(w1[t], w0[t], j) : w0[t];
                    const uint32_t h = hash3(x & 0xffu, (x >> 8) & 0xffu, (x >> 16) & 0xffu);
                    const bool live = 256u * t + 4u * lane + j < sampled;
                    uint32_t old = 0, old2 = 0;
                    if (live) old = atomicOr(&set[h >> 5], 1u << (h & 31u));            // (same-word lanes are served one after the other: each sees the earlier ones' bits)
                    const bool again = live && ((old >> (h & 31u)) & 1u);
                    if (again) old2 = atomicOr(&set[1024u + (h >> 5)], 1u << (h & 31u));
                    repeats += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(again));
                    thirds += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(again && ((old2 >> (h & 31u)) & 1u)));
                }
            }
            dense = sample_is_dense(repeats, thirds, sampled, L);
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        }
        if (lane == 0) link_stat[c] = dense ? kDenseMark : 0u;
    }
}

// The two lists, each in chunk order (one workgroup; appended by atomics their order was arbitrary, and lz_links' workgroups,
// which take list entries w, w + G, ..., ended up with uneven shares of config 2's full and 4-byte chunks).
__global__ __launch_bounds__(1024) void lz_lists_kernel(const uint32_t* __restrict__ in_len, const uint32_t* __restrict__ link_stat, uint32_t n,
                                                        uint32_t* __restrict__ dense_list, uint32_t* __restrict__ sparse_list, uint32_t* __restrict__ tickets) {
    __shared__ uint32_t s_d[16], s_s[16];
    const uint32_t tid = threadIdx.x, lane = lane_id(), wave = tid >> 6;
    uint32_t nd = 0, ns = 0;
    for (uint32_t c0 = 0; c0 < n; c0 += 1024u) {
        const uint32_t c = c0 + tid;
        const bool live = c < n && in_len[c] != 0u, dense = live && link_stat[c] == kDenseMark, sparse = live && !dense;
        const uint64_t md = __builtin_amdgcn_ballot_w64(dense), ms = __builtin_amdgcn_ballot_w64(sparse);
        if (lane == 0) { s_d[wave] = (uint32_t)__popcll(md); s_s[wave] = (uint32_t)__popcll(ms); }
        __syncthreads();
        uint32_t bd = nd, bs = ns, td = 0, ts = 0;
        for (uint32_t w = 0; w < 16u; w++) { bd += w < wave ? s_d[w] : 0u; bs += w < wave ? s_s[w] : 0u; td += s_d[w]; ts += s_s[w]; }
        if (dense) dense_list[bd + rank_in(md)] = c;
        if (sparse) sparse_list[bs + rank_in(ms)] = c;
        nd += td; ns += ts;
        __syncthreads();
    }
    if (tid == 0) { tickets[kTicketDenseCount] = nd; tickets[kTicketSparseCount] = ns; }
}

// ------------------------------------------------------------------------------------------------
// lz_sort.  The table holds two 16-bit counters a dword (bucket h in half h & 1 of dword h >> 1): 64 KiB, two workgroups a CU.
// A counter never carries into its neighbour: it ends at bucket start + bucket size <= 65 533.
// returning adds the ranking wave keeps in flight (a trip's worth): the step is the LDS's LATENCY for a returning atomic divided by what is in flight, and the
// kernel's two workgroups a CU leave a wave 256 registers -- 4: 7.81 ms for the links stage on text, 8 (round 3): 7.33, 16: 7.00, 24: 6.93
#ifndef ZWZ_SORT_DEPTH
#define ZWZ_SORT_DEPTH 16
#endif
constexpr uint32_t kSortDepth = ZWZ_SORT_DEPTH;
__global__ __launch_bounds__(kSortThreads) void lz_sort_kernel(const uint8_t* __restrict__ in, const uint64_t* __restrict__ in_off,
                                                               const uint32_t* __restrict__ in_len, const uint32_t* __restrict__ list,
                                                               uint32_t* __restrict__ tickets, uint32_t* __restrict__ sorted,
                                                               uint16_t* __restrict__ hbuf /* the chunks' dead link arrays */,
                                                               uint32_t* __restrict__ scratch /* the chunks' entries space (lz_lazy's bucket ends), or null */) {
    __shared__ __attribute__((aligned(16))) uint32_t tab[16384];
    __shared__ uint32_t s_wsum[kSortThreads / 64];
    __shared__ uint32_t s_chunk;
    const uint32_t tid = threadIdx.x, lane = lane_id(), wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t n_list = tickets[kTicketDenseCount];
    for (;;) {
        __syncthreads();                                           // (s_chunk and the table are free again)
        if (tid == 0) s_chunk = atomicAdd(&tickets[kTicketSortNext], 1u);
        __syncthreads();
        const uint32_t t = s_chunk;
        if (t >= n_list) break;
        const uint32_t chunk = list[t];
        const uint32_t L = in_len[chunk];
        const uint32_t n = L >= kMinMatch ? L - (kMinMatch - 1u) : 0u;     // positions with a trigram
        if (n == 0) continue;
        const uint32_t* d32 = reinterpret_cast<const uint32_t*>(in + in_off[chunk]);   // 16-byte aligned; readable to L rounded up to 16
        const uint32_t nd = ((L + 15u) & ~15u) >> 2;
        uint16_t* hb = hbuf + (size_t)chunk * kLinkStride;
        uint16_t* out = reinterpret_cast<uint16_t*>(sorted + (size_t)chunk * kSortedStride);   // dest[p]: p's index in (bucket, position) order
        {
            uint4* t4 = reinterpret_cast<uint4*>(tab);
            for (uint32_t i = tid; i < 4096u; i += kSortThreads) t4[i] = make_uint4(0, 0, 0, 0);
        }
        __syncthreads();
        // histogram: a thread takes sixteen positions a trip (a 16-byte vector and the dword behind it), eight trips' loads in flight
        // together (one at a time this loop was sixty-four HBM round trips: most of the kernel); the hashes go out to hbuf for the ranking
        {
            const uint4* d4 = reinterpret_cast<const uint4*>(d32);
            const uint32_t nv = nd >> 2;                                        // 16-byte vectors of the slot
#pragma unroll 1
            for (uint32_t i0 = tid; 16u * i0 < n; i0 += 8u * kSortThreads) {
                uint4 v[8]; uint32_t nx[8];
#pragma unroll
                for (uint32_t r = 0; r < 8; r++) {
                    const uint32_t i = i0 + r * kSortThreads;
                    v[r] = i < nv ? d4[i] : make_uint4(0, 0, 0, 0);
                    nx[r] = i + 1u < nv ? d32[4u * i + 4u] : 0u;
                }
#pragma unroll
                for (uint32_t r = 0; r < 8; r++) {
                    const uint32_t i = i0 + r * kSortThreads;
                    if (16u * i >= n) break;
                    const uint32_t w[5] = {v[r].x, v[r].y, v[r].z, v[r].w, nx[r]};
                    uint32_t h[16];
#pragma unroll
                    for (uint32_t j = 0; j < 16; j++) {
                        const uint32_t x = (j & 3u) ? __builtin_amdgcn_alignbyte(w[(j >> 2) + 1u], w[j >> 2], j & 3u) : w[j >> 2];
                        h[j] = hash3(x & 0xffu, (x >> 8) & 0xffu, (x >> 16) & 0xffu);
                        if (16u * i + j < n) atomicAdd(&tab[h[j] >> 1], (h[j] & 1u) ? 0x10000u : 1u);
                    }
                    // (what goes out is the counter's place as the ranking wave wants it: byte offset of the dword | which half -- a lone
                    // wave pays ~7 cycles an instruction, and this is done here by four)
#pragma unroll
                    for (uint32_t j = 0; j < 16; j++) h[j] = (h[j] >> 1) << 2 | (h[j] & 1u);
                    uint4* hb4 = reinterpret_cast<uint4*>(hb + 16u * i);
                    hb4[0] = make_uint4(h[0] | h[1] << 16, h[2] | h[3] << 16, h[4] | h[5] << 16, h[6] | h[7] << 16);
                    hb4[1] = make_uint4(h[8] | h[9] << 16, h[10] | h[11] << 16, h[12] | h[13] << 16, h[14] | h[15] << 16);
                }
            }
        }
        __syncthreads();
        // exclusive scan of the 32768 counters, in place: a wave owns 4096 dwords, 64 rows of 64
        {
            const uint32_t w_base = wave * 4096u;
            uint32_t tot = 0;
            for (uint32_t r = 0; r < 64u; r++) { const uint32_t v = tab[w_base + r * 64u + lane]; tot += (v & 0xffffu) + (v >> 16); }
            tot = wave_scan_incl(tot);
            if (lane == 63) s_wsum[wave] = tot;
            __syncthreads();
            uint32_t carry = 0;
            for (uint32_t i = 0; i < kSortThreads / 64u; i++) carry += i < wave ? s_wsum[i] : 0u;
            for (uint32_t r = 0; r < 64u; r++) {
                const uint32_t idx = w_base + r * 64u + lane;
                const uint32_t v = tab[idx], lo = v & 0xffffu, hi = v >> 16, own = lo + hi;
                const uint32_t incl = wave_scan_incl(own), ex = carry + incl - own;
                tab[idx] = ex | (ex + lo) << 16;
                carry += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
            }
        }
        __syncthreads();
        // ranking: positions in order, 64 a step, by ONE wave: the returning add hands same-bucket lanes their slots in lane order
        // (= position order), steps follow one another in program order.
        // (Round 5, measured and dropped: ALL FOUR waves ranking, each the positions whose bucket lies in its quarter of the table -- buckets do not
        // care about each other, so it is exact (all oracle tests passed) -- on the idea that the step is latency over what is in flight: links stage
        // 7.1 -> 10.4 ms on text.  Every wave then loads all the hashes, and the per-lane guards around add and store are the exec-mask bookkeeping
        // the unguarded trips below got rid of.  Also measured and dropped: NO histogram -- the ranking's returning add counts from zero and hands a
        // position its rank inside its bucket, the scan comes afterwards, and a last pass of plain LDS reads adds the bucket's start to every rank
        // (on the idea that the LDS's atomics bound the kernel and the histogram is a third of them): exact, 7.1 -> 8.5 ms.  The histogram's adds
        // overlap the other workgroup's ranking; the last pass's two global round trips a position vector do not.)
        if (wave == 0) {
            // Whole trips of eight steps run without a single test (every lane has a position: guarded per lane, the loop was
            // mostly exec-mask bookkeeping); the next trip's hashes are on their way while this one ranks.
            constexpr uint32_t K = kSortDepth;                                      // steps a trip: that many returning adds in flight
            const uint32_t full = n / (64u * K);                                   // trips of 64 K positions
            // (running pointers, so that a trip's eight loads and eight stores are one address and constant offsets; hb holds byte
            // offset | half, see the histogram: per step the wave is left with and + two shifts + the add, and a shift + the store)
            auto bump = [&](uint32_t w) { return atomicAdd(reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(tab) + (w & 0xfffcu)), 1u << ((w & 1u) << 4)); };
            const uint16_t* hin = hb + lane;
            uint16_t* o = out + lane;
            uint32_t hv[K];
            auto ask = [&](uint32_t* h8) {
#pragma unroll
                for (uint32_t j = 0; j < K; j++) h8[j] = hin[j * 64u];
                hin += 64u * K;
            };
            if (full) ask(hv);
            uint32_t hp[K], op[K];                                              // the previous trip's entries and what its adds returned
            for (uint32_t t = 0; t < full; t++) {
                uint32_t hn[K], old[K];
                if (t + 1u < full) ask(hn);
#pragma unroll
                for (uint32_t j = 0; j < K; j++) old[j] = bump(hv[j]);
                // (the previous trip's results are written out while this trip's adds are on their way through the LDS)
                if (t) {
#pragma unroll
                    for (uint32_t j = 0; j < K; j++) o[j * 64u] = (uint16_t)(op[j] >> ((hp[j] & 1u) << 4));
                    o += 64u * K;
                }
#pragma unroll
                for (uint32_t j = 0; j < K; j++) { hp[j] = hv[j]; op[j] = old[j]; hv[j] = hn[j]; }
            }
            if (full) {
#pragma unroll
                for (uint32_t j = 0; j < K; j++) o[j * 64u] = (uint16_t)(op[j] >> ((hp[j] & 1u) << 4));
            }
            for (uint32_t p = full * 64u * K + lane; p - lane < n; p += 64u) {  // the ragged end, a step at a time
                if (p < n) {
                    const uint32_t w = hb[p];
                    out[p] = (uint16_t)(bump(w) >> ((w & 1u) << 4));
                }
            }
        }
        // the table now holds every bucket's END in the sorted array (a counter ran from its bucket's start): lz_lazy's bucket bounds
        if (scratch) {
            __syncthreads();
            uint4* o4 = reinterpret_cast<uint4*>(scratch + (size_t)chunk * kLazyScratchWords + kLazyBendOff);
            const uint4* t4 = reinterpret_cast<const uint4*>(tab);
            for (uint32_t i = tid; i < 4096u; i += kSortThreads) o4[i] = t4[i];
        }
    }
}

// ------------------------------------------------------------------------------------------------
// lz_place: dest[p] -> the sorted array itself, position of sorted index u at spos[u].  The inverse of a permutation is a
// scatter; done through HBM it costs a 64-line store per wave (lz_sort spent 5x its time on it), so the whole chunk's
// array is scattered in LDS (128 KiB of 16-bit positions) and leaves as whole lines.
__global__ __launch_bounds__(kPlaceThreads) void lz_place_kernel(const uint32_t* __restrict__ in_len, const uint32_t* __restrict__ list,
                                                                 uint32_t* __restrict__ tickets, uint32_t* __restrict__ sorted) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint16_t* stage = reinterpret_cast<uint16_t*>(smem);
    __shared__ uint32_t s_chunk;
    const uint32_t tid = threadIdx.x;
    const uint32_t n_list = tickets[kTicketDenseCount];
    for (;;) {
        __syncthreads();
        if (tid == 0) s_chunk = atomicAdd(&tickets[kTicketPlaceNext], 1u);
        __syncthreads();
        const uint32_t t = s_chunk;
        if (t >= n_list) break;
        const uint32_t chunk = list[t];
        const uint32_t L = in_len[chunk];
        const uint32_t n = L >= kMinMatch ? L - (kMinMatch - 1u) : 0u;
        const uint4* d4 = reinterpret_cast<const uint4*>(sorted + (size_t)chunk * kSortedStride);            // dest[p], 16 bits each
        uint4* o4 = reinterpret_cast<uint4*>(reinterpret_cast<uint16_t*>(sorted + (size_t)chunk * kSortedStride) + 65536);   // spos[u]
        uint4 d[8];
#pragma unroll
        for (uint32_t r = 0; r < 8; r++) if (8u * (tid + kPlaceThreads * r) < n) d[r] = d4[tid + kPlaceThreads * r];
#pragma unroll
        for (uint32_t r = 0; r < 8; r++) {
            const uint32_t p0 = 8u * (tid + kPlaceThreads * r);
            const uint32_t dw[4] = {d[r].x, d[r].y, d[r].z, d[r].w};
#pragma unroll
            for (uint32_t j = 0; j < 8; j++) if (p0 + j < n) stage[(dw[j >> 1] >> (16u * (j & 1u))) & 0xffffu] = (uint16_t)(p0 + j);
        }
        __syncthreads();
        for (uint32_t i = tid; 8u * i < n; i += kPlaceThreads) o4[i] = reinterpret_cast<const uint4*>(stage)[i];
    }
}

// ------------------------------------------------------------------------------------------------
// lz_match_band.  Per chunk: bytes -> LDS, dest[] -> registers (64 positions a thread, kept for all tiles).  Per tile of
// kBandTile sorted entries (+ the 128 in front of them):
//   scatter   every thread looks at its 64 dests; the ones inside the tile drop (bucket << 16 | position) into their slot
//   build     the 8-byte comparison word of every entry; "pure" (one trigram per bucket, so the word starts behind the trigram)
//             unless two neighbours of one bucket differ in their trigrams -- then the words are rebuilt from the trigram on
//   count     candidates per entry (binary search over the monotone band_valid, asked as a range test, six entries a thread in flight together);
//             the chunk's last positions are finished here, byte by byte
//   order     runs of eight consecutive entries, sorted by their greatest count: a wave's 64 lanes are eight runs of similar
//             length (a trip lasts as long as its longest band: 0.66 of the lanes busy in array order, 0.89 this way), and
//             each run still reads 64 consecutive LDS bytes per step
//   pass 1    the banded keys, two candidates a register (see the loop)
//   pass 2    the flagged entries, compacted into full waves, walk their sharers (csrc/lz_band.h band_deep)
constexpr uint32_t kBandArr = kBandTile + kBand;                    // a tile's arrays: 128 halo entries, then the tile's own
constexpr uint32_t kBandDataBytes = 65536 + 64;                     // the chunk + slack for comparisons that run past its end
constexpr uint32_t kBandOffS = kBandDataBytes, kBandOffE = kBandOffS + kBandArr * 4, kBandOffCk = kBandOffE + kBandArr * 8,
                   kBandOffHas = kBandOffCk + kBandTile * 2;
static_assert(kBandOffHas + 8192 == kBandLdsBytes, "lz_match_band LDS layout");
static_assert(kBandTile % 64 == 0 && kBandOffE % 8 == 0 && kBandOffS % 16 == 0 && kBandOffCk % 16 == 0, "lz_match_band LDS alignment");
// entries a run of the order phase -- the first pass in cycle units per 10 000 text chunks: 8: 13 604 k, order phase 562 k;
// 4: 13 583 k, order 935 k (1 504 runs a tile are two a thread, and twice the atomics) and 12 bytes of scratch in the plain build -- the lanes are busier
// (0.87 against 0.85, tools/exp/band_pass1_replay.py) but a run's 32 consecutive bytes a step cost in LDS conflicts what that gives; 2: s_order does not fit
#ifndef ZWZ_BAND_RUN
#define ZWZ_BAND_RUN 8
#endif
constexpr uint32_t kBandRun = ZWZ_BAND_RUN;                         // consecutive entries a run of the order phase
static_assert(kBandRun == 8 || kBandRun == 4 || kBandRun == 2, "lz_match_band: a run is 8, 4 or 2 entries");
constexpr uint32_t kBandRuns = kBandTile / kBandRun, kBandRunsPer = (kBandRuns + kBandThreads - 1) / kBandThreads;
// s_order holds a run's index in 16 bits beside 1 072 bytes of other static arrays: runs of 2 (6 016 bytes) do not fit the CU's 160 KB with a tile
// of 6 016 entries, and nothing of the tile's arrays is dead during the first pass
static_assert(kBandLdsBytes + 1072u + 2u * kBandRuns <= 160u * 1024u, "lz_match_band: s_order does not fit beside the tile");

#ifndef ZWZ_BAND_WAVES
#define ZWZ_BAND_WAVES 4
#endif
// hops a run-ahead step of the second pass may take before the wave meets for a compare again, 0 = as many as it takes -- the pass in cycle units per
// 10 000 text chunks: 4: 4.41 M, 6: 4.20 M, 8: 4.29 M, 12: 4.53 M, 16: 4.87 M, unbounded: 8.72 M; the batched walk it replaces: 6.02 M
#ifndef ZWZ_BAND_P2_RUN
#define ZWZ_BAND_P2_RUN 6
#endif
constexpr uint32_t kP2Run = ZWZ_BAND_P2_RUN;
// Lv (zwz_common.h: LzLevel<N>) = the compression level, a template argument and not a value: the unrolling and the register budget below were tuned
// with the constants in place, and LzLevel<6> gives the kernel it always was.  What a level changes: the count stops at its max_chain (the halo stays 128
// entries wide), the short chain's snapshot is taken behind snap_chain candidates, the second pass stops at its nice length.
template <class Lv>
__global__ __launch_bounds__(kBandThreads, ZWZ_BAND_WAVES) void lz_match_band_kernel(const uint8_t* __restrict__ in, const uint64_t* __restrict__ in_off,
                                                                    const uint32_t* __restrict__ in_len, const uint32_t* __restrict__ list,
                                                                    uint32_t* __restrict__ tickets, const uint32_t* __restrict__ sorted,
                                                                    uint2* __restrict__ entries, uint64_t* __restrict__ has128) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint8_t* sdata = smem;
    uint32_t* S = reinterpret_cast<uint32_t*>(smem + kBandOffS);
    uint2* E = reinterpret_cast<uint2*>(smem + kBandOffE);
    uint16_t* ck = reinterpret_cast<uint16_t*>(smem + kBandOffCk);       // per own entry: candidates | k of the nearest sharer << 8
    uint32_t* hasb = reinterpret_cast<uint32_t*>(smem + kBandOffHas);    // has128 bits of the whole chunk
    uint16_t* flist = reinterpret_cast<uint16_t*>(E + kBand);            // pass 2's work list: over the own entries' words, dead by then
    __shared__ uint32_t s_chunk, s_grp[2], s_nflag, s_nrun;
    __shared__ uint16_t s_halo_link[kBand];                              // the links of a tile's last 128 entries, for the next tile's halo
    __shared__ uint32_t s_bin[132];
    __shared__ uint16_t s_order[kBandRuns];
#if ZWZ_BAND_EXP & 16
    __shared__ uint64_t s_p2_start;                                      // second pass: when it began (thread 0's clock)
#endif
    const uint32_t tid = threadIdx.x, lane = lane_id(), wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t n_list = tickets[kTicketDenseCount];
    for (uint32_t i = tid; i < 2048u; i += kBandThreads) hasb[i] = 0;
#if ZWZ_BAND_EXP & 16
    uint64_t stamp_ = __builtin_amdgcn_s_memtime();
#endif
    for (;;) {
        __syncthreads();
        ZWZ_STAMP(7);
        if (tid == 0) s_chunk = atomicAdd(&tickets[kTicketBandNext], 1u);
        __syncthreads();
        const uint32_t tk = s_chunk;
        if (tk >= n_list) break;
        const uint32_t chunk = list[tk];
        const uint32_t L = in_len[chunk];
        const uint32_t n = L >= kMinMatch ? L - (kMinMatch - 1u) : 0u;
        uint2* ent = entries + (size_t)chunk * kEntryStride;
        uint64_t* hm = has128 + (size_t)chunk * kMaskWords;
        const uint4* spos4 = reinterpret_cast<const uint4*>(reinterpret_cast<const uint16_t*>(sorted + (size_t)chunk * kSortedStride) + 65536);   // lz_place: position of sorted index u
        copy_vec16(reinterpret_cast<uint4*>(sdata), reinterpret_cast<const uint4*>(in + in_off[chunk]), (L + 15u) >> 4);
        ZWZ_STAMP(0);
        bool prev_pure = false;
        // a tile's positions (eight a thread) are asked for one tile ahead: an HBM round trip per tile otherwise stands in the open
        auto spos_of = [&](uint32_t a_) { return 8u * tid < kBandArr && 8u * tid + a_ >= kBand && 8u * tid + a_ - kBand < n ? spos4[(8u * tid + a_ - kBand) >> 3] : make_uint4(0, 0, 0, 0); };
        static_assert(kBandArr <= 8u * kBandThreads, "a thread holds eight of a tile's positions");
        uint4 v_next = spos_of(0u);
        for (uint32_t a = 0; a < n; a += kBandTile) {
            const uint32_t b = min(a + kBandTile, n), m = b - a + kBand;      // array index i <-> sorted index a - 128 + i
            if (a < kBand) for (uint32_t i = tid; i < kBand - a; i += kBandThreads) S[i] = kBandHaloWord;   // (a = 0: the first tile)
            if (tid == 0) { s_grp[0] = 0; s_grp[1] = 0; s_nflag = 0; s_nrun = 0; }
            if (tid < 132u) s_bin[tid] = 0;
            __syncthreads();                                                  // (also: the chunk's bytes are in place)
            // ---- the tile's entries and the 128 in front of them: positions from lz_place's array; bucket AND the eight comparison bytes
            // out of ONE read of the four dwords that hold bytes p .. p + 10 (round 3 read the trigram here and then, in a second phase,
            // the trigram again, the previous entry's, and two unaligned words behind it: ten dword gathers an entry where four do, and
            // both phases were the LDS pipe's -- 12 % of the kernel)
            bool mixed = false;
            {
                const uint32_t pw[4] = {v_next.x, v_next.y, v_next.z, v_next.w};
                if (8u * tid + a >= kBand) {                                    // (before the array's start: halo words, set above)
                    uint32_t prev_w = 0, prev_t = 0;
#pragma unroll
                    for (uint32_t j = 0; j < 8; j++) {
                        const uint32_t p = (pw[j >> 1] >> (16u * (j & 1u))) & 0xffffu;
                        const uint32_t* d = reinterpret_cast<const uint32_t*>(sdata) + (p >> 2);
                        const uint32_t w0 = d[0], w1 = d[1], w2 = d[2], w3 = d[3];           // bytes (p & ~3) .. + 15: p + 10 <= (p & ~3) + 13
                        const uint32_t x = __builtin_amdgcn_alignbyte(w1, w0, p & 3u) & 0xffffffu;
                        const uint32_t word = band_word(hash3(x & 0xffu, (x >> 8) & 0xffu, x >> 16), p);
                        const bool up = (p & 3u) != 0u;                                       // bytes p + 3 .. start in w1 (p & 3 >= 1) or in w0
                        const uint32_t ea = up ? w1 : w0, eb = up ? w2 : w1, ec = up ? w3 : w2, sh = (p + 3u) & 3u;
                        if (8u * tid + j < m) {
                            S[8u * tid + j] = word;
                            E[8u * tid + j] = make_uint2(__builtin_amdgcn_alignbyte(eb, ea, sh), __builtin_amdgcn_alignbyte(ec, eb, sh));
                            if (j) mixed |= band_hash(word) == band_hash(prev_w) && x != prev_t;      // one bucket, two trigrams (j = 0: below)
                        }
                        prev_w = word; prev_t = x;
                    }
                }
                v_next = spos_of(a + kBandTile);                                // (a and 128 are multiples of 8)
            }
            __syncthreads();
            ZWZ_STAMP(1);
            // ---- "pure" (every bucket of the tile holds one trigram only: the words start behind the trigram) unless two neighbours of one
            // bucket differ in their trigrams -- then the words are rebuilt from the trigram on.  Neighbours inside a thread's eight were
            // compared above; here every thread looks across the seam in front of its first entry.
            bool pure;
            {
                const uint32_t i = 8u * tid;
                if (i && i < m) {
                    const uint32_t w = S[i], wp = S[i - 1u];
                    const uint32_t tg = load_u32(sdata, band_pos(w)), tp = load_u32(sdata, band_pos(wp));
                    mixed |= w != kBandHaloWord && wp != kBandHaloWord && band_hash(w) == band_hash(wp) && ((tg ^ tp) & 0xffffffu) != 0u;
                }
                pure = !__syncthreads_or((int)mixed);
                if (!pure) {
                    for (uint32_t i2 = tid; i2 < m; i2 += kBandThreads) { const uint32_t q = band_pos(S[i2]); E[i2] = make_uint2(load_u32(sdata, q), load_u32(sdata, q + 4u)); }
                }
            }
            const uint32_t off = pure ? 3u : 0u, deep = pure ? 11u : 8u;
            auto Sf = [&](uint32_t i) { return S[i]; };
            ZWZ_STAMP(2);
            // (Tried in round 4 and dropped: the bucket's start from a scan of head flags -- a max-scan over the wave plus the last head of the
            // two blocks in front -- and ONE gather to check that the farthest candidate so found is in reach, the binary search only for
            // the entries that fail the check.  On the text corpus nearly every wave holds such an entry (a rare trigram's candidates lie
            // further back than MAX_DIST for every position in the chunk's second half), so the search ran anyway, behind the scan and a
            // barrier: this phase 3.93 M -> 5.45 M cycles >> 8 per 10 000 chunks, 6.56 M with the fallback's searches advancing together.)
            // (Round 5, measured and dropped: a thread takes six CONSECUTIVE entries, searches the first and derives each next count from the one before
            // -- an entry behind one of its own bucket has that one as a candidate plus those of its candidates still in reach, so its count is
            // the previous + 1 less what fell out at the far end: one probe there and one more per entry that did, ~23 probes a thread where the
            // searches make 48.  Exact (all oracle tests); this phase 3.67 M -> 4.77 M, text match stage 68.5 -> 70.7 ms: the 23 probes hang on one
            // another, the six searches run side by side -- the phase is the LDS round trip times the length of the chain, not its probes.)
            // ---- count (thread <-> entries kBand + tid + 1024 j: the searches of a thread's entries advance together)
            {
                constexpr uint32_t kOwnPer = (kBandTile + kBandThreads - 1) / kBandThreads;
                // the greatest count looked for is the level's max_chain, not the band's width: a count beyond it would let pass 1 fold candidates
                // zlib's chain never reaches (lz_band.h band_count caps the same way)
                constexpr uint32_t kCap = Lv::max_chain;
                static_assert(kCap <= kBand && (kCap & (kCap - 1u)) == 0u, "the count is a binary search over [0, max_chain] inside the halo");
                uint32_t own[kOwnPer], k[kOwnPer];
#pragma unroll
                for (uint32_t j = 0; j < kOwnPer; j++) { const uint32_t i = kBand + tid + kBandThreads * j; own[j] = i < m ? S[i] : kBandHaloWord; k[j] = 0; }
                // A probe is band_in_reach (csrc/lz_band.h, with the proof that it is band_valid): subtract, compare, and the search's place moves
                // under the mask -- four vector instructions where band_valid and the `t <= kCap` guard took thirteen and a branch.  The place is a
                // pointer kCap words in front of the entry the search stands on, so a step's word lies at a constant offset behind it.  An entry
                // that has all kCap candidates (the first step) goes on with an empty range: nothing passes, its place stays.
                static_assert(kBandOffS >= 4u * kCap, "the running pointer stays inside the LDS block");
                uint32_t lo[kOwnPer], span[kOwnPer];
                const uint32_t* at[kOwnPer];
                bool open = false;                                              // inside a long bucket every entry has all max_chain candidates: nothing to search
#pragma unroll
                for (uint32_t j = 0; j < kOwnPer; j++) { lo[j] = band_lo(own[j]); span[j] = own[j] - lo[j]; at[j] = S + (kBand - kCap) + tid + kBandThreads * j; }
                {
                    uint32_t c[kOwnPer];
#pragma unroll
                    for (uint32_t j = 0; j < kOwnPer; j++) c[j] = at[j][0];
#pragma unroll
                    for (uint32_t j = 0; j < kOwnPer; j++) {
                        const bool all = c[j] - lo[j] < span[j];
                        k[j] = all ? kCap : 0u;
                        span[j] = all ? 0u : span[j];
                        open |= kBand + tid + kBandThreads * j < m && !all;
                    }
                }
                if (__builtin_amdgcn_ballot_w64(open) != 0) {
#pragma unroll
                    for (uint32_t step = kCap / 2u; step >= 1u; step >>= 1) {
                        uint32_t c[kOwnPer];
#pragma unroll
                        for (uint32_t j = 0; j < kOwnPer; j++) c[j] = at[j][kCap - step];
#pragma unroll
                        for (uint32_t j = 0; j < kOwnPer; j++) at[j] -= c[j] - lo[j] < span[j] ? step : 0u;
                    }
#pragma unroll
                    for (uint32_t j = 0; j < kOwnPer; j++) k[j] += (uint32_t)(S + (kBand - kCap) + tid + kBandThreads * j - at[j]);
                }
#pragma unroll
                for (uint32_t j = 0; j < kOwnPer; j++) {
                    const uint32_t i = kBand + tid + kBandThreads * j;
                    if (i < m) {
                        if (k[j] == 0u && band_first_at_max_dist(own[j], S[i - 1u])) k[j] = 1u;
                        ck[i - kBand] = (uint16_t)k[j];
                    }
                }
            }
            __syncthreads();
            ZWZ_STAMP(3);
            // The halo's entries were the previous tile's last: their links (to sharers under THAT tile's word format) carry over
            // when the format is the same; else a walk that reaches the halo starts again the slow way (band_deep).
            const bool halo_links = a == 0u || prev_pure == pure;
            if (tid < kBand) reinterpret_cast<uint16_t*>(S)[2u * tid + 1u] = a != 0u && halo_links ? s_halo_link[tid] : (uint16_t)kBandNoLink;
            prev_pure = pure;
            // ---- order: counting sort of the runs by their greatest count, longest first (runs without candidates drop out)
            const uint32_t n_run = (b - a + kBandRun - 1u) / kBandRun;
            uint32_t run_key[kBandRunsPer];
#pragma unroll
            for (uint32_t t = 0; t < kBandRunsPer; t++) {
                const uint32_t r = tid + kBandThreads * t;
                run_key[t] = 0;
                if (r < n_run) {
                    uint32_t cw[4] = {0, 0, 0, 0};                              // (counts behind the tile's end are stale: masked below)
                    if constexpr (kBandRun == 8) { const uint4 c8 = *reinterpret_cast<const uint4*>(ck + 8u * r); cw[0] = c8.x; cw[1] = c8.y; cw[2] = c8.z; cw[3] = c8.w; }
                    else if constexpr (kBandRun == 4) { const uint2 c4 = *reinterpret_cast<const uint2*>(ck + 4u * r); cw[0] = c4.x; cw[1] = c4.y; }
                    else cw[0] = *reinterpret_cast<const uint32_t*>(ck + 2u * r);
#pragma unroll
                    for (uint32_t j = 0; j < kBandRun; j++) if (kBandRun * r + j < b - a) run_key[t] = max(run_key[t], (cw[j >> 1] >> (16u * (j & 1u))) & 0xffu);
                    if (run_key[t]) atomicAdd(&s_bin[128u - run_key[t]], 1u);
                }
            }
            __syncthreads();
            if (wave == 0) {                                                    // exclusive scan of the 128 bins
                const uint32_t v0 = s_bin[lane], v1 = s_bin[64u + lane];
                const uint32_t i0 = wave_scan_incl(v0), t0 = (uint32_t)__builtin_amdgcn_readlane((int)i0, 63);
                const uint32_t i1 = wave_scan_incl(v1);
                s_bin[lane] = i0 - v0; s_bin[64u + lane] = t0 + i1 - v1;
                if (lane == 63) s_nrun = t0 + i1;
            }
            __syncthreads();
#pragma unroll
            for (uint32_t t = 0; t < kBandRunsPer; t++) if (run_key[t]) s_order[atomicAdd(&s_bin[128u - run_key[t]], 1u)] = (uint16_t)(tid + kBandThreads * t);
            __syncthreads();
            ZWZ_STAMP(8);
            constexpr uint32_t kRunsWave = 64u / kBandRun;                      // runs a wave takes at a time
            const uint32_t n_act = s_nrun, n_grp = (n_act + kRunsWave - 1u) / kRunsWave;
            const uint32_t none = pure ? kBandKeyNonePure : kBandKeyNoneImpure;
            // ---- first pass
            for (;;) {
                uint32_t g = 0;
                if (lane == 0) g = atomicAdd(&s_grp[0], 1u);
                g = __builtin_amdgcn_readfirstlane(g);
                if (g >= n_grp) break;
                const uint32_t ri = kRunsWave * g + lane / kBandRun;
                const uint32_t i = kBand + kBandRun * (ri < n_act ? (uint32_t)s_order[ri] : 0u) + (lane & (kBandRun - 1u));
                const bool active = ri < n_act && i < m;
                const uint32_t w = S[i], p = band_pos(w);                       // (i < kBandArr whatever the lane)
                const uint32_t cntb = active ? (uint32_t)ck[i - kBand] : 0u;
                const uint2 own = E[i];
                // The band, eight candidates a trip, nearest first, two candidates an instruction: the keys are 12 bits, so a pair's live in the
                // 16-bit halves of one register (csrc/lz_band.h band_key_pair is the specification).  A pair costs thirteen vector instructions --
                // four XORs, four find-first-bits that write their halves themselves (SDWA: 0xffffffff of an all-equal word leaves as 0xffff and
                // stays in its half; no v_perm to join them), | 32 on the upper words' halves, packed minimum, mask, shift-or with the pair's two
                // 129 - k from a scalar register, packed running maximum -- 6.5 a candidate where the 32-bit form paid 8.5.  The two halves' maxima
                // meet once behind the loops; the short chain's snapshot stays packed until then as well (a select a trip).
                // Up to the smallest count among the lanes that have candidates nothing needs masking.  Beyond it a lane's mask of the length
                // field (0x78) comes from a register whose bytes say which of the trip's eight candidates the lane still has
                // (band_trip_mask: seven instructions a trip, a v_perm a pair -- 8.25 a candidate with the trip's address and snapshot select, where
                // compare + select + max made it 10.5; the unmasked trip is 55 instructions, 6.9 a candidate; with the pair's masks from two compares
                // and two selects instead, the pass was 13 840 k cycle units per 10 000 text chunks against 13 614 k, the 32-bit keys 16 374 k):
                // a candidate beyond the count leaves as the key of length 0, 129 - k alone.  No such key wins.  A lane that has a
                // beyond-count candidate k has cntb >= 1 and k >= 2 (lanes without candidates: below), so the key is <= 127, and the
                // lane's nearest candidate, k = 1, always valid, has a key >= 128 in the trip's or an earlier trip's maximum.  The maximum
                // is taken per half, and a half may be won by such a key, but the two halves' maximum is not: the k = 1 key is in the low
                // half from the first trip on, so behind every trip -- the snapshot's trip included -- the halves' maximum is the maximum
                // over the valid keys and the start value (pure: 0, below every key; impure: 0x2ff, which the length-0 keys are below as
                // well).  Lanes without any candidate start from a maximum nothing can beat and get `none` behind the loop.
                const uint32_t kmax = (ZWZ_BAND_EXP & 2) ? 0u : (uint32_t)__builtin_amdgcn_readlane((int)wave_scan_max_incl(cntb), 63);
                const uint32_t kmin = 128u - (uint32_t)__builtin_amdgcn_readlane((int)wave_scan_max_incl(cntb ? 128u - cntb : 0u), 63);   // (128 if nobody has any)
                uint32_t best, snap = none;
                const uint2* Ei = E + i;                                        // (i - k >= 0 for every lane: k <= 128 <= i)
                auto key2_of = [&](const uint2 ca, const uint2 cb, uint32_t tags, uint32_t mask) {
                    uint32_t t0, t1, m, key;
                    asm("v_ffbl_b32_sdwa %0, %1 dst_sel:WORD_0 dst_unused:UNUSED_PAD src0_sel:DWORD" : "=v"(t0) : "v"(own.x ^ ca.x));   // 0xffff for 0
                    asm("v_ffbl_b32_sdwa %0, %1 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:DWORD" : "+v"(t0) : "v"(own.x ^ cb.x));
                    asm("v_ffbl_b32_sdwa %0, %1 dst_sel:WORD_0 dst_unused:UNUSED_PAD src0_sel:DWORD" : "=v"(t1) : "v"(own.y ^ ca.y));
                    asm("v_ffbl_b32_sdwa %0, %1 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:DWORD" : "+v"(t1) : "v"(own.y ^ cb.y));
                    asm("v_pk_min_u16 %0, %1, %2" : "=v"(m) : "v"(t0), "v"(t1 | 0x00200020u));   // first differing bit of the 64, a half each
                    asm("v_lshl_or_b32 %0, %1, 5, %2" : "=v"(key) : "v"(m & mask), "s"(tags));
                    return key;
                };
                const uint32_t la = L - p;
                const bool tail = active && la < deep;                          // the word reaches past the data
                if (__builtin_amdgcn_ballot_w64(tail) == 0) {
                    uint32_t best2 = cntb ? none | none << 16 : 0xffffffffu, snap2 = none | none << 16;
                    auto both = [](uint32_t x) { return max(x & 0xffffu, x >> 16); };
                    uint32_t k0 = 0;
                    for (; k0 + 8u <= kmin; k0 += 8u) {
                        uint2 c[8];
#pragma unroll
                        for (uint32_t j = 0; j < 8; j++) c[j] = Ei[-(int)(k0 + j + 1u)];
                        const uint32_t tg = (128u - k0) * 0x10001u;             // candidate k0 + j + 1 in the low half, k0 + j + 2 in the high one
#pragma unroll
                        for (uint32_t j = 0; j < 8; j += 2) {
                            const uint32_t key = key2_of(c[j], c[j + 1], tg - (j * 0x10001u + 0x10000u), kBandPairLenMask);
                            asm("v_pk_max_u16 %0, %0, %1" : "+v"(best2) : "v"(key));
                        }
                        if (k0 + 8u == Lv::snap_chain) snap2 = best2;
                    }
                    for (; k0 < kmax; k0 += 8u) {
                        uint2 c[8];
#pragma unroll
                        for (uint32_t j = 0; j < 8; j++) c[j] = Ei[-(int)(k0 + j + 1u)];
                        const uint32_t tg = (128u - k0) * 0x10001u;
                        const uint64_t have = band_trip_mask(k0, cntb);
#pragma unroll
                        for (uint32_t j = 0; j < 8; j += 2) {
                            const uint32_t hw = (uint32_t)(have >> (j & 4u ? 32 : 0));
                            const uint32_t mask = __builtin_amdgcn_perm(hw, hw, j & 2u ? 0x0c030c02u : 0x0c010c00u);   // = band_pair_mask(have, j)
                            const uint32_t key = key2_of(c[j], c[j + 1], tg - (j * 0x10001u + 0x10000u), mask);
                            asm("v_pk_max_u16 %0, %0, %1" : "+v"(best2) : "v"(key));
                        }
                        if (k0 + 8u == Lv::snap_chain) snap2 = best2;
                    }
                    best = both(best2); snap = both(snap2);
                } else {                                                        // a handful of groups per chunk: the plain loop, XORs masked to the bytes that exist
                    const uint32_t nb = tail ? band_tail_bytes(pure, la) : 8u, m_lo = band_tail_mask(nb, 0), m_hi = band_tail_mask(nb, 1);
                    best = none;
                    for (uint32_t k = 1; k <= kmax; k++) {
                        const uint2 c = Ei[-(int)k];
                        const uint32_t key = band_key_masked(own.x, own.y, c.x, c.y, m_lo, m_hi, k);
                        best = max(best, k <= cntb ? key : 0u);
                        if (k == Lv::snap_chain) snap = best;
                    }
                }
                if (cntb == 0u) best = none;
                const uint32_t key32 = cntb > Lv::snap_chain ? snap : best;
                uint32_t e128 = 0, e32 = 0, k1 = 0;
                if (best != none) {
                    if (band_key_len(best) == 15u && !tail && !(ZWZ_BAND_EXP & 1)) k1 = band_key_k(best);
                    else e128 = band_record(best, pure, p, band_pos(S[i - band_key_k(best)]), la);
                }
                if (key32 != none && (tail || band_key_len(key32) != 15u)) e32 = band_record(key32, pure, p, band_pos(S[i - band_key_k(key32)]), la);
                if (active) {
                    if (k1) {
                        ck[i - kBand] = (uint16_t)(cntb | k1 << 8);
                        reinterpret_cast<uint16_t*>(S)[2u * i + 1u] = (uint16_t)(i - k1);   // the bucket field has done its work: now the link
                        if (k1 > Lv::snap_chain && !(ZWZ_BAND_EXP & 4)) reinterpret_cast<uint32_t*>(ent + p)[1] = e32;   // final; the second pass writes the rest
                        atomicOr(&hasb[p >> 5], 1u << (p & 31u));
                    } else {
                        reinterpret_cast<uint16_t*>(S)[2u * i + 1u] = (uint16_t)kBandNoLink;
                        if (e128) {
                            if (!(ZWZ_BAND_EXP & 4)) ent[p] = make_uint2(e128, e32); else asm volatile("" :: "v"(e128), "v"(e32), "v"(p));
                            atomicOr(&hasb[p >> 5], 1u << (p & 31u));
                        }
                    }
                }
            }
            // entries of runs that were left out (no candidates anywhere in the run) link nowhere either
            for (uint32_t i = kBand + tid; i < m; i += kBandThreads) if ((uint32_t)ck[i - kBand] == 0u) reinterpret_cast<uint16_t*>(S)[2u * i + 1u] = (uint16_t)kBandNoLink;
            __syncthreads();
            ZWZ_STAMP(4);
            // ---- second pass: the flagged entries, gathered into full waves, walk their sharers (csrc/lz_band.h, band_deep_probed).  An
            // entry's word holds its position and its link, so following a chain is one LDS read a hop; the sixteen bytes behind the
            // compared ones, which settle all but the longest matches, are read only of the sharers that pass a one-byte probe.
            // A thread's entries' words are read together and the wave adds its total to s_nflag ONCE -- an add a trip was six returning
            // atomics a wave, one behind the other, sixteen waves on the one word.  The list's order is another; every walk is its entry's own.
            {
                constexpr uint32_t kOwnPer = (kBandTile + kBandThreads - 1) / kBandThreads;
                uint32_t fl[kOwnPer], total = 0;
#pragma unroll
                for (uint32_t t = 0; t < kOwnPer; t++) { const uint32_t i = kBand + tid + kBandThreads * t; fl[t] = i < m ? (uint32_t)ck[i - kBand] >> 8 : 0u; }
#pragma unroll
                for (uint32_t t = 0; t < kOwnPer; t++) total += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(fl[t] != 0u));
                if (total) {
                    uint32_t base = 0;
                    if (lane == 0) base = atomicAdd(&s_nflag, total);
                    base = __builtin_amdgcn_readfirstlane(base);
#pragma unroll
                    for (uint32_t t = 0; t < kOwnPer; t++) {
                        const uint64_t fm = __builtin_amdgcn_ballot_w64(fl[t] != 0u);
                        if (fl[t] != 0u) flist[base + rank_in(fm)] = (uint16_t)(kBand + tid + kBandThreads * t);
                        base += (uint32_t)__popcll(fm);
                    }
                }
            }
#if ZWZ_BAND_EXP & 16
            if (tid == 0) s_p2_start = __builtin_amdgcn_s_memtime();
#endif
            __syncthreads();
            ZWZ_STAMP(9);
            // (Round 4, measured and dropped: the walks measured first -- the same chase through the links, nothing compared -- and then taken
            // longest first.  Taken 64 at a time in array order a third of the lanes are busy, sorted by length four fifths
            // (tools/exp/band_pass2_skew.py), and nothing the first pass leaves behind predicts the length.  The walk itself fell by 18 %
            // (6.99 M -> 5.75 M cycle units per 10 000 chunks), measuring and sorting cost 2.75 M: a hop's price is its lanes' LDS gathers,
            // not the trip.  Text match stage 70.4 -> 73.7 ms.)
            const uint32_t n_flag = s_nflag;
            for (;;) {
                uint32_t g = 0;
                if (lane == 0) g = atomicAdd(&s_grp[1], 1u);
                g = __builtin_amdgcn_readfirstlane(g);
                if (64u * g >= n_flag) break;
#if ZWZ_BAND_EXP & 16
                // (tickets[16 + 10]: from the pass's start to the moment the middle group is handed out -- "half of the groups done")
                if (lane == 0 && g == ((n_flag + 63u) >> 6) / 2u) atomicAdd(&tickets[16 + 10], (uint32_t)((__builtin_amdgcn_s_memtime() - s_p2_start) >> 8));
#endif
                const bool on = 64u * g + lane < n_flag;
                const uint32_t i = on ? (uint32_t)flist[64u * g + lane] : kBand;
                const uint32_t c = ck[i - kBand], cnt = c & 0xffu, k1 = c >> 8;
                const uint32_t p = band_pos(S[i]), la = L - p;
                const uint32_t max_len = la < kMaxMatch ? la : kMaxMatch, nice = la < Lv::nice ? la : Lv::nice;
                // (sixteen bytes behind the compared ones, not eight: with eight, some lane of the wave fell out into match_len_from's serial loop
                // at nearly every hop -- a third identical word in a row is a 2-3 % event per lane, i.e. an 85 % event per wave --
                // and a hop cost ~1 500 cycles; sixteen settle all but ~1 in 2 000 visits)
                const uint32_t own2_lo = load_u32(sdata, p + deep), own2_hi = load_u32(sdata, p + deep + 4u);
                const uint32_t own3_lo = load_u32(sdata, p + deep + 8u), own3_hi = load_u32(sdata, p + deep + 12u);
                // The walk behind a probe (csrc/lz_band.h, band_deep_probed, is the specification and has the proof): a sharer can change the
                // result only if it is longer than `best`, and then its byte at offset `best` is the entry's -- zlib's scan_end test.  Four visits
                // in five fail it (tools/exp/band_pass2_probe.py), and a wave of 64 nearly always holds a lane that passes, so masking the compare
                // per sharer would skip nothing: the lanes run ahead through rejected sharers on their own and meet only for the compares.
                //   compare    one sharer, for the lanes that stand on a candidate (at first every lane, on its nearest sharer, unprobed): its
                //              sixteen bytes against the entry's, the length without a branch, best / snapshot / nice stop by selects, the next
                //              sharer's word asked for beside the data; a lane that improved reloads its probe byte, sdata[p + best];
                //   run-ahead  hops: the byte at the sharer's offset `best` and the word behind its link, asked for together, so a rejected
                //              sharer costs one LDS round trip; a lane stops at a probe hit or at its chain's end, the loop ends when no lane
                //              hops or after kP2Run hops.
                // The short chain's snapshot is taken at the compares only: best changes nowhere else, so "best in front of the first sharer
                // with k > snap_chain" is best at the first COMPARED sharer with such a k -- or, if none follows, the final best, which the
                // record falls back to anyway.  The probe reads inside the data (c + best < p + best < L while best < nice); the reload behind
                // an improvement that ends the walk may read the slack behind the chunk, and nothing looks at it.
                // `reach`: the candidates the links lead to -- all of them, or, in front of a halo of another word format, the tile's own.  A walk
                // that would go on into such a halo is the plain walk's, from the start (`slow`, found out behind the loop).
                const uint32_t reach = halo_links ? cnt : min(cnt, i - kBand);
                uint32_t best = 0, best_pos = 0, snap = 0xffffffffu, pb = 0;
                // (k > snap_chain, asked of a sharer at position q: a bucket's entries lie in position order, so it is "q lies in front of
                // candidate snap_chain's position" -- one read a walk instead of a candidate number carried through every hop)
                const uint32_t q_snap = cnt > Lv::snap_chain ? band_pos(S[i - Lv::snap_chain]) : 0u;
                uint32_t w = S[on ? i - k1 : kBand];
                bool slow = on && k1 > reach;
                bool cand = on && !slow, hop = false;
                while (__builtin_amdgcn_ballot_w64(cand || hop) != 0) {
                    if (__builtin_amdgcn_ballot_w64(cand) != 0) {
                        // the five dwords that hold the sharer's sixteen bytes, the length by minimum over the four words' first differing
                        // bits -- no branch (with one, the compiler reads the upper eight bytes only where the lower eight agree, behind a
                        // wait of their own)
                        const uint32_t q = band_pos(w), sh = (q + deep) & 3u;
                        const uint32_t* d = reinterpret_cast<const uint32_t*>(sdata) + ((q + deep) >> 2);
                        const uint32_t d0 = d[0], d1 = d[1], d2 = d[2], d3 = d[3], d4 = d[4];
                        const uint32_t kn = i - (w >> 16);                          // (kBandNoLink: wraps far beyond any count)
                        const bool more = kn <= reach;
                        const uint32_t wn = S[more ? w >> 16 : kBand];
                        uint32_t t0, t1, t2, t3;
                        asm("v_ffbl_b32 %0, %1" : "=v"(t0) : "v"(__builtin_amdgcn_alignbyte(d1, d0, sh) ^ own2_lo));   // 0xffffffff for 0
                        asm("v_ffbl_b32 %0, %1" : "=v"(t1) : "v"(__builtin_amdgcn_alignbyte(d2, d1, sh) ^ own2_hi));
                        asm("v_ffbl_b32 %0, %1" : "=v"(t2) : "v"(__builtin_amdgcn_alignbyte(d3, d2, sh) ^ own3_lo));
                        asm("v_ffbl_b32 %0, %1" : "=v"(t3) : "v"(__builtin_amdgcn_alignbyte(d4, d3, sh) ^ own3_hi));
                        const uint32_t tm = min(min(t0, t1 | 32u), min(t2 | 64u, t3 | 96u));       // first differing bit of the 128
                        uint32_t l = deep + (tm >> 3);
                        if (cand && tm == 0xffffffffu) l = match_len_from(sdata, q, p, deep + 16u, max_len);   // (~1 in 2 000 of the batched walk's visits)
                        l = l < max_len ? l : max_len;
                        if (cand && q < q_snap && snap == 0xffffffffu) snap = best ? entry_pack(best, p - best_pos) : 0u;
                        if (cand && l > best) { best = l; best_pos = q; pb = sdata[p + l]; }
                        const bool on_ = cand && best < nice && more;               // the walk goes on
                        hop = hop || on_;
                        if (on_) w = wn;
                        cand = false;
                    }
                    for (uint32_t r = 0; (kP2Run == 0u || r < kP2Run) && __builtin_amdgcn_ballot_w64(hop) != 0; r++) {
                        const uint32_t cb = sdata[band_pos(w) + best];
                        const uint32_t kn = i - (w >> 16);
                        const bool more = kn <= reach;
                        const uint32_t wn = S[more ? w >> 16 : kBand];
                        const bool hit = cb == pb;
                        cand = cand || (hop && hit);
                        hop = hop && !hit && more;
                        if (hop) w = wn;
                    }
                }
                // (w is the last sharer the lane stood on: a walk that ended below `nice` because its next link leads into the halo)
                if (!halo_links) slow = slow || (on && best < nice && i - (w >> 16) <= cnt && i - (w >> 16) > reach);
                uint32_t e128 = entry_pack(best, p - best_pos), e32 = snap != 0xffffffffu ? snap : e128;
                if (slow) {
                    const uint64_t own = (uint64_t)load_u32(sdata, p + off) | (uint64_t)load_u32(sdata, p + off + 4u) << 32;
                    band_deep<Lv>(sdata, Sf, [&](uint32_t jj) { return S[jj] >> 16; },
                              [&](uint32_t jj) { const uint2 e = E[jj]; return (uint64_t)e.x | (uint64_t)e.y << 32; },   // (halo entries only)
                              kBand, i, cnt, k1, deep, L, own, e128, e32);
                }
                if (on) {
                    if (ZWZ_BAND_EXP & 4) asm volatile("" :: "v"(e128), "v"(e32), "v"(p));
                    if (!(ZWZ_BAND_EXP & 4)) {
                        reinterpret_cast<uint32_t*>(ent + p)[0] = e128;
                        if (k1 <= Lv::snap_chain) reinterpret_cast<uint32_t*>(ent + p)[1] = e32;
                    }
                }
            }
            __syncthreads();
            if (tid < kBand && b < n) {                                       // (a further tile follows: this one is full, m = kBandArr)
                const uint32_t lk = S[m - kBand + tid] >> 16;
                s_halo_link[tid] = (uint16_t)(lk != kBandNoLink && lk >= m - kBand ? lk - (m - kBand) : kBandNoLink);
            }
            __syncthreads();                                                  // the next tile overwrites S, E, ck and the counters
            ZWZ_STAMP(5);
        }
        __syncthreads();
        for (uint32_t i = tid; i < ((L + 63u) >> 6); i += kBandThreads) {
            hm[i] = (uint64_t)hasb[2 * i] | ((uint64_t)hasb[2 * i + 1] << 32);
            hasb[2 * i] = 0; hasb[2 * i + 1] = 0;
        }
        ZWZ_STAMP(6);
    }
}

// ------------------------------------------------------------------------------------------------
uint32_t exp_flags_band() { return (uint32_t)(ZWZ_BAND_EXP); }

hipError_t configure_band_kernels() {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(lz_place_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kPlaceLdsBytes);
    if (e != hipSuccess) return e;
    // more than 64 KB of dynamic LDS: EVERY instantiation needs the attribute, or its first launch fails
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(lz_match_band_kernel<LzLevel<4>>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kBandLdsBytes);
    if (e != hipSuccess) return e;
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(lz_match_band_kernel<LzLevel<5>>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kBandLdsBytes);
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(lz_match_band_kernel<LzLevel<6>>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kBandLdsBytes);
}

// which: 0 = by a sample of each chunk (production), 2 = every chunk is chain-heavy (tests).
hipError_t launch_dense_list(const DeflateArgs& a, hipStream_t s, uint32_t which) {
    const uint32_t cus = a.cu_count ? a.cu_count : 256u, want = (a.n + kDenseThreads / 64u - 1u) / (kDenseThreads / 64u);
    hipLaunchKernelGGL(lz_dense_list_kernel, dim3(want < 8u * cus ? want : 8u * cus), dim3(kDenseThreads), 0, s, a.in, a.in_off, a.in_len, a.n, a.link_stat, which);
    hipLaunchKernelGGL(lz_lists_kernel, dim3(1), dim3(1024), 0, s, a.in_len, a.link_stat, a.n, a.dense_list, a.sparse_list, a.tickets);
    return hipGetLastError();
}

hipError_t launch_sort(const DeflateArgs& a, hipStream_t s) {
    const uint32_t cus = a.cu_count ? a.cu_count : 256u;
    const uint32_t G = a.n < 2u * cus ? a.n : 2u * cus;
    hipLaunchKernelGGL(lz_sort_kernel, dim3(G), dim3(kSortThreads), 0, s, a.in, a.in_off, a.in_len, a.dense_list, a.tickets, a.sorted, a.links,
                       reinterpret_cast<uint32_t*>(a.entries));
    return hipGetLastError();
}

hipError_t launch_place(const DeflateArgs& a, hipStream_t s) {
    const uint32_t cus = a.cu_count ? a.cu_count : 256u;
    const uint32_t G = a.n < cus ? a.n : cus;
    hipLaunchKernelGGL(lz_place_kernel, dim3(G), dim3(kPlaceThreads), kPlaceLdsBytes, s, a.in_len, a.dense_list, a.tickets, a.sorted);
    return hipGetLastError();
}

hipError_t launch_match_band(const DeflateArgs& a, hipStream_t s) {
    const uint32_t cus = a.cu_count ? a.cu_count : 256u;
    const uint32_t G = a.n < cus ? a.n : cus;
    switch (a.level) {
#define ZWZ_BAND_LAUNCH(N) case N: hipLaunchKernelGGL(lz_match_band_kernel<LzLevel<N>>, dim3(G), dim3(kBandThreads), kBandLdsBytes, s, a.in, a.in_off, a.in_len, a.dense_list, \
                                                 a.tickets, a.sorted, a.entries, a.has128); break;
        ZWZ_BAND_LAUNCH(4) ZWZ_BAND_LAUNCH(5) ZWZ_BAND_LAUNCH(6)
#undef ZWZ_BAND_LAUNCH
        default: return hipErrorInvalidValue;        // a level without a kernel is an error, never another level's kernel
    }
    return hipGetLastError();
}

}  // namespace zwz
