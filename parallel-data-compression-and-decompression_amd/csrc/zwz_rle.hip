// zwz_rle.hip -- the parse of libz's search-free strategies (rle_core.h): Z_HUFFMAN_ONLY and Z_RLE.  One kernel in the place of
// lz_links, lz_sort, lz_place, lz_match, lz_match_band, lz_lazy and lz_parse: it writes what lz_parse hands blockify and encode -- a
// chunk's symbol and match-start words, the chosen records of its matches (distance 1) compact and in stream order, and
// ChunkInfo{n_sym, n_blocks}.
//
// A workgroup of four waves per chunk, not a wave: the kernel moves bytes (64 KB in, under 20 KB out a chunk) and a wave alone would
// have to keep 64 KB of loads in flight by itself; 256 lanes hold the chunk in sixteen 16-byte loads each, all issued before the
// first is used; 90 registers and 18 KB of LDS leave room for five workgroups on a CU, 320 KB of loads in flight.
//   1  every lane turns its sixteen 16-byte vectors into E bits (rle_eq16), sixteen at a time, and puts them into LDS: 1024 words.
//      The byte in front of a vector is the neighbouring lane's last one (DPP); a wave's first lane reads it from memory.
//   2  two scans over the words: back[w], the start of the run that runs into word w + 1, and fwd[w], the first run end from word
//      w on.  Runs span words -- the whole chunk if it must be -- so no lane ever walks.
//   3  a word that touches no run of four is all literals (rle_word_quiet): a lane settles four words that way, and text and
//      incompressible bytes have hardly any other.  The rest take a wave a word, a lane a position: the run's ends from E, back and
//      fwd (rle_run_of), the position's fate (rle_fate), the symbol and match-start words by ballot.
//   4  the matches' ranks -- a prefix count of the match-start words -- and then the records, by the wave that made the word.
// The Huffman-only form is the degenerate case: every valid position a symbol, no match, no byte of the chunk read.
#include <hip/hip_runtime.h>

#include "rle_core.h"
#include "zwz_kernels.h"
#include "zwz_device.h"

namespace zwz {

constexpr uint32_t kRleThreads = 256, kRleWaves = kRleThreads / 64;
constexpr uint32_t kRleVecs = 65536 / 16 / kRleThreads;        // 16-byte vectors a lane: 16
constexpr uint32_t kRleWordsPerLane = kMaskWords / kRleThreads;  // 4
static_assert(kRleVecs == 16 && kRleWordsPerLane == 4, "a chunk is sixteen vectors and four mask words a lane");

template <uint32_t kStrategy>
__global__ __launch_bounds__(kRleThreads) void strategy_parse_kernel(const uint8_t* __restrict__ in, const uint64_t* __restrict__ in_off,
                                                                   const uint32_t* __restrict__ in_len, uint64_t* __restrict__ sym,
                                                                   uint64_t* __restrict__ mst, ChunkInfo* __restrict__ info,
                                                                   uint16_t* __restrict__ links) {
    static_assert(kStrategy == kStrategyHuffman || kStrategy == kStrategyRle, "the two strategies with a closed form");
    const uint32_t chunk = blockIdx.x, tid = threadIdx.x, lane = lane_id(), wave = tid >> 6;
    const uint32_t L = min(in_len[chunk], kChunk);
    const uint32_t nwords = (L + 63u) >> 6;
    uint64_t* gsym = sym + (size_t)chunk * kMaskWords;
    uint64_t* gmst = mst + (size_t)chunk * kMaskWords;
    auto valid_word = [&](uint32_t w) -> uint64_t { return L - (w << 6) >= 64u ? ~0ull : (1ull << (L & 63u)) - 1ull; };     // w < nwords

    if constexpr (kStrategy == kStrategyHuffman) {
        for (uint32_t w = tid; w < nwords; w += kRleThreads) { gsym[w] = valid_word(w); gmst[w] = 0ull; }
        if (tid == 0) info[chunk] = ChunkInfo{L, strategy_blocks(L)};
    } else {
        __shared__ uint64_t s_e[kMaskWords];                       // E: bit p = byte p equals byte p - 1
        __shared__ uint32_t s_back[kMaskWords], s_fwd[kMaskWords + 1];
        __shared__ uint16_t s_mrank[kMaskWords];                   // match starts of every word (at most 16)
        __shared__ uint32_t s_wmax[kRleWaves], s_wmin[kRleWaves], s_wcnt[kRleWaves], s_nsym;
        const uint8_t* data = in + in_off[chunk];
        const uint4* d4 = reinterpret_cast<const uint4*>(data);    // readable up to L rounded up to 16 (the API's contract)
        const uint32_t ngroups = (L + 15u) >> 4;

        // 1: wave v holds vectors [1024 v, 1024 v + 1024), lane l those at 1024 v + 64 u + l: a wave-instruction reads 1 KB in a row
        uint4 v[kRleVecs];
        const uint32_t g_first = wave * (64u * kRleVecs) + lane;
#pragma unroll
        for (uint32_t u = 0; u < kRleVecs; u++) { const uint32_t g = g_first + 64u * u; v[u] = g < ngroups ? d4[g] : make_uint4(0u, 0u, 0u, 0u); }
        uint32_t carry = 0;                                        // lane 63's last byte of the round before: lane 0's predecessor
        if (lane == 0 && wave != 0 && g_first < ngroups) carry = data[(size_t)g_first * 16u - 1u];
        if (tid == 0) s_nsym = 0;
        uint16_t* e16 = reinterpret_cast<uint16_t*>(s_e);          // (little-endian: vector g's sixteen bits are bits 16 (g & 3).. of word g >> 2)
#pragma unroll
        for (uint32_t u = 0; u < kRleVecs; u++) {
            const uint32_t g = g_first + 64u * u;
            const uint32_t last = v[u].w >> 24;
            uint32_t prev = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)last, 0x138, 0xf, 0xf, true);      // wave_shr:1 -- lane l - 1's last byte
            if (lane == 0) prev = carry;
            carry = (uint32_t)__builtin_amdgcn_readlane((int)last, 63);
            uint32_t bits = rle_eq16(v[u].x, v[u].y, v[u].z, v[u].w, prev);
            if (g == 0) bits &= ~1u;                               // position 0 has no predecessor
            const uint32_t p0 = g << 4;
            bits = p0 >= L ? 0u : L - p0 >= 16u ? bits : bits & ((1u << (L - p0)) - 1u);     // nothing from the length on (what lies there is not the chunk's)
            e16[g] = (uint16_t)bits;
        }
        __syncthreads();

        // 2: lane t takes words 4t .. 4t + 3 for back and, from the far end, words 1023 - 4t .. 1020 - 4t for fwd (a running minimum from
        // behind = a running maximum of the complement, taken in reverse)
        {
            uint32_t bk[kRleWordsPerLane], fw[kRleWordsPerLane], bmax = 0, fmax = 0;
#pragma unroll
            for (uint32_t k = 0; k < kRleWordsPerLane; k++) {
                const uint32_t wb = tid * kRleWordsPerLane + k, wf = kMaskWords - 1u - wb;
                bmax = max(bmax, rle_word_last_clear(s_e[wb], wb)); bk[k] = bmax;
                fmax = max(fmax, ~rle_word_first_clear(s_e[wf], wf)); fw[k] = fmax;
            }
            const uint32_t binc = wave_scan_max_incl(bmax), finc = wave_scan_max_incl(fmax);
            if (lane == 63) { s_wmax[wave] = binc; s_wmin[wave] = finc; }
            __syncthreads();
            uint32_t bbase = 0, fbase = 0;                          // everything in front of this lane: earlier waves, earlier lanes
            for (uint32_t i = 0; i < wave; i++) { bbase = max(bbase, s_wmax[i]); fbase = max(fbase, s_wmin[i]); }
            const uint32_t bex = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)binc, 0x138, 0xf, 0xf, true);      // wave_shr:1: exclusive (0 in lane 0)
            const uint32_t fex = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)finc, 0x138, 0xf, 0xf, true);
            bbase = max(bbase, bex); fbase = max(fbase, fex);
#pragma unroll
            for (uint32_t k = 0; k < kRleWordsPerLane; k++) {
                const uint32_t wb = tid * kRleWordsPerLane + k, wf = kMaskWords - 1u - wb;
                s_back[wb] = max(bbase, bk[k]);
                s_fwd[wf] = ~max(fbase, fw[k]);
            }
            if (tid == 0) s_fwd[kMaskWords] = kRleNone;
        }
        __syncthreads();

        // 3 and 4 share this: word w (wave-uniform) -> this lane's fate
        auto fate_of = [&](uint32_t w) -> RleFate {
            RleFate f{1u, 0u, 0u};
            const uint32_t p = (w << 6) + lane;
            if (p < L) {
                const uint64_t e = s_e[w];
                uint32_t s, end;
                rle_run_of(p, L, [&](uint32_t) { return e; }, [&](uint32_t i) { return s_back[i]; }, [&](uint32_t i) { return s_fwd[i]; }, s, end);
                f = rle_fate(p, s, end);
            }
            return f;
        };
        // 3: lane t looks at words 4t .. 4t + 3 -- its wave's 256 words are [256 wave, 256 wave + 256).  A quiet word is all literals
        // and is written at once; the others (busy) wait for the wave.  (A wave a word for every word was 4.1 ms per 50 000 chunks of
        // text, nearly all of it the thousand quiet tests a chunk; section 21 of DESIGN.md.)
        uint32_t n_lit = 0, busy = 0;
#pragma unroll
        for (uint32_t k = 0; k < kRleWordsPerLane; k++) {
            const uint32_t w = tid * kRleWordsPerLane + k;
            if (w >= nwords) { s_mrank[w] = 0; continue; }
            const uint64_t e = s_e[w], ep = w ? s_e[w - 1u] : 0ull, en = w + 1u < kMaskWords ? s_e[w + 1u] : 0ull;
            if (rle_word_quiet(e, ep, en)) {
                const uint64_t vw = valid_word(w);
                gsym[w] = vw; gmst[w] = 0ull; s_mrank[w] = 0;
                n_lit += (uint32_t)__popcll(vw);
            } else busy |= 1u << k;
        }
        uint32_t n_sym = 0;                                        // of the busy words: wave-uniform
#pragma unroll
        for (uint32_t k = 0; k < kRleWordsPerLane; k++) {
            for (uint64_t todo = __ballot((busy >> k) & 1u); todo; todo &= todo - 1ull) {
                const uint32_t w = (wave * 64u + (uint32_t)__builtin_ctzll(todo)) * kRleWordsPerLane + k;
                const RleFate f = fate_of(w);
                const uint64_t vw = valid_word(w), sw = __ballot(f.sym != 0u) & vw, mw = __ballot(f.mst != 0u) & vw;
                n_sym += (uint32_t)__popcll(sw);
                if (lane == 0) { gsym[w] = sw; gmst[w] = mw; s_mrank[w] = (uint16_t)__popcll(mw); }
            }
        }
        n_lit = wave_scan_incl(n_lit);
        if (lane == 63) atomicAdd(&s_nsym, n_lit + n_sym);
        __syncthreads();

        // 4: matches in front of every word, then the records, by the wave whose words they are
        uint32_t c[kRleWordsPerLane], rank[kRleWordsPerLane], tsum = 0;
#pragma unroll
        for (uint32_t k = 0; k < kRleWordsPerLane; k++) { c[k] = s_mrank[tid * kRleWordsPerLane + k]; tsum += c[k]; }
        const uint32_t incl = wave_scan_incl(tsum);
        if (lane == 63) s_wcnt[wave] = incl;
        __syncthreads();
        uint32_t run = incl - tsum;
        for (uint32_t i = 0; i < wave; i++) run += s_wcnt[i];
#pragma unroll
        for (uint32_t k = 0; k < kRleWordsPerLane; k++) { rank[k] = run; run += c[k]; }
        if (tid == 0) { const uint32_t n = s_nsym; info[chunk] = ChunkInfo{n, strategy_blocks(n)}; }
        uint32_t* chosen = reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(links + (size_t)chunk * kLinkStride) + kChosenOffset);
#pragma unroll
        for (uint32_t k = 0; k < kRleWordsPerLane; k++) {
            for (uint64_t todo = __ballot(c[k] != 0u); todo; todo &= todo - 1ull) {
                const uint32_t l = (uint32_t)__builtin_ctzll(todo), w = (wave * 64u + l) * kRleWordsPerLane + k;
                const uint32_t before = (uint32_t)__builtin_amdgcn_readlane((int)rank[k], (int)l);
                const RleFate f = fate_of(w);
                const uint64_t mw = __ballot(f.mst != 0u) & valid_word(w);
                // (the index is clamped as lz_parse clamps it: whatever the input, no store leaves the chunk's own link space)
                if ((mw >> lane) & 1ull) chosen[min(before + rank_in(mw), kChosenCap - 1u)] = entry_pack(f.len, 1u);
            }
        }
    }
}

hipError_t launch_strategy_parse(const DeflateArgs& a, hipStream_t s) {
    if (a.strategy == kStrategyHuffman)
        hipLaunchKernelGGL(strategy_parse_kernel<kStrategyHuffman>, dim3(a.n), dim3(kRleThreads), 0, s, a.in, a.in_off, a.in_len, a.sym, a.mst, a.info, a.links);
    else if (a.strategy == kStrategyRle)
        hipLaunchKernelGGL(strategy_parse_kernel<kStrategyRle>, dim3(a.n), dim3(kRleThreads), 0, s, a.in, a.in_off, a.in_len, a.sym, a.mst, a.info, a.links);
    else return hipErrorInvalidValue;                              // a strategy without a kernel is an error
    return hipGetLastError();
}

}  // namespace zwz
