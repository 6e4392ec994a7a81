// band_pass2_probe_emu.cpp -- TEST INFRASTRUCTURE.  Host build of the banded match search (csrc/lz_band.h) in lz_match_band's
// decomposition, at a compression level, with the second pass as the kernel runs it since round 8: the sharers' walk behind a
// one-byte probe at the best length (band_deep_probed).  Tiles, word formats, carried halo links and the slow path of a halo of
// another format are band_pass2_emu.cpp's.  tests/test_band_pass2_probe_cpu.py diffs its records against band_deep's (mode 0) and
// lz_search's; tests/test_gpu_band_pass2_probe.py asks it what a constructed chunk's walks look like before the chunk goes to the
// GPU.  Built with assertions on: band_deep_probed's bound on the probe's address is checked on every visit.  Never shipped or
// linked into the product library.
#undef NDEBUG
#include <algorithm>
#include <cstring>
#include <vector>

#include "../../parallel-data-compression-and-decompression_amd/csrc/lz_band.h"

using namespace zwz;

enum : uint8_t {
    kFlagged = 1,      // the position went through the second pass
    kHalo = 2,         // its sharers' chain reaches into the tile's halo
    kSlow = 4,         // ... of another word format: the kernel's slow path
    kPure = 8,         // its tile holds one trigram a bucket
    kNice = 16,        // the walk stopped at a sharer of `nice` length with sharers left
};

template <class Lv>
static void search_records(const uint8_t* in, uint32_t L, uint32_t* e128, uint32_t* e32) {
    std::vector<uint8_t> data(L + 16, 0);
    if (L) memcpy(data.data(), in, L);
    std::vector<uint16_t> link(L + 1, 0), head(32768, 0);
    for (uint32_t p = 0; p + 3 <= L; p++) { const uint32_t h = hash3(data[p], data[p + 1], data[p + 2]); link[p] = head[h]; head[h] = (uint16_t)p; }
    for (uint32_t p = 0; p < L; p++) lz_search<Lv>(data.data(), link.data(), 0, p, L, e128[p], e32[p]);
}

// Records by lz_search at `level`, the specification.  Returns 0, 1 for a level that does not exist.
extern "C" int emu_probe_search_records(const uint8_t* in, uint32_t L, int level, uint32_t* e128, uint32_t* e32) {
    switch (level) {
        case 4: search_records<LzLevel<4>>(in, L, e128, e32); return 0;
        case 5: search_records<LzLevel<5>>(in, L, e128, e32); return 0;
        case 6: search_records<LzLevel<6>>(in, L, e128, e32); return 0;
    }
    return 1;
}

template <class Lv>
static uint32_t band_pass2(const uint8_t* in, uint32_t L, uint32_t tile, int format, int mode, uint32_t* e128, uint32_t* e32, uint16_t* chain,
                           uint16_t* visited, uint16_t* visited_ref, uint16_t* compared, uint16_t* k1_out, uint8_t* flags) {
    std::vector<uint8_t> data(L + 64, 0);
    if (L) memcpy(data.data(), in, L);
    for (uint32_t i = L; i < L + 64; i++) data[i] = (uint8_t)(0xa5 + 7 * i);          // whatever lies behind a chunk
    for (uint32_t p = 0; p < L; p++) { e128[p] = 0; e32[p] = 0; chain[p] = 0; visited[p] = 0; visited_ref[p] = 0; compared[p] = 0; k1_out[p] = 0; flags[p] = 0; }
    const uint32_t n = L >= kMinMatch ? L - (kMinMatch - 1) : 0;
    std::vector<uint32_t> count(32769, 0), sorted(n);
    for (uint32_t p = 0; p < n; p++) count[hash3(data[p], data[p + 1], data[p + 2]) + 1]++;
    for (uint32_t h = 0; h < 32768; h++) count[h + 1] += count[h];
    for (uint32_t p = 0; p < n; p++) { const uint32_t h = hash3(data[p], data[p + 1], data[p + 2]); sorted[count[h]++] = band_word(h, p); }
    uint32_t pure_tiles = 0;
    bool prev_pure = false;
    std::vector<uint32_t> S(tile + kBand), link(tile + kBand), halo_link(kBand, kBandNoLink);
    std::vector<uint64_t> E(tile + kBand);
    for (uint32_t a = 0; a < n; a += tile) {
        const uint32_t b = std::min(a + tile, n), m = b - a + kBand;                  // array index i <-> sorted index a - 128 + i
        for (uint32_t i = 0; i < m; i++) S[i] = (a + i >= kBand) ? sorted[a + i - kBand] : kBandHaloWord;
        auto trig = [&](uint32_t w) { const uint32_t p = band_pos(w); return (uint32_t)data[p] | data[p + 1] << 8 | data[p + 2] << 16; };
        bool pure = format != 0;
        for (uint32_t i = 1; i < m && pure; i++)
            if (S[i] != kBandHaloWord && S[i - 1] != kBandHaloWord && band_hash(S[i]) == band_hash(S[i - 1]) && trig(S[i]) != trig(S[i - 1])) pure = false;
        pure_tiles += pure;
        const uint32_t deep = pure ? 11u : 8u, off = pure ? 3u : 0u;
        const bool halo_links = a == 0u || prev_pure == pure;                         // the kernel's rule
        prev_pure = pure;
        for (uint32_t i = 0; i < m; i++) {
            uint64_t v = 0;
            if (S[i] != kBandHaloWord) memcpy(&v, data.data() + band_pos(S[i]) + off, 8);
            E[i] = v;
            link[i] = i < kBand && a != 0u && halo_links ? halo_link[i] : kBandNoLink;
        }
        auto Sf = [&](uint32_t i) { return S[i]; };
        std::vector<uint32_t> cnt(m, 0), k1(m, 0);
        for (uint32_t u = kBand; u < m; u++) {                                       // first pass
            const uint32_t p = band_pos(S[u]);
            cnt[u] = band_count<Lv>(Sf, u);
            const bool tail = L - p < deep;
            const uint32_t nb = tail ? band_tail_bytes(pure, L - p) : 8u, m_lo = band_tail_mask(nb, 0), m_hi = band_tail_mask(nb, 1);
            const uint32_t none = pure ? kBandKeyNonePure : kBandKeyNoneImpure;
            uint32_t best = none, snap = none;
            for (uint32_t k = 1; k <= cnt[u]; k++) {
                const uint32_t key = band_key_masked((uint32_t)E[u], (uint32_t)(E[u] >> 32), (uint32_t)E[u - k], (uint32_t)(E[u - k] >> 32), m_lo, m_hi, k);
                best = std::max(best, key);
                if (k == Lv::snap_chain) snap = best;
            }
            const uint32_t key32 = cnt[u] > Lv::snap_chain ? snap : best;
            auto rec = [&](uint32_t key) { return key == none || (!tail && band_key_len(key) == 15u) ? 0u : band_record(key, pure, p, band_pos(S[u - band_key_k(key)]), L - p); };
            e128[p] = rec(best); e32[p] = rec(key32);
            if (pure) flags[p] |= kPure;
            if (tail) continue;
            if (best != none && band_key_len(best) == 15u) { k1[u] = band_key_k(best); link[u] = u - k1[u]; }
        }
        const uint32_t first_own = halo_links ? 0u : kBand;                          // where the links hold; in front of it the eight bytes are looked at
        auto lk = [&](uint32_t j) { return link[j]; };
        auto Ef = [&](uint32_t j) { return E[j]; };
        for (uint32_t u = kBand; u < m; u++) {                                       // second pass
            if (!k1[u]) continue;
            const uint32_t p = band_pos(S[u]);
            uint32_t seen = 0, seen_ref = 0, full = 0, d128 = e128[p], d32 = e32[p], x128 = e128[p], x32 = e32[p];
            band_deep<Lv>(data.data(), Sf, lk, Ef, first_own, u, cnt[u], k1[u], deep, L, E[u], d128, d32);
            { uint32_t y128 = e128[p], y32 = e32[p]; band_deep_batched<1, Lv>(data.data(), Sf, lk, Ef, first_own, u, cnt[u], k1[u], deep, L, E[u], y128, y32, &seen_ref); }
            band_deep_probed<Lv>(data.data(), Sf, lk, Ef, first_own, u, cnt[u], k1[u], deep, L, E[u], x128, x32, &seen, &full);
            e128[p] = mode ? x128 : d128; e32[p] = mode ? x32 : d32;
            // the chain as the links (or, in a halo of another format, the eight bytes) give it, whatever the lengths
            uint32_t len = 0, j = u - k1[u];
            bool halo = false;
            for (;;) {
                len++;
                halo = halo || j < kBand;
                uint32_t j2 = kBandNoLink;
                if (j >= first_own) { j2 = link[j]; if (j2 != kBandNoLink && u - j2 > cnt[u]) j2 = kBandNoLink; }
                else { uint32_t k2 = u - j + 1u; while (k2 <= cnt[u] && E[u - k2] != E[u]) k2++; if (k2 <= cnt[u]) j2 = u - k2; }
                if (j2 == kBandNoLink) break;
                j = j2;
            }
            chain[p] = (uint16_t)len; visited[p] = (uint16_t)seen; visited_ref[p] = (uint16_t)seen_ref; compared[p] = (uint16_t)full; k1_out[p] = (uint16_t)k1[u];
            flags[p] |= kFlagged | (halo ? kHalo : 0) | (halo && !halo_links ? kSlow : 0) | (seen < len ? kNice : 0);
        }
        if (b < n)
            for (uint32_t t = 0; t < kBand; t++) {
                const uint32_t l = link[m - kBand + t];
                halo_link[t] = l != kBandNoLink && l >= m - kBand ? l - (m - kBand) : kBandNoLink;
            }
    }
    return pure_tiles;
}

// mode: 0 = band_deep's records, 1 = band_deep_probed's.  format: -1 = as the kernel decides, 0 = every tile impure.
// chain[p] = sharers in p's band, visited[p] = sharers band_deep_probed looked at, visited_ref[p] = sharers the plain walk looks at
// (band_deep_batched<1>'s count), compared[p] = those it compared, k1[p] = which
// candidate the nearest sharer is.  Returns the number of pure tiles, 0xffffffff for a level that does not exist.
extern "C" uint32_t emu_band_pass2_probe(const uint8_t* in, uint32_t L, uint32_t tile, int format, int level, int mode, uint32_t* e128, uint32_t* e32,
                                         uint16_t* chain, uint16_t* visited, uint16_t* visited_ref, uint16_t* compared, uint16_t* k1_out, uint8_t* flags) {
    switch (level) {
        case 4: return band_pass2<LzLevel<4>>(in, L, tile, format, mode, e128, e32, chain, visited, visited_ref, compared, k1_out, flags);
        case 5: return band_pass2<LzLevel<5>>(in, L, tile, format, mode, e128, e32, chain, visited, visited_ref, compared, k1_out, flags);
        case 6: return band_pass2<LzLevel<6>>(in, L, tile, format, mode, e128, e32, chain, visited, visited_ref, compared, k1_out, flags);
    }
    return 0xffffffffu;
}
