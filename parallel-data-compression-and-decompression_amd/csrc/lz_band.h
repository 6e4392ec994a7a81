// lz_band.h -- match records from the chunk's positions SORTED by (hash bucket, position): the candidates zlib's
// longest_match() would walk for a position (consumer(), compression.cpp:119-131) are then the entries right in front
// of it, so "the chain walk" becomes a banded comparison of neighbouring array elements -- no pointer chase.
//
// Same records as lz_core.h's lz_search() (which stays the specification and what sparse chunks run):
//   * entry u of the sorted array = (h << 16 | p); entry u - k is p's k-th candidate, newest first, as long as it is in
//     the same bucket, is not position 0 (zlib's NIL), and lies within MAX_DIST (band_count);
//   * zlib keeps the FIRST candidate of the greatest length, so the answer is max over k of (length, -k): one
//     v_max_u32 per candidate on a packed key (band_key; the kernel takes two candidates' keys in the 16-bit halves of a word,
//     band_key_pair / band_first_pass).  Lengths are compared on eight bytes kept beside each
//     entry -- bytes 3..10 behind the trigram where every bucket of the tile holds one trigram only ("pure"), else bytes
//     0..7 -- which settles every length below kDeep (11 / 8);
//   * a position whose best candidate agrees on all eight bytes is finished by a second pass that visits only the
//     candidates agreeing on all eight (its "sharers", chained nearest-first through link[]), comparing real bytes;
//   * zlib's short chain (32 candidates once the previous match is "good") is the key after the 32nd candidate (at level 6; the level's snap_chain-th in general).
// The last positions of a chunk (lookahead < kDeep): their eight bytes reach past the data, so their XORs are masked
// down to the bytes that exist (band_tail_mask) -- "all of them agree" then means "agrees to the end of the data", which
// is as long as a match can get there (and zlib stops at the first such candidate: the nearest).
//
// The compression level (zwz_common.h: LzLevel<N>, template argument Lv, level 6 where none is named) enters in three places: band_count
// stops at the level's max_chain (16 or 32 candidates, not the band's 128: the halo may stay 128 wide), the short chain's key is the one
// after snap_chain candidates, and the second pass stops at the level's nice length.  Every level's nice length is above kDeep, so the
// first pass still settles only lengths below `nice` and the nice stop stays the second pass's business (static_assert in LzLevelOf);
// tail positions (lookahead < nice) take nice = lookahead from band_generic / the masked keys as before.
//
// Portable (host + device): tests/emu builds band_records() on the CPU and diffs it against lz_search().
#pragma once
#include <cassert>

#include "lz_core.h"

namespace zwz {

constexpr uint32_t kBand = kMaxChain;            // candidates a position may look at: the band's width
constexpr uint32_t kBandNoLink = 0xffffu;
constexpr uint32_t kBandHaloWord = 0xffff0000u;  // "no entry": bucket 0xffff (no hash is), position 0

// lz_dense_list's sample: the chunk's first kDenseSample trigrams.
constexpr uint32_t kDenseSample = 2048;
// Round 5: the rule weighs what the search would have to walk, not how often buckets repeat.  The sample counts the positions that are at least the SECOND
// in their bucket (repeats) and those that are at least the THIRD (thirds).  With the tail taken as geometric the mean number of earlier same-bucket
// positions in the sample would be repeats + thirds / (1 - thirds / repeats), over `sampled`; text's buckets are heavier-tailed than that (its commonest
// trigrams: 12.6 candidates a position in an 8 KB chunk where the geometric tail says 5.9), so the tail term counts three times; over the whole chunk
// the mean is L / sampled times the sample's.  Chain-heavy = 3.6 or more: where the two paths cross on image-like files (mean 16 KB: sort + band 26.7 ms,
// chain walk 28.1 per 1.3 GB; mean 6.8 KB -- BASELINE configs[3] --: 33.1 against 22.5), with text-like chunks on the band from 4 KB up (44 against
// 89 ms) -- tools/exp/dense_crossover.sh, tools/exp/dense_sample.py; tests/test_emu.py pins the choices.  (Rounds 3 - 4: repeats >= sampled / 5, whatever
// the length: the 7 KB image-like files, 0.24 repeats and 1.2 candidates a position, went to the band.)  Either path gives the same records: the
// choice is speed only.
ZWZ_HD bool sample_is_dense(uint32_t repeats, uint32_t thirds, uint32_t sampled, uint32_t L) {
    if (repeats == 0u || sampled == 0u) return false;
    if (thirds >= repeats) return true;                                       // every repeat is a third one: a run
    const float walk = ((float)repeats + 3.0f * (float)thirds * (float)repeats / (float)(repeats - thirds)) * (float)L / ((float)sampled * (float)sampled);
    return walk >= 3.6f;
}

ZWZ_HD uint32_t band_word(uint32_t h, uint32_t p) { return h << 16 | p; }
ZWZ_HD uint32_t band_pos(uint32_t w) { return w & 0xffffu; }
ZWZ_HD uint32_t band_hash(uint32_t w) { return w >> 16; }

// Is `c` (a sorted-array word) a candidate of the position behind `own`, as the second or a later one of its chain?
// (same bucket; not position 0, which reads back as NIL and ends any chain; nearer than MAX_DIST.)  Monotone along the
// array: once an entry fails, every entry further back fails too.
ZWZ_HD bool band_valid(uint32_t own, uint32_t c) {
    // (with equal buckets the words' difference IS the positions' difference: c precedes own in its bucket)
    const uint32_t d = own - c;
    return (own ^ c) < 0x10000u && d < kMaxDist && d != band_pos(own);
}
// band_valid as a range test, for a search that asks it of many words c with one `own` (band_count, lz_match_band's count phase):
// band_lo(own) is the lowest word that can be a candidate of `own`, found once, and a probe is one subtraction and one unsigned
// compare -- band_in_reach(own, lo, c) == band_valid(own, c) for every c != own.
// Proof.  Let h, p be own's bucket and position, q_lo = max(p - (kMaxDist - 1), 1) for p >= 1 and 0 for p = 0; lo = h << 16 | q_lo.
// Then q_lo <= p, so lo <= own and span = own - lo = p - q_lo < kMaxDist: c - lo < span (unsigned) says lo <= c < own with nothing
// wrapping, i.e. c has own's upper half -- bucket h -- and a position q with q_lo <= q < p.  band_valid asks for bucket h, d = p - q
// in [0, kMaxDist) -- q <= p and q >= p - (kMaxDist - 1) -- and q != 0: bucket h and max(p - (kMaxDist - 1), 1) <= q <= p, which for
// c != own (q != p) is the same set, and for p = 0 the empty one on both sides (span = 0).  The halo word as `own` is position 0: no
// candidates; as c it is bucket 0xffff, above every own, and a word of an earlier bucket is below lo.  (c == own: band_valid says yes
// where p != 0, the range says no -- an entry is never its own predecessor in the array, so no search asks.)
ZWZ_HD uint32_t band_lo(uint32_t own) {
    const uint32_t p = band_pos(own), far = p > kMaxDist - 1u ? p - (kMaxDist - 1u) : 0u, one = p < 1u ? p : 1u;
    return (own & 0xffff0000u) | (far > one ? far : one);
}
ZWZ_HD bool band_in_reach(uint32_t own, uint32_t lo, uint32_t c) { return c - lo < own - lo; }

// The first candidate alone may sit at exactly MAX_DIST -- unless zlib's window has slid by then (lz_search's start test).
ZWZ_HD bool band_first_at_max_dist(uint32_t own, uint32_t c) {
    const uint32_t p = band_pos(own), q = band_pos(c);
    return band_hash(c) == band_hash(own) && q != 0u && p - q == kMaxDist && !(p >= kSlidePos && q <= kWSize);
}

// Number of candidates of entry u: binary search over the monotone band_valid.  S(i) -> word of array index i (the
// caller's array starts kBand entries before its first own entry, filled with kBandHaloWord where nothing exists).
template <class Lv = LzDefaultLevel, class SFn>
ZWZ_HD uint32_t band_count(SFn S, uint32_t u) {
    const uint32_t own = S(u), lo = band_lo(own);
    uint32_t k = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t step = kBand; step >= 1u; step >>= 1) {      // largest k in [0, 128] with band_valid(S(u - k)), asked as band_in_reach
        const uint32_t t = k + step;
        if (t <= kBand && band_in_reach(own, lo, S(u - t))) k = t;
    }
    if (k == 0u && band_first_at_max_dist(own, S(u - 1u))) k = 1u;
    return k < Lv::max_chain ? k : Lv::max_chain;             // the level's chain, not the band's width (the halo stays 128 entries)
}

// Packed comparison key of the k-th candidate: (equal leading bytes of the two 8-byte words) << 8 | (129 - k); 15 in the
// length field = all eight agree.  Greater key = longer, then nearer.
ZWZ_HD uint32_t band_ctz64(uint32_t lo, uint32_t hi) {
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t t0, t1;
    asm("v_ffbl_b32 %0, %1" : "=v"(t0) : "v"(lo));            // 0xffffffff for 0
    asm("v_ffbl_b32 %0, %1" : "=v"(t1) : "v"(hi));
    t1 |= 32u;
    return t0 < t1 ? t0 : t1;
#else
    if (lo) return (uint32_t)__builtin_ctz(lo);
    if (hi) return 32u + (uint32_t)__builtin_ctz(hi);
    return 0xffffffffu;
#endif
}
ZWZ_HD uint32_t band_key(uint32_t own_lo, uint32_t own_hi, uint32_t c_lo, uint32_t c_hi, uint32_t k) {
    const uint32_t t = band_ctz64(own_lo ^ c_lo, own_hi ^ c_hi);
    return ((t & 0x78u) << 5) | (129u - k);
}
// Masked form for a position whose word reaches past the end of the data: only the first `nbytes` bytes count.
ZWZ_HD uint32_t band_key_masked(uint32_t own_lo, uint32_t own_hi, uint32_t c_lo, uint32_t c_hi, uint32_t m_lo, uint32_t m_hi, uint32_t k) {
    const uint32_t t = band_ctz64((own_lo ^ c_lo) & m_lo, (own_hi ^ c_hi) & m_hi);
    return ((t & 0x78u) << 5) | (129u - k);
}
// Two candidates an instruction (lz_match_band's first pass): a key is 12 bits, so the keys of candidates k and k + 1 live in the low and
// the high 16 bits of one word, and so do the running maximum (a maximum per half; the two meet behind the loop) and the values `none`.
// `mask` holds, per half, the mask of the first differing bit's byte field: kBandPairLenMask's 0x78 for a candidate the position has, 0
// for one beyond its count -- that one's key is then of length 0, 129 - k alone.  Such a key (k >= 2: it lies beyond a count >= 1) is
// below the key of the position's first candidate (>= 128), which is always among the keys the maximum is taken over, and below
// kBandKeyNoneImpure: it never wins, so nothing has to keep it out of the maximum (band_first_pass below is the whole argument, run).
constexpr uint32_t kBandPairLenMask = 0x00780078u;
ZWZ_HD uint32_t band_key_pair(uint32_t own_lo, uint32_t own_hi, uint32_t a_lo, uint32_t a_hi, uint32_t b_lo, uint32_t b_hi, uint32_t k, uint32_t mask) {
    // (the halves of a first differing bit: 0 .. 63, or 0xffff for "none" -- what the kernel's 16-bit find-first-bit results and minimum give)
    const uint32_t ta = band_ctz64(own_lo ^ a_lo, own_hi ^ a_hi) & 0xffffu, tb = band_ctz64(own_lo ^ b_lo, own_hi ^ b_hi) & 0xffffu;
    return (((ta | tb << 16) & mask) << 5) | (129u - k) | (128u - k) << 16;
}
// The masks of a trip of eight candidates k0 + 1 .. k0 + 8 for a position of `cnt` candidates, a byte a candidate (0x78 or 0), and
// the mask of the pair j, j + 1 (j even) out of them.
ZWZ_HD uint64_t band_trip_mask(uint32_t k0, uint32_t cnt) {
    const int32_t over = (int32_t)(k0 + 8u) - (int32_t)cnt;                   // the trip's candidates beyond the count
    const uint32_t d = over < 0 ? 0u : over > 8 ? 8u : (uint32_t)over;
    return 0x7878787878787878ull >> (8u * d < 63u ? 8u * d : 63u);            // (all eight beyond: 63 bits leave nothing of 0x78...)
}
ZWZ_HD uint32_t band_pair_mask(uint64_t trip_mask, uint32_t j) {
    return ((uint32_t)(trip_mask >> (8u * j)) & 0xffu) | ((uint32_t)(trip_mask >> (8u * j + 8u)) & 0xffu) << 16;
}
ZWZ_HD uint32_t band_pair_max(uint32_t pair) { return (pair & 0xffffu) > (pair >> 16) ? pair & 0xffffu : pair >> 16; }
// The first pass of a position that is no tail, in the order lz_match_band takes it (and its specification): trips of eight candidates,
// unmasked up to `kmin` (the smallest count among the wave's lanes that have candidates: any value from 0 to cnt here), masked by
// band_trip_mask up to `kmax` (the wave's greatest count: any value >= cnt), the short chain's snapshot behind the trip that ends at
// snap_chain.  E(k) -> the k-th candidate's 8-byte word as lo | hi << 32; candidates beyond cnt may hold anything.  Same best and
// snapshot as the maximum of band_key over the candidates 1 .. cnt (tests/test_band_pass1_cpu.py).
template <class Lv = LzDefaultLevel, class EFn>
ZWZ_HD void band_first_pass(uint64_t own, EFn E, uint32_t cnt, uint32_t kmin, uint32_t kmax, uint32_t none, uint32_t& best, uint32_t& snap) {
    const uint32_t own_lo = (uint32_t)own, own_hi = (uint32_t)(own >> 32);
    uint32_t best2 = cnt ? none | none << 16 : 0xffffffffu;
    snap = none;
    for (uint32_t k0 = 0; k0 < kmax; k0 += 8u) {
        const bool masked = k0 + 8u > kmin;
        const uint64_t have = band_trip_mask(k0, cnt);
        for (uint32_t j = 0; j < 8u; j += 2u) {
            const uint64_t a = E(k0 + j + 1u), b = E(k0 + j + 2u);
            const uint32_t key = band_key_pair(own_lo, own_hi, (uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b, (uint32_t)(b >> 32), k0 + j + 1u,
                                               masked ? band_pair_mask(have, j) : kBandPairLenMask);
            const uint32_t lo = (key & 0xffffu) > (best2 & 0xffffu) ? key & 0xffffu : best2 & 0xffffu, hi = (key >> 16) > (best2 >> 16) ? key >> 16 : best2 >> 16;
            best2 = lo | hi << 16;
        }
        if (k0 + 8u == Lv::snap_chain) snap = band_pair_max(best2);
    }
    best = cnt ? band_pair_max(best2) : none;
}

ZWZ_HD uint32_t band_tail_bytes(bool pure, uint32_t lookahead) {      // bytes of the word inside the data (lookahead >= 3)
    const uint32_t nb = pure ? lookahead - 3u : lookahead;
    return nb < 8u ? nb : 8u;
}
ZWZ_HD uint32_t band_tail_mask(uint32_t nbytes, uint32_t word /* 0 = low, 1 = high */) {
    const uint32_t nb = nbytes > 4u * word ? nbytes - 4u * word : 0u;
    return nb >= 4u ? 0xffffffffu : (1u << (8u * nb)) - 1u;
}
constexpr uint32_t kBandKeyNonePure = 0u;          // below every key
constexpr uint32_t kBandKeyNoneImpure = 0x2ffu;    // above every key of fewer than three equal bytes: the trigram itself differs
ZWZ_HD uint32_t band_key_len(uint32_t key) { return key >> 8; }            // equal bytes of the eight, 15 = all
ZWZ_HD uint32_t band_key_k(uint32_t key) { return 129u - (key & 0xffu); }

// Record of a key: cand = position of the winner.  "All eight agree" (15) is a record only for a tail position, whose
// match then runs to the end of the data (lookahead bytes); elsewhere it is the second pass's business.
ZWZ_HD uint32_t band_record(uint32_t key, bool pure, uint32_t p, uint32_t cand_pos, uint32_t tail_len = 0) {
    const uint32_t len = band_key_len(key) == 15u ? tail_len : band_key_len(key) + (pure ? 3u : 0u), dist = p - cand_pos;
    if (len == kMinMatch && dist > kTooFar) return 0u;
    return entry_pack(len, dist);
}

// The chunk's last positions (and the specification of the whole scheme): candidates u - 1 .. u - cnt, real bytes.
template <class Lv = LzDefaultLevel, class SFn>
ZWZ_HD void band_generic(const uint8_t* data, SFn S, uint32_t u, uint32_t cnt, uint32_t L, uint32_t& e128, uint32_t& e32) {
    const uint32_t p = band_pos(S(u)), lookahead = L - p;
    const uint32_t max_len = lookahead < kMaxMatch ? lookahead : kMaxMatch, nice = lookahead < Lv::nice ? lookahead : Lv::nice;
    uint32_t best = kMinMatch - 1u, best_pos = 0, snap = 0xffffffffu;
    for (uint32_t k = 1; k <= cnt; k++) {
        const uint32_t c = band_pos(S(u - k));
        const uint32_t len = match_len_from(data, c, p, 0u, max_len);
        if (len > best) { best = len; best_pos = c; }
        if (k == Lv::snap_chain) snap = best >= kMinMatch ? entry_pack(best, p - best_pos) : 0u;
        if (best >= nice) break;
    }
    e128 = best >= kMinMatch ? entry_pack(best, p - best_pos) : 0u;
    e32 = snap != 0xffffffffu ? snap : e128;
    if (entry_len(e128) == kMinMatch && entry_dist(e128) > kTooFar) e128 = 0;
    if (entry_len(e32) == kMinMatch && entry_dist(e32) > kTooFar) e32 = 0;
}

// Second pass of a position whose nearest sharer is its k1-th candidate: the sharers, nearest first, compared byte by
// byte from kDeep on.  link(j) -> array index of the nearest sharer of entry j, kBandNoLink if none in ITS band; valid
// for the tile's own entries (j >= first_own) -- through the halo in front of them the sharers are found by their
// eight bytes (E(j) -> the 8-byte word as lo | hi << 32, asked for halo entries only).
template <class Lv = LzDefaultLevel, class SFn, class LinkFn, class EFn>
ZWZ_HD void band_deep(const uint8_t* data, SFn S, LinkFn link, EFn E, uint32_t first_own, uint32_t u, uint32_t cnt, uint32_t k1,
                      uint32_t deep, uint32_t L, uint64_t own /* entry u's 8-byte word */, uint32_t& e128,
                      uint32_t& e32 /* in: the first pass's, kept if k1 > snap_chain */) {
    const uint32_t p = band_pos(S(u)), lookahead = L - p;
    const uint32_t max_len = lookahead < kMaxMatch ? lookahead : kMaxMatch, nice = lookahead < Lv::nice ? lookahead : Lv::nice;
    uint32_t best = 0, best_pos = 0, snap = 0xffffffffu;
    uint32_t j = u - k1;
    for (;;) {
        const uint32_t k = u - j;
        if (k > Lv::snap_chain && snap == 0xffffffffu) snap = best ? entry_pack(best, p - best_pos) : 0u;   // (0 only if k1 > snap_chain: then unused)
        const uint32_t c = band_pos(S(j));
        const uint32_t len = match_len_from(data, c, p, deep, max_len);
        if (len > best) { best = len; best_pos = c; if (len >= nice) break; }
        if (j >= first_own) {
            const uint32_t j2 = link(j);
            if (j2 == kBandNoLink || u - j2 > cnt) break;
            j = j2;
        } else {
            uint32_t k2 = k + 1u;
            while (k2 <= cnt && E(u - k2) != own) k2++;
            if (k2 > cnt) break;
            j = u - k2;
        }
    }
    e128 = entry_pack(best, p - best_pos);
    if (k1 <= Lv::snap_chain) e32 = snap != 0xffffffffu ? snap : e128;
}

// band_deep in the order lz_match_band's second pass takes it (and its specification): H sharers a batch.
//   chase    the next H sharers, by their links alone -- the only step that hangs on the one before it;
//   compare  the batch's H lengths, each on its own;
//   fold     the lengths into best / snapshot / nice stop IN SHARER ORDER: the first of the greatest length wins, the walk
//            ends behind the first sharer whose length reaches `nice` (sharers chased beyond it are ignored), the short
//            chain's snapshot is taken at the first sharer with k > snap_chain (32 at level 6).
// Same arguments, same records as band_deep for every H >= 1 (tests/test_band_pass2_cpu.py).  `visited`, if given, receives
// the number of sharers the walk looked at.
template <uint32_t H, class Lv = LzDefaultLevel, class SFn, class LinkFn, class EFn>
ZWZ_HD void band_deep_batched(const uint8_t* data, SFn S, LinkFn link, EFn E, uint32_t first_own, uint32_t u, uint32_t cnt, uint32_t k1,
                              uint32_t deep, uint32_t L, uint64_t own, uint32_t& e128, uint32_t& e32, uint32_t* visited = nullptr) {
    static_assert(H >= 1, "a batch holds a sharer");
    const uint32_t p = band_pos(S(u)), lookahead = L - p;
    const uint32_t max_len = lookahead < kMaxMatch ? lookahead : kMaxMatch, nice = lookahead < Lv::nice ? lookahead : Lv::nice;
    auto next = [&](uint32_t j) -> uint32_t {                  // the sharer behind entry j, kBandNoLink where the band ends
        if (j >= first_own) {
            const uint32_t j2 = link(j);
            return j2 == kBandNoLink || u - j2 > cnt ? kBandNoLink : j2;
        }
        uint32_t k2 = u - j + 1u;
        while (k2 <= cnt && E(u - k2) != own) k2++;
        return k2 > cnt ? kBandNoLink : u - k2;
    };
    uint32_t best = 0, best_pos = 0, snap = 0xffffffffu, seen = 0;
    uint32_t j = u - k1;
    bool walking = true;
    while (walking) {
        uint32_t jv[H], len[H], nv = 1;
        jv[0] = j;
        for (uint32_t h = 1; h < H; h++) {                      // chase
            const uint32_t j2 = next(jv[h - 1u]);
            if (j2 == kBandNoLink) break;
            jv[h] = j2; nv++;
        }
        for (uint32_t h = 0; h < nv; h++) len[h] = match_len_from(data, band_pos(S(jv[h])), p, deep, max_len);   // compare
        bool alive = true;
        for (uint32_t h = 0; h < nv; h++) {                     // fold
            if (!alive) break;
            if (u - jv[h] > Lv::snap_chain && snap == 0xffffffffu) snap = best ? entry_pack(best, p - best_pos) : 0u;
            if (len[h] > best) { best = len[h]; best_pos = band_pos(S(jv[h])); }
            seen++;
            alive = best < nice;
        }
        j = alive && nv == H ? next(jv[H - 1u]) : kBandNoLink;
        walking = j != kBandNoLink;
    }
    if (visited) *visited = seen;
    e128 = entry_pack(best, p - best_pos);
    if (k1 <= Lv::snap_chain) e32 = snap != 0xffffffffu ? snap : e128;
}

// band_deep as lz_match_band's second pass takes it since round 8 (and its specification): zlib's own scan_end test (longest_match
// looks at the byte at offset best_len before it compares anything), which the sharers' walk never had.  The walk's first sharer is
// always compared; a later sharer at position c is compared only if data[c + best] == data[p + best], else it counts as looked at
// and changes nothing.
// Same records as band_deep:
//   * a length is the number of equal leading bytes, so len > best means the bytes 0 .. best agree, the one at offset `best` among
//     them: a sharer that fails the probe has len <= best and cannot meet the only condition under which best / best_pos change;
//   * the snapshot (at the first sharer with k > snap_chain, before it is considered), the count limit and the nice stop hang on k
//     and best alone, and best is what it would have been;
//   * the probe reads inside the data: the walk goes on only while best < nice <= max_len = min(258, L - p), and a sharer lies in
//     front of its position, c < p, so c + best < p + best < L (asserted in host builds).
// Same arguments as band_deep_batched; `visited` receives the sharers looked at (band_deep_batched's number), `compared` those
// that went through match_len_from.  tests/test_band_pass2_probe_cpu.py.
template <class Lv = LzDefaultLevel, class SFn, class LinkFn, class EFn>
ZWZ_HD void band_deep_probed(const uint8_t* data, SFn S, LinkFn link, EFn E, uint32_t first_own, uint32_t u, uint32_t cnt, uint32_t k1,
                             uint32_t deep, uint32_t L, uint64_t own, uint32_t& e128, uint32_t& e32, uint32_t* visited = nullptr,
                             uint32_t* compared = nullptr) {
    const uint32_t p = band_pos(S(u)), lookahead = L - p;
    const uint32_t max_len = lookahead < kMaxMatch ? lookahead : kMaxMatch, nice = lookahead < Lv::nice ? lookahead : Lv::nice;
    uint32_t best = 0, best_pos = 0, snap = 0xffffffffu, seen = 0, full = 0;
    uint32_t j = u - k1;
    for (;;) {
        const uint32_t k = u - j;
        if (k > Lv::snap_chain && snap == 0xffffffffu) snap = best ? entry_pack(best, p - best_pos) : 0u;
        const uint32_t c = band_pos(S(j));
        bool probe = seen == 0u;
        if (!probe) {
#if !defined(__HIP_DEVICE_COMPILE__)
            assert(c < p && best < nice && p + best < L);
#endif
            probe = data[c + best] == data[p + best];
        }
        seen++;
        if (probe) {
            full++;
            const uint32_t len = match_len_from(data, c, p, deep, max_len);
            if (len > best) { best = len; best_pos = c; if (len >= nice) break; }
        }
        if (j >= first_own) {
            const uint32_t j2 = link(j);
            if (j2 == kBandNoLink || u - j2 > cnt) break;
            j = j2;
        } else {
            uint32_t k2 = k + 1u;
            while (k2 <= cnt && E(u - k2) != own) k2++;
            if (k2 > cnt) break;
            j = u - k2;
        }
    }
    if (visited) *visited = seen;
    if (compared) *compared = full;
    e128 = entry_pack(best, p - best_pos);
    if (k1 <= Lv::snap_chain) e32 = snap != 0xffffffffu ? snap : e128;
}

}  // namespace zwz
