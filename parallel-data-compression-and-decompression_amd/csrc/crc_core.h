// crc_core.h -- CRC-32 (IEEE 802.3, reflected, zlib's crc32) as linear algebra over GF(2), for the BGZF path.
//
// Portable (host + device), so that a CPU build (tests/emu_bgzf) checks every formula here against zlib.crc32.
//
// Representation: a 32-bit word is a polynomial of degree < 32 in reflected order -- bit 31 is x^0, bit 0 is x^31 --
// and P = 0xedb88320 is the generator without its x^32 term.  "raw" below is the CRC register run from 0 without
// pre- or post-conditioning; it is linear in the message and blind to leading zero bytes:
//     raw(A || B) = raw(A) * x^(8|B|)  ^  raw(B)          (mod P)
//     crc32(M)    = raw(M) ^ (~0 * x^(8|M|)) ^ ~0
// The device kernel (zwz_bgzf.hip) lets lane t of a workgroup of T lanes fold the 16-byte vectors t, t + T, t + 2T, ...
// by Horner's rule with the constant x^(8 * 16T), then combines the lanes with x^(8 * 16 (T - 1 - t)) and adds the
// short tail once per block.  The ~0 initial register is the same as complementing the first four message bytes, so it
// enters as one xor into vector 0 (into the bytewise tail when there is no whole vector); crc_lanes_host restates that
// schedule on the host.
#pragma once
#include <stddef.h>

#include "zwz_common.h"

namespace zwz {

constexpr uint32_t kCrcPoly = 0xedb88320u;
constexpr uint32_t kCrcVecTables = 16;    // slicing tables: T_k[b] = raw(b, then k zero bytes), k = 0..15
constexpr uint32_t kCrcMulTables = 4;     // a multiply by a fixed constant, byte-sliced

// one raw step of 8 bits (the register after a byte that is already xored in)
ZWZ_HD uint32_t crc_shift8(uint32_t c) {
#pragma unroll
    for (int i = 0; i < 8; i++) c = (c & 1u) ? (c >> 1) ^ kCrcPoly : c >> 1;
    return c;
}

// a * b mod P
ZWZ_HD uint32_t crc_mulmod(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (uint32_t m = 1u << 31; m; m >>= 1) {
        if (a & m) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ kCrcPoly : b >> 1;
    }
    return p;
}

// x^(8n) mod P by square-and-multiply over the bits of n
ZWZ_HD uint32_t crc_xpow8n(uint64_t n) {
    uint32_t r = 1u << 31;          // x^0
    uint32_t sq = 1u << 23;         // x^8
    while (n) {
        if (n & 1u) r = crc_mulmod(r, sq);
        sq = crc_mulmod(sq, sq);
        n >>= 1;
    }
    return r;
}

// crc32(A || B) from crc32(A), crc32(B) and |B| (zlib's crc32_combine)
ZWZ_HD uint32_t crc_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b) {
    return crc_mulmod(crc_a, crc_xpow8n(len_b)) ^ crc_b;
}

// raw -> crc32 for a message of n bytes
ZWZ_HD uint32_t crc_finish(uint32_t raw, uint64_t n) {
    return raw ^ crc_mulmod(0xffffffffu, crc_xpow8n(n)) ^ 0xffffffffu;
}

// bytewise raw update (the tail of a block, tests)
ZWZ_HD uint32_t crc_raw_bytes(uint32_t c, const uint8_t* p, uint32_t n) {
    for (uint32_t i = 0; i < n; i++) c = crc_shift8(c ^ p[i]);
    return c;
}

// Table column b (one lane per b builds it): vec[k * 256 + b] = T_k[b]; mul[j * 256 + b] = (b << 8j) * K mod P.
ZWZ_HD void crc_fill_column(uint32_t* vec, uint32_t* mul, uint32_t b, uint32_t K) {
    uint32_t c = b;
    for (uint32_t k = 0; k < kCrcVecTables; k++) { c = crc_shift8(c); vec[k * 256u + b] = c; }
    for (uint32_t j = 0; j < kCrcMulTables; j++) mul[j * 256u + b] = crc_mulmod(b << (8u * j), K);
}

// raw CRC of one 16-byte vector (four little-endian words), by the slicing tables
ZWZ_HD uint32_t crc_vec16(const uint32_t* vec, uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3) {
    uint32_t r = 0;
    const uint32_t w[4] = {w0, w1, w2, w3};
#pragma unroll
    for (uint32_t q = 0; q < 4; q++)
#pragma unroll
        for (uint32_t i = 0; i < 4; i++) r ^= vec[(15u - (4u * q + i)) * 256u + ((w[q] >> (8u * i)) & 255u)];
    return r;
}

// v * K mod P by the byte-sliced tables of K
ZWZ_HD uint32_t crc_mul_tab(const uint32_t* mul, uint32_t v) {
    return mul[v & 255u] ^ mul[256u + ((v >> 8) & 255u)] ^ mul[512u + ((v >> 16) & 255u)] ^ mul[768u + (v >> 24)];
}

// The vector layout of a block of L bytes seen by lane t of T: V = L / 16 whole vectors, padded at the FRONT with zero vectors
// to Vp = K * T (raw CRC ignores leading zeros), so that every lane folds exactly K slots and its last slot ends 16 (T - 1 - t)
// bytes before the end of the whole-vector part.  Slot k of lane t is vector k * T + t - (Vp - V) (none if negative).
ZWZ_HD uint32_t crc_lane_slots(uint32_t L, uint32_t T) { return (L / 16u + T - 1u) / T; }

// Host restatement of the device schedule (tests): crc32 of p[0, L) as T lanes compute it.
inline uint32_t crc_lanes_host(const uint8_t* p, uint32_t L, uint32_t T) {
    static uint32_t vec[kCrcVecTables * 256], mul[kCrcMulTables * 256];
    static uint32_t built_for = 0;
    if (built_for != T) { const uint32_t K = crc_xpow8n(16ull * T); for (uint32_t b = 0; b < 256; b++) crc_fill_column(vec, mul, b, K); built_for = T; }
    const uint32_t V = L / 16u, slots = crc_lane_slots(L, T), pad = slots * T - V;
    uint32_t raw = 0;
    for (uint32_t t = 0; t < T; t++) {
        uint32_t acc = 0;
        for (uint32_t k = 0; k < slots; k++) {
            const int64_t v = (int64_t)k * T + t - pad;
            acc = crc_mul_tab(mul, acc);
            if (v >= 0) {
                uint32_t w[4];
                for (int q = 0; q < 4; q++) w[q] = (uint32_t)p[v * 16 + 4 * q] | (uint32_t)p[v * 16 + 4 * q + 1] << 8 | (uint32_t)p[v * 16 + 4 * q + 2] << 16 | (uint32_t)p[v * 16 + 4 * q + 3] << 24;
                if (v == 0) w[0] ^= 0xffffffffu;          // the initial register
                acc ^= crc_vec16(vec, w[0], w[1], w[2], w[3]);
            }
        }
        raw ^= crc_mulmod(acc, crc_xpow8n(16ull * (T - 1u - t)));
    }
    const uint32_t r = L & 15u;
    raw = crc_raw_bytes(V ? raw : 0xffffffffu, p + (size_t)V * 16u, r);      // (the register update shifts raw by 8r itself)
    return raw ^ 0xffffffffu;
}

}  // namespace zwz
