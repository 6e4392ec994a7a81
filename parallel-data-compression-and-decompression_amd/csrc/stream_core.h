// stream_core.h -- the wrappers around DEFLATE streams of any size (zwz_inflate_streams_dev): zlib (RFC 1950) and gzip (RFC 1952)
// headers and trailers, the member loop of a gzip stream, and the checksum formulas of stream_check_kernel.
//
// Portable (host + device): inflate_kernel's stream form runs these on lane 0 over the stream's bytes in global memory (a header
// can be longer than the 2 KiB ring: an FNAME of any length), and tests/emu_stream runs the same functions on the host.  Statuses
// are libz 1.2.11's verdicts, at libz's granularity: a field is judged once all of its bytes are there, a stream that ends before
// that wants more input.
#pragma once
#include "crc_core.h"
#include "inflate_core.h"

namespace zwz {

enum StreamWrap : uint32_t { kWrapRaw = 0, kWrapZlib = 1, kWrapGzip = 2 };
// Per-stream statuses beyond InflateStatus's 0..3 (include/zwz.h: zwz_stream_status)
enum StreamStatus : uint32_t { kStrBadHeader = 32, kStrChecksum = 33, kStrLength = 34, kStrTrailing = 35, kStrTooLarge = 36 };
// The limits of the kernel's 32-bit positions: bit positions of the input, byte positions of the output
constexpr uint64_t kStreamMaxIn = 1ull << 29, kStreamMaxOut = 1ull << 32;

// What the decoder of one stream hands the check: the output below `checked` is covered by `expect` (the Adler-32 of a zlib stream,
// the CRC-32 of every gzip member whose CRC field was read, combined), `has_check` says whether any was read, `status` is the
// verdict if the checksum holds.
struct StreamRecord { uint32_t checked, expect, has_check, status; };

ZWZ_HD uint32_t le32_at(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
ZWZ_HD uint32_t be32_at(const uint8_t* p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | (uint32_t)p[3]; }

// zlib header at p[0, n): libz's order of checks.  Returns kInfRunning with *body = 2, or the stream's status.  A preset dictionary
// (FDICT) is refused once its 4-byte id is there, as libz asks for the dictionary only then.
ZWZ_HD uint32_t zlib_header(const uint8_t* p, uint32_t n, uint32_t* body) {
    if (n < 2) return kInfNeedInput;
    const uint32_t cmf = p[0], flg = p[1];
    if (((cmf << 8) | flg) % 31u || (cmf & 15u) != 8u || (cmf >> 4) > 7u) return kStrBadHeader;
    if (flg & 0x20u) return n < 6 ? (uint32_t)kInfNeedInput : (uint32_t)kStrBadHeader;
    *body = 2;
    return kInfRunning;
}

// gzip member header at p[at, n).  Returns kInfRunning with *body = the first byte of the DEFLATE data, or the stream's status:
// BAD_HEADER for a wrong magic, CM != 8, reserved flag bits or an FHCRC that is not the low 16 bits of the header's CRC-32.
ZWZ_HD uint32_t gzip_header(const uint8_t* p, uint32_t n, uint32_t at, uint32_t* body) {
    uint32_t q = at;
    if (n - q < 2) return kInfNeedInput;
    if (p[q] != 0x1fu || p[q + 1] != 0x8bu) return kStrBadHeader;
    if (n - q < 4) return kInfNeedInput;
    const uint32_t flg = p[q + 3];
    if (p[q + 2] != 8u || (flg & 0xe0u)) return kStrBadHeader;
    q += 10;                                                      // magic, CM, FLG, MTIME, XFL, OS
    if (q > n) return kInfNeedInput;
    if (flg & 4u) {                                               // FEXTRA: XLEN, then XLEN bytes
        if (n - q < 2) return kInfNeedInput;
        const uint32_t xlen = (uint32_t)p[q] | (uint32_t)p[q + 1] << 8;
        q += 2;
        if (n - q < xlen) return kInfNeedInput;
        q += xlen;
    }
    for (uint32_t f = 8u; f <= 16u; f <<= 1) {                    // FNAME, FCOMMENT: zero-terminated
        if (!(flg & f)) continue;
        while (q < n && p[q]) q++;
        if (q == n) return kInfNeedInput;
        q++;
    }
    if (flg & 2u) {                                               // FHCRC
        if (n - q < 2) return kInfNeedInput;
        const uint32_t want = (uint32_t)p[q] | (uint32_t)p[q + 1] << 8;
        const uint32_t crc = crc_raw_bytes(0xffffffffu, p + at, q - at) ^ 0xffffffffu;
        if ((crc & 0xffffu) != want) return kStrBadHeader;
        q += 2;
    }
    *body = q;
    return kInfRunning;
}

// The first member of a gzip stream: an input that is empty or holds only zero bytes has no member (status 1).
ZWZ_HD uint32_t gzip_first_member(const uint8_t* p, uint32_t n, uint32_t first_nonzero, uint32_t* body) {
    if (first_nonzero >= n) return kInfNeedInput;
    return gzip_header(p, n, 0, body);
}

// Start of a stream (after the first member's zero scan for gzip).  Returns kInfRunning with *body, or the stream's status.
ZWZ_HD uint32_t stream_begin(uint32_t wrap, const uint8_t* p, uint32_t n, uint32_t first_nonzero, uint32_t* body) {
    *body = 0;
    if (wrap == kWrapZlib) return zlib_header(p, n, body);
    if (wrap == kWrapGzip) return gzip_first_member(p, n, first_nonzero, body);
    return kInfRunning;
}

// After a member's final block.  q = the byte after it (the reader aligned to a byte), member = its decoded length.  zlib: the
// stored Adler-32 becomes the expected checksum of the whole output.  gzip: the stored CRC-32 is folded into rec.expect (every
// member so far), ISIZE is checked; *next = where the zero skip starts.  Returns kInfRunning if a gzip stream may go on, else its
// provisional status.  raw: nothing follows.
ZWZ_HD uint32_t stream_trailer(uint32_t wrap, const uint8_t* p, uint32_t n, uint32_t q, uint32_t out_pos, uint32_t member,
                               StreamRecord& rec, uint32_t* next) {
    if (wrap == kWrapRaw) return kInfEnd;
    if (wrap == kWrapZlib) {
        if (n - q < 4 || q > n) return kInfNeedInput;
        rec.expect = be32_at(p + q); rec.checked = out_pos; rec.has_check = 1;
        return kInfEnd;
    }
    if (q > n || n - q < 4) return kInfNeedInput;
    rec.expect = crc_combine(rec.expect, le32_at(p + q), member); rec.checked = out_pos; rec.has_check = 1;
    if (n - q < 8) return kInfNeedInput;
    if (le32_at(p + q + 4) != member) return kStrLength;
    *next = q + 8;
    return kInfRunning;
}

// Behind the zero bytes that follow a gzip member (q = the first non-zero byte, or n): the end of the stream, another member
// (kInfRunning, *body), or TRAILING.
ZWZ_HD uint32_t gzip_next_member(const uint8_t* p, uint32_t n, uint32_t q, uint32_t* body) {
    if (q >= n) return kInfEnd;
    if (n - q < 2 || p[q] != 0x1fu || p[q + 1] != 0x8bu) return kStrTrailing;
    return gzip_header(p, n, q, body);
}

// ---- Adler-32 (RFC 1950) as sums a workgroup can split ---------------------------------------------------------------------------
// Over bytes b_0 .. b_{n-1}:  A = 1 + S0,  B = n + n S0 - S1  (mod 65521)  with  S0 = sum b_i,  S1 = sum i b_i.
// Both sums are plain sums over the bytes, so any lane may take any 16-byte vector: vector v adds its byte sum s and
// 16 v s + sum_j j b_{16v+j} to S1.  Lanes reduce mod 65521 after every vector (zlib's NMAX rule, for one vector: the terms stay far
// below 2^32) and their sums are added.
constexpr uint32_t kAdlerMod = 65521u;

// one 16-byte vector at byte position `at` (four little-endian words): its contribution to (S0, S1), both < 65521
ZWZ_HD void adler_vec16(uint32_t at, uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t& s0, uint32_t& s1) {
    const uint32_t w[4] = {w0, w1, w2, w3};
    uint32_t s = 0, sj = 0;
#pragma unroll
    for (uint32_t q = 0; q < 4; q++)
#pragma unroll
        for (uint32_t i = 0; i < 4; i++) { const uint32_t b = (w[q] >> (8u * i)) & 255u; s += b; sj += (4u * q + i) * b; }
    s0 = (s0 + s) % kAdlerMod;
    s1 = (s1 + (at % kAdlerMod) * s + sj) % kAdlerMod;             // < 65521 * 4080 + 30600 + 65521 < 2^32
}

ZWZ_HD void adler_bytes(uint32_t at, const uint8_t* p, uint32_t n, uint32_t& s0, uint32_t& s1) {
    for (uint32_t i = 0; i < n; i++) { s0 = (s0 + p[i]) % kAdlerMod; s1 = (s1 + ((at + i) % kAdlerMod) * p[i]) % kAdlerMod; }
}

// the Adler-32 of n bytes from the sums (each < 65521)
ZWZ_HD uint32_t adler_finish(uint32_t s0, uint32_t s1, uint32_t n) {
    const uint32_t nm = n % kAdlerMod;
    const uint32_t a = (1u + s0) % kAdlerMod;
    const uint32_t b = (nm + (uint32_t)(((uint64_t)nm * s0) % kAdlerMod) + kAdlerMod - s1) % kAdlerMod;
    return b << 16 | a;
}

// the final status of a stream: a checksum that does not hold over the checked members beats any later stop
ZWZ_HD uint32_t stream_verdict(const StreamRecord& r, uint32_t actual) {
    return r.has_check && actual != r.expect ? (uint32_t)kStrChecksum : r.status;
}

}  // namespace zwz
