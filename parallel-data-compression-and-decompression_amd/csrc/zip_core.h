// zip_core.h -- the ZIP container (APPNOTE 6.3.x: local headers, central directory, end records, ZIP64) as arithmetic on bytes.
//
// Portable (host + device), so that a CPU build (tests/emu_zip) checks every record against a reference writer and the parse
// against Python's zipfile.  What is fixed here so that an archive's bytes are a function of its entries alone:
//   local header    PK\3\4 | needed | flags | method 8 | time | date | CRC | csize | usize | name length | extra length | name | extra
//   needed          20; 45 in a record that carries a ZIP64 extra field
//   flags           0x0800 (UTF-8) iff a name byte is >= 0x80
//   big entry       csize or usize >= 0xFFFFFFFF: both 32-bit sizes are 0xFFFFFFFF and the local extra is 01 00 10 00 | usize | csize
//   central record  PK\1\2 | made-by 0x032D (Unix, 4.5) | the same fields | comment 0 | disk 0 | internal 0 | external | header offset;
//                   the offset saturated with its own ZIP64 field when >= 0xFFFFFFFF; the extra holds only the saturated fields, in
//                   the order usize, csize, offset
//   end records     ZIP64 end record (PK\6\6, size 44, made-by 0x032D, needed 45) + locator when the count >= 0xFFFF or the
//                   directory's size or offset >= 0xFFFFFFFF; the classic end record's fields saturated with min
// `force64` makes every entry big, every offset saturated and the ZIP64 end records present (the context option "zip_force_zip64").
#pragma once
#include <stddef.h>

#include "zwz_common.h"

namespace zwz {

constexpr uint32_t kZipLocalFixed = 30, kZipCentralFixed = 46, kZipEndBytes = 22, kZip64EndBytes = 56, kZip64LocatorBytes = 20;
constexpr uint32_t kZipSat32 = 0xffffffffu, kZipSat16 = 0xffffu;
constexpr uint32_t kZipMadeBy = 0x032du;
constexpr uint32_t kZipTile = 65280;          // bytes of one copy tile and of one CRC tile: a multiple of 16 (dstream_core.h's kPieceBytes)
constexpr uint32_t kZipMaxComment = 65535;
constexpr uint16_t kZipDefaultDate = 0x0021;  // 1980-01-01
constexpr uint32_t kZipDefaultAttr = 0100644u << 16;

// What a record is written from.  name_len 1..65535.
struct ZipRec {
    uint64_t csize, usize, offset;
    uint32_t crc, attr, name_len;
    uint16_t flags, time, date;
    uint32_t force64;
};

ZWZ_HD bool zip_big(const ZipRec& r) { return r.force64 || r.csize >= kZipSat32 || r.usize >= kZipSat32; }
ZWZ_HD bool zip_off_sat(const ZipRec& r) { return r.force64 || r.offset >= kZipSat32; }
ZWZ_HD uint32_t zip_local_extra(bool big) { return big ? 20u : 0u; }
ZWZ_HD uint32_t zip_central_extra(bool big, bool off_sat) { return big || off_sat ? 4u + (big ? 16u : 0u) + (off_sat ? 8u : 0u) : 0u; }
ZWZ_HD uint32_t zip_local_bytes(uint32_t name_len, bool big) { return kZipLocalFixed + name_len + zip_local_extra(big); }
ZWZ_HD uint32_t zip_central_bytes(uint32_t name_len, bool big, bool off_sat) { return kZipCentralFixed + name_len + zip_central_extra(big, off_sat); }
ZWZ_HD bool zip_end64(uint64_t n, uint64_t cd_size, uint64_t cd_off, bool force64) { return force64 || n >= kZipSat16 || cd_size >= kZipSat32 || cd_off >= kZipSat32; }
ZWZ_HD uint32_t zip_end_bytes(bool end64) { return (end64 ? kZip64EndBytes + kZip64LocatorBytes : 0u) + kZipEndBytes; }
ZWZ_HD uint16_t zip_name_flags(const uint8_t* name, uint32_t len) {
    for (uint32_t i = 0; i < len; i++) if (name[i] >= 0x80u) return 0x0800u;
    return 0;
}
// The most an entry under a name of name_len bytes can need beyond its data: both headers with every ZIP64 field
ZWZ_HD uint64_t zip_entry_overhead(uint32_t name_len) { return (uint64_t)kZipLocalFixed + 20u + kZipCentralFixed + 28u + 2ull * name_len; }

ZWZ_HD void zip_put16(uint8_t* p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); }
ZWZ_HD void zip_put32(uint8_t* p, uint32_t v) { zip_put16(p, v); zip_put16(p + 2, v >> 16); }
ZWZ_HD void zip_put64(uint8_t* p, uint64_t v) { zip_put32(p, (uint32_t)v); zip_put32(p + 4, (uint32_t)(v >> 32)); }
ZWZ_HD uint32_t zip_get16(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
ZWZ_HD uint32_t zip_get32(const uint8_t* p) { return zip_get16(p) | zip_get16(p + 2) << 16; }
ZWZ_HD uint64_t zip_get64(const uint8_t* p) { return (uint64_t)zip_get32(p) | (uint64_t)zip_get32(p + 4) << 32; }

// The local header's 30 fixed bytes at p and its extra at p + 30 + name_len; the name is the caller's to copy.  Returns the header's length.
ZWZ_HD uint32_t zip_write_local(uint8_t* p, const ZipRec& r) {
    const bool big = zip_big(r);
    zip_put32(p, 0x04034b50u);
    zip_put16(p + 4, big ? 45u : 20u);
    zip_put16(p + 6, r.flags);
    zip_put16(p + 8, 8u);
    zip_put16(p + 10, r.time);
    zip_put16(p + 12, r.date);
    zip_put32(p + 14, r.crc);
    zip_put32(p + 18, big ? kZipSat32 : (uint32_t)r.csize);
    zip_put32(p + 22, big ? kZipSat32 : (uint32_t)r.usize);
    zip_put16(p + 26, r.name_len);
    zip_put16(p + 28, zip_local_extra(big));
    if (big) {
        uint8_t* x = p + kZipLocalFixed + r.name_len;
        zip_put16(x, 1u); zip_put16(x + 2, 16u); zip_put64(x + 4, r.usize); zip_put64(x + 12, r.csize);
    }
    return zip_local_bytes(r.name_len, big);
}

// The central record's 46 fixed bytes at p and its extra at p + 46 + name_len.  Returns the record's length.
ZWZ_HD uint32_t zip_write_central(uint8_t* p, const ZipRec& r) {
    const bool big = zip_big(r), sat = zip_off_sat(r);
    const uint32_t extra = zip_central_extra(big, sat);
    zip_put32(p, 0x02014b50u);
    zip_put16(p + 4, kZipMadeBy);
    zip_put16(p + 6, extra ? 45u : 20u);
    zip_put16(p + 8, r.flags);
    zip_put16(p + 10, 8u);
    zip_put16(p + 12, r.time);
    zip_put16(p + 14, r.date);
    zip_put32(p + 16, r.crc);
    zip_put32(p + 20, big ? kZipSat32 : (uint32_t)r.csize);
    zip_put32(p + 24, big ? kZipSat32 : (uint32_t)r.usize);
    zip_put16(p + 28, r.name_len);
    zip_put16(p + 30, extra);
    zip_put16(p + 32, 0u);        // comment
    zip_put16(p + 34, 0u);        // disk
    zip_put16(p + 36, 0u);        // internal attributes
    zip_put32(p + 38, r.attr);
    zip_put32(p + 42, sat ? kZipSat32 : (uint32_t)r.offset);
    if (extra) {
        uint8_t* x = p + kZipCentralFixed + r.name_len;
        zip_put16(x, 1u); zip_put16(x + 2, extra - 4u);
        x += 4;
        if (big) { zip_put64(x, r.usize); zip_put64(x + 8, r.csize); x += 16; }
        if (sat) zip_put64(x, r.offset);
    }
    return kZipCentralFixed + r.name_len + extra;
}

// The end records behind a directory of n records, cd_size bytes at cd_off.  Returns their length (22 or 98).
ZWZ_HD uint32_t zip_write_end(uint8_t* p, uint64_t n, uint64_t cd_size, uint64_t cd_off, bool force64) {
    const bool e64 = zip_end64(n, cd_size, cd_off, force64);
    if (e64) {
        zip_put32(p, 0x06064b50u); zip_put64(p + 4, 44u); zip_put16(p + 12, kZipMadeBy); zip_put16(p + 14, 45u);
        zip_put32(p + 16, 0u); zip_put32(p + 20, 0u);
        zip_put64(p + 24, n); zip_put64(p + 32, n); zip_put64(p + 40, cd_size); zip_put64(p + 48, cd_off);
        p += kZip64EndBytes;
        zip_put32(p, 0x07064b50u); zip_put32(p + 4, 0u); zip_put64(p + 8, cd_off + cd_size); zip_put32(p + 16, 1u);
        p += kZip64LocatorBytes;
    }
    const uint32_t n16 = n < kZipSat16 ? (uint32_t)n : kZipSat16;
    zip_put32(p, 0x06054b50u); zip_put16(p + 4, 0u); zip_put16(p + 6, 0u); zip_put16(p + 8, n16); zip_put16(p + 10, n16);
    zip_put32(p + 12, cd_size < kZipSat32 ? (uint32_t)cd_size : kZipSat32);
    zip_put32(p + 16, cd_off < kZipSat32 ? (uint32_t)cd_off : kZipSat32);
    zip_put16(p + 20, 0u);
    return zip_end_bytes(e64);
}

// ---- names and times --------------------------------------------------------------------------------------------------------------
// A name that may be created below a destination directory: not empty, not absolute, no `..` component, no backslash, no NUL.
// (`.` and empty components are harmless: the file system folds them.)
ZWZ_HD bool zip_name_ok(const uint8_t* s, uint32_t n) {
    if (!n || s[0] == '/') return false;
    uint32_t start = 0;
    for (uint32_t i = 0; i <= n; i++) {
        if (i < n && (s[i] == '\\' || s[i] == 0)) return false;
        if (i == n || s[i] == '/') {
            if (i - start == 2 && s[start] == '.' && s[start + 1] == '.') return false;
            start = i + 1;
        }
    }
    return true;
}

// Broken-down local time (year as written, month 1..12) -> MS-DOS time and date as zipfile and Info-ZIP store them: the year clamped
// to 1980..2107 (a time before 1980 becomes 1980-01-01 00:00:00, one after 2107 becomes 2107-12-31 23:59:58), seconds halved.
ZWZ_HD void zip_dos_time(int year, int mon, int day, int hour, int min, int sec, uint16_t* time, uint16_t* date) {
    if (year < 1980) { year = 1980; mon = 1; day = 1; hour = 0; min = 0; sec = 0; }
    if (year > 2107) { year = 2107; mon = 12; day = 31; hour = 23; min = 59; sec = 59; }
    *date = (uint16_t)((year - 1980) << 9 | mon << 5 | day);
    *time = (uint16_t)(hour << 11 | min << 5 | sec >> 1);
}
ZWZ_HD void zip_dos_untime(uint16_t time, uint16_t date, int* year, int* mon, int* day, int* hour, int* min, int* sec) {
    *year = 1980 + (date >> 9); *mon = (date >> 5) & 15; *day = date & 31;
    *hour = time >> 11; *min = (time >> 5) & 63; *sec = (time & 31) * 2;
}

// ---- the parse (host) -------------------------------------------------------------------------------------------------------------
// One central-directory record as read; the layout of include/zwz.h's zwz_zip_entry.
struct ZipEntry {
    uint64_t header_off, data_off, csize, usize, name_off;
    uint32_t crc32, external_attr;
    uint16_t name_len, method, flags, dos_time, dos_date, made_by;
};
struct ZipParseError { const char* what; uint64_t entry, offset; };      // entry ~0: none

enum : int { kZipParseOk = 0, kZipParseFormat = 1, kZipParseCap = 2 };

// An archive in memory as zip_parse's source.  A source hands out `len` bytes at `off` (inside the archive: the parse checks every
// range first), valid until the next call.
struct ZipMem {
    const uint8_t* z;
    const uint8_t* at(uint64_t off, uint64_t) const { return z + off; }
};

// Walks an archive of n bytes: the end record behind a comment of up to 65535 bytes, the ZIP64 locator and record, every central
// record with its ZIP64 extra field, every local header.  e may be null (count only); with cap < *count entries kZipParseCap.
template <class Src>
inline int zip_parse(Src& S, uint64_t n, ZipEntry* e, uint64_t cap, uint64_t* count, ZipParseError* err) {
    auto fail = [&](const char* what, uint64_t entry, uint64_t off) { err->what = what; err->entry = entry; err->offset = off; return (int)kZipParseFormat; };
    const uint64_t none = ~0ull;
    *count = 0;
    if (n < kZipEndBytes) return fail("no end record", none, 0);
    // the rightmost end record whose comment ends exactly at the archive's end
    uint64_t eo = none;
    const uint64_t tail_len = n < kZipMaxComment + kZipEndBytes + kZip64LocatorBytes ? n : kZipMaxComment + kZipEndBytes + kZip64LocatorBytes;
    const uint64_t tail_at = n - tail_len;
    const uint8_t* z = S.at(tail_at, tail_len) - tail_at;          // (indexed by archive offsets, from tail_at on)
    for (uint64_t back = 0; back <= kZipMaxComment && back + kZipEndBytes <= n; back++) {
        const uint64_t p = n - kZipEndBytes - back;
        if (zip_get32(z + p) == 0x06054b50u && zip_get16(z + p + 20) == back) { eo = p; break; }
    }
    if (eo == none) return fail("no end record", none, n);
    if (zip_get16(z + eo + 4) != 0 || zip_get16(z + eo + 6) != 0) return fail("a disk number other than 0", none, eo);
    uint64_t total = zip_get16(z + eo + 10), here = zip_get16(z + eo + 8), cd_size = zip_get32(z + eo + 12), cd_off = zip_get32(z + eo + 16);
    uint64_t cd_end = eo;
    const bool has_loc = eo >= kZip64LocatorBytes && zip_get32(z + eo - kZip64LocatorBytes) == 0x07064b50u;
    if (has_loc) {
        const uint64_t lo = eo - kZip64LocatorBytes;
        if (zip_get32(z + lo + 4) != 0 || zip_get32(z + lo + 16) > 1u) return fail("a disk number other than 0", none, lo);
        const uint64_t ro = zip_get64(z + lo + 8);
        if (ro > lo || lo - ro < kZip64EndBytes) return fail("the ZIP64 end record runs past the archive", none, lo);
        z = S.at(ro, kZip64EndBytes) - ro;
        if (zip_get32(z + ro) != 0x06064b50u) return fail("wrong signature of the ZIP64 end record", none, ro);
        const uint64_t rsize = zip_get64(z + ro + 4);
        if (rsize < 44u || rsize > lo - ro - 12u || ro + 12u + rsize != lo) return fail("the ZIP64 end record does not end at its locator", none, ro);
        if (zip_get32(z + ro + 16) != 0 || zip_get32(z + ro + 20) != 0) return fail("a disk number other than 0", none, ro);
        here = zip_get64(z + ro + 24); total = zip_get64(z + ro + 32); cd_size = zip_get64(z + ro + 40); cd_off = zip_get64(z + ro + 48);
        cd_end = ro;
    } else if (total == kZipSat16 || here == kZipSat16 || cd_size == kZipSat32 || cd_off == kZipSat32) {
        return fail("saturated end record without a ZIP64 locator", none, eo);
    }
    if (here != total) return fail("a disk number other than 0", none, eo);
    if (cd_size > cd_end) return fail("the central directory runs past the archive", none, eo);
    if (cd_off != cd_end - cd_size) return fail("the stated directory offset is not where the directory is (prepended data is not supported)", none, cd_end - cd_size);
    if (total > cd_size / kZipCentralFixed) return fail("the entry count disagrees with the records present", none, cd_off);
    *count = total;
    const bool store = e != nullptr && cap >= total;
    uint64_t p = cd_off;
    for (uint64_t i = 0; i < total; i++) {
        if (cd_end - p < kZipCentralFixed) return fail("the entry count disagrees with the records present", i, p);
        const uint8_t* z = S.at(p, kZipCentralFixed) - p;
        if (zip_get32(z + p) != 0x02014b50u) return fail("wrong signature of a central record", i, p);
        const uint32_t nlen = zip_get16(z + p + 28), xlen = zip_get16(z + p + 30), clen = zip_get16(z + p + 32);
        if ((uint64_t)nlen + xlen + clen > cd_end - p - kZipCentralFixed) return fail("a central record runs past the directory", i, p);
        ZipEntry r;
        r.made_by = (uint16_t)zip_get16(z + p + 4); r.flags = (uint16_t)zip_get16(z + p + 8); r.method = (uint16_t)zip_get16(z + p + 10);
        r.dos_time = (uint16_t)zip_get16(z + p + 12); r.dos_date = (uint16_t)zip_get16(z + p + 14);
        r.crc32 = zip_get32(z + p + 16); r.csize = zip_get32(z + p + 20); r.usize = zip_get32(z + p + 24);
        r.name_len = (uint16_t)nlen; r.name_off = p + kZipCentralFixed;
        const uint32_t disk = zip_get16(z + p + 34);
        r.external_attr = zip_get32(z + p + 38); r.header_off = zip_get32(z + p + 42);
        // the ZIP64 field holds the saturated values only, in this order
        const uint8_t* x = S.at(p + kZipCentralFixed + nlen, xlen);
        for (uint32_t q = 0; q + 4u <= xlen;) {
            const uint32_t id = zip_get16(x + q), sz = zip_get16(x + q + 2);
            if (sz > xlen - q - 4u) return fail("an extra field runs past its record", i, p + kZipCentralFixed + nlen + q);
            if (id == 1u) {
                uint32_t k = 0;
                const uint8_t* f = x + q + 4;
                if (r.usize == kZipSat32) { if (k + 8u > sz) return fail("a ZIP64 extra field is too short", i, p); r.usize = zip_get64(f + k); k += 8; }
                if (r.csize == kZipSat32) { if (k + 8u > sz) return fail("a ZIP64 extra field is too short", i, p); r.csize = zip_get64(f + k); k += 8; }
                if (r.header_off == kZipSat32) { if (k + 8u > sz) return fail("a ZIP64 extra field is too short", i, p); r.header_off = zip_get64(f + k); k += 8; }
            }
            q += 4u + sz;
        }
        if (disk != 0 && disk != kZipSat16) return fail("a disk number other than 0", i, p);
        if (r.header_off > cd_off || cd_off - r.header_off < kZipLocalFixed) return fail("a local header outside the archive's data", i, r.header_off);
        const uint8_t* l = S.at(r.header_off, kZipLocalFixed);
        if (zip_get32(l) != 0x04034b50u) return fail("wrong signature of a local header", i, r.header_off);
        r.data_off = r.header_off + kZipLocalFixed + zip_get16(l + 26) + zip_get16(l + 28);
        if (r.data_off > cd_off || r.csize > cd_off - r.data_off) return fail("an entry's data outside the archive's data", i, r.data_off);
        if (store) e[i] = r;
        p += kZipCentralFixed + nlen + xlen + clen;
    }
    if (p != cd_end) return fail("the entry count disagrees with the records present", total, p);
    return e != nullptr && cap < total ? (int)kZipParseCap : (int)kZipParseOk;
}

}  // namespace zwz
