// zwz_zip.h -- ZIP archives: the kernels that frame a batch of raw DEFLATE streams as one archive and take one apart
// (zwz_zip.hip) and their host driver (zwz_zip.cpp).  zip_core.h has the format.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "zwz_bgzf.h"

namespace zwz {

// ---- writing ----------------------------------------------------------------------------------------------------------------------
// Per entry, built on the host (n + 1 of them: the last one carries the tile count in tfirst)
struct ZipIn {
    uint64_t soff;             // the entry's gzip stream in the staging
    uint64_t name_off;         // its name in the names' bytes
    uint64_t usize;            // the input's length
    uint64_t tfirst;           // its first copy tile: entry i has max(1, ceil(bound of its raw stream / kZipTile)) tiles
    uint32_t name_len, attr;
    uint32_t time_date;        // time | date << 16
    uint32_t flags;
};
struct ZipTotals { uint64_t cd_off, cd_size, need; uint32_t ok, pad; };
struct ZipWrite {
    const ZipIn* in; const uint8_t* names; const uint8_t* stage;
    const uint64_t* glen; const uint32_t* gst;      // the gzip streams' lengths and statuses (zwz_deflate_streams_dev's results)
    uint64_t *hoff, *coff;                          // the scans: every local header's offset; every central record's, from the directory's start
    ZipTotals* tot;
    uint8_t* out; uint64_t out_cap; uint64_t* out_len; uint32_t* status;
    uint32_t n, force64, partial;                   // partial: local headers and data only; their length is the result
};
hipError_t launch_zip_scan(const ZipWrite& W, hipStream_t s);
hipError_t launch_zip_pack(const ZipWrite& W, uint32_t tiles, hipStream_t s);
hipError_t launch_zip_directory(const ZipWrite& W, hipStream_t s);

// ---- reading ----------------------------------------------------------------------------------------------------------------------
enum : uint32_t { kUnzSkip = 0, kUnzDeflated = 1, kUnzStored = 2 };
// Per entry, built on the host (n + 1: the last one carries the tile counts)
struct UnzIn {
    uint64_t src, len;         // the entry's data in the archive
    uint64_t dst;              // where the gather puts it: in the staging (deflated) or in the output (stored)
    uint64_t out_off, usize;
    uint32_t tfirst, ctfirst;  // its first copy tile (of ceil(len / kZipTile); none when skipped) and CRC tile (of ceil(usize / kZipTile))
    uint32_t kind, pre;        // kUnz*; the verdict the host already has (0: none)
    uint32_t crc, pad;
};
struct ZipRead {
    const UnzIn* in; const uint8_t* zip; uint8_t* stage; uint8_t* out;
    uint64_t* toff; uint32_t *tlen, *tcrc;          // per CRC tile, for crc32_blocks
    const uint32_t* ist;                            // inflate's statuses
    uint64_t* out_len; uint32_t* status;
    uint32_t n;
};
hipError_t launch_zip_gather(const ZipRead& R, uint32_t tiles, hipStream_t s);
hipError_t launch_zip_crc_layout(const ZipRead& R, uint32_t ctiles, hipStream_t s);
hipError_t launch_zip_verdict(const ZipRead& R, hipStream_t s);

}  // namespace zwz
