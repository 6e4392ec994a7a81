// Host build of csrc/split_core.h on inflate_core.h and stream_core.h for tests/test_inflate_split_cpu.py (g++ -shared; no HIP):
// zwz_inflate_split_streams_dev's decomposition run sequentially -- head, scan (16 bytes a "lane"), the candidate ceiling, one
// measuring run per candidate under the budget, link, pointer jumping and marks level by level, resolve with the trailer, one decode
// per chain segment into its place, the checksum from 65 280-byte pieces joined with dstream_core.h's sums -- and, for every stream
// that does not split, the one-wave path of tests/emu_stream.
#include <string.h>

#include <vector>

#include "../../parallel-data-compression-and-decompression_amd/csrc/dstream_core.h"
#include "../../parallel-data-compression-and-decompression_amd/csrc/split_core.h"
#include "../emu_stream/stream_emu.cpp"

using namespace zwz;

namespace {

template <class Sum>
uint32_t joined(const uint8_t* out, uint32_t total, bool crc) {
    uint32_t acc = Sum::identity();
    for (uint64_t at = 0; at < total; at += kPieceBytes) {
        const uint32_t len = (uint32_t)(total - at < kPieceBytes ? total - at : kPieceBytes);
        const uint32_t v = crc ? crc_lanes_host(out + at, len, 256) : adler_lanes(out + at, len, 256);
        acc = Sum::join(acc, v, Sum::pof(len));
    }
    return acc;
}

}  // namespace

extern "C" {

// One stream: the final status; *out_len = decoded length; *segments = chain segments decoded one by one, 0 if the stream fell back;
// *candidates = what the scan found (0 for a stream that is not scanned).
uint32_t emu_inflate_split(uint32_t wrap, const uint8_t* in_, uint64_t n64, uint8_t* out, uint64_t cap64, uint64_t* out_len, uint32_t* segments,
                           uint32_t* candidates, uint32_t min_bytes, uint32_t budget, uint32_t max_candidates) {
    *segments = 0; *candidates = 0;
    auto fall_back = [&] { return emu_inflate_stream(wrap, in_, n64, out, cap64, out_len); };
    // (the device reads whole 16-byte vectors: the stream is readable up to its length rounded up to 16)
    std::vector<uint8_t> padded((size_t)((n64 < kStreamMaxIn ? n64 : 0) + 31) & ~(size_t)15, 0);
    if (n64 < kStreamMaxIn && n64) memcpy(padded.data(), in_, n64);
    const uint8_t* in = padded.data();
    uint32_t body = 0;
    if (!split_eligible(wrap, in, n64, cap64, min_bytes, &body)) return fall_back();
    const uint32_t n = (uint32_t)n64;
    // scan
    std::vector<uint32_t> pos;
    for (uint32_t o = 0; o < ((n + 15u) & ~15u); o += 16) {
        uint32_t w[5] = {0, 0, 0, 0, 0};
        if (o) memcpy(&w[0], in + o - 4, 4);
        memcpy(&w[1], in + o, 16);
        uint32_t mask = split_candidate_mask(w, o, body, n);
        for (uint32_t j = 0; j < 16; j++) if (mask >> j & 1u) pos.push_back(o + j);
    }
    *candidates = (uint32_t)pos.size();
    const uint32_t m = (uint32_t)pos.size();
    if (m < 2 || m > max_candidates) return fall_back();
    // measure: every candidate, from its own 16-byte aligned base as the device's waves start
    std::vector<SegMeasure> meas(m);
    for (uint32_t k = 0; k < m; k++) {
        const uint32_t base = pos[k] & ~15u;
        meas[k] = split_run(in + base, split_wave_input(pos[k], n, budget), pos[k] & 15u, nullptr, kSplitMeasureCap);
        meas[k].end += base;
    }
    // link, jump, mark
    const uint32_t levels = split_levels(m);
    std::vector<uint32_t> jump((size_t)levels * m), mark(m, 0);
    for (uint32_t k = 0; k < m; k++) jump[k] = meas[k].kind == kSegFlush ? split_find(pos.data(), 0, m, meas[k].end) : kSplitNil;
    for (uint32_t d = 1; d < levels; d++)
        for (uint32_t k = 0; k < m; k++) { const uint32_t a = jump[(size_t)(d - 1) * m + k]; jump[(size_t)d * m + k] = a == kSplitNil ? kSplitNil : jump[(size_t)(d - 1) * m + a]; }
    mark[0] = 1;
    for (uint32_t d = levels; d-- > 0;) {
        const std::vector<uint32_t> seen(mark);                     // (one launch: marks of this level come from the level above)
        for (uint32_t k = 0; k < m; k++) if (seen[k] && jump[(size_t)d * m + k] != kSplitNil) mark[jump[(size_t)d * m + k]] = 1;
    }
    // resolve
    uint64_t total = 0;
    uint32_t nseg = 0, last = 0;
    std::vector<uint32_t> ostart(m, 0);
    for (uint32_t k = 0; k < m; k++) if (mark[k]) { ostart[k] = (uint32_t)(total < kSplitMeasureCap ? total : kSplitMeasureCap); total += meas[k].count; nseg++; last = k; }
    uint32_t expect = 0;
    bool ok = meas[last].kind == kSegFinal && nseg >= 2 && total <= cap64 && total < kSplitMeasureCap - 16u;
    if (ok) ok = split_trailer_ok(wrap, in, n, meas[last].end, (uint32_t)total, &expect);
    if (!ok) return fall_back();
    // decode: a segment's wave sees its input up to the byte behind its last block and may write its own bytes only
    for (uint32_t k = 0; k < m; k++) {
        if (!mark[k]) continue;
        const uint32_t base = pos[k] & ~15u;
        const SegMeasure r = split_run(in + base, meas[k].end - base, pos[k] & 15u, out + ostart[k], meas[k].count);
        if (r.kind == kSegBad || r.count != meas[k].count) { *out_len = (uint32_t)total; *segments = nseg; return kInfDataError; }
    }
    *out_len = total; *segments = nseg;
    if (wrap == kWrapRaw) return kInfEnd;
    const uint32_t actual = wrap == kWrapGzip ? joined<CrcSum>(out, (uint32_t)total, true) : joined<AdlerSum>(out, (uint32_t)total, false);
    return actual != expect ? (uint32_t)kStrChecksum : (uint32_t)kInfEnd;
}

}  // extern "C"
