// split_core.h -- the portable half of zwz_inflate_split_streams_dev: a long stream with full-flush points is decoded by one wave per
// piece between two of them.  Host + device, so that a CPU build (tests/emu_split) runs the device's decomposition step by step.
//
// A flush writes an empty stored block -- three header bits, padding to a byte, LEN / NLEN = 00 00 ff ff -- so the byte behind every
// flush is a byte-aligned block start that the four bytes in front of it give away.  After a FULL flush nothing refers back across
// it.  The method splits only there:
//   scan      a CANDIDATE is the body's first byte and every body offset p with bytes [p - 4, p) = 00 00 ff ff.  False ones (the
//             pattern in stored data or Huffman bits) are expected.
//   measure   one wave per candidate decodes from p with an empty window and only counts output.  It stops behind the first
//             non-final empty stored block (kSegFlush), behind a final block (kSegFinal), or for any other reason (kSegBad: an
//             error, a match that reaches before p's own first output byte, the end of the input or of the budget).
//   resolve   the CHAIN of a stream starts at the body and goes from each kSegFlush segment to the candidate at its end (which always
//             exists: the segment ends in the marker).  Only starts on the chain are true block starts; the other candidates'
//             results are dropped.  A stream SPLITS if its chain ends in kSegFinal with a fine trailer, has at least two segments
//             and its counts add up to at most the capacity.  Everything else is decoded by the one-wave path, untouched.
//   decode    one wave per chain segment writes its bytes at the exclusive sum of the counts in front of it.
#pragma once
#include "stream_core.h"

namespace zwz {

enum SegKind : uint32_t { kSegBad = 0, kSegFlush = 1, kSegFinal = 2 };
// What a measuring wave leaves: how it stopped, the stream offset of the byte behind its last block (kSegFlush: the next chain
// candidate; kSegFinal: where the trailer starts), the bytes it would have written, the decoder's status -- which says nothing of
// a segment that ended at its final block, so there the word holds the final block's end bit within its byte (0: on a boundary).
struct SegMeasure { uint32_t kind, end, count, status; };
ZWZ_HD uint32_t split_measure_word(uint32_t kind, uint32_t bit_pos, uint32_t status) { return kind == 2u /* kSegFinal */ ? bit_pos & 7u : status; }
// The first bit behind the final block, from a kSegFinal measurement's `end` and that word
ZWZ_HD uint64_t split_final_end_bit(uint64_t end, uint32_t low3) { return low3 ? 8u * (end - 1u) + low3 : 8u * end; }

// Defaults of the context options "split_min_bytes", "split_budget" and "split_max_candidates" 
constexpr uint32_t kSplitMinBytes = 65536;          // a shorter stream is not scanned: one wave is through it in about 2 ms
constexpr uint32_t kSplitBudget = 4u << 20;         // input bytes a measuring wave may read: above any piece a 1 MiB flush interval writes
constexpr uint32_t kSplitMaxCandidates = 1u << 17;  // per stream: 2^32 output bytes in pieces of 65 280 are 65 794 segments
constexpr uint32_t kSplitSliceBytes = 64u << 20;    // "split_slice_bytes": compressed bytes zwz_inflate_stream_file holds on the device at a time
constexpr uint32_t kSplitMaxTrailing = 4096;        // zero bytes behind a gzip trailer that the split path looks through itself
constexpr uint32_t kSplitTile = 4096;               // input bytes per scan workgroup: 256 lanes, 16 bytes each
constexpr uint32_t kSplitNil = 0xffffffffu;
constexpr uint32_t kSplitMeasureCap = 0xfffffff0u;  // the measuring form's output bound: a count that would pass it ends the segment as kSegBad

constexpr uint32_t kSplitMarkerWord = 0xffff0000u;  // 00 00 ff ff read as a little-endian word

// Candidates among the 16 stream offsets [o, o + 16), o a multiple of 16, as a bit mask.  w[0] is the little-endian word at o - 4
// (anything for o = 0), w[1..4] the vector at o.  Offset p counts if p == body, or p >= body + 4 with the marker at [p - 4, p);
// always p < n.
ZWZ_HD uint32_t split_candidate_mask(const uint32_t w[5], uint32_t o, uint32_t body, uint32_t n) {
    uint32_t mask = 0;
    for (uint32_t j = 0; j < 16; j++) {
        const uint32_t p = o + j, q = j >> 2, r = j & 3u;
        const uint32_t word = r ? (w[q] >> (8u * r)) | (w[q + 1] << (32u - 8u * r)) : w[q];
        const bool hit = p == body || (p >= body + 4u && word == kSplitMarkerWord);
        if (hit && p < n) mask |= 1u << j;
    }
    return mask;
}

// The stop rule of the measuring and the segment form, asked after every block that ended with the decoder still running: `last` the
// block's BFINAL, `stored_empty` whether it was a stored block with LEN = 0.
ZWZ_HD uint32_t split_stop(uint32_t last, bool stored_empty) { return last ? kSegFinal : stored_empty ? kSegFlush : kSegBad; }

// The input a wave that starts at stream offset p sees: from p rounded down to 16 (the kernels read whole vectors), the body offset
// p & 15, and -- measuring -- at most `budget` bytes from p on.
ZWZ_HD uint32_t split_wave_input(uint32_t p, uint32_t n, uint32_t budget) {
    const uint64_t left = n - (p & ~15u), want = (uint64_t)(p & 15u) + budget;
    return (uint32_t)(want < left ? want : left);
}

// Index of the candidate at stream offset `target` in the ascending offsets pos[lo, hi), or kSplitNil
ZWZ_HD uint32_t split_find(const uint32_t* pos, uint32_t lo, uint32_t hi, uint32_t target) {
    const uint32_t end = hi;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (pos[mid] < target) lo = mid + 1u; else hi = mid;
    }
    return lo < end && pos[lo] == target ? lo : kSplitNil;
}

// Levels of pointer jumping that reach every node of a chain of at most `count` nodes from its head: 2^levels > count - 1
ZWZ_HD uint32_t split_levels(uint32_t count) {
    uint32_t d = 1;
    while (d < 31u && (1u << d) < count) d++;
    return d;
}

// What follows the chain's final block at stream offset q: the wrapper's trailer, judged by stream_trailer, and for gzip nothing but
// at most kSplitMaxTrailing zero bytes.  True if the stream may commit to the split result; *expect = the stored checksum.
ZWZ_HD bool split_trailer_ok(uint32_t wrap, const uint8_t* p, uint32_t n, uint32_t q, uint32_t total, uint32_t* expect) {
    StreamRecord rec{0, 0, 0, kInfRunning};
    uint32_t next = 0;
    const uint32_t st = stream_trailer(wrap, p, n, q, total, total, rec, &next);
    *expect = rec.expect;
    if (wrap != kWrapGzip) return st == kInfEnd;
    if (st != kInfRunning || n - next > kSplitMaxTrailing) return false;
    for (uint32_t i = next; i < n; i++) if (p[i]) return false;
    return true;
}

// Whether a stream is scanned at all (the rest is the existing path's: too large, too short, a header verdict other than "fine", zeros
// in front of a gzip member); *body = the first byte of the DEFLATE data.
ZWZ_HD bool split_eligible(uint32_t wrap, const uint8_t* p, uint64_t n, uint64_t cap, uint32_t min_bytes, uint32_t* body) {
    *body = 0;
    if (n >= kStreamMaxIn || cap >= kStreamMaxOut || n < min_bytes || n == 0) return false;
    return stream_begin(wrap, p, (uint32_t)n, p[0] ? 0u : (uint32_t)n, body) == kInfRunning && *body < n;
}

// One wave's work, sequentially (the device runs the same state machine in inflate_kernel's split forms): decode from stream offset p
// with an empty window until the stop rule says so.  out == nullptr measures; otherwise the bytes go to out[0, cap) and the count
// may not pass cap.  `in` is the stream, n its length (already clipped to the budget when measuring).
inline SegMeasure split_run(const uint8_t* in, uint32_t n, uint32_t p, uint8_t* out, uint32_t cap) {
    InflateState st;
    static thread_local InflateTables t;
    uint8_t lens[320];
    uint32_t batch[kBatch], pos[kBatch];
    st.br.init(in, n); st.out_pos = 0; st.last = 0; st.status = kInfRunning;
    st.br.seek_bit(p * 8u);
    uint32_t kind = kSegBad;
    while (st.status == kInfRunning) {
        uint32_t src = 0, len = 0;
        const uint32_t blk = inflate_block_header(st, t, lens, src, len);
        if (blk == kBlkStop) break;
        if (blk == kBlkStored) {
            const uint32_t cp = len < cap - st.out_pos ? len : cap - st.out_pos;
            if (out) for (uint32_t i = 0; i < cp; i++) out[st.out_pos + i] = in[src + i];
            st.out_pos += cp;
            if (cp < len) st.status = kInfOverflow;
        } else {
            bool done = false;
            while (!done) {
                const uint32_t k = inflate_decode_batch<false, true>(st, t, cap, batch, pos, done, kBatch, 0);
                if (out) for (uint32_t i = 0; i < k; i++) {
                    if (batch[i] < 256) out[pos[i]] = (uint8_t)batch[i];
                    else for (uint32_t j = 0, l = batch[i] >> 16, d = batch[i] & 0xffff; j < l; j++) out[pos[i] + j] = out[pos[i] + j - d];
                }
            }
        }
        if (st.status != kInfRunning) break;
        kind = split_stop(st.last, blk == kBlkStored && len == 0);
        if (kind != kSegBad) break;
    }
    return SegMeasure{kind, (st.br.bit_pos() + 7u) >> 3, st.out_pos, st.status};
}

}  // namespace zwz
