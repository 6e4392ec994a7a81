// legfile_core.h -- the portable rules of the decode in legs over a FILE (zwz_inflate_legs_file, zwz_legs_file.cpp): one
// stream of any length passes through an input window and an output window of bounded size, and what a leg has made final is COMMITTED --
// written, summed, indexed -- before the next leg reuses the windows.  Host + device: the same rules run in the host loop and in its CPU
// restatement (tests/emu_legfile); LegStage is what inflate_kernel's leg form reads when its windows lie in staging.
#pragma once
#include <vector>

#include "dstream_core.h"
#include "leg_core.h"

namespace zwz {

constexpr uint64_t kLegFileBytesDefault = 67108864u, kLegFileBytesMin = 4096u;                     // "leg_file_bytes"
constexpr uint64_t kLegFileOutBytesDefault = 268435456u, kLegFileOutBytesMin = 65536u;             // "leg_file_out_bytes"
constexpr uint64_t kLegFileOutBytesMax = kStreamMaxOut - 65536u;

// Where a leg's windows lie when they are staging and not the whole stream's ranges (sp.legf[i]; null in zwz_inflate_legs_dev): the output
// window's first byte is out + out_at, and the index array holds a header's room and `ent_slots` entries of which the first is entry
// `ent_first` of the stream -- the restart point's own, which this leg writes again.
struct LegStage { uint64_t out_at; uint32_t ent_first, ent_slots; };
static_assert(sizeof(LegStage) == 16, "LegStage layout (host and device share it)");

// The bytes a plan's windows take in staging: the input zero-padded to its length rounded up to 16, plus 16; the output with the 16 bytes
// of slack a workgroup copy may read past its source
ZWZ_HD uint64_t legfile_in_bytes(const LegPlan& w) { return (((uint64_t)w.in_len + 15u) & ~15ull) + 16u; }
ZWZ_HD uint64_t legfile_out_bytes(const LegPlan& w) { return (uint64_t)w.out_len + 16u; }
// The entries one leg can write into an output window of out_len bytes: its restart point's, then one per `span` decoded bytes at most
ZWZ_HD uint32_t legfile_entry_slots(uint32_t out_len, uint32_t span) { return out_len / span + 2u; }

// The carry: before a leg runs, decoded bytes [w.out_base, s.out) -- leg_hist(s) bytes and the 0..15 down to the 16-byte boundary -- stand at
// the head of its output window.  They lie in the window of the leg before, whose first byte was decoded byte prev_base, at *from.
ZWZ_HD uint32_t legfile_carry(const LegState& s, const LegPlan& w, uint64_t prev_base, uint64_t* from) {
    *from = w.out_base - prev_base;
    return (uint32_t)(s.out - w.out_base);
}

// What a leg that left state s has made final: the decoded bytes below the restart point after a rewound leg, below the end after a
// finished one; and the index entries below s.mk_count -- a restart point's own entry is not among them, the next leg writes it again.
ZWZ_HD uint64_t legfile_final_out(const LegState& s) { return s.done ? s.end_out : s.out; }
ZWZ_HD uint32_t legfile_final_entries(const LegState& s) { return s.mk_count; }

// The running checksum of the committed bytes.  `run` covers [0, bytes); `val` is the value at `val_at`, the latest `checked` seen.
struct LegSum { uint64_t bytes, val_at; uint32_t run, val, have; };
ZWZ_HD LegSum legfile_sum_fresh(uint32_t init) { return LegSum{0, 0, init, init, 0}; }
// Whether the range [lo, hi) about to be committed is cut at the state's `checked`: the trailer that set it was read in the leg that made
// these bytes final, so it lies in [lo, hi].  -1: it does not (cannot happen: the call fails), 0: no cut, 1: cut at *at.
ZWZ_HD int legfile_cut(const LegState& s, const LegSum& sum, uint64_t lo, uint64_t hi, uint64_t* at) {
    if (!s.has_check || (sum.have && sum.val_at == s.checked)) return 0;
    if (s.checked < lo || s.checked > hi) return -1;
    *at = s.checked;
    return 1;
}
// join(run, piece value, the parameter of the piece's length) for every piece of a committed part, then: the part ended at `checked`
template <class Sum>
ZWZ_HD void legfile_sum_add(LegSum& sum, uint32_t piece_val, uint32_t piece_len) {
    sum.run = Sum::join(sum.run, piece_val, Sum::pof(piece_len));
    sum.bytes += piece_len;
}
ZWZ_HD void legfile_sum_mark(LegSum& sum) { sum.val = sum.run; sum.val_at = sum.bytes; sum.have = 1; }

// stream_verdict's rule at the end: a checksum over the checked bytes that does not hold beats the provisional status
ZWZ_HD uint32_t legfile_verdict(const LegState& s, const LegSum& sum) {
    return s.has_check && (!sum.have || sum.val_at != s.checked || sum.val != s.expect) ? (uint32_t)kStrChecksum : s.status;
}

// The index in parts, as the loop collects it: the entries (24 bytes each, in memory: an index below 2^32 bytes has fewer than 2^17 with a
// full window, 3 MiB), and of the windows -- which go wherever the caller keeps them, a spool file -- their length and CRC register.
struct LegIndexParts {
    std::vector<uint8_t> entries;
    uint64_t win_bytes = 0;
    uint32_t win_reg = 0xffffffffu;
    void windows(const uint8_t* p, uint64_t n) { win_reg = crc_raw_long(win_reg, p, n); win_bytes += n; }
    uint32_t count() const { return (uint32_t)(entries.size() / kIdxEntry); }
    uint64_t padded() const { return (kIdxHeader + entries.size() + win_bytes + 15u) & ~15ull; }
    uint32_t pad() const { return (uint32_t)(padded() - kIdxHeader - entries.size() - win_bytes); }
    // The sealed header (index_seal's fields): the index CRC joined from the entries' and that of the windows and the zero padding
    void header(uint8_t* h, uint32_t wrap, uint32_t span, uint64_t stream_len, const LegState& s) const {
        const uint8_t zeros[16] = {};
        const uint32_t crc_e = crc_raw_long(0xffffffffu, entries.data(), entries.size()) ^ 0xffffffffu;
        const uint32_t crc_w = crc_raw_long(win_reg, zeros, pad()) ^ 0xffffffffu;
        index_put_header(h, IndexHeader{wrap, span, stream_len, s.end_out, count(), s.mk_end, s.has_check ? s.expect : 0u,
                                        CrcSum::join(crc_e, crc_w, CrcSum::pof(win_bytes + pad()))});
    }
};

// The capacity the planner is given: none.  (An output window that runs out is then always a rewind, never the stream's status 3.)
constexpr uint64_t kLegFileOutCap = ~0ull;
// The index capacity the leg form is given: an index of 2^32 bytes or more is not made (mk_full)
constexpr uint64_t kLegFileIdxCap = 0xffffffffull;

// stats of zwz_inflate_legs_file (include/zwz.h)
enum : uint32_t { kLfLegs = 0, kLfRewound, kLfGrown, kLfCommits, kLfMaxIn, kLfMaxOut, kLfEntries, kLfBytes, kLfStats };

// How the loop ended: the final state with the checksum's verdict in `status`, or -- too_large -- the last restart point
struct LegFileEnd { LegState s; uint32_t status; bool too_large; };

// The loop: zwz_legs.cpp's round for one stream, over staging windows.  `io` is where the windows live -- device staging and files in the
// product (zwz_legs_file.cpp), host memory in the CPU restatement -- and every call of it returns 0 or the error that ends the loop:
//   io.input(w)                        bytes [w.in_base, w.in_base + w.in_len) of the stream are the input window, zero-padded
//   io.output(w, from, n, slots)       the output window holds legfile_out_bytes(w) and the index array `slots` entries; the n bytes at
//                                      `from` of the window as it was stand at its head (source and destination may overlap)
//   io.leg(&s, w, g)                   one leg from state s; s becomes the state it left
//   io.sum<Sum>(at, n, &sum)           legfile_sum_add for the pieces of the n bytes at `at` of the output window
//   io.bytes(at, n)                    those bytes are final: the next of the decoded file
//   io.entries(slot, k, base, &parts)  the k entries from `slot` of the index array are final: into parts.entries, their windows -- each
//                                      entry.hist bytes in front of byte entry.off - base of the output window -- through parts.windows()
template <class IO>
int legfile_loop(IO& io, uint32_t wrap, uint64_t stream_len, uint32_t span, bool want_idx, uint64_t leg_bytes, uint64_t leg_out_bytes, uint64_t max_in,
                 uint64_t max_out, LegIndexParts* parts, LegFileEnd* end, uint64_t* stats) {
    LegState s = leg_fresh();
    LegPlan w{};
    LegSum sum = legfile_sum_fresh(dstream_check_init(wrap));
    uint64_t committed = 0, prev_base = 0;
    uint32_t ent_committed = 0;
    end->too_large = false;
    for (;;) {
        bool grew = false;
        const uint32_t v = leg_next(s, stream_len, kLegFileOutCap, leg_bytes, leg_out_bytes, max_in, max_out, &w, &grew);
        if (v == kLegDone) break;
        if (v == kLegTooLarge) { end->s = s; end->status = kStrTooLarge; end->too_large = true; return 0; }
        stats[kLfLegs]++; stats[kLfGrown] += grew;
        if (w.in_len > stats[kLfMaxIn]) stats[kLfMaxIn] = w.in_len;
        if (w.out_len > stats[kLfMaxOut]) stats[kLfMaxOut] = w.out_len;
        if (int rc = io.input(w)) return rc;
        uint64_t from = 0;
        const uint32_t carry = legfile_carry(s, w, prev_base, &from);
        const uint32_t slots = legfile_entry_slots(w.out_len, span);
        if (int rc = io.output(w, from, carry, slots)) return rc;
        prev_base = w.out_base;
        const uint32_t ent_first = s.mk_count;
        if (int rc = io.leg(&s, w, LegStage{0, ent_first, slots})) return rc;
        stats[kLfRewound] += !s.done;
        // the commit: bytes [committed, hi), cut at `checked`; entries [ent_committed, s.mk_count)
        const uint64_t hi = legfile_final_out(s);
        if (wrap != kWrapRaw) {
            uint64_t at = hi;
            const int cut = legfile_cut(s, sum, committed, hi, &at);
            if (cut < 0) return 1;                 // (every io error is negative: include/zwz.h)
            if (int rc = wrap == kWrapGzip ? io.template sum<CrcSum>(committed - w.out_base, at - committed, &sum) : io.template sum<AdlerSum>(committed - w.out_base, at - committed, &sum)) return rc;
            if (cut) legfile_sum_mark(sum);
            if (int rc = wrap == kWrapGzip ? io.template sum<CrcSum>(at - w.out_base, hi - at, &sum) : io.template sum<AdlerSum>(at - w.out_base, hi - at, &sum)) return rc;
        }
        if (hi > committed) {
            if (int rc = io.bytes(committed - w.out_base, hi - committed)) return rc;
            stats[kLfCommits]++;
            committed = hi;
        }
        const uint32_t ent_end = legfile_final_entries(s);
        if (want_idx && ent_end > ent_committed) {
            if (int rc = io.entries(ent_committed - ent_first, ent_end - ent_committed, w.out_base, parts)) return rc;
            ent_committed = ent_end;
        }
    }
    stats[kLfEntries] = ent_committed;
    end->s = s;
    end->status = legfile_verdict(s, sum);
    return 0;
}

// The stop position a finished leg leaves in the state's two pad words: the bit the reader stood at, from the stream's first byte
ZWZ_HD void leg_put_stop(LegState& s, uint64_t bit) { s.pad[0] = (uint32_t)bit; s.pad[1] = (uint32_t)(bit >> 32); }
ZWZ_HD uint64_t leg_stop_bit(const LegState& s) { return (uint64_t)s.pad[1] << 32 | s.pad[0]; }

}  // namespace zwz
