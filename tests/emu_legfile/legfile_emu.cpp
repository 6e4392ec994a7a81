// Host build of the file loop of the decode in legs for tests/test_legs_file_cpu.py (g++ -shared; no HIP): csrc/legfile_core.h's legfile_loop
// -- the very loop zwz_inflate_legs_file runs, with its rules: the committed range, the entries committed, the cut at `checked`, where the
// carry comes from, the staging a plan needs -- over windows in host memory.  The leg itself is tests/emu_legs/legs_emu.cpp's restatement
// (included, not edited); the pieces of a committed range are restated here with plain byte-by-byte checksums.  What the test compares
// with comes from libz and from legs_emu.cpp's whole-stream call, which shares nothing with the loop.
// Two things the restated leg does not do: it writes an entry at its number in the stream, not rebased, so the index array here has room
// from entry 0 and the leg's entries are moved down to slot 0 afterwards; and it leaves no reader position, so the stop reported for a
// finished stream is the end of the last leg's input window, an upper bound of the position the kernel leaves in the state's pad words.
#include "../emu_legs/legs_emu.cpp"

#include "../../parallel-data-compression-and-decompression_amd/csrc/legfile_core.h"

namespace {

struct EmuIO {
    uint32_t wrap, span;
    const uint8_t* file;
    bool want_idx;
    std::vector<uint8_t> in, out, ent, dst, spool;
    std::vector<uint64_t> trace;              // per leg: start kind, bit, decoded offset, origin, hist, carried bytes
    uint64_t last_in_end = 0;
    uint32_t carried = 0;

    int input(const LegPlan& w) {
        in.assign((size_t)legfile_in_bytes(w), 0);
        if (w.in_len) memcpy(in.data(), file + w.in_base, w.in_len);
        last_in_end = w.in_base + w.in_len;
        return 0;
    }
    int output(const LegPlan& w, uint64_t from, uint32_t n, uint32_t slots) {
        std::vector<uint8_t> carry(out.begin() + (n ? (size_t)from : 0), out.begin() + (n ? (size_t)from + n : 0));
        out.assign((size_t)legfile_out_bytes(w), 0xa5);        // (a fresh window: nothing of the leg before is left but the carry)
        if (n) memcpy(out.data(), carry.data(), n);
        carried = n;
        (void)slots;
        return 0;
    }
    int leg(LegState* s, const LegPlan& w, const LegStage& g) {
        const uint64_t t[6] = {s->start, s->bit, s->out, s->origin, leg_hist(*s), carried};
        trace.insert(trace.end(), t, t + 6);
        ent.assign(kIdxHeader + ((size_t)g.ent_first + g.ent_slots + 1) * kIdxEntry, 0);
        emu_leg_run(wrap, in.data(), out.data() + g.out_at, span, want_idx ? ent.data() : nullptr, kLegFileIdxCap, s, &w);
        if (want_idx && !s->mk_full && s->mk_count - g.ent_first > g.ent_slots) return -100;      // the slots a leg is given hold what it writes
        memmove(ent.data() + kIdxHeader, ent.data() + kIdxHeader + (size_t)g.ent_first * kIdxEntry, (size_t)(g.ent_slots + 1) * kIdxEntry);
        if (s->done) leg_put_stop(*s, last_in_end * 8u);
        return 0;
    }
    template <class Sum>
    int sum(uint64_t at, uint64_t n, LegSum* sm) {
        if (!n) return 0;
        const uint32_t head = index_head_bytes((uint32_t)(at & 15u), n);
        const uint64_t pieces = index_piece_count(wrap, head, n);
        for (uint64_t j = 0; j < pieces; j++) {
            const uint8_t* p = out.data() + at + index_piece_start(head, j);
            const uint32_t len = index_piece_bytes(head, n, j);
            legfile_sum_add<Sum>(*sm, wrap == kWrapGzip ? crc_plain(p, len) : adler_plain(p, len), len);
        }
        return 0;
    }
    int bytes(uint64_t at, uint64_t n) {
        dst.insert(dst.end(), out.begin() + (size_t)at, out.begin() + (size_t)(at + n));
        return 0;
    }
    int entries(uint32_t slot, uint32_t k, uint64_t base, LegIndexParts* parts) {
        const uint8_t* e = ent.data() + kIdxHeader + (size_t)slot * kIdxEntry;
        parts->entries.insert(parts->entries.end(), e, e + (size_t)k * kIdxEntry);
        for (uint32_t i = 0; i < k; i++, e += kIdxEntry) {
            const uint64_t off = le64_of(e + 8);
            const uint32_t hist = le32_at(e + 16);
            if (off < base + hist || off - base > out.size()) return -101;
            const uint8_t* w = out.data() + (off - hist - base);
            parts->windows(w, hist);
            spool.insert(spool.end(), w, w + hist);
        }
        return 0;
    }
};

}  // namespace

extern "C" {

// zwz_inflate_legs_file on a file in memory.  Returns its return code (0, -6 ZWZ_E_FORMAT, -7 ZWZ_E_CHECKSUM; -100 / -101: a rule of the
// loop did not hold); *status: the stream's status; dst / idx (either may be null: not wanted) receive the decoded bytes and the index
// when the code is 0 -- nothing otherwise, as the product leaves no file; stats: the call's first seven words; *stop: the compressed byte
// offset named on ZWZ_E_FORMAT; trace: six words a leg, up to trace_cap legs; *trace_len: the legs traced.
int emu_legfile(uint32_t wrap, const uint8_t* file, uint64_t n, uint32_t span, uint64_t leg_bytes, uint64_t leg_out_bytes, uint64_t max_in, uint64_t max_out,
                uint8_t* dst, uint64_t dst_cap, uint64_t* dst_len, uint8_t* idx, uint64_t idx_cap, uint64_t* idx_len, uint32_t* status, uint64_t* stats,
                uint64_t* stop, uint64_t* trace, uint32_t trace_cap, uint32_t* trace_len) {
    EmuIO io{wrap, span, file, idx != nullptr};
    LegIndexParts parts;
    LegFileEnd end{};
    uint64_t st[kLfStats] = {};
    *dst_len = *idx_len = *stop = 0; *status = 0; *trace_len = 0;
    const int rc = legfile_loop(io, wrap, n, span, idx != nullptr, leg_bytes, leg_out_bytes, max_in, max_out, &parts, &end, st);
    for (uint32_t i = 0; i < 7; i++) stats[i] = st[i];
    const uint32_t legs = (uint32_t)(io.trace.size() / 6);
    *trace_len = legs < trace_cap ? legs : trace_cap;
    if (trace && *trace_len) memcpy(trace, io.trace.data(), (size_t)*trace_len * 6 * sizeof(uint64_t));
    if (rc) return rc > 0 ? -102 : rc;
    *status = end.status;
    const LegState& s = end.s;
    if (end.too_large) { *stop = s.bit >> 3; return -6; }
    if (end.status == kStrChecksum || end.status == kStrLength) return -7;
    if (end.status != kInfEnd) { *stop = leg_stop_bit(s) >> 3; return -6; }
    if (idx) {
        if (s.mk_full || s.mk_second || !s.mk_have_end || !s.mk_count) return -6;
        if (parts.count() != s.mk_count || kIdxHeader + parts.entries.size() + parts.win_bytes != s.mk_bytes || parts.padded() > idx_cap) return -103;
        parts.header(idx, wrap, span, n, s);
        memcpy(idx + kIdxHeader, parts.entries.data(), parts.entries.size());
        if (!io.spool.empty()) memcpy(idx + kIdxHeader + parts.entries.size(), io.spool.data(), io.spool.size());
        memset(idx + kIdxHeader + parts.entries.size() + io.spool.size(), 0, parts.pad());
        *idx_len = parts.padded();
    }
    if (dst) {
        if (io.dst.size() > dst_cap) return -104;
        if (!io.dst.empty()) memcpy(dst, io.dst.data(), io.dst.size());
        *dst_len = io.dst.size();
    }
    return 0;
}

}  // extern "C"
