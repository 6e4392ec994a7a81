// leg_core.h -- the portable half of the decode in LEGS (zwz_inflate_legs_dev): an ordinary raw / zlib / gzip stream of
// any length decoded, and indexed, by one wave in several launches.  Host + device: the state, the snapshot rule, the index entry and the
// planner are one code for the kernel (inflate_kernel's leg form, zwz_kernels.hip), the host loop (zwz_legs.cpp) and the CPU restatement
// (tests/emu_legs/legs_emu.cpp).
//
// inflate_kernel keeps 32-bit bit and byte positions.  A LEG is one launch of a wave over a WINDOW of the stream's input and a window of its
// output, both small enough for those positions; what is 64 bits wide -- the windows' bases, the member's origin, the checksum record, the
// marking form's counters -- is carried from leg to leg in a LegState.  While it decodes, lane 0 keeps the latest RESTART POINT: the state
// as it stood at the last block header at which a checkpoint was due (index_core.h's rule, whether or not an entry was written), or at
// the last member start.  A leg that runs out of its input or output window before the stream does is REWOUND: the state it leaves is the
// restart point, the next leg starts there, and what was decoded behind it is decoded again.  A leg rewound to the very point it started
// from gets double the window that ran out (leg_next).
#pragma once
#include "index_core.h"

namespace zwz {

// inflate_kernel's sixth form (index_core.h has 3 and 4)
constexpr uint32_t kFormLeg = 5;

constexpr uint64_t kLegMaxIn = kStreamMaxIn - 16u, kLegMaxOut = kStreamMaxOut - 16u;                 // where the growth of a window stops
constexpr uint64_t kLegBytesDefault = 268435456u, kLegBytesMin = 4096u;                             // "leg_bytes"
constexpr uint64_t kLegOutBytesDefault = kStreamMaxOut - 65536u, kLegOutBytesMin = 65536u;          // "leg_out_bytes"

// Where a leg starts: in front of the wrapper's header; at a block header (a bit offset, `hist` decoded bytes in memory in front of it);
// at a member start (a byte position: zeros, then a gzip header or the end, with an empty window)
enum LegStart : uint32_t { kLegFresh = 0, kLegBlock = 1, kLegMember = 2 };

// Every offset counts from the stream's first byte / first decoded byte.
struct LegState {
    uint64_t bit;          // the restart point: the block header's first bit; a member start's byte * 8
    uint64_t out;          // the decoded offset there
    uint64_t origin;       // the current member's first decoded byte
    uint64_t checked;      // stream_core.h's StreamRecord: the output below `checked` is covered by `expect`
    uint64_t mk_last, mk_end, mk_bytes;      // the marking form's counters: decoded offset of the last due header, end bit of the first member, index bytes so far
    uint64_t end_out;      // done: the decoded length
    uint32_t start;        // LegStart
    uint32_t expect, has_check;
    uint32_t mk_count;     // entries written
    uint32_t mk_seen;      // headers at which a mark was due (= mk_count while an index is being made)
    uint32_t mk_full, mk_have_end, mk_second;
    uint32_t done;         // 1: `status` is the stream's provisional status; 0: rewound, `status` says which window ran out (1 input, 3 output)
    uint32_t status;
    uint32_t pad[2];
};
static_assert(sizeof(LegState) == 112, "LegState layout (host and device share it)");

ZWZ_HD LegState leg_fresh() {
    LegState s{};
    s.mk_bytes = kIdxHeader;
    return s;
}

// The window bytes in memory in front of a restart point
ZWZ_HD uint32_t leg_hist(const LegState& s) { return s.start == kLegBlock ? index_hist_bound(s.out - s.origin) : 0u; }

// index_mark_due on 64-bit offsets: the body's first block always, then every header at least `span` decoded bytes behind the last due one
ZWZ_HD bool leg_mark_due(uint32_t seen, uint64_t out, uint64_t last, uint32_t span) { return seen == 0u || out - last >= span; }

// An index entry with its high halves (the marking form writes words 1 and 3 as 0)
ZWZ_HD void leg_put_entry(uint32_t* e, uint64_t bit, uint64_t off, uint32_t hist) {
    e[0] = (uint32_t)bit; e[1] = (uint32_t)(bit >> 32); e[2] = (uint32_t)off; e[3] = (uint32_t)(off >> 32); e[4] = hist; e[5] = 0;
}

// The snapshot rule at a block header whose first bit is `bit`, at decoded offset `out` (lane 0).  Where a mark is due the state as it
// stands BEFORE the mark becomes the restart point -- a leg that starts there finds the mark due again and notes the same entry -- and
// the mark is noted: into `idx` (the stream's index, null: none wanted) unless it is full or a second member has begun.
// ent_first, ent_slots: the index array at `idx` holds `ent_slots` entries of which the first is the stream's entry ent_first (the file
// loop rebases the array every leg, legfile_core.h; the device call's array is the index itself).
ZWZ_HD void leg_at_header(LegState& cur, LegState& snap, uint64_t bit, uint64_t out, uint32_t span, uint8_t* idx, uint64_t idx_cap, uint32_t ent_first = 0,
                          uint32_t ent_slots = 0xffffffffu) {
    if (!leg_mark_due(cur.mk_seen, out, cur.mk_last, span)) return;
    snap = cur; snap.start = kLegBlock; snap.bit = bit; snap.out = out;
    if (idx && !cur.mk_full && !cur.mk_second) {
        const uint32_t hist = index_hist_bound(out);
        const uint64_t need = cur.mk_bytes + kIdxEntry + hist;
        if (need + 15u > idx_cap || cur.mk_count - ent_first >= ent_slots) cur.mk_full = 1;         // the index would not fit: none is made, the decode goes on
        else {
            leg_put_entry(reinterpret_cast<uint32_t*>(idx + kIdxHeader + (size_t)(cur.mk_count - ent_first) * kIdxEntry), bit, out, hist);
            cur.mk_count++; cur.mk_bytes = need;
        }
    }
    cur.mk_seen++; cur.mk_last = out;
}

// The snapshot at a member start: byte `at` of the stream, behind the trailer of the member before
ZWZ_HD void leg_at_member(const LegState& cur, LegState& snap, uint64_t at, uint64_t out) {
    snap = cur; snap.start = kLegMember; snap.bit = at * 8u; snap.out = out;
}

// stream_trailer on 64-bit offsets, over the leg's input window p[0, n): q = the byte after the final block in the window, out = the
// decoded offset, member = the member's decoded length.  ISIZE is the member's length mod 2^32.
ZWZ_HD uint32_t leg_trailer(uint32_t wrap, const uint8_t* p, uint32_t n, uint32_t q, uint64_t out, uint64_t member, LegState& cur, uint32_t* next) {
    if (wrap == kWrapRaw) return kInfEnd;
    if (wrap == kWrapZlib) {
        if (n - q < 4 || q > n) return kInfNeedInput;
        cur.expect = be32_at(p + q); cur.checked = out; cur.has_check = 1;
        return kInfEnd;
    }
    if (q > n || n - q < 4) return kInfNeedInput;
    cur.expect = crc_combine(cur.expect, le32_at(p + q), member); cur.checked = out; cur.has_check = 1;
    if (n - q < 8) return kInfNeedInput;
    if (le32_at(p + q + 4) != (uint32_t)member) return kStrLength;
    *next = q + 8;
    return kInfRunning;
}

// Whether a leg that ended with `status` is rewound: its window ran out, the stream did not
ZWZ_HD bool leg_rewound(uint32_t status, bool in_final, bool out_final) {
    return (status == kInfNeedInput && !in_final) || (status == kInfOverflow && !out_final);
}

// ---- the planner ------------------------------------------------------------------------------------------------------------------
// One leg's windows: input bytes [in_base, in_base + in_len) of the stream, decoded bytes [out_base, out_base + out_len) of its output
// (both bases multiples of 16), whether they reach the stream's end / its capacity.  budget_*: what the windows may span; from_*: the
// restart point the leg starts from.  The same record is the planner's memory from one leg to the next.
struct LegPlan {
    uint64_t in_base, out_base;
    uint32_t in_len, out_len;
    uint32_t in_final, out_final;
    uint64_t budget_in, budget_out;
    uint64_t from_bit; uint32_t from_start, ran;
};
enum LegVerdict : uint32_t { kLegGo = 0, kLegDone = 1, kLegTooLarge = 2 };

// The next leg of a stream of stream_len bytes that decodes into out_cap: kLegGo with *plan, or the final verdict -- kLegDone (the state
// holds the stream's status) or kLegTooLarge (one stretch between restart points is beyond max_in input or max_out output bytes; the
// last restart point's decoded offset, s.out, is what was decoded).  *plan: zeroed before a stream's first leg, then the leg before.
// *grew: a window was doubled.
ZWZ_HD uint32_t leg_next(const LegState& s, uint64_t stream_len, uint64_t out_cap, uint64_t leg_bytes, uint64_t leg_out_bytes, uint64_t max_in,
                         uint64_t max_out, LegPlan* plan, bool* grew) {
    *grew = false;
    if (s.done) return kLegDone;
    uint64_t bin = leg_bytes < max_in ? leg_bytes : max_in, bout = leg_out_bytes < max_out ? leg_out_bytes : max_out;
    if (plan->ran && s.bit == plan->from_bit && s.start == plan->from_start) {
        // rewound to where it started: double the window that ran out
        bin = plan->budget_in; bout = plan->budget_out;
        uint64_t& b = s.status == kInfOverflow ? bout : bin;
        const uint64_t lim = s.status == kInfOverflow ? max_out : max_in;
        if (b >= lim) return kLegTooLarge;
        b = 2u * b < lim ? 2u * b : lim;
        *grew = true;
    }
    const uint64_t first = s.start == kLegFresh ? 0u : s.bit >> 3;
    plan->in_base = first & ~15ull;
    plan->out_base = (s.out - leg_hist(s)) & ~15ull;
    const uint64_t in_left = stream_len - plan->in_base, out_left = out_cap > plan->out_base ? out_cap - plan->out_base : 0u;
    plan->in_final = in_left <= bin; plan->in_len = (uint32_t)(plan->in_final ? in_left : bin);
    plan->out_final = out_left <= bout; plan->out_len = (uint32_t)(plan->out_final ? out_left : bout);
    plan->budget_in = bin; plan->budget_out = bout;
    plan->from_bit = s.bit; plan->from_start = s.start; plan->ran = 1;
    return kLegGo;
}

}  // namespace zwz
