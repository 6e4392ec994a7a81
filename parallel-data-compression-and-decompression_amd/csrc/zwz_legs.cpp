// zwz_legs.cpp -- zwz_inflate_legs_dev of include/zwz.h: ordinary raw / zlib / gzip streams of any length decoded, and indexed, in LEGS.
// leg_core.h has the state, the snapshot rule and the planner; the kernel is inflate_kernel's leg form (zwz_kernels.hip).  Per round the
// host plans the next leg of every unfinished stream (leg_next), one launch runs a wave per such stream, and the states come back; once
// every stream has its provisional verdict the checksum is taken from pieces of the whole output and the windows are copied into the
// indexes (zwz_index.hip), as after the one-launch marking form.
#include <vector>

#include "zwz_api_internal.h"
#include "zwz_index.h"

using namespace zwz;

namespace {

// The per-stream arrays of one call.  The first `upload` bytes are filled on the host once; legw and order are uploaded every round,
// leg comes back every round, rec goes up once the decode is over.
struct LegArrays {
    uint64_t *out_off, *in_len, *idx_off, *idx_cap; LegState* leg;
    size_t upload;
    LegPlan* legw; uint4* order; IndexStream* rec;
    uint64_t* fin_len; uint32_t* fin_status;            // the verdicts the host gives (ZWZ_STREAM_TOO_LARGE)
};
LegArrays legs_layout(Carver& w, size_t n) {
    LegArrays A;
    A.out_off = w.take<uint64_t>(n); A.in_len = w.take<uint64_t>(n); A.idx_off = w.take<uint64_t>(n); A.idx_cap = w.take<uint64_t>(n); A.leg = w.take<LegState>(n);
    A.upload = w.used;
    A.legw = w.take<LegPlan>(n); A.order = w.take<uint4>(n); A.rec = w.take<IndexStream>(n);
    A.fin_len = w.take<uint64_t>(n); A.fin_status = w.take<uint32_t>(n);
    return A;
}

struct PieceArrays { uint64_t* off; uint32_t *len, *val; };
PieceArrays pieces_layout(Carver& w, size_t nc) { return PieceArrays{w.take<uint64_t>(nc), w.take<uint32_t>(nc), w.take<uint32_t>(nc)}; }

}  // namespace

extern "C" int zwz_inflate_legs_dev(zwz_ctx* c, int wrap, const uint8_t* d_in, const uint64_t* in_off, const uint64_t* in_len, uint32_t n, uint8_t* d_out,
                                    const uint64_t* out_off, const uint64_t* out_cap, uint64_t* d_out_len, uint32_t* d_status, uint32_t span, uint8_t* d_idx,
                                    const uint64_t* idx_off, const uint64_t* idx_cap, uint64_t* d_idx_len, uint32_t* legs) {
    if (!c || wrap < ZWZ_WRAP_RAW || wrap > ZWZ_WRAP_GZIP) return ZWZ_E_INVALID;
    if (span == 0) span = c->index_span_bytes;
    if (!index_span_ok(span)) return ZWZ_E_INVALID;
    if (n && (!d_in || !in_off || !in_len || !d_out || !out_off || !out_cap || !d_out_len || !d_status)) return ZWZ_E_INVALID;
    if (n && d_idx && (!idx_off || !idx_cap || !d_idx_len)) return ZWZ_E_INVALID;
    if (((uintptr_t)d_in & 15u) || ((uintptr_t)d_out & 15u) || ((uintptr_t)d_idx & 15u)) return ZWZ_E_INVALID;
    for (uint32_t i = 0; i < n; i++) if ((in_off[i] & 15u) || (out_off[i] & 15u) || (d_idx && (idx_off[i] & 15u))) return ZWZ_E_INVALID;
    if (n == 0) return ZWZ_OK;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const size_t bytes = layout_bytes([&](Carver& w) { legs_layout(w, n); });
    if (int rc = c->buf[kBufLegs].reserve(c, 0, bytes)) return rc;
    if (int rc = c->buf[kBufLegsHost].reserve(c, 0, bytes)) return rc;
    if (int rc = ensure_crc_tables(c)) return rc;                 // (the index CRC, whatever the wrapper)
    HIPCHK(hipStreamSynchronize(st));                             // (an earlier call's copies may still read the pinned arrays)
    Carver wd(c->buf[kBufLegs].p), wh(c->buf[kBufLegsHost].p);
    const LegArrays D = legs_layout(wd, n), H = legs_layout(wh, n);
    for (uint32_t i = 0; i < n; i++) {
        H.out_off[i] = out_off[i]; H.in_len[i] = in_len[i]; H.idx_off[i] = d_idx ? idx_off[i] : 0u; H.idx_cap[i] = d_idx ? idx_cap[i] : 0u;
        H.leg[i] = leg_fresh(); H.legw[i] = LegPlan{};
        if (legs) legs[3 * i] = legs[3 * i + 1] = legs[3 * i + 2] = 0;
    }
    HIPCHK(hipMemcpyAsync(D.out_off, H.out_off, H.upload, hipMemcpyHostToDevice, st));
    // 0: unfinished; 1: the wave left its verdict; 2: the planner did (ZWZ_STREAM_TOO_LARGE)
    std::vector<uint8_t> fin(n, 0);
    for (;;) {
        uint32_t m = 0;
        for (uint32_t i = 0; i < n; i++) {
            if (fin[i]) continue;
            bool g = false;
            const uint32_t v = leg_next(H.leg[i], in_len[i], out_cap[i], c->leg_bytes, c->leg_out_bytes, kLegMaxIn, kLegMaxOut, &H.legw[i], &g);
            if (v == kLegDone) { fin[i] = 1; continue; }
            if (v == kLegTooLarge) { fin[i] = 2; continue; }
            const uint64_t at = in_off[i] + H.legw[i].in_base;
            H.order[m++] = make_uint4((uint32_t)at, (uint32_t)(at >> 32), H.legw[i].in_len, i);
            if (legs) { legs[3 * i]++; legs[3 * i + 2] += g; }
        }
        if (m == 0) break;
        HIPCHK(hipMemcpyAsync(D.legw, H.legw, (size_t)n * sizeof(LegPlan), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(D.order, H.order, (size_t)m * sizeof(uint4), hipMemcpyHostToDevice, st));
        HIPCHK(launch_inflate_legs(InflateLegArgs{d_in, D.order, m, d_out, D.out_off, d_out_len, d_status, d_idx, D.idx_off, D.idx_cap, d_idx_len, span, D.legw, D.leg,
                                                  (uint32_t)wrap, c->inflate_serial_header}, st));
        HIPCHK(hipMemcpyAsync(H.leg, D.leg, (size_t)n * sizeof(LegState), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (legs) for (uint32_t j = 0; j < m; j++) legs[3 * H.order[j].w + 1] += !H.leg[H.order[j].w].done;
    }
    // the checksum of every stream's checked output from pieces, the verdicts of the planner, the windows into the indexes
    const uint32_t shift = 0;                                      // (d_out and every out_off[i] are multiples of 16: a stream's first piece is empty)
    uint64_t nc = 0;
    for (uint32_t i = 0; i < n; i++) {
        const LegState& s = H.leg[i];
        IndexStream& r = H.rec[i];
        r = IndexStream{0, in_len[i], 0, out_off[i], 0, 0, (uint32_t)wrap, s.expect, 0, 0, 0, 0, 0};
        if (fin[i] == 2) { r.refused = kStrTooLarge; H.fin_len[i] = s.out; H.fin_status[i] = kStrTooLarge; continue; }
        if (wrap == ZWZ_WRAP_RAW || !s.has_check) continue;
        r.nseg = 1; r.total = s.checked; r.head = index_head_bytes(shift, r.total);
        const uint64_t k = index_piece_count((uint32_t)wrap, r.head, r.total);
        if (nc + k > 0xffffffffull) { set_error("zwz_inflate_legs_dev: more than 2^32 - 1 checksum pieces in one call"); return ZWZ_E_INVALID; }
        r.piece0 = (uint32_t)nc; r.pieces = (uint32_t)k; nc += k;
    }
    const size_t pbytes = layout_bytes([&](Carver& w) { pieces_layout(w, (size_t)nc); });
    if (int rc = c->buf[kBufLegPieces].reserve(c, 0, pbytes)) return rc;
    Carver wp(c->buf[kBufLegPieces].p);
    const PieceArrays P = pieces_layout(wp, (size_t)nc);
    HIPCHK(hipMemcpyAsync(D.rec, H.rec, (size_t)n * sizeof(IndexStream), hipMemcpyHostToDevice, st));
    for (uint32_t i = 0; i < n; i++) {
        if (fin[i] != 2) continue;
        HIPCHK(hipMemcpyAsync(d_out_len + i, H.fin_len + i, sizeof(uint64_t), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_status + i, H.fin_status + i, sizeof(uint32_t), hipMemcpyHostToDevice, st));
        if (d_idx) HIPCHK(hipMemsetAsync(d_idx_len + i, 0, sizeof(uint64_t), st));
    }
    const CrcTables* tab = c->buf[kBufCrcTables].as<const CrcTables>();
    HIPCHK(launch_legs_check(tab, LegsCheck{d_out, D.rec, n, (uint32_t)wrap, P.off, P.len, P.val, (uint32_t)nc, d_status}, c->cu_count, st));
    if (d_idx) HIPCHK(launch_index_windows(tab, IndexBuild{d_out, D.out_off, D.in_len, d_status, n, (uint32_t)wrap, span, d_idx, D.idx_off, d_idx_len}, st));
    return ZWZ_OK;
}
