// zwz_bgzf_walk.h -- the walk of BGZF member chains on the device (zwz_bgzf_walk.hip; bgzf_core.h has the method).
#pragma once
#include <vector>

#include "bgzf_core.h"

struct zwz_ctx;

namespace zwz {

// What bgzf_walk_spans leaves: a result per span on the host, the members of all spans in the context's workspace (device; valid
// until the context's next BGZF call).  Span s's members are slots [res[s].first, res[s].first + res[s].count).
struct BgzfWalk {
    std::vector<BgzfSpanResult> res;
    const uint64_t* d_moff = nullptr;       // member offsets
    const uint32_t* d_misize = nullptr;     // their ISIZE fields
    uint64_t slots = 0;                     // slots in use (the lists lie in span order, at most two unused slots behind each)
    uint64_t candidates = 0;                // what the scan found
};

// Walks ns spans of d_gz[0, n) (16-byte aligned) in one batch.  spans: host memory, ascending and disjoint (head[s + 1] >= stop[s]),
// head <= stop <= n.  Synchronous on the context's stream.  ZWZ_OK whatever the chains hold: failures are in res.
int bgzf_walk_spans(zwz_ctx* c, const uint8_t* d_gz, uint64_t n, const BgzfSpan* spans, uint32_t ns, BgzfWalk* out);

}  // namespace zwz
