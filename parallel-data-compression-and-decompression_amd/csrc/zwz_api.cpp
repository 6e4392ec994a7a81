// zwz_api.cpp -- C ABI (include/zwz.h) over the kernel pipeline: context, workspace, batch slicing,
// pinned staging for host buffers.  No CPU codec lives here: without a GPU every entry point fails.
#include "zwz_api_internal.h"
#include "zwz_bgzf.h"

#include <cerrno>
#include <climits>
#include <cstdarg>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <new>
#include <string>
#include <vector>

namespace zwz {

thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}

int hip_fail(hipError_t e, const char* what) {
    set_error("%s: %s", what, hipGetErrorString(e));
    return ZWZ_E_HIP;
}

}  // namespace zwz

using namespace zwz;

namespace {

// Known-answer test of lz_links, run once per context.  The kernel's feeders keep input loads in flight across several
// hand-overs in registers the compiler merely promises not to touch, and its inserter is one block of hand-scheduled
// assembly: a toolchain change could break either without a diagnostic, and wrong links mean shards that are no longer
// the reference's.  Three chunks -- text-like with long chains, incompressible, a ragged short one -- go through the
// kernel and every link is compared with zlib's insert restated on the host (prev[p] = head[h]; head[h] = p).
// Returns ZWZ_OK with *bad = 0, or bit 0 set (lz_links' links are wrong) / bit 1 set (lz_sort's order is wrong) and the text of the
// first finding in zwz_last_error(); a HIP failure is returned as such.
int links_self_test(zwz_ctx* c, uint32_t* bad) {
    *bad = 0;
    // three workgroups for eight chunks: each one runs on from chunk to chunk (full, short, one-block, empty and tiny ones)
    constexpr uint32_t K = 8;
    const uint32_t lens[K] = {65535u, 40000u, 0u, 2049u + 37u, 5u, 6144u, 65535u, 2u};
    std::vector<uint8_t> h_in((size_t)K * ZWZ_DEV_STRIDE, 0);
    uint32_t rng = 0x2545f491u;
    uint64_t offs[K];
    for (uint32_t k = 0; k < K; k++) {
        uint8_t* d = h_in.data() + (size_t)k * ZWZ_DEV_STRIDE;
        offs[k] = (uint64_t)k * ZWZ_DEV_STRIDE;
        for (uint32_t i = 0; i < lens[k]; i++) {
            rng = rng * 1664525u + 1013904223u;
            if (k & 1u) d[i] = (uint8_t)(rng >> 24);                                   // incompressible
            else d[i] = (rng >> 28) < 3 && i >= 7 ? d[i - 7 + ((rng >> 20) & 3u)] : (uint8_t)(97u + ((rng >> 16) % 6u));   // six letters and short copies: long chains
        }
    }
    uint8_t* d_in = nullptr; uint64_t* d_off = nullptr; uint32_t* d_len = nullptr; uint16_t* d_links = nullptr; uint32_t* d_stat = nullptr;
    uint32_t *d_sorted = nullptr, *d_list = nullptr, *d_tickets = nullptr;
    auto cleanup = [&] { (void)hipFree(d_in); (void)hipFree(d_off); (void)hipFree(d_len); (void)hipFree(d_links); (void)hipFree(d_stat);
                         (void)hipFree(d_sorted); (void)hipFree(d_list); (void)hipFree(d_tickets); };
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&d_in), h_in.size());
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&d_off), sizeof offs);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&d_len), sizeof lens);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&d_links), K * (size_t)kLinkStride * sizeof(uint16_t));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&d_stat), K * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&d_sorted), K * (size_t)kSortedStride * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&d_list), K * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&d_tickets), kTicketBytes);
    if (e == hipSuccess) e = hipMemsetAsync(d_tickets, 0, kTicketBytes, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(d_sorted, 0xa5, K * (size_t)kSortedStride * sizeof(uint32_t), c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_in, h_in.data(), h_in.size(), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_off, offs, sizeof offs, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_len, lens, sizeof lens, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(d_links, 0xa5, K * (size_t)kLinkStride * sizeof(uint16_t), c->stream);
    DeflateArgs a{};
    a.in = d_in; a.in_off = d_off; a.in_len = d_len; a.n = K; a.links = d_links; a.link_stat = d_stat; a.cu_count = 3;
    a.sorted = d_sorted; a.dense_list = d_list; a.sparse_list = d_list; a.tickets = d_tickets;   // (every chunk goes onto the dense list here)
    if (e == hipSuccess) e = launch_links_only(a, c->stream);
    std::vector<uint16_t> got(K * (size_t)kLinkStride);
    uint32_t stat[K] = {};
    if (e == hipSuccess) e = hipMemcpyAsync(got.data(), d_links, got.size() * sizeof(uint16_t), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(stat, d_stat, sizeof stat, hipMemcpyDeviceToHost, c->stream);
    // lz_sort over the same chunks (it overwrites their link arrays, read back above): its ranking pass stands on the lane
    // order of the returning LDS add
    std::vector<uint32_t> srt(K * (size_t)kSortedStride);
    if (e == hipSuccess) e = launch_dense_list(a, c->stream, 2u);
    if (e == hipSuccess) e = launch_sort(a, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(srt.data(), d_sorted, srt.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    cleanup();
    if (e != hipSuccess) return hip_fail(e, "lz_links / lz_sort self-test");
    std::vector<uint16_t> head(32768);
    for (uint32_t k = 0; k < K; k++) {
        const uint8_t* d = h_in.data() + (size_t)k * ZWZ_DEV_STRIDE;
        std::fill(head.begin(), head.end(), (uint16_t)0);
        uint32_t linked = 0;
        for (uint32_t p = 0; p + kMinMatch <= lens[k]; p++) {
            const uint32_t h = hash3(d[p], d[p + 1], d[p + 2]);
            const uint16_t want = head[h];
            head[h] = (uint16_t)p;
            linked += want != 0;
            if (got[(size_t)k * kLinkStride + p] != want) {
                if (!(*bad & 1u)) set_error("zwz_ctx_create: lz_links self-test failed (chunk %u, position %u: link %u, expected %u) -- the kernel's hand-scheduled "
                                            "code does not survive this toolchain", k, p, (unsigned)got[(size_t)k * kLinkStride + p], (unsigned)want);
                *bad |= 1u;
                break;
            }
        }
        for (uint32_t p = lens[k] >= kMinMatch ? lens[k] - (kMinMatch - 1u) : 0u; p < lens[k]; p++) {   // the last positions have no trigram: NIL
            if (got[(size_t)k * kLinkStride + p] != 0 && !(*bad & 1u)) { set_error("zwz_ctx_create: lz_links self-test failed (chunk %u: a link behind the last trigram)", k); *bad |= 1u; }
        }
        if (stat[k] != linked && !(*bad & 1u)) { set_error("zwz_ctx_create: lz_links self-test failed (chunk %u: %u linked positions counted, %u expected)", k, stat[k], linked); *bad |= 1u; }
        // the sorted array: a stable counting sort of the positions by bucket
        const uint32_t n = lens[k] >= kMinMatch ? lens[k] - (kMinMatch - 1u) : 0u;
        std::vector<uint32_t> start(32769, 0);
        for (uint32_t p = 0; p < n; p++) start[hash3(d[p], d[p + 1], d[p + 2]) + 1]++;
        for (uint32_t h = 0; h < 32768; h++) start[h + 1] += start[h];
        for (uint32_t p = 0; p < n; p++) {
            const uint32_t h = hash3(d[p], d[p + 1], d[p + 2]), want = start[h]++;
            const uint32_t got_d = reinterpret_cast<const uint16_t*>(srt.data() + (size_t)k * kSortedStride)[p];
            if (got_d != want) {
                if (!(*bad & 2u)) set_error("zwz_ctx_create: lz_sort self-test failed (chunk %u, position %u: sorted index %u, expected %u) -- the returning LDS add does not "
                                            "serve same-address lanes in lane order on this device", k, p, got_d, want);
                *bad |= 2u;
                break;
            }
        }
    }
    return ZWZ_OK;
}

// Known-answer test of the two other users of the ordered LDS add: the wave form of the block flush (zwz_plan.hip:
// next_code[len]++ in symbol order) and inflate's wave-built decoding tables (wave_build_decode_table: a symbol's place in sorted[] and
// hence its code).  Three small chunks with dynamic-Huffman blocks -- text-like, a geometric byte distribution whose tree is deep, one
// with long matches and far distances -- are deflated with the serial and the wave flush and inflated with serial and wave headers:
// the serial forms must reproduce the input (else the device cannot run the codec at all), and a wave form that disagrees with its
// serial form is switched off for this context.  A few milliseconds per context.
int codec_self_test(zwz_ctx* c) {
    constexpr uint32_t K = 3;
    const uint32_t lens[K] = {24000u, 30000u, 40000u};
    std::vector<uint8_t> in;
    uint64_t offs[K];
    uint32_t rng = 0x9e3779b9u;
    auto next = [&] { rng = rng * 1664525u + 1013904223u; return rng >> 8; };
    for (uint32_t k = 0; k < K; k++) {
        offs[k] = in.size();
        const size_t base = in.size();
        for (uint32_t i = 0; i < lens[k]; i++) {
            uint8_t b;
            if (k == 0) b = (next() & 15u) < 3 && i >= 9 ? in[base + i - 9 + (next() & 3u)] : (uint8_t)(97u + next() % 7u);
            else if (k == 1) { uint32_t r = next() | 1u << 23, z = 0; while (!(r & 1u)) { r >>= 1; z++; } b = (uint8_t)(32u + z); }   // P(32 + z) = 2^-(z + 1): a tree as deep as its alphabet
            else b = i >= 20000u && ((i / 37u) & 1u) ? in[base + i - 20000u] : (uint8_t)next();                                       // far copies in noise: long distance codes
            in.push_back(b);
        }
    }
    const uint32_t keep_plan = c->plan_serial, keep_hdr = c->inflate_serial_header;
    std::vector<uint8_t> p_serial((size_t)K * ZWZ_CHUNK_SIZE), p_wave((size_t)K * ZWZ_CHUNK_SIZE), back((size_t)K * ZWZ_CHUNK_SIZE);
    uint32_t l_serial[K], l_wave[K], l_back[K], st[K];
    uint64_t poffs[K];
    for (uint32_t k = 0; k < K; k++) poffs[k] = (uint64_t)k * ZWZ_CHUNK_SIZE;
    auto same_as_input = [&] {
        for (uint32_t k = 0; k < K; k++) if (st[k] != ZWZ_INF_END || l_back[k] != lens[k] || memcmp(back.data() + (size_t)k * ZWZ_CHUNK_SIZE, in.data() + offs[k], lens[k])) return false;
        return true;
    };
    c->plan_serial = 1;
    int rc = zwz_deflate_batch(c, in.data(), offs, lens, K, p_serial.data(), l_serial);
    c->inflate_serial_header = 1;
    if (rc == ZWZ_OK) rc = zwz_inflate_batch(c, p_serial.data(), poffs, l_serial, K, back.data(), l_back, st);
    if (rc != ZWZ_OK) return rc;
    if (!same_as_input()) { set_error("zwz_ctx_create: codec self-test failed -- three chunks do not survive deflate + inflate on this device even in the kernels' order-free forms"); return ZWZ_E_NO_DEVICE; }
    if (!keep_plan) {
        c->plan_serial = 0;
        rc = zwz_deflate_batch(c, in.data(), offs, lens, K, p_wave.data(), l_wave);
        if (rc != ZWZ_OK) return rc;
        bool same = true;
        for (uint32_t k = 0; k < K; k++) same = same && l_wave[k] == l_serial[k] && !memcmp(p_wave.data() + (size_t)k * ZWZ_CHUNK_SIZE, p_serial.data() + (size_t)k * ZWZ_CHUNK_SIZE, l_serial[k]);
        if (!same) { c->plan_serial = 1; c->forbidden |= kForbidPlanWave; fprintf(stderr, "zwz: the wave form of the block flush disagrees with the lane-serial one on this device: using the lane-serial kernel\n"); }
    }
    if (!keep_hdr) {
        c->inflate_serial_header = 0;
        rc = zwz_inflate_batch(c, p_serial.data(), poffs, l_serial, K, back.data(), l_back, st);
        if (rc != ZWZ_OK) return rc;
        if (!same_as_input()) { c->inflate_serial_header = 1; c->forbidden |= kForbidInflateWave; fprintf(stderr, "zwz: inflate's wave-built tables decode wrongly on this device: block headers go to lane 0\n"); }
    }
    return ZWZ_OK;
}

}  // namespace

extern "C" {

const char* zwz_strerror(int s) {
    switch (s) {
        case ZWZ_OK: return "ok";
        case ZWZ_E_INVALID: return "invalid argument";
        case ZWZ_E_HIP: return "HIP runtime error";
        case ZWZ_E_NO_DEVICE: return "no usable GPU (this library has no CPU fallback)";
        case ZWZ_E_IO: return "I/O error";
        case ZWZ_E_NOMEM: return "out of memory";
        case ZWZ_E_FORMAT: return "malformed .zwz shard";
        case ZWZ_E_CHECKSUM: return "BGZF checksum mismatch (CRC-32 or ISIZE)";
        default: return "unknown status";
    }
}

const char* zwz_last_error(void) { return g_err; }

int zwz_device_count(int* count) {
    if (!count) return ZWZ_E_INVALID;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { *count = 0; (void)hipGetLastError(); return ZWZ_E_NO_DEVICE; }
    *count = n;
    return ZWZ_OK;
}

int zwz_ctx_create(int device, uint32_t max_batch, zwz_ctx** out) {
    if (!out) return ZWZ_E_INVALID;
    *out = nullptr;
    int n = 0;
    if (zwz_device_count(&n) != ZWZ_OK || n <= 0) { set_error("hipGetDeviceCount found no device"); return ZWZ_E_NO_DEVICE; }
    if (device < 0 || device >= n) return ZWZ_E_INVALID;
    HIPCHK(hipSetDevice(device));
    zwz_ctx* c = new (std::nothrow) zwz_ctx();
    if (!c) return ZWZ_E_NOMEM;
    c->device = device;
    c->max_batch = max_batch ? max_batch : 8192u;
    { int cus = 0; if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) c->cu_count = (uint32_t)cus; }
    hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = configure_kernels();
    for (int i = 0; i < kNumDeflateStages + 1 && e == hipSuccess; i++) e = hipEventCreate(&c->ev[i]);
    for (int i = 0; i < 2 && e == hipSuccess; i++) e = hipEventCreate(&c->ev_inf[i]);
    if (e != hipSuccess) { int rc = hip_fail(e, "zwz_ctx_create"); zwz_ctx_destroy(c); return rc; }
    if (const uint32_t xk = exp_flags_kernels(), xb = exp_flags_band(); xk | xb)     // never silent: an instrumented build must not pass for the product
        fprintf(stderr, "zwz: EXPERIMENT BUILD (ZWZ_MATCH_EXP=%u ZWZ_PARSE_EXP=%u ZWZ_ENC_EXP=%u ZWZ_INF_EXP=%u ZWZ_BAND_EXP=%u): timings only, not the product library\n",
                xk & 255u, (xk >> 8) & 255u, (xk >> 16) & 255u, xk >> 24, xb);
    // Test switches, read ONCE per context (a stray variable is still honoured, but no launch re-reads the environment: ADVICE r3)
    // (a value that is not understood is said so: ZWZ_MATCH=bnad used to be ignored without a word)
    auto from_env = [&](const char* var, const char* option) {
        if (const char* v = getenv(var)) if (zwz_ctx_set_option(c, option, v) != ZWZ_OK) fprintf(stderr, "zwz: %s=%s is not a value of option \"%s\": ignored\n", var, v, option);
    };
    from_env("ZWZ_MATCH", "match"); from_env("ZWZ_PLAN", "plan"); from_env("ZWZ_INFLATE_HEADER", "inflate_header");
    from_env("ZWZ_ZIP_SLICE_BYTES", "zip_slice_bytes"); from_env("ZWZ_ZIP_FORCE_ZIP64", "zip_force_zip64");       // (for `main zip` / `main unzip`)
    from_env("ZWZ_SPLIT_SLICE_BYTES", "split_slice_bytes");      // (for `main gunzip`: the slice of zwz_inflate_stream_file)
    from_env("ZWZ_LEG_FILE_BYTES", "leg_file_bytes"); from_env("ZWZ_LEG_FILE_OUT_BYTES", "leg_file_out_bytes");      // (for `main gunzip` / `main gzindex`: zwz_inflate_legs_file's windows)
    const bool tl = getenv("ZWZ_TIMELINE") != nullptr || getenv("ZWZ_VERBOSE") != nullptr;
    const auto t_create = std::chrono::steady_clock::now();
    auto mark = [&](const char* what) { if (tl) fprintf(stderr, "zwz: context: %s at +%.3f s\n", what, std::chrono::duration<double>(std::chrono::steady_clock::now() - t_create).count()); };
    // Three kernels stand on LDS behaviour the ISA manual does not promise: lz_links on the lane order of
    // ds_wrxchg_rtn, lz_sort / the wave plan / inflate's wave-built tables on that of ds_add_rtn.  Each is checked here against a
    // host restatement or its own order-free form; a failed check selects the form that does not need the property, and only a
    // device on which no search kernel is left gets no context.
    {
        bool xchg_ok = false;
        e = probe_exchange_order(c->stream, &xchg_ok);
        if (e != hipSuccess) { int rc = hip_fail(e, "zwz_ctx_create: exchange-order probe"); zwz_ctx_destroy(c); return rc; }
        mark("exchange-order probe done");
        uint32_t bad = 0;
        const int rc = links_self_test(c, &bad);
        mark("lz_links / lz_sort known-answer tests done");
        if (rc != ZWZ_OK) { zwz_ctx_destroy(c); return rc; }
        const bool links_ok = xchg_ok && !(bad & 1u), sort_ok = !(bad & 2u);
        if (!links_ok && !sort_ok) {
            if (bad == 2u || !bad) set_error("zwz_ctx_create: neither ds_wrxchg_rtn_b32 nor ds_add_rtn_u32 serves same-address lanes in lane order on this device: no match search can run on it");
            zwz_ctx_destroy(c);
            return ZWZ_E_NO_DEVICE;
        }
        // (a test hook: ZWZ_FORCE_SELFTEST_FAIL=links|sort pretends that check failed, so that the fallback configurations run through the
        //  oracle comparison once -- tests/test_gpu_codec.py)
        const char* force = getenv("ZWZ_FORCE_SELFTEST_FAIL");
        const bool f_links = force && strstr(force, "links"), f_sort = force && strstr(force, "sort");
        if (!links_ok || f_links) c->forbidden |= kForbidLinks;
        if (!sort_ok || f_sort) c->forbidden |= kForbidSort | kForbidPlanWave | kForbidInflateWave;
        if (f_links && !f_sort) { c->match_mode = kMatchBand; fprintf(stderr, "zwz: (forced) lz_links counts as failed: every chunk takes the sort + band search\n"); }
        if (f_sort) { c->match_mode = kMatchWalk; c->plan_serial = 1; c->inflate_serial_header = 1; fprintf(stderr, "zwz: (forced) lz_sort counts as failed: chain walk, lane-serial block flush and inflate headers\n"); }
        if (!links_ok) { c->match_mode = kMatchBand; fprintf(stderr, "zwz: lz_links' exchange order does not hold on this device: every chunk takes the sort + band search (%s)\n", zwz_last_error()); }
        if (!sort_ok) {
            c->match_mode = kMatchWalk; c->plan_serial = 1; c->inflate_serial_header = 1;
            fprintf(stderr, "zwz: the returning LDS add is not served in lane order on this device: chain walk, lane-serial block flush and lane-serial inflate headers (%s)\n", zwz_last_error());
        }
    }
    { const int rc = codec_self_test(c); if (rc != ZWZ_OK) { zwz_ctx_destroy(c); return rc; } }
    mark("codec known-answer test done");
    // The default level, read once like ZWZ_MATCH -- but taken up only here: the self-tests above ran at level 6.
    if (const char* v = getenv("ZWZ_LEVEL")) {
        char* end = nullptr;
        errno = 0;
        const long x = strtol(v, &end, 10);
        if (!*v || *end || errno || x < INT_MIN || x > INT_MAX || zwz_ctx_set_level(c, (int)x) != ZWZ_OK) fprintf(stderr, "zwz: ZWZ_LEVEL=%s is not a level this library writes (4, 5, 6; 0 = default): ignored\n", v);
    }
    if (const char* v = getenv("ZWZ_STRATEGY")) {     // the default strategy, as ZWZ_LEVEL: by name, as the CLI's flags spell them
        const std::string x = v;
        const int st = x == "huffman" ? ZWZ_STRATEGY_HUFFMAN : x == "rle" ? ZWZ_STRATEGY_RLE : x == "default" ? ZWZ_STRATEGY_DEFAULT : -1;
        if (st < 0 || zwz_ctx_set_strategy(c, st) != ZWZ_OK) fprintf(stderr, "zwz: ZWZ_STRATEGY=%s is not a strategy this library writes (huffman, rle; default): ignored\n", v);
    }
    *out = c;
    return ZWZ_OK;
}

int zwz_ctx_set_strategy(zwz_ctx* c, int strategy) {
    if (!c) return ZWZ_E_INVALID;
    if (!strategy_exists(strategy)) {
        set_error("zwz_ctx_set_strategy: no strategy %d; 0 (default), 2 (Z_HUFFMAN_ONLY) and 3 (Z_RLE) exist\n"
                  "  2, 3: libz's deflate_huff and deflate_rle look at no hash chain, and what becomes of a position has a closed form: one kernel in place of the search and the parse\n"
                  "  1 (Z_FILTERED): changes the lazy parse's acceptance of short matches, in three parse forms at three levels\n"
                  "  4 (Z_FIXED): changes the plan's choice of block type in its three forms\n"
                  "  each of those two is its own piece of work", strategy);
        return ZWZ_E_INVALID;
    }
    c->strategy = (uint32_t)strategy;
    return ZWZ_OK;
}

int zwz_ctx_strategy(zwz_ctx* c) { return c ? (int)c->strategy : ZWZ_E_INVALID; }

int zwz_ctx_set_level(zwz_ctx* c, int level) {
    if (!c) return ZWZ_E_INVALID;
    if (level == 0) level = kLevelDefault;
    if (level < kLevelMin || level > kLevelMax) {
        set_error("zwz_ctx_set_level: no level %d; levels 4, 5 and 6 exist (0 = the default, 6)\n"
                  "  1-3: libz's deflate_fast skips hash insertions inside matches, so the chains depend on the parse: the position-parallel search does not hold\n"
                  "  7-9: chains of 256-4096 and max_lazy up to 258: past the 128-wide band and the 13-position parse step\n"
                  "  0: a different encoder (stored blocks only)", level);
        return ZWZ_E_INVALID;
    }
    c->level = (uint32_t)level;
    return ZWZ_OK;
}

int zwz_ctx_level(zwz_ctx* c) { return c ? (int)c->level : ZWZ_E_INVALID; }
uint32_t zwz_ctx_index_span(zwz_ctx* c) { return c ? c->index_span_bytes : 0u; }

int zwz_ctx_set_option(zwz_ctx* c, const char* name, const char* value) {
    if (!c || !name || !value) return ZWZ_E_INVALID;
    const std::string n = name, v = value;
    // A form this device failed its self-test of stays off (include/zwz.h promises the same bytes from every setting, which a
    // failing kernel form would break): asking for it is ZWZ_E_NO_DEVICE, and "auto" / "wave" keep meaning "what this device can run".
    const bool no_links = c->forbidden & kForbidLinks, no_sort = c->forbidden & kForbidSort;
    auto refuse = [&](const char* what) { set_error("zwz_ctx_set_option: %s=%s needs a kernel form that failed its self-test on this device", what, v.c_str()); return ZWZ_E_NO_DEVICE; };
    if (n == "match") {
        uint32_t m;
        if (v == "auto" || v.empty()) m = kMatchAuto; else if (v == "walk") m = kMatchWalk; else if (v == "band") m = kMatchBand; else if (v == "lazy") m = kMatchLazy;
        else if (v == "autoband") m = kMatchAutoBand; else if (v == "autolazy") m = kMatchAutoLazy; else return ZWZ_E_INVALID;
        const bool needs_links = m == kMatchAuto || m == kMatchWalk || m == kMatchAutoBand || m == kMatchAutoLazy;
        const bool needs_sort = m == kMatchAuto || m == kMatchBand || m == kMatchLazy || m == kMatchAutoBand || m == kMatchAutoLazy;
        if (m == kMatchAuto && (no_links || no_sort)) m = no_sort ? kMatchWalk : kMatchBand;          // "auto" on a device with one search left: that one
        else if ((needs_links && no_links) || (needs_sort && no_sort)) return refuse("match");
        c->match_mode = m;
    } else if (n == "plan") {
        if (v == "wave" || v.empty()) { if (c->forbidden & kForbidPlanWave) { if (v.empty()) return ZWZ_OK; return refuse("plan"); } c->plan_serial = 0; }
        else if (v == "serial") c->plan_serial = 1; else return ZWZ_E_INVALID;
    } else if (n == "inflate_header") {
        if (v == "wave" || v.empty()) { if (c->forbidden & kForbidInflateWave) { if (v.empty()) return ZWZ_OK; return refuse("inflate_header"); } c->inflate_serial_header = 0; }
        else if (v == "serial") c->inflate_serial_header = 1; else return ZWZ_E_INVALID;
    } else if (n == "split_slice_bytes") {
        char* end = nullptr;
        const unsigned long long x = strtoull(v.c_str(), &end, 10);
        if (!v.empty() && (*end || end == v.c_str() || x < 4096 || x > (1ull << 28))) return ZWZ_E_INVALID;
        c->split_slice_bytes = v.empty() ? kSplitSliceBytes : (uint32_t)x & ~15u;
    } else if (n == "split_min_bytes" || n == "split_budget" || n == "split_max_candidates") {
        // zwz_inflate_split_streams_dev (split_core.h): an empty value restores the default
        char* end = nullptr;
        const unsigned long long x = strtoull(v.c_str(), &end, 10);
        if ((!v.empty() && (*end || end == v.c_str())) || x > 0x7fffffffull) return ZWZ_E_INVALID;
        if (n == "split_min_bytes") c->split_min_bytes = v.empty() ? kSplitMinBytes : (uint32_t)x;
        else if (n == "split_budget") { if (!v.empty() && x < 16) return ZWZ_E_INVALID; c->split_budget = v.empty() ? kSplitBudget : (uint32_t)x; }
        else { if (!v.empty() && x < 2) return ZWZ_E_INVALID; c->split_max_candidates = v.empty() ? kSplitMaxCandidates : (uint32_t)x; }
    } else if (n == "index_span_bytes") {
        // zwz_inflate_streams_index_dev (index_core.h): decoded bytes between two checkpoints, a power of two
        char* end = nullptr;
        const unsigned long long x = strtoull(v.c_str(), &end, 10);
        if (!v.empty() && (*end || end == v.c_str() || x > kIdxSpanMax || !index_span_ok((uint32_t)x))) return ZWZ_E_INVALID;
        c->index_span_bytes = v.empty() ? kIdxSpanDefault : (uint32_t)x;
    } else if (n == "leg_bytes" || n == "leg_out_bytes") {
        // zwz_inflate_legs_dev (leg_core.h): the compressed bytes a leg may read (a multiple of 16), the decoded bytes it may write
        char* end = nullptr;
        const unsigned long long x = strtoull(v.c_str(), &end, 10);
        const bool in = n == "leg_bytes";
        if (!v.empty() && (*end || end == v.c_str() || x < (in ? kLegBytesMin : kLegOutBytesMin) || x > (in ? kLegMaxIn : kLegOutBytesDefault) || (in && (x & 15u)))) return ZWZ_E_INVALID;
        if (in) c->leg_bytes = v.empty() ? kLegBytesDefault : x;
        else c->leg_out_bytes = v.empty() ? kLegOutBytesDefault : x;
    } else if (n == "leg_file_bytes" || n == "leg_file_out_bytes") {
        // zwz_inflate_legs_file (legfile_core.h): the staging windows a file passes through, multiples of 16
        char* end = nullptr;
        const unsigned long long x = strtoull(v.c_str(), &end, 10);
        const bool in = n == "leg_file_bytes";
        if (!v.empty() && (*end || end == v.c_str() || x < (in ? kLegFileBytesMin : kLegFileOutBytesMin) || x > (in ? kLegMaxIn : kLegFileOutBytesMax) || (x & 15u))) return ZWZ_E_INVALID;
        if (in) c->leg_file_bytes = v.empty() ? kLegFileBytesDefault : x;
        else c->leg_file_out_bytes = v.empty() ? kLegFileOutBytesDefault : x;
    } else if (n == "zip_force_zip64") {
        if (v == "0" || v.empty()) c->zip_force_zip64 = 0; else if (v == "1") c->zip_force_zip64 = 1; else return ZWZ_E_INVALID;
    } else if (n == "zip_slice_bytes") {
        char* end = nullptr;
        const unsigned long long x = strtoull(v.c_str(), &end, 10);
        if (!v.empty() && (*end || end == v.c_str() || x < 4096 || x > (1ull << 40))) return ZWZ_E_INVALID;
        c->zip_slice_bytes = v.empty() ? 268435456ull : x;
    } else return ZWZ_E_INVALID;
    return ZWZ_OK;
}

void zwz_ctx_destroy(zwz_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (Buffer& b : c->buf) b.release();
    if (c->ds_copied) (void)hipEventDestroy(c->ds_copied);
    if (c->zip_copied) (void)hipEventDestroy(c->zip_copied);
    for (auto& e : c->ev) if (e) (void)hipEventDestroy(e);
    for (auto& e : c->ev_inf) if (e) (void)hipEventDestroy(e);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

void* zwz_ctx_stream(zwz_ctx* c) { return c ? (void*)c->stream : nullptr; }

int zwz_ctx_sync(zwz_ctx* c) {
    if (!c) return ZWZ_E_INVALID;
    HIPCHK(hipStreamSynchronize(c->stream));
    return ZWZ_OK;
}

int zwz_ctx_set_profiling(zwz_ctx* c, int on) {
    if (!c) return ZWZ_E_INVALID;
    c->profiling = on != 0;
    return ZWZ_OK;
}

int zwz_ctx_stage_ms(zwz_ctx* c, float* ms, int reset) {
    if (!c || !ms) return ZWZ_E_INVALID;
    for (int i = 0; i < ZWZ_NUM_STAGES; i++) ms[i] = c->stage_ms[i];
    if (reset) for (auto& v : c->stage_ms) v = 0.f;
    return ZWZ_OK;
}

int zwz_deflate_batch_dev(zwz_ctx* c, const uint8_t* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len, uint32_t n,
                          uint8_t* d_out, uint64_t out_stride, uint32_t* d_out_len) {
    return zwz::deflate_batch_dev_skip(c, d_in, d_in_off, d_in_len, nullptr, n, d_out, out_stride, d_out_len);
}

}  // extern "C"

int zwz::deflate_batch_dev_skip(zwz_ctx* c, const uint8_t* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len, const uint32_t* d_skip, uint32_t n,
                                uint8_t* d_out, uint64_t out_stride, uint32_t* d_out_len) {
    if (!c || (n && (!d_in || !d_in_off || !d_in_len || !d_out || !d_out_len))) return ZWZ_E_INVALID;
    if (out_stride < ZWZ_DEV_STRIDE || (out_stride & 15u) || ((uintptr_t)d_in & 15u) || ((uintptr_t)d_out & 15u)) return ZWZ_E_INVALID;
    HIPCHK(hipSetDevice(c->device));
    {   // the workspace grows to the largest slice seen (never past max_batch): small jobs and pure
        // decompression never pay for the full ~5.6 GB
        const uint32_t want = n < c->max_batch ? n : c->max_batch;
        if (int rc = ensure_workspace(c, want)) return rc;
    }
    for (uint32_t done = 0; done < n; done += c->max_batch) {
        const uint32_t m = n - done < c->max_batch ? n - done : c->max_batch;
        DeflateArgs a;
        a.in = d_in; a.in_off = d_in_off + done; a.in_len = d_in_len + done; a.n = m;
        a.out = d_out + (size_t)done * out_stride; a.out_stride = out_stride; a.out_len = d_out_len + done;
        carve_workspace(c, a);
        a.skip = d_skip ? d_skip + done : nullptr;
        a.match_mode = c->match_mode; a.plan_serial = c->plan_serial; a.level = c->level; a.strategy = c->strategy;
        HIPCHK(launch_deflate(a, c->stream, c->profiling ? c->ev : nullptr));
        if (c->profiling) {   // profiling serialises slices: stage times are read back per slice
            HIPCHK(hipEventSynchronize(c->ev[kNumDeflateStages]));
            for (int i = 0; i < kNumDeflateStages; i++) {
                float ms = 0.f;
                HIPCHK(hipEventElapsedTime(&ms, c->ev[i], c->ev[i + 1]));
                c->stage_ms[i] += ms;
            }
        }
    }
    return ZWZ_OK;
}

extern "C" {

int zwz_md5_files_dev(zwz_ctx* c, const uint8_t* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len, const uint32_t* d_files,
                      uint32_t n_files, uint8_t* d_digests) {
    if (!c || (n_files && (!d_in || !d_in_off || !d_in_len || !d_files || !d_digests))) return ZWZ_E_INVALID;
    if ((uintptr_t)d_digests & 3u) return ZWZ_E_INVALID;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(launch_md5_files(d_in, d_in_off, d_in_len, d_files, n_files, reinterpret_cast<uint32_t*>(d_digests), c->stream));
    return ZWZ_OK;
}

int zwz_inflate_batch_dev(zwz_ctx* c, const uint8_t* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len, uint32_t n,
                          uint8_t* d_out, uint64_t out_stride, uint32_t* d_out_len, uint32_t* d_status) {
    if (!c || (n && (!d_in || !d_in_off || !d_in_len || !d_out || !d_out_len || !d_status))) return ZWZ_E_INVALID;
    if (out_stride < ZWZ_CHUNK_SIZE || ((uintptr_t)d_in & 15u)) return ZWZ_E_INVALID;
    HIPCHK(hipSetDevice(c->device));
    if (int rc = ensure_inf_order(c, n)) return rc;
    InflateArgs a{d_in, d_in_off, d_in_len, n, d_out, out_stride, d_out_len, d_status, c->buf[kBufInfOrder].as<uint4>(), c->inflate_serial_header};
    if (c->profiling) HIPCHK(hipEventRecord(c->ev_inf[0], c->stream));
    HIPCHK(launch_inflate(a, c->stream));
    if (c->profiling) {
        HIPCHK(hipEventRecord(c->ev_inf[1], c->stream));
        HIPCHK(hipEventSynchronize(c->ev_inf[1]));
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, c->ev_inf[0], c->ev_inf[1]));
        c->stage_ms[kNumDeflateStages] += ms;
    }
    return ZWZ_OK;
}

int zwz_inflate_streams_dev(zwz_ctx* c, int wrap, const uint8_t* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len, uint32_t n,
                            uint8_t* d_out, const uint64_t* d_out_off, const uint64_t* d_out_cap, uint64_t* d_out_len, uint32_t* d_status) {
    if (!c || wrap < ZWZ_WRAP_RAW || wrap > ZWZ_WRAP_GZIP) return ZWZ_E_INVALID;
    if (n && (!d_in || !d_in_off || !d_in_len || !d_out || !d_out_off || !d_out_cap || !d_out_len || !d_status)) return ZWZ_E_INVALID;
    if (((uintptr_t)d_in & 15u) || ((uintptr_t)d_out & 15u)) return ZWZ_E_INVALID;
    if (n == 0) return ZWZ_OK;
    HIPCHK(hipSetDevice(c->device));
    if (int rc = ensure_inf_order(c, n)) return rc;
    if (int rc = c->buf[kBufStreamRec].reserve(c, n, (size_t)n * sizeof(uint4))) return rc;     // what the decode hands the check
    if (wrap == ZWZ_WRAP_GZIP) if (int rc = ensure_crc_tables(c)) return rc;
    uint4* rec = c->buf[kBufStreamRec].as<uint4>();
    InflateStreamArgs a{d_in, d_in_off, d_in_len, n, d_out, d_out_off, d_out_cap, d_out_len, d_status, c->buf[kBufInfOrder].as<uint4>(), rec,
                        (uint32_t)wrap, c->inflate_serial_header};
    HIPCHK(launch_inflate_streams(a, c->stream));
    HIPCHK(launch_stream_check(c->buf[kBufCrcTables].as<const CrcTables>(), d_out, d_out_off, rec, n, (uint32_t)wrap, d_status,
                               c->cu_count, c->stream));
    return ZWZ_OK;
}

// ---- host-buffer variants: pack chunks into 65536-byte slots of a pinned buffer, one H2D, run,
// one D2H, unpack at the reference's 65535-byte stride.  status = null: deflate, else inflate.
static int batch_host(zwz_ctx* c, const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, uint32_t n, uint8_t* out,
                      uint32_t* out_len, uint32_t* status) {
    for (uint32_t i = 0; i < n; i++) if (in_len[i] > ZWZ_CHUNK_SIZE) return ZWZ_E_INVALID;
    HIPCHK(hipSetDevice(c->device));
    const uint32_t slice = c->max_batch;
    for (uint32_t done = 0; done < n; done += slice) {
        const uint32_t m = n - done < slice ? n - done : slice;
        int rc = ensure_staging(c, m);
        if (rc) return rc;
        StageView v = stage_view(c, 0);
        for (uint32_t i = 0; i < m; i++) {
            memcpy(v.h_in + (size_t)i * ZWZ_DEV_STRIDE, in + in_off[done + i], in_len[done + i]);
            v.h_off[i] = (uint64_t)i * ZWZ_DEV_STRIDE;
            v.h_len[i] = in_len[done + i];
        }
        HIPCHK(hipMemcpyAsync(v.d_in, v.h_in, (size_t)m * ZWZ_DEV_STRIDE, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(v.d_off, v.h_off, m * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(v.d_len, v.h_len, m * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        rc = status ? zwz_inflate_batch_dev(c, v.d_in, v.d_off, v.d_len, m, v.d_out, ZWZ_DEV_STRIDE, v.d_olen, v.d_status)
                    : zwz_deflate_batch_dev(c, v.d_in, v.d_off, v.d_len, m, v.d_out, ZWZ_DEV_STRIDE, v.d_olen);
        if (rc) return rc;
        HIPCHK(hipMemcpyAsync(v.h_out, v.d_out, (size_t)m * ZWZ_DEV_STRIDE, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(v.h_olen, v.d_olen, m * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        if (status) HIPCHK(hipMemcpyAsync(v.h_status, v.d_status, m * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        for (uint32_t i = 0; i < m; i++) {
            out_len[done + i] = v.h_olen[i];
            if (status) status[done + i] = v.h_status[i];
            memcpy(out + (size_t)(done + i) * ZWZ_CHUNK_SIZE, v.h_out + (size_t)i * ZWZ_DEV_STRIDE, v.h_olen[i]);
        }
    }
    return ZWZ_OK;
}

int zwz_deflate_batch(zwz_ctx* c, const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, uint32_t n, uint8_t* out,
                      uint32_t* out_len) {
    if (!c || (n && (!in || !in_off || !in_len || !out || !out_len))) return ZWZ_E_INVALID;
    return batch_host(c, in, in_off, in_len, n, out, out_len, nullptr);
}

int zwz_inflate_batch(zwz_ctx* c, const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, uint32_t n, uint8_t* out,
                      uint32_t* out_len, uint32_t* status) {
    if (!c || (n && (!in || !in_off || !in_len || !out || !out_len || !status))) return ZWZ_E_INVALID;
    return batch_host(c, in, in_off, in_len, n, out, out_len, status);
}

}  // extern "C"

namespace zwz {

int Buffer::reserve(zwz_ctx* c, size_t want_count, size_t want_bytes) {
    if (want_count <= count && want_bytes <= bytes) return ZWZ_OK;
    HIPCHK(hipStreamSynchronize(c->stream));
    release();
    const hipError_t e = pinned ? hipHostMalloc(&p, want_bytes, hipHostMallocDefault) : hipMalloc(&p, want_bytes);
    if (e != hipSuccess) { p = nullptr; return hip_fail(e, pinned ? "pinned buffer allocation" : "device buffer allocation"); }
    bytes = want_bytes; count = want_count;
    return ZWZ_OK;
}

void Buffer::release() {
    if (p) (void)(pinned ? hipHostFree(p) : hipFree(p));
    p = nullptr; bytes = 0; count = 0;
}

int ensure_inf_order(zwz_ctx* c, uint32_t n) { return c->buf[kBufInfOrder].reserve(c, n, (size_t)n * sizeof(uint4)); }

int ensure_crc_tables(zwz_ctx* c) {
    Buffer& b = c->buf[kBufCrcTables];
    if (b.p) return ZWZ_OK;
    if (int rc = b.reserve(c, 1, sizeof(CrcTables))) return rc;
    HIPCHK(launch_crc_tables(b.as<CrcTables>(), c->stream));
    return ZWZ_OK;
}

// The deflate workspace for n chunks
static void workspace_layout(Carver& w, size_t n, DeflateArgs& a) {
    a.entries = w.take<uint2>(n * kEntryStride);
    a.links = w.take<uint16_t>(n * kLinkStride);
    a.has128 = w.take<uint64_t>(n * kMaskWords);
    a.sym = w.take<uint64_t>(n * kMaskWords);
    a.mst = w.take<uint64_t>(n * kMaskWords);
    a.perm = w.take<uint16_t>(n * kTile);
    a.link_stat = w.take<uint32_t>(n);
    a.tickets = w.take<uint32_t>(kTicketBytes / sizeof(uint32_t));
    a.sorted = w.take<uint32_t>(n * kSortedStride);
    a.dense_list = w.take<uint32_t>(n);
    a.sparse_list = w.take<uint32_t>(n);
    a.info = w.take<ChunkInfo>(n);
    a.blocks = w.take<BlockInfo>(n * kMaxBlocks);
    a.plans = w.take<BlockOut>(n * kMaxBlocks);
    static_assert(kMaxBlocks * sizeof(BlockProbe) <= kLinkStride * sizeof(uint16_t), "probes alias the link array");
    a.probes = reinterpret_cast<BlockProbe*>(a.links);
}

int ensure_workspace(zwz_ctx* c, uint32_t chunks) {
    DeflateArgs a;
    return c->buf[kBufWorkspace].reserve(c, chunks, layout_bytes([&](Carver& w) { workspace_layout(w, chunks, a); }));
}

void carve_workspace(zwz_ctx* c, DeflateArgs& a) {
    Carver w(c->buf[kBufWorkspace].p);
    workspace_layout(w, c->buf[kBufWorkspace].count, a);
    a.cu_count = c->cu_count;
}

static void stage_layout(Carver& w, size_t cap, size_t first, uint8_t*& in, uint8_t*& out, uint64_t*& off, uint32_t*& len, uint32_t*& olen, uint32_t*& st) {
    in = w.take<uint8_t>(cap * ZWZ_DEV_STRIDE) + first * ZWZ_DEV_STRIDE;
    out = w.take<uint8_t>(cap * ZWZ_DEV_STRIDE) + first * ZWZ_DEV_STRIDE;
    off = w.take<uint64_t>(cap) + first;
    len = w.take<uint32_t>(cap) + first; olen = w.take<uint32_t>(cap) + first; st = w.take<uint32_t>(cap) + first;
}

StageView stage_view(zwz_ctx* c, uint32_t first) {
    StageView v;
    Carver h(c->buf[kBufStageHost].p), d(c->buf[kBufStageDev].p);
    stage_layout(h, c->buf[kBufStageHost].count, first, v.h_in, v.h_out, v.h_off, v.h_len, v.h_olen, v.h_status);
    stage_layout(d, c->buf[kBufStageDev].count, first, v.d_in, v.d_out, v.d_off, v.d_len, v.d_olen, v.d_status);
    return v;
}

int ensure_staging(zwz_ctx* c, uint32_t m) {
    StageView v;
    const size_t bytes = layout_bytes([&](Carver& w) { stage_layout(w, m, 0, v.d_in, v.d_out, v.d_off, v.d_len, v.d_olen, v.d_status); });
    if (int rc = c->buf[kBufStageDev].reserve(c, m, bytes)) return rc;
    return c->buf[kBufStageHost].reserve(c, m, bytes);
}

}  // namespace zwz
