// zwz_zip.cpp -- the "ZIP archives" section of include/zwz.h: the host-only index, the host drivers of zwz_zip_dev and zwz_unzip_dev
// around zwz_deflate_streams_dev / zwz_inflate_split_streams_dev and the kernels of zwz_zip.hip, and the two file functions.
//
// Writing compresses every entry as a gzip stream into bound-spaced staging (the 10-byte header is skipped when the data is packed,
// the CRC-32 is read from the trailer), so the staging costs about the input's size again, and the packed archive is one more copy of
// the compressed bytes than zwz_deflate_streams_dev alone makes.
#include <dirent.h>
#include <fcntl.h>
#include <sys/stat.h>
#include <time.h>
#include <utime.h>

#include <algorithm>
#include <cerrno>
#include <cstring>
#include <string>
#include <vector>

#include "dstream_core.h"
#include "zip_core.h"
#include "zwz_api_internal.h"
#include "zwz_filejob.h"
#include "zwz_zip.h"

using namespace zwz;

static_assert(sizeof(zwz_zip_entry) == sizeof(ZipEntry) && offsetof(zwz_zip_entry, made_by) == offsetof(ZipEntry, made_by), "zwz_zip_entry is zip_core.h's ZipEntry");

namespace {

int parse_result(int pr, const ZipParseError& err, const char* what) {
    if (pr == kZipParseFormat) {
        if (err.entry == ~0ull) set_error("%s: %s at byte offset %llu", what, err.what, (unsigned long long)err.offset);
        else set_error("%s: entry %llu: %s at byte offset %llu", what, (unsigned long long)err.entry, err.what, (unsigned long long)err.offset);
        return ZWZ_E_FORMAT;
    }
    return pr == kZipParseCap ? ZWZ_E_INVALID : ZWZ_OK;
}

// The device arrays of one zwz_zip_dev call: what the host uploads (ZipIn per entry and the names) and what the kernels fill
struct ZipWriteView { ZipIn* in; uint8_t* names; uint64_t *glen, *hoff, *coff; uint32_t* gst; ZipTotals* tot; };
ZipWriteView zip_write_layout(Carver& w, size_t n, size_t name_bytes) {
    ZipWriteView v;
    v.in = w.take<ZipIn>(n + 1); v.names = w.take<uint8_t>(name_bytes);           // (uploaded together: one after the other)
    v.glen = w.take<uint64_t>(n); v.hoff = w.take<uint64_t>(n); v.coff = w.take<uint64_t>(n);
    v.gst = w.take<uint32_t>(n); v.tot = w.take<ZipTotals>(1);
    return v;
}

// partial: local headers and data only, *d_out_len their length (the file function keeps the directory on the host)
int zip_launch(zwz_ctx* c, const uint8_t* d_in, const uint64_t* in_off, const uint64_t* in_len, const char* const* names, const zwz_zip_meta* meta,
               uint32_t n, uint8_t* d_out, uint64_t out_cap, uint64_t* d_out_len, uint32_t* d_status, bool partial) {
    std::vector<uint64_t> soff(n), scap(n);
    std::vector<uint32_t> nlen(n);
    uint64_t stage = 0, name_bytes = 0, tiles = 0;
    for (uint32_t i = 0; i < n; i++) {
        const size_t l = names[i] ? strlen(names[i]) : 0;
        if (l == 0 || l > 65535) { set_error("zwz_zip_dev: entry %u: a name has 1 to 65535 bytes", i); return ZWZ_E_INVALID; }
        if (in_off[i] & 15u) { set_error("zwz_zip_dev: entry %u: offsets must be multiples of 16", i); return ZWZ_E_INVALID; }
        nlen[i] = (uint32_t)l;
        scap[i] = dstream_bound(in_len[i], kWrapGzip);
        soff[i] = stage;
        stage += round_up(scap[i], 16) + 16;
        name_bytes += l;
        tiles += std::max<uint64_t>(1, (dstream_bound(in_len[i], kWrapRaw) + kZipTile - 1) / kZipTile);
    }
    if (tiles > 0x7fffffffull) { set_error("zwz_zip_dev: more than 2^31 tiles of %u bytes in one call", kZipTile); return ZWZ_E_INVALID; }
    const size_t up_bytes = round_up(((size_t)n + 1) * sizeof(ZipIn), 256) + name_bytes;
    if (!c->zip_copied) HIPCHK(hipEventCreateWithFlags(&c->zip_copied, hipEventDisableTiming));
    if (int rc = c->buf[kBufZipStage].reserve(c, 0, stage + 256)) return rc;
    if (int rc = c->buf[kBufZipDev].reserve(c, 0, layout_bytes([&](Carver& w) { zip_write_layout(w, n, name_bytes); }))) return rc;
    if (int rc = c->buf[kBufZipHost].reserve(c, 0, up_bytes)) return rc;
    Carver w(c->buf[kBufZipDev].p);
    const ZipWriteView v = zip_write_layout(w, n, name_bytes);
    // the pinned arrays may still be the source of the previous call's copy
    HIPCHK(hipEventSynchronize(c->zip_copied));
    ZipIn* h = c->buf[kBufZipHost].as<ZipIn>();
    uint8_t* hn = c->buf[kBufZipHost].as<uint8_t>() + round_up(((size_t)n + 1) * sizeof(ZipIn), 256);
    uint64_t no = 0, t = 0;
    for (uint32_t i = 0; i < n; i++) {
        ZipIn& e = h[i];
        e.soff = soff[i]; e.name_off = no; e.usize = in_len[i]; e.tfirst = t; e.name_len = nlen[i];
        e.attr = meta ? meta[i].external_attr : kZipDefaultAttr;
        e.time_date = meta ? (uint32_t)meta[i].dos_time | (uint32_t)meta[i].dos_date << 16 : (uint32_t)kZipDefaultDate << 16;
        memcpy(hn + no, names[i], nlen[i]);
        e.flags = zip_name_flags(hn + no, nlen[i]);
        no += nlen[i];
        t += std::max<uint64_t>(1, (dstream_bound(in_len[i], kWrapRaw) + kZipTile - 1) / kZipTile);
    }
    h[n] = ZipIn{};
    h[n].tfirst = t;
    static_assert(sizeof(ZipIn) % 8 == 0, "ZipIn is laid out in whole words");
    HIPCHK(hipMemcpyAsync(v.in, h, up_bytes, hipMemcpyHostToDevice, c->stream));       // (v.names follows v.in at the same distance)
    HIPCHK(hipEventRecord(c->zip_copied, c->stream));
    uint8_t* d_stage = c->buf[kBufZipStage].as<uint8_t>();
    if (n) if (int rc = zwz_deflate_streams_dev(c, ZWZ_WRAP_GZIP, d_in, in_off, in_len, n, d_stage, soff.data(), scap.data(), v.glen, v.gst)) return rc;
    ZipWrite W{};
    W.in = v.in; W.names = v.names; W.stage = d_stage; W.glen = v.glen; W.gst = v.gst; W.hoff = v.hoff; W.coff = v.coff; W.tot = v.tot;
    W.out = d_out; W.out_cap = out_cap; W.out_len = d_out_len; W.status = d_status; W.n = n; W.force64 = c->zip_force_zip64; W.partial = partial ? 1u : 0u;
    HIPCHK(launch_zip_scan(W, c->stream));
    HIPCHK(launch_zip_pack(W, (uint32_t)tiles, c->stream));
    if (!partial) HIPCHK(launch_zip_directory(W, c->stream));
    return ZWZ_OK;
}

// Device arrays of one zwz_unzip_dev call: uploaded (UnzIn per entry, then inflate's four arrays), then what the kernels fill
struct ZipReadView { UnzIn* in; uint64_t *in_off, *in_len, *out_off, *out_cap, *toff; uint32_t *tlen, *tcrc, *ist; };
size_t unz_upload_bytes(size_t n) { return round_up((n + 1) * sizeof(UnzIn), 256) + 4 * round_up(n * 8, 256); }
ZipReadView zip_read_layout(Carver& w, size_t n, size_t ctiles) {
    ZipReadView v;
    v.in = w.take<UnzIn>(n + 1);
    v.in_off = w.take<uint64_t>(n); v.in_len = w.take<uint64_t>(n); v.out_off = w.take<uint64_t>(n); v.out_cap = w.take<uint64_t>(n);
    v.toff = w.take<uint64_t>(ctiles); v.tlen = w.take<uint32_t>(ctiles); v.tcrc = w.take<uint32_t>(ctiles); v.ist = w.take<uint32_t>(n);
    return v;
}

}  // namespace

extern "C" int zwz_zip_index(const uint8_t* zip, uint64_t n, zwz_zip_entry* e, uint32_t cap, uint32_t* n_entries) {
    if (!n_entries || (n && !zip)) return ZWZ_E_INVALID;
    *n_entries = 0;
    ZipParseError err{};
    uint64_t count = 0;
    ZipMem src{zip};
    const int pr = zip_parse(src, n, reinterpret_cast<ZipEntry*>(e), cap, &count, &err);
    if (count > 0xffffffffull) { set_error("zwz_zip_index: more than 2^32 - 1 entries"); return ZWZ_E_FORMAT; }
    *n_entries = (uint32_t)count;
    return parse_result(pr, err, "zwz_zip_index");
}

extern "C" uint64_t zwz_zip_bound(const uint64_t* in_len, const char* const* names, uint32_t n) {
    uint64_t b = zip_end_bytes(true);
    for (uint32_t i = 0; i < n; i++) b += dstream_bound(in_len ? in_len[i] : 0, kWrapRaw) + zip_entry_overhead(names && names[i] ? (uint32_t)std::min<size_t>(strlen(names[i]), 65535) : 0u);
    return b;
}

extern "C" int zwz_zip_dev(zwz_ctx* c, const uint8_t* d_in, const uint64_t* in_off, const uint64_t* in_len, const char* const* names, const zwz_zip_meta* meta,
                           uint32_t n, uint8_t* d_out, uint64_t out_cap, uint64_t* d_out_len, uint32_t* d_status) {
    if (!c || !d_out || !d_out_len || !d_status) return ZWZ_E_INVALID;
    if (n && (!d_in || !in_off || !in_len || !names)) return ZWZ_E_INVALID;
    if (((uintptr_t)d_in & 15u) || ((uintptr_t)d_out & 15u)) return ZWZ_E_INVALID;
    HIPCHK(hipSetDevice(c->device));
    return zip_launch(c, d_in, in_off, in_len, names, meta, n, d_out, out_cap, d_out_len, d_status, false);
}

extern "C" int zwz_unzip_dev(zwz_ctx* c, const uint8_t* d_zip, uint64_t zip_len, const zwz_zip_entry* entries, uint32_t n, uint8_t* d_out,
                             const uint64_t* out_off, uint64_t* d_out_len, uint32_t* d_status, uint32_t* d_segments) {
    if (!c) return ZWZ_E_INVALID;
    if (n && (!d_zip || !entries || !d_out || !out_off || !d_out_len || !d_status)) return ZWZ_E_INVALID;
    if (((uintptr_t)d_zip & 15u) || ((uintptr_t)d_out & 15u)) return ZWZ_E_INVALID;
    for (uint32_t i = 0; i < n; i++) if (out_off[i] & 15u) { set_error("zwz_unzip_dev: entry %u: output offsets must be multiples of 16", i); return ZWZ_E_INVALID; }
    if (n == 0) return ZWZ_OK;
    HIPCHK(hipSetDevice(c->device));
    // what the host can judge, and the three layouts: copy tiles, staging, CRC tiles
    uint64_t tiles = 0, ctiles = 0, stage = 0;
    uint32_t n_deflated = 0;
    if (int rc = c->buf[kBufZipHost].reserve(c, 0, unz_upload_bytes(n))) return rc;
    if (!c->zip_copied) HIPCHK(hipEventCreateWithFlags(&c->zip_copied, hipEventDisableTiming));
    HIPCHK(hipEventSynchronize(c->zip_copied));
    UnzIn* h = c->buf[kBufZipHost].as<UnzIn>();
    uint64_t* h_arr = reinterpret_cast<uint64_t*>(c->buf[kBufZipHost].as<uint8_t>() + round_up(((size_t)n + 1) * sizeof(UnzIn), 256));
    const size_t stride = round_up((size_t)n * 8, 256) / 8;
    uint64_t *h_in_off = h_arr, *h_in_len = h_arr + stride, *h_out_off = h_arr + 2 * stride, *h_out_cap = h_arr + 3 * stride;
    for (uint32_t i = 0; i < n; i++) {
        const zwz_zip_entry& z = entries[i];
        UnzIn& u = h[i];
        u = UnzIn{};
        u.src = z.data_off; u.len = z.csize; u.out_off = out_off[i]; u.usize = z.usize; u.crc = z.crc32;
        u.tfirst = (uint32_t)tiles; u.ctfirst = (uint32_t)ctiles;
        if ((z.method != 0 && z.method != 8) || (z.flags & 1u)) u.pre = ZWZ_ZIP_UNSUPPORTED;
        else if (z.data_off > zip_len || z.csize > zip_len - z.data_off || (z.method == 0 && z.csize != z.usize)) u.pre = ZWZ_ZIP_BAD_ENTRY;
        else if (z.method == 8 && (z.csize >= kStreamMaxIn || z.usize >= kStreamMaxOut)) u.pre = ZWZ_STREAM_TOO_LARGE;
        h_in_off[i] = 0; h_in_len[i] = 0; h_out_off[i] = out_off[i]; h_out_cap[i] = 0;
        if (!u.pre) {
            u.kind = z.method == 8 ? kUnzDeflated : kUnzStored;
            if (u.kind == kUnzDeflated) {
                u.dst = stage;
                h_in_off[i] = stage; h_in_len[i] = z.csize; h_out_cap[i] = z.usize;
                stage += round_up(z.csize, 16) + 16;
                n_deflated++;
            } else {
                u.dst = out_off[i];
            }
            tiles += (z.csize + kZipTile - 1) / kZipTile;
            ctiles += (z.usize + kZipTile - 1) / kZipTile;
        }
        if (tiles > 0x7fffffffull || ctiles > 0x7fffffffull) { set_error("zwz_unzip_dev: more than 2^31 tiles of %u bytes up to entry %u", kZipTile, i); return ZWZ_E_INVALID; }
    }
    h[n] = UnzIn{};
    h[n].tfirst = (uint32_t)tiles; h[n].ctfirst = (uint32_t)ctiles;
    if (int rc = ensure_crc_tables(c)) return rc;
    if (int rc = c->buf[kBufZipStage].reserve(c, 0, stage + 256)) return rc;
    if (int rc = c->buf[kBufZipDev].reserve(c, 0, layout_bytes([&](Carver& w) { zip_read_layout(w, n, ctiles); }))) return rc;
    Carver w(c->buf[kBufZipDev].p);
    const ZipReadView v = zip_read_layout(w, n, ctiles);
    HIPCHK(hipMemcpyAsync(v.in, h, unz_upload_bytes(n), hipMemcpyHostToDevice, c->stream));   // (the four arrays follow v.in at the same distances)
    HIPCHK(hipEventRecord(c->zip_copied, c->stream));
    ZipRead R{};
    R.in = v.in; R.zip = d_zip; R.stage = c->buf[kBufZipStage].as<uint8_t>(); R.out = d_out; R.toff = v.toff; R.tlen = v.tlen; R.tcrc = v.tcrc;
    R.ist = v.ist; R.out_len = d_out_len; R.status = d_status; R.n = n;
    HIPCHK(launch_zip_gather(R, (uint32_t)tiles, c->stream));
    if (n_deflated) {
        // NOT asynchronous: the split decode waits for the context's stream (include/zwz.h)
        if (int rc = zwz_inflate_split_streams_dev(c, ZWZ_WRAP_RAW, R.stage, v.in_off, v.in_len, n, d_out, v.out_off, v.out_cap, d_out_len, v.ist, d_segments)) return rc;
    } else if (d_segments) {
        HIPCHK(hipMemsetAsync(d_segments, 0, (size_t)n * sizeof(uint32_t), c->stream));
    }
    HIPCHK(launch_zip_crc_layout(R, (uint32_t)ctiles, c->stream));
    HIPCHK(launch_crc32_blocks(c->buf[kBufCrcTables].as<const CrcTables>(), d_out, v.toff, v.tlen, (uint32_t)ctiles, v.tcrc, c->cu_count, c->stream));
    HIPCHK(launch_zip_verdict(R, c->stream));
    return ZWZ_OK;
}

// ---- files ------------------------------------------------------------------------------------------------------------------------
namespace {

struct DirFile { std::string name; uint64_t size; time_t mtime; uint32_t mode; };

// The regular files below dir (no symlinks, nothing through symlinked directories), names relative with '/'
int walk_dir(const std::string& dir, const std::string& rel, std::vector<DirFile>& out) {
    DIR* d = opendir(dir.c_str());
    if (!d) { set_error("cannot open directory %s", dir.c_str()); return ZWZ_E_IO; }
    std::vector<std::string> subs;
    while (dirent* e = readdir(d)) {
        const std::string nm = e->d_name;
        if (nm == "." || nm == "..") continue;
        struct stat st {};
        if (lstat((dir + "/" + nm).c_str(), &st) != 0) continue;
        if (S_ISDIR(st.st_mode)) subs.push_back(nm);
        else if (S_ISREG(st.st_mode)) out.push_back({rel + nm, (uint64_t)st.st_size, st.st_mtime, (uint32_t)st.st_mode});
    }
    closedir(d);
    for (const std::string& s : subs) if (int rc = walk_dir(dir + "/" + s, rel + s + "/", out)) return rc;
    return ZWZ_OK;
}

bool write_all(FILE* f, const void* p, size_t n) { return n == 0 || fwrite(p, 1, n, f) == n; }

int mkdirs_for(const std::string& path) {          // every directory in front of the last '/'
    for (size_t i = 1; i < path.size(); i++)
        if (path[i] == '/') {
            const std::string d = path.substr(0, i);
            if (mkdir(d.c_str(), 0777) != 0 && errno != EEXIST) { set_error("cannot create directory %s", d.c_str()); return ZWZ_E_IO; }
        }
    return ZWZ_OK;
}

// zip_parse's source for a file: two windows of the file, filled on a miss in turn (the directory and the local headers are each
// read front to back, alternately)
struct ZipFileSrc {
    int fd; uint64_t size; bool io_err = false;
    std::vector<uint8_t> win[2]; uint64_t at0[2] = {0, 0}; int next = 0;
    std::vector<uint8_t> zero;
    const uint8_t* at(uint64_t off, uint64_t len) {
        for (int k = 0; k < 2; k++) if (off >= at0[k] && off + len <= at0[k] + win[k].size()) return win[k].data() + (off - at0[k]);
        const int k = next;
        next ^= 1;
        const uint64_t want = std::min<uint64_t>(std::max<uint64_t>(len, 1u << 20), size - off);
        win[k].resize(want);
        at0[k] = off;
        uint64_t got = 0;
        while (got < want) {
            const ssize_t r = pread(fd, win[k].data() + got, want - got, (off_t)(off + got));
            if (r <= 0) break;
            got += (uint64_t)r;
        }
        if (got < len) { io_err = true; win[k].clear(); zero.assign(len, 0); return zero.data(); }
        win[k].resize(got);
        return win[k].data();
    }
};

}  // namespace

// Slices of whole files in name order.  Per slice: its files are read into pinned memory at 16-byte aligned offsets (a reader thread,
// one slice ahead), compressed and packed on the GPU (local headers and data only), and written by a writer thread while the next
// slice runs.  The host reads every entry's CRC and compressed size back out of the packed local headers and keeps the central
// records, which follow the last slice with the end records.  The buffers are sized for the largest slice: a file larger than
// "zip_slice_bytes" is a slice of its own.
extern "C" int zwz_zip_dir(zwz_ctx* c, const char* src_dir, const char* dst_zip) {
    if (!c || !src_dir || !dst_zip) return ZWZ_E_INVALID;
    HIPCHK(hipSetDevice(c->device));
    std::string base = src_dir;
    while (base.size() > 1 && base.back() == '/') base.pop_back();
    std::vector<DirFile> files;
    if (int rc = walk_dir(base, "", files)) return rc;
    std::sort(files.begin(), files.end(), [](const DirFile& a, const DirFile& b) { return a.name < b.name; });
    if (files.size() > 0xffffffffull) { set_error("zwz_zip_dir: more than 2^32 - 1 files"); return ZWZ_E_INVALID; }
    for (const DirFile& f : files) if (f.name.size() > 65535) { set_error("zwz_zip_dir: a name of %zu bytes: %s", f.name.size(), f.name.c_str()); return ZWZ_E_INVALID; }
    const uint32_t nf = (uint32_t)files.size();
    // the slices, and the largest one's needs
    std::vector<uint32_t> first{0};
    uint64_t in_max = 16, out_max = 16, in_now = 0, out_now = 0;
    uint32_t cnt_max = 1;
    for (uint32_t i = 0; i < nf; i++) {
        const uint64_t a = round_up(files[i].size, 16), o = dstream_bound(files[i].size, kWrapRaw) + kZipLocalFixed + 20u + files[i].name.size();
        if (i > first.back() && in_now + a > c->zip_slice_bytes) { first.push_back(i); in_now = 0; out_now = 0; }
        in_now += a; out_now += o;
        in_max = std::max(in_max, in_now); out_max = std::max(out_max, out_now);
        cnt_max = std::max(cnt_max, i + 1 - first.back());
    }
    first.push_back(nf);
    const size_t n_slices = first.size() - 1;
    std::string read_fail;                                      // (outlives the job, whose destructor joins the reader)
    tzset();
    FileJob job;
    job.part = std::string(dst_zip) + ".part";
    job.out = fopen(job.part.c_str(), "wb");
    if (!job.out) { set_error("cannot create %s", job.part.c_str()); return ZWZ_E_IO; }
    if (nf) if (int rc = job.alloc({in_max + 16, in_max + 16, out_max + 16, out_max + 16, 64}, {in_max + 16, out_max + 16, 64})) return rc;
    std::vector<uint8_t> central;
    std::vector<uint64_t> off(cnt_max), len(cnt_max);
    std::vector<const char*> names(cnt_max);
    std::vector<zwz_zip_meta> meta(cnt_max);
    uint64_t written = 0;
    auto read_slice = [&](size_t s, uint8_t* dst) {            // (on the reader thread)
        uint64_t at = 0;
        for (uint32_t i = first[s]; i < first[s + 1]; i++) {
            const std::string path = base + "/" + files[i].name;
            FILE* f = fopen(path.c_str(), "rb");
            bool err = f == nullptr;
            if (f) { if (read_full(f, dst + at, files[i].size, &err) != files[i].size) err = true; fclose(f); }
            if (err && read_fail.empty()) read_fail = path;
            at += round_up(files[i].size, 16);
        }
    };
    if (n_slices && nf) { job.reader = std::thread(read_slice, 0, job.hp(0)); }
    for (size_t s = 0; s < n_slices && nf; s++) {
        const int b = (int)(s & 1);
        job.reader.join();
        if (!read_fail.empty()) { job.join(); set_error("zwz_zip_dir: cannot read %s (or its size changed)", read_fail.c_str()); return ZWZ_E_IO; }
        const uint32_t m = first[s + 1] - first[s];
        uint64_t at = 0;
        for (uint32_t k = 0; k < m; k++) {
            const DirFile& f = files[first[s] + k];
            off[k] = at; len[k] = f.size; names[k] = f.name.c_str();
            struct tm tmv {};
            localtime_r(&f.mtime, &tmv);
            zip_dos_time(tmv.tm_year + 1900, tmv.tm_mon + 1, tmv.tm_mday, tmv.tm_hour, tmv.tm_min, tmv.tm_sec, &meta[k].dos_time, &meta[k].dos_date);
            meta[k].external_attr = f.mode << 16;
            at += round_up(f.size, 16);
        }
        uint64_t* d_res = job.dp<uint64_t>(2);
        uint64_t* h_res = job.hp<uint64_t>(4);
        HIPJOB(hipMemcpyAsync(job.d[0], job.h[b], at, hipMemcpyHostToDevice, c->stream));
        if (int rc = zip_launch(c, job.dp(0), off.data(), len.data(), names.data(), meta.data(), m, job.dp(1), out_max, d_res, reinterpret_cast<uint32_t*>(d_res + 1), true)) { job.join(); return rc; }
        HIPJOB(hipMemcpyAsync(h_res, d_res, 16, hipMemcpyDeviceToHost, c->stream));
        HIPJOB(hipStreamSynchronize(c->stream));
        if (s + 1 < n_slices) job.reader = std::thread(read_slice, s + 1, job.hp(b ^ 1));      // (slice s's input is on the device)
        if ((uint32_t)h_res[1] != 0 || h_res[0] > out_max) { job.join(); set_error("zwz_zip_dir: a slice needs %llu bytes, above its bound (status %u)", (unsigned long long)h_res[0], (uint32_t)h_res[1]); return ZWZ_E_FORMAT; }
        const uint64_t got = h_res[0];
        if (int rc = job.finish_write()) { job.join(); return rc; }                             // (two writes back: this buffer is free)
        uint8_t* hout = job.hp(2 + b);
        HIPJOB(hipMemcpyAsync(hout, job.d[1], got, hipMemcpyDeviceToHost, c->stream));
        HIPJOB(hipStreamSynchronize(c->stream));
        // the central records, from the local headers as they were packed
        uint64_t p = 0;
        for (uint32_t k = 0; k < m; k++) {
            const uint8_t* l = hout + p;
            ZipRec r{};
            r.name_len = zip_get16(l + 26);
            const uint32_t xlen = zip_get16(l + 28);
            r.crc = zip_get32(l + 14); r.csize = zip_get32(l + 18); r.usize = len[k];
            if (xlen) r.csize = zip_get64(l + kZipLocalFixed + r.name_len + 12);
            r.offset = written + p; r.attr = meta[k].external_attr; r.flags = (uint16_t)zip_get16(l + 6); r.time = meta[k].dos_time; r.date = meta[k].dos_date;
            r.force64 = c->zip_force_zip64;
            const size_t o = central.size();
            central.resize(o + zip_central_bytes(r.name_len, zip_big(r), zip_off_sat(r)));
            zip_write_central(central.data() + o, r);
            memcpy(central.data() + o + kZipCentralFixed, names[k], r.name_len);
            p += kZipLocalFixed + r.name_len + xlen + r.csize;
        }
        if (p != got) { job.join(); set_error("zwz_zip_dir: a slice's headers do not add up to its length"); return ZWZ_E_FORMAT; }
        job.start_write(hout, got);
        written += got;
    }
    if (int rc = job.finish_write()) return rc;
    uint8_t end[kZip64EndBytes + kZip64LocatorBytes + kZipEndBytes];
    const uint32_t end_len = zip_write_end(end, nf, central.size(), written, c->zip_force_zip64 != 0);
    if (!write_all(job.out, central.data(), central.size()) || !write_all(job.out, end, end_len)) { set_error("write error on %s", job.part.c_str()); return ZWZ_E_IO; }
    return job.commit(dst_zip);
}

// The tail and the central directory are read and checked first (zip_parse over windows of the file), then every name, before
// anything is created.  Entries are taken in the order of their data; runs of consecutive ones whose bytes (local headers included)
// and decoded bytes both fit "zip_slice_bytes" go through zwz_unzip_dev together -- a larger entry alone, the buffers sized for the
// largest run -- and their files are written by a handful of threads.
extern "C" int zwz_unzip_file(zwz_ctx* c, const char* src_zip, const char* dst_dir) {
    if (!c || !src_zip || !dst_dir) return ZWZ_E_INVALID;
    HIPCHK(hipSetDevice(c->device));
    tzset();
    FileJob job;
    job.fd = open(src_zip, O_RDONLY);
    if (job.fd < 0) { set_error("cannot open %s", src_zip); return ZWZ_E_IO; }
    struct stat st {};
    if (fstat(job.fd, &st) != 0) { set_error("cannot stat %s", src_zip); return ZWZ_E_IO; }
    ZipFileSrc src{job.fd, (uint64_t)st.st_size};
    ZipParseError err{};
    uint64_t count = 0;
    int pr = zip_parse(src, src.size, nullptr, 0, &count, &err);
    if (src.io_err) { set_error("read error on %s", src_zip); return ZWZ_E_IO; }
    if (int rc = parse_result(pr, err, "zwz_unzip_file")) return rc;
    if (count > 0xffffffffull) { set_error("zwz_unzip_file: more than 2^32 - 1 entries"); return ZWZ_E_FORMAT; }
    const uint32_t n = (uint32_t)count;
    std::vector<ZipEntry> ent(n);
    pr = zip_parse(src, src.size, ent.data(), n, &count, &err);
    if (src.io_err) { set_error("read error on %s", src_zip); return ZWZ_E_IO; }
    if (int rc = parse_result(pr, err, "zwz_unzip_file")) return rc;
    std::string base = dst_dir;
    while (base.size() > 1 && base.back() == '/') base.pop_back();
    // names: checked before anything is created
    std::vector<std::string> names(n);
    for (uint32_t i = 0; i < n; i++) {
        const uint8_t* p = src.at(ent[i].name_off, ent[i].name_len);
        names[i].assign(reinterpret_cast<const char*>(p), ent[i].name_len);
        if (src.io_err) { set_error("read error on %s", src_zip); return ZWZ_E_IO; }
        if (!zip_name_ok(p, ent[i].name_len)) { set_error("zwz_unzip_file: entry %u: the name is empty, absolute, or has a .. component, a backslash or a NUL", i); return ZWZ_E_FORMAT; }
        if (ent[i].method == 8 && (ent[i].csize >= kStreamMaxIn || ent[i].usize >= kStreamMaxOut)) {
            set_error("zwz_unzip_file: entry %u (%s): a deflated entry of %llu compressed and %llu decoded bytes is above the device call's limits (2^29, 2^32)", i, names[i].c_str(),
                      (unsigned long long)ent[i].csize, (unsigned long long)ent[i].usize);
            return ZWZ_E_FORMAT;
        }
    }
    {
        std::vector<uint32_t> by_name(n);
        for (uint32_t i = 0; i < n; i++) by_name[i] = i;
        std::sort(by_name.begin(), by_name.end(), [&](uint32_t a, uint32_t b) { return names[a] != names[b] ? names[a] < names[b] : a < b; });
        for (uint32_t k = 1; k < n; k++) if (names[by_name[k]] == names[by_name[k - 1]]) { set_error("zwz_unzip_file: entry %u: duplicate name %s", by_name[k], names[by_name[k]].c_str()); return ZWZ_E_FORMAT; }
    }
    if (mkdir(base.c_str(), 0777) != 0 && errno != EEXIST) { set_error("cannot create directory %s", base.c_str()); return ZWZ_E_IO; }
    // directories first; the files in the order of their data
    std::vector<uint32_t> order;
    for (uint32_t i = 0; i < n; i++) {
        if (names[i].back() == '/' && ent[i].usize == 0) { if (int rc = mkdirs_for(base + "/" + names[i])) return rc; }
        else order.push_back(i);
    }
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return ent[a].header_off < ent[b].header_off; });
    const uint64_t S = c->zip_slice_bytes;
    std::vector<uint32_t> first{0};
    uint64_t in_max = 16, out_max = 16, cnt_max = 1;
    {
        uint64_t lo = 0, out_now = 0;
        for (uint32_t k = 0; k < order.size(); k++) {
            const ZipEntry& e = ent[order[k]];
            const uint64_t end = e.data_off + e.csize, o = round_up(e.usize, 16);
            if (k == first.back()) lo = e.header_off;
            else if (end - lo > S || out_now + o > S) { first.push_back(k); lo = e.header_off; out_now = 0; }
            out_now += o;
            in_max = std::max(in_max, end - lo); out_max = std::max(out_max, out_now); cnt_max = std::max<uint64_t>(cnt_max, k + 1 - first.back());
        }
        first.push_back((uint32_t)order.size());
    }
    if (!order.empty()) if (int rc = job.alloc({in_max + 32, 0, out_max + 16, 0, cnt_max * 4}, {in_max + 32, out_max + 16, cnt_max * 16})) return rc;
    std::vector<zwz_zip_entry> rel(cnt_max);
    std::vector<uint64_t> ooff(cnt_max);
    for (size_t s = 0; s + 1 < first.size() && !order.empty(); s++) {
        const uint32_t k0 = first[s], m = first[s + 1] - k0;
        const uint64_t lo = ent[order[k0]].header_off;
        uint64_t hi = lo, out_now = 0;
        for (uint32_t k = 0; k < m; k++) {
            const ZipEntry& e = ent[order[k0 + k]];
            hi = std::max(hi, e.data_off + e.csize);
            memcpy(&rel[k], &e, sizeof e);
            rel[k].header_off -= lo; rel[k].data_off -= lo;
            ooff[k] = out_now;
            out_now += round_up(e.usize, 16);
        }
        const uint64_t span = hi - lo;
        uint64_t got = 0;
        while (got < span) {
            const ssize_t r = pread(job.fd, job.hp(0) + got, span - got, (off_t)(lo + got));
            if (r <= 0) { set_error("read error on %s", src_zip); return ZWZ_E_IO; }
            got += (uint64_t)r;
        }
        memset(job.hp(0) + span, 0, 16);
        uint64_t* d_len = job.dp<uint64_t>(2);
        uint32_t* d_st = reinterpret_cast<uint32_t*>(d_len + cnt_max);
        HIPCHK(hipMemcpyAsync(job.d[0], job.h[0], round_up(span, 16), hipMemcpyHostToDevice, c->stream));
        if (int rc = zwz_unzip_dev(c, job.dp(0), span, rel.data(), m, job.dp(1), ooff.data(), d_len, d_st, nullptr)) return rc;
        uint32_t* h_st = job.hp<uint32_t>(4);
        HIPCHK(hipMemcpyAsync(h_st, d_st, (size_t)m * 4, hipMemcpyDeviceToHost, c->stream));
        if (out_now) HIPCHK(hipMemcpyAsync(job.h[2], job.d[1], out_now, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        // the files of the slice, each written whole by one of a few threads; entries with a verdict get none
        const uint32_t nthreads = std::min<uint32_t>(8, m);
        std::vector<std::thread> pool;
        std::vector<int> fail(nthreads, -1);
        for (uint32_t t = 0; t < nthreads; t++)
            pool.emplace_back([&, t] {
                for (uint32_t k = t; k < m; k += nthreads) {
                    if (h_st[k]) continue;
                    const uint32_t i = order[k0 + k];
                    const ZipEntry& e = ent[i];
                    const std::string path = base + "/" + names[i];
                    bool ok = mkdirs_for(path) == ZWZ_OK;
                    FILE* f = ok ? fopen(path.c_str(), "wb") : nullptr;
                    ok = f != nullptr && write_all(f, job.hp(2) + ooff[k], e.usize);
                    if (f && fclose(f) != 0) ok = false;
                    if (!ok) { if (fail[t] < 0) fail[t] = (int)k; unlink(path.c_str()); continue; }
                    const uint32_t mode = (e.external_attr >> 16) & 0777u;
                    if ((e.made_by >> 8) == 3 && mode) chmod(path.c_str(), mode);
                    int Y, M, D, h, mi, sec;
                    zip_dos_untime(e.dos_time, e.dos_date, &Y, &M, &D, &h, &mi, &sec);
                    struct tm tmv {};
                    tmv.tm_year = Y - 1900; tmv.tm_mon = M - 1; tmv.tm_mday = D; tmv.tm_hour = h; tmv.tm_min = mi; tmv.tm_sec = sec; tmv.tm_isdst = -1;
                    const time_t when = mktime(&tmv);
                    if (when != (time_t)-1) { struct utimbuf ut { when, when }; utime(path.c_str(), &ut); }
                }
            });
        for (std::thread& t : pool) t.join();
        for (uint32_t t = 0; t < nthreads; t++) if (fail[t] >= 0) { set_error("zwz_unzip_file: cannot write %s/%s", base.c_str(), names[order[k0 + fail[t]]].c_str()); return ZWZ_E_IO; }
        for (uint32_t k = 0; k < m; k++)
            if (h_st[k]) {
                const uint32_t i = order[k0 + k];
                unlink((base + "/" + names[i]).c_str());
                const bool sum = h_st[k] == ZWZ_ZIP_CRC_MISMATCH || h_st[k] == ZWZ_ZIP_SIZE_MISMATCH;
                set_error("zwz_unzip_file: entry %u (%s) at byte offset %llu: status %u", i, names[i].c_str(), (unsigned long long)ent[i].header_off, h_st[k]);
                return sum ? ZWZ_E_CHECKSUM : ZWZ_E_FORMAT;
            }
    }
    return ZWZ_OK;
}
