// sync_reader.cpp -- see sync_reader.h.  The device does the parsing; what is left here is per slab (copies, capacities) and per
// locus (the chromosome's name, the position).
#include "sync_reader.h"
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <thread>

namespace pgh {

namespace {
double clk() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// offsets of the three per-locus arrays inside one block of `loci` rows: 16-byte aligned each
struct LabelLayout {
    size_t pos, off, clen, bytes;
    explicit LabelLayout(int64_t loci) {
        auto up = [](size_t x) { return (x + 15) & ~(size_t)15; };
        pos = 0;
        off = pos + up(sizeof(uint64_t) * (size_t)loci);
        clen = off + up(sizeof(int64_t) * (size_t)loci);
        bytes = clen + up(sizeof(int32_t) * (size_t)loci) + 16;
    }
};
} // namespace

SyncReader::SyncReader(int device) : device_(device), slab_bytes_((size_t)256 << 20) {
    if (const char *s = std::getenv("PGH_SYNC_SLAB_BYTES")) { // (the result does not depend on it: tests force several slabs with it)
        const long long v = std::atoll(s);
        if (v > 0) slab_bytes_ = (size_t)v;
    }
    if (pg_create(&ctx_, device, nullptr) != PG_OK) throw std::runtime_error(std::string("--sync-parser gpu: ") + pg_last_error(nullptr));
}

SyncReader::~SyncReader() {
    if (std::getenv("PGH_TIMING") && bytes_ > 0)
        std::fprintf(stderr, "poolgen: sync reader on GPU %d, %.1f MB of text: copy into pinned memory %.3f s, H2D of the text %.3f s, parse call %.3f s, "
                             "D2H of the labels %.3f s, label bookkeeping %.3f s\n",
                     device_, bytes_ / 1e6, t_pin_, t_h2d_, t_parse_, t_d2h_, t_labels_);
    if (ctx_) pg_destroy(ctx_);
}

pg_sync_info SyncReader::slab(const char *s, int64_t bytes, int expect_n, int slot, const char *origin, const std::string &what, int n_threads,
                              SyncBatch &sb, int &last) {
    double t0 = clk();
    char *pin = static_cast<char *>(pin_text_.reserve((size_t)bytes));
    if (!pin) throw std::runtime_error("out of pinned memory for a slab of " + what);
    {
        const int parts = (int)std::max<int64_t>(1, std::min<int64_t>(n_threads, bytes >> 20));
        std::vector<std::thread> th;
        for (int t = 1; t < parts; ++t)
            th.emplace_back([=] { std::memcpy(pin + bytes * t / parts, s + bytes * t / parts, (size_t)(bytes * (t + 1) / parts - bytes * t / parts)); });
        std::memcpy(pin, s, (size_t)(bytes / parts));
        for (auto &x : th) x.join();
    }
    t_pin_ += clk() - t0; t0 = clk();
    text_dev_.reserve((size_t)bytes, "a slab of sync text");
    hip_ok(hipMemcpy(text_dev_.get(), pin, (size_t)bytes, hipMemcpyHostToDevice), "copy of a slab of sync text");
    t_h2d_ += clk() - t0; t0 = clk();
    bytes_ += bytes;
    pg_sync_info info;
    for (int attempt = 0;; ++attempt) { // the capacities of the slab before serve this one; when they do not, its sizes are known
        const LabelLayout lay(cap_loci_);
        char *r = rows_dev_.get();
        uint32_t *c = counts_dev_[slot].get();
        const bool have = r && c;
        const int rc = pg_sync_parse_dev(ctx_, text_dev_.get(), bytes, expect_n, have ? c : nullptr, have ? reinterpret_cast<uint64_t *>(r + lay.pos) : nullptr,
                                         have ? reinterpret_cast<int64_t *>(r + lay.off) : nullptr, have ? reinterpret_cast<int32_t *>(r + lay.clen) : nullptr,
                                         have ? cap_loci_ : 0, have ? cap_counts_[slot] : 0, &info);
        if (rc == PG_OK) break;
        if (info.err_reason) { // where the host parser throws: the line and why
            const char *line = s + info.err_line_off;
            const int64_t number = 1 + std::count(origin, line, '\n');
            const char *le = static_cast<const char *>(std::memchr(line, '\n', (size_t)(s + bytes - line)));
            const std::string first(line, std::min<size_t>(20, (size_t)((le ? le : s + bytes) - line)));
            throw std::runtime_error("Input file error, i.e. '" + what + "' at line " + std::to_string(number) + ", with the first 20 characters as: " + first +
                                     ". " + pg_last_error(ctx_));
        }
        const int64_t need_counts = info.kept * info.n_pools * 6;
        if (attempt > 0 || (have && info.kept <= cap_loci_ && need_counts <= cap_counts_[slot])) throw std::runtime_error(std::string("sync: ") + pg_last_error(ctx_));
        if (!r || info.kept > cap_loci_) {
            cap_loci_ = std::max<int64_t>(info.kept + info.kept / 8, 1024);
            rows_dev_.reset(LabelLayout(cap_loci_).bytes, "the labels of a slab of sync text");
        }
        if (!c || need_counts > cap_counts_[slot]) {
            cap_counts_[slot] = std::max<int64_t>(need_counts + need_counts / 8, 1024);
            counts_dev_[slot].reset(sizeof(uint32_t) * (size_t)cap_counts_[slot], "the counts of a slab of sync text");
        }
    }
    t_parse_ += clk() - t0; t0 = clk();
    const int64_t k = info.kept;
    if (k > 0) {
        const LabelLayout lay(cap_loci_);
        char *rows = static_cast<char *>(pin_rows_.reserve(lay.bytes));
        if (!rows) throw std::runtime_error("out of pinned memory for the labels of " + what);
        hip_ok(hipMemcpy(rows, rows_dev_.get(), lay.clen + sizeof(int32_t) * (size_t)k, hipMemcpyDeviceToHost), "copy of the labels of a slab");
        t_d2h_ += clk() - t0; t0 = clk();
        const uint64_t *pos = reinterpret_cast<const uint64_t *>(rows + lay.pos);
        const int64_t *off = reinterpret_cast<const int64_t *>(rows + lay.off);
        const int32_t *clen = reinterpret_cast<const int32_t *>(rows + lay.clen);
        sb.pos.insert(sb.pos.end(), pos, pos + k);
        std::vector<std::string> &nm = sb.chrom_names;
        const size_t at = sb.chrom_id.size();
        sb.chrom_id.resize(at + (size_t)k);
        for (int64_t i = 0; i < k; ++i) { // the chromosome's name: the one before, most of the time
            const char *name = s + off[i];
            const size_t len = (size_t)clen[i];
            if (last < 0 || nm[last].size() != len || std::memcmp(nm[last].data(), name, len) != 0) {
                last = -1;
                for (size_t j = 0; j < nm.size(); ++j)
                    if (nm[j].size() == len && std::memcmp(nm[j].data(), name, len) == 0) { last = (int)j; break; }
                if (last < 0) { nm.emplace_back(name, len); last = (int)nm.size() - 1; }
            }
            sb.chrom_id[at + (size_t)i] = last;
        }
        t_labels_ += clk() - t0;
    }
    return info;
}

SyncBatch SyncReader::parse_dev(const char *b, const char *e, int expect_n, int slot, const char *origin, const std::string &what, int n_threads) {
    hip_ok(hipSetDevice(device_), "hipSetDevice");
    SyncBatch sb;
    if (e <= b) return sb;
    int last = -1;
    const pg_sync_info info = slab(b, e - b, expect_n, slot, origin, what, n_threads, sb, last);
    sb.n = info.n_pools;
    sb.L = info.kept;
    sb.counts_dev = info.kept > 0 ? counts_dev_[slot].get() : nullptr;
    return sb;
}

SyncBatch SyncReader::parse_host(const char *b, const char *e, int expect_n, const SyncAlloc &alloc, const char *origin, const std::string &what,
                                 int n_threads) {
    hip_ok(hipSetDevice(device_), "hipSetDevice");
    SyncBatch sb;
    std::vector<uint32_t> counts;
    int n = expect_n, last = -1;
    for (const char *s = b; s < e;) {
        // the slab: as many whole lines as fit (one line when it alone is longer)
        const char *z = e;
        if ((size_t)(e - s) > slab_bytes_) {
            const void *nl = ::memrchr(s, '\n', slab_bytes_);
            if (!nl) nl = std::memchr(s + slab_bytes_, '\n', (size_t)(e - s) - slab_bytes_);
            z = nl ? (const char *)nl + 1 : e;
        }
        const pg_sync_info info = slab(s, z - s, n, 0, origin, what, n_threads, sb, last); // (n > 0: every later slab has the pools of the first)
        if (info.n_pools > 0) n = info.n_pools;
        if (info.kept > 0) {
            double t0 = clk();
            const size_t at = counts.size(), cnt = (size_t)info.kept * (size_t)info.n_pools * 6;
            counts.resize(at + cnt);
            hip_ok(hipMemcpy(counts.data() + at, counts_dev_[0].get(), sizeof(uint32_t) * cnt, hipMemcpyDeviceToHost), "copy of the counts of a slab");
            t_d2h_ += clk() - t0;
        }
        s = z;
    }
    sb.n = n;
    sb.L = (int64_t)sb.pos.size();
    if (sb.n == 0) return sb;
    const size_t cbytes = sizeof(uint32_t) * counts.size();
    sb.counts = static_cast<uint32_t *>(alloc.alloc ? alloc.alloc(cbytes ? cbytes : 1) : std::malloc(cbytes ? cbytes : 1));
    if (alloc.alloc) sb.release = alloc.release ? alloc.release : [](void *) {};
    if (!sb.counts) throw std::runtime_error("out of memory for the allele counts of " + what);
    if (cbytes) std::memcpy(sb.counts, counts.data(), cbytes);
    return sb;
}

SyncBatch parse_sync_file_gpu(int device, const std::string &fname, int n_threads, const SyncAlloc &alloc) {
    const MappedFile mf(fname);
    SyncReader reader(device);
    return reader.parse_host(mf.data(), mf.data() + mf.size(), 0, alloc, mf.data(), fname, n_threads);
}

} // namespace pgh
