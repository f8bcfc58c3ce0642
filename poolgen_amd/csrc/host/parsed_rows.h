// parsed_rows.h -- the rows a text parser on the device (pg_vcf_parse_dev, pg_pileup_parse_dev) leaves for one slab, and what the
// host makes of them: one block of five arrays, copied back in one piece, appended to the batch of the range being read -- or,
// for a conversion with --sync-writer gpu, left on the device and formatted there (DeviceSyncWriter).
#pragma once
#include "../../../include/poolgen_hip.h"
#include "gpu_mem.h"
#include "host_util.h"
#include "pileup.h"
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>
#include <fcntl.h>
#include <unistd.h>

namespace pgh {

// offsets of the five per-locus arrays inside one block of `loci` rows, behind `counts` elements: 16-byte aligned each
struct RowLayout {
    size_t counts, pos, off, clen, ref, bytes;
    RowLayout(int64_t loci, int64_t ncounts) {
        auto up = [](size_t x) { return (x + 15) & ~(size_t)15; };
        counts = 0;
        pos = up(sizeof(uint32_t) * (size_t)ncounts);
        off = pos + up(sizeof(uint64_t) * (size_t)loci);
        clen = off + up(sizeof(int64_t) * (size_t)loci);
        ref = clen + up(sizeof(int32_t) * (size_t)loci);
        bytes = ref + up((size_t)loci) + 16;
    }
};

// `rows`: the host copy of a block laid out by `lay`, of which the first k rows of n pools are valid; `slab`: the text the rows'
// line offsets point into.  Appends counts and positions, interns the chromosome names (`last`: the name of the row before, -1 at
// first) and, with `sync_text`, appends the rows' sync lines to it (n_threads format them).
inline void append_parsed_rows(const char *rows, const RowLayout &lay, int64_t k, int n, const char *slab, SyncBatch &sb, std::vector<uint32_t> &counts,
                               int &last, int n_threads, std::string *sync_text) {
    const uint32_t *c = reinterpret_cast<const uint32_t *>(rows + lay.counts);
    const uint64_t *pos = reinterpret_cast<const uint64_t *>(rows + lay.pos);
    const int64_t *off = reinterpret_cast<const int64_t *>(rows + lay.off);
    const int32_t *clen = reinterpret_cast<const int32_t *>(rows + lay.clen);
    const uint8_t *ref = reinterpret_cast<const uint8_t *>(rows + lay.ref);
    counts.insert(counts.end(), c, c + (size_t)k * n * 6);
    sb.pos.insert(sb.pos.end(), pos, pos + k);
    std::vector<std::string> &nm = sb.chrom_names;
    for (int64_t i = 0; i < k; ++i) { // the chromosome's name: the one before, most of the time
        const char *name = slab + off[i];
        const size_t len = (size_t)clen[i];
        if (last < 0 || nm[last].size() != len || std::memcmp(nm[last].data(), name, len) != 0) {
            last = -1;
            for (size_t j = 0; j < nm.size(); ++j)
                if (nm[j].size() == len && std::memcmp(nm[j].data(), name, len) == 0) { last = (int)j; break; }
            if (last < 0) { nm.emplace_back(name, len); last = (int)nm.size() - 1; }
        }
        sb.chrom_id.push_back(last);
    }
    if (!sync_text) return;
    const int parts = (int)std::min<int64_t>(n_threads, k);
    std::vector<std::string> text(parts);
    std::vector<std::thread> th;
    for (int t = 0; t < parts; ++t)
        th.emplace_back([&, t] {
            for (int64_t i = k * t / parts; i < k * (t + 1) / parts; ++i)
                append_sync_line(text[t], slab + off[i], (size_t)clen[i], pos[i], ref[i], n, c + (size_t)i * n * 6);
        });
    for (auto &x : th) x.join();
    for (const std::string &t : text) *sync_text += t;
}

// --sync-writer gpu: the sync file of a conversion whose lines the device formats (pg_sync_format_rows_dev).  Per slab the rows
// stay where the parser left them; only their text comes back, into pinned memory, and is appended to the file.  The file is
// created at construction (it must not exist) and written slab by slab, so an error on the way must not leave it behind: the
// destructor REMOVES the file unless finish() has been reached.
class DeviceSyncWriter {
public:
    explicit DeviceSyncWriter(const std::string &out_fname) : fname_(out_fname) {
        const int ofd = ::open(out_fname.c_str(), O_WRONLY | O_CREAT | O_EXCL, 0644);
        if (ofd < 0) throw std::runtime_error("Unable to create file: " + out_fname + " (it must not exist)");
        fo_ = ::fdopen(ofd, "w");
    }
    ~DeviceSyncWriter() {
        if (fo_) { std::fclose(fo_); ::unlink(fname_.c_str()); }
        if (std::getenv("PGH_TIMING") && text_bytes_ > 0)
            std::fprintf(stderr, "poolgen: sync writer on the GPU, %.1f MB of text: format calls %.3f s, D2H of the text %.3f s, file writes %.3f s\n",
                         text_bytes_ / 1e6, t_format_, t_d2h_, t_write_);
    }
    DeviceSyncWriter(const DeviceSyncWriter &) = delete;
    DeviceSyncWriter &operator=(const DeviceSyncWriter &) = delete;
    // the header line (with its newline) as far as it is known; the one in force when the first lines arrive is written in front of them
    void set_header(const std::string &h) { header_ = h; }
    // the k rows of n pools that a parser on `ctx` left in the device block `rows_dev` (laid out by `lay`), parsed from the
    // slab_bytes bytes at slab_dev
    void append_rows(pg_ctx *ctx, const char *slab_dev, int64_t slab_bytes, const char *rows_dev, const RowLayout &lay, int64_t k, int n) {
        auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
        double t0 = now();
        int64_t need = 0;
        for (int attempt = 0;; ++attempt) { // the buffer of the slab before serves this one; when it does not, the size is known
            const int rc = pg_sync_format_rows_dev(ctx, slab_dev, slab_bytes, reinterpret_cast<const uint32_t *>(rows_dev + lay.counts),
                                                   reinterpret_cast<const uint64_t *>(rows_dev + lay.pos), reinterpret_cast<const uint8_t *>(rows_dev + lay.ref),
                                                   reinterpret_cast<const int64_t *>(rows_dev + lay.off), reinterpret_cast<const int32_t *>(rows_dev + lay.clen),
                                                   n, k, text_dev_.get(), cap_, &need);
            if (rc == PG_OK) break;
            if (attempt > 0 || need <= cap_) throw std::runtime_error(std::string("--sync-writer gpu: ") + pg_last_error(ctx));
            cap_ = need + need / 8;
            text_dev_.reset((size_t)cap_, "the sync lines of a slab");
        }
        hip_ok(hipDeviceSynchronize(), "formatting the sync lines of a slab");
        t_format_ += now() - t0; t0 = now();
        char *pin = static_cast<char *>(pin_.reserve((size_t)need));
        if (!pin) throw std::runtime_error("out of pinned memory for the sync lines of a slab");
        hip_ok(hipMemcpy(pin, text_dev_.get(), (size_t)need, hipMemcpyDeviceToHost), "copy of the sync lines of a slab");
        t_d2h_ += now() - t0; t0 = now();
        if (!started_) { put(header_.data(), header_.size()); written_header_ = header_; started_ = true; }
        put(pin, (size_t)need);
        t_write_ += now() - t0;
        text_bytes_ += (double)need;
        loci_ += k;
    }
    // The last step: `header` is the header line the file must start with.  It is the one already written, unless the input named
    // its pools only behind its first kept lines (a VCF whose last "#CHROM" line follows data lines): the lines are then copied
    // behind the right header into a file that takes this one's place.  Returns the number of loci written.
    int64_t finish(const std::string &header) {
        if (!started_) { put(header.data(), header.size()); written_header_ = header; started_ = true; }
        if (std::fclose(fo_) != 0) { fo_ = nullptr; ::unlink(fname_.c_str()); throw std::runtime_error("write error on " + fname_); }
        fo_ = nullptr;
        if (written_header_ != header) {
            const std::string tmp = fname_ + ".header-rewrite";
            try {
                FILE *in = std::fopen(fname_.c_str(), "r");
                const int ofd = ::open(tmp.c_str(), O_WRONLY | O_CREAT | O_EXCL, 0644);
                FILE *out = ofd >= 0 ? ::fdopen(ofd, "w") : nullptr;
                bool ok = in && out && std::fseek(in, (long)written_header_.size(), SEEK_SET) == 0 &&
                          std::fwrite(header.data(), 1, header.size(), out) == header.size();
                std::vector<char> buf(1 << 20);
                for (size_t got; ok && (got = std::fread(buf.data(), 1, buf.size(), in)) > 0;) ok = std::fwrite(buf.data(), 1, got, out) == got;
                if (in) std::fclose(in);
                if (out) ok = std::fclose(out) == 0 && ok;
                if (!ok || std::rename(tmp.c_str(), fname_.c_str()) != 0) throw std::runtime_error("write error on " + fname_);
            } catch (...) {
                ::unlink(tmp.c_str());
                ::unlink(fname_.c_str());
                throw;
            }
        }
        return loci_;
    }

private:
    void put(const char *p, size_t bytes) {
        if (bytes && std::fwrite(p, 1, bytes, fo_) != bytes) throw std::runtime_error("write error on " + fname_);
    }
    std::string fname_, header_, written_header_;
    FILE *fo_ = nullptr;
    bool started_ = false;
    DeviceBuf<char> text_dev_;
    PinnedBuf pin_;
    int64_t cap_ = 0, loci_ = 0;
    double text_bytes_ = 0, t_format_ = 0, t_d2h_ = 0, t_write_ = 0;
};

} // namespace pgh
