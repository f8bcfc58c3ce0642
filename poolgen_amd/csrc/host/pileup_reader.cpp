// pileup_reader.cpp -- see pileup_reader.h.  The device does the parsing; what is left here is per slab (copies, capacities)
// and per KEPT locus (the chromosome's name, the sync line).
#include "pileup_reader.h"
#include "parsed_rows.h"
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <thread>
#include <fcntl.h>
#include <unistd.h>

namespace pgh {

namespace {
double clk() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
} // namespace

PileupReader::PileupReader(int device, const PileupFilter &f) : device_(device), f_(f), slab_bytes_((size_t)256 << 20) {
    if (const char *s = std::getenv("PGH_PILEUP_SLAB_BYTES")) { // (the result does not depend on it: tests force several slabs with it)
        const long long v = std::atoll(s);
        if (v > 0) slab_bytes_ = (size_t)v;
    }
    if (pg_create(&ctx_, device, nullptr) != PG_OK) throw std::runtime_error(std::string("--pileup-parser gpu: ") + pg_last_error(nullptr));
}

PileupReader::~PileupReader() {
    if (std::getenv("PGH_TIMING") && bytes_ > 0)
        std::fprintf(stderr, "poolgen: pileup reader on GPU %d, %.1f MB of text: copy into pinned memory and H2D of the text %.3f s, parse call %.3f s, "
                             "%s %.3f s\n",
                     device_, bytes_ / 1e6, t_h2d_, t_parse_, dev_written_ ? "the sync writer (--sync-writer gpu)" : "D2H of the rows and label bookkeeping", t_rows_);
    if (ctx_) pg_destroy(ctx_);
}

SyncBatch PileupReader::parse(const char *b, const char *e, const SyncAlloc &alloc, const char *origin, const std::string &what, int n_threads,
                              std::string *sync_text, DeviceSyncWriter *dev_writer) {
    hip_ok(hipSetDevice(device_), "hipSetDevice");
    if (n_threads < 1) n_threads = 1;
    SyncBatch sb;
    std::vector<uint32_t> counts;
    const int n = (int)f_.pool_sizes.size();
    int last = -1;
    for (const char *s = b; s < e;) {
        // the slab: as many whole lines as fit (one line when it alone is longer)
        const char *z = e;
        if ((size_t)(e - s) > slab_bytes_) {
            const void *nl = ::memrchr(s, '\n', slab_bytes_);
            if (!nl) nl = std::memchr(s + slab_bytes_, '\n', (size_t)(e - s) - slab_bytes_);
            z = nl ? (const char *)nl + 1 : e;
        }
        const int64_t bytes = z - s;
        double t0 = clk();
        char *pin = static_cast<char *>(pin_text_.reserve((size_t)bytes));
        if (!pin) throw std::runtime_error("out of pinned memory for a slab of " + what);
        std::memcpy(pin, s, (size_t)bytes);
        text_dev_.reserve((size_t)bytes, "a slab of pileup text");
        hip_ok(hipMemcpy(text_dev_.get(), pin, (size_t)bytes, hipMemcpyHostToDevice), "copy of a slab of pileup text");
        bytes_ += (double)bytes;
        t_h2d_ += clk() - t0; t0 = clk();
        pg_pileup_info info;
        RowLayout lay(cap_loci_, cap_counts_);
        for (int attempt = 0;; ++attempt) { // the capacities of the slab before serve this one; when they do not, its sizes are known
            lay = RowLayout(cap_loci_, cap_counts_);
            char *r = rows_dev_.get();
            const int rc = pg_pileup_parse_dev(ctx_, text_dev_.get(), bytes, f_.pool_sizes.data(), n, f_.remove_ns ? 1 : 0, f_.keep_lowercase_reference ? 1 : 0,
                                               f_.max_base_error_rate, f_.min_coverage_depth, f_.min_coverage_breadth, f_.min_allele_frequency,
                                               r ? reinterpret_cast<uint32_t *>(r + lay.counts) : nullptr, r ? reinterpret_cast<uint64_t *>(r + lay.pos) : nullptr,
                                               r ? reinterpret_cast<uint8_t *>(r + lay.ref) : nullptr, r ? reinterpret_cast<int64_t *>(r + lay.off) : nullptr,
                                               r ? reinterpret_cast<int32_t *>(r + lay.clen) : nullptr, r ? cap_loci_ : 0, r ? cap_counts_ : 0, &info);
            if (rc == PG_OK) break;
            if (info.err_reason) { // where the reference panics: the line and why
                const char *line = s + info.err_line_off;
                const int64_t number = 1 + std::count(origin, line, '\n');
                const char *le = static_cast<const char *>(std::memchr(line, '\n', (size_t)(e - line)));
                const std::string first(line, std::min<size_t>(20, (size_t)((le ? le : e) - line)));
                throw std::runtime_error("Input pileup file error, i.e. '" + what + "' at line " + std::to_string(number) +
                                         ", with the first 20 characters as: " + first + ". " + pg_last_error(ctx_));
            }
            const int64_t need_counts = info.kept * n * 6;
            if (attempt > 0 || (info.kept <= cap_loci_ && need_counts <= cap_counts_ && r)) throw std::runtime_error(std::string("pileup: ") + pg_last_error(ctx_));
            cap_loci_ = std::max<int64_t>(info.kept + info.kept / 8, 1024);
            cap_counts_ = std::max<int64_t>(need_counts + need_counts / 8, 1024);
            rows_dev_.reset(RowLayout(cap_loci_, cap_counts_).bytes, "the rows of a slab of pileup text");
        }
        const int64_t k = info.kept;
        if (k > 0 && dev_writer) { // --sync-writer gpu: the rows stay on the device, their text comes back
            t_parse_ += clk() - t0; t0 = clk();
            dev_written_ = true;
            dev_writer->append_rows(ctx_, text_dev_.get(), bytes, rows_dev_.get(), lay, k, n);
            t_rows_ += clk() - t0;
        } else if (k > 0) {
            // the rows come back in one copy: everything the device wrote lies in front of lay.ref + k (the copy waits for the emit pass)
            char *rows = static_cast<char *>(pin_rows_.reserve(lay.bytes));
            if (!rows) throw std::runtime_error("out of pinned memory for the rows of " + what);
            hip_ok(hipMemcpy(rows, rows_dev_.get(), lay.ref + (size_t)k, hipMemcpyDeviceToHost), "copy of the rows of a slab");
            t_parse_ += clk() - t0; t0 = clk();
            append_parsed_rows(rows, lay, k, n, s, sb, counts, last, n_threads, sync_text);
            t_rows_ += clk() - t0;
        } else
            t_parse_ += clk() - t0;
        s = z;
    }
    sb.n = n;
    sb.L = (int64_t)sb.pos.size();
    const size_t cbytes = sizeof(uint32_t) * counts.size();
    sb.counts = static_cast<uint32_t *>(alloc.alloc ? alloc.alloc(cbytes ? cbytes : 1) : std::malloc(cbytes ? cbytes : 1));
    if (alloc.alloc) sb.release = alloc.release ? alloc.release : [](void *) {};
    if (!sb.counts) throw std::runtime_error("out of memory for the allele counts of " + what);
    if (cbytes) std::memcpy(sb.counts, counts.data(), cbytes);
    return sb;
}

SyncBatch parse_pileup_file_gpu(int device, const std::string &fname, int n_threads, const PileupFilter &f, const SyncAlloc &alloc) {
    const MappedFile mf(fname);
    PileupReader reader(device, f);
    return reader.parse(mf.data(), mf.data() + mf.size(), alloc, mf.data(), fname, n_threads);
}

int64_t pileup_to_sync_file_gpu(int device, const std::string &fname, const std::vector<std::string> &pool_names, const PileupFilter &f,
                                const std::string &out_fname, int n_threads, bool gpu_writer) {
    const MappedFile mf(fname);
    PileupReader reader(device, f);
    if (gpu_writer) { // the lines are formatted on the device and written slab by slab; an error on the way removes the file (DeviceSyncWriter)
        std::string header = "#chr\tpos\tref";
        for (const std::string &nm : pool_names) { header.push_back('\t'); header += nm; }
        header.push_back('\n');
        DeviceSyncWriter writer(out_fname);
        writer.set_header(header);
        reader.parse(mf.data(), mf.data() + mf.size(), SyncAlloc(), mf.data(), fname, n_threads, nullptr, &writer);
        return writer.finish(header);
    }
    std::string text;
    const SyncBatch sb = reader.parse(mf.data(), mf.data() + mf.size(), SyncAlloc(), mf.data(), fname, n_threads, &text);
    const int ofd = ::open(out_fname.c_str(), O_WRONLY | O_CREAT | O_EXCL, 0644);
    if (ofd < 0) throw std::runtime_error("Unable to create file: " + out_fname + " (it must not exist)");
    FILE *fo = ::fdopen(ofd, "w");
    std::string header = "#chr\tpos\tref";
    for (const std::string &nm : pool_names) { header.push_back('\t'); header += nm; }
    header.push_back('\n');
    std::fwrite(header.data(), 1, header.size(), fo);
    std::fwrite(text.data(), 1, text.size(), fo);
    std::fclose(fo);
    return sb.L;
}

} // namespace pgh
