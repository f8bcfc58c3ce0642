// vcf.cpp -- see vcf.h.  The device does the parsing; what is left here is per slab (copies, capacities) and per KEPT locus
// (the chromosome's name, the sync line).
#include "vcf.h"
#include "parsed_rows.h"
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <thread>
#include <fcntl.h>
#include <unistd.h>

namespace pgh {

VcfReader::VcfReader(int device, const PileupFilter &f) : device_(device), f_(f), slab_bytes_((size_t)64 << 20) {
    if (const char *s = std::getenv("PGH_VCF_SLAB_BYTES")) { // (the result does not depend on it: tests force several slabs with it)
        const long long v = std::atoll(s);
        if (v > 0) slab_bytes_ = (size_t)v;
    }
    if (pg_create(&ctx_, device, nullptr) != PG_OK)
        throw std::runtime_error(std::string("a VCF input is parsed on the GPU and there is no host fallback: ") + pg_last_error(nullptr));
}

VcfReader::~VcfReader() {
    if (ctx_) pg_destroy(ctx_);
}

// "#chr\tpos\tref\t" + the pool names: fields 9.. of a "#CHROM" line (vcf.rs:343-359); false when the line has no such fields
static bool vcf_sync_header(const std::string &chrom_line, std::string &header) {
    std::string names;
    int field = 0;
    for (size_t i = 0; i < chrom_line.size(); ++i) {
        if (chrom_line[i] == '\t') {
            ++field;
            if (field > 9) names.push_back('\t');
        } else if (field >= 9)
            names.push_back(chrom_line[i]);
    }
    header = "#chr\tpos\tref\t" + names + "\n";
    return field >= 9;
}

SyncBatch VcfReader::parse(const char *b, const char *e, const SyncAlloc &alloc, const std::string &what, int n_threads, std::string *sync_text,
                           std::string *chrom_line, DeviceSyncWriter *dev_writer) {
    hip_ok(hipSetDevice(device_), "hipSetDevice");
    if (n_threads < 1) n_threads = 1;
    SyncBatch sb;
    std::vector<uint32_t> counts;
    int n = -1;
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
        char *pin = static_cast<char *>(pin_text_.reserve((size_t)bytes));
        if (!pin) throw std::runtime_error("out of pinned memory for a slab of " + what);
        std::memcpy(pin, s, (size_t)bytes);
        text_dev_.reserve((size_t)bytes, "a slab of VCF text");
        hip_ok(hipMemcpy(text_dev_.get(), pin, (size_t)bytes, hipMemcpyHostToDevice), "copy of a slab of VCF text");
        pg_vcf_info info;
        RowLayout lay(cap_loci_, cap_counts_);
        for (int attempt = 0;; ++attempt) { // the capacities of the slab before serve this one; when they do not, its sizes are known
            lay = RowLayout(cap_loci_, cap_counts_);
            char *r = rows_dev_.get();
            const int rc = pg_vcf_parse_dev(ctx_, text_dev_.get(), bytes, f_.pool_sizes.data(), (int)f_.pool_sizes.size(), f_.min_coverage_depth,
                                            f_.min_coverage_breadth, f_.min_allele_frequency, r ? reinterpret_cast<uint32_t *>(r + lay.counts) : nullptr,
                                            r ? reinterpret_cast<uint64_t *>(r + lay.pos) : nullptr, r ? reinterpret_cast<uint8_t *>(r + lay.ref) : nullptr,
                                            r ? reinterpret_cast<int64_t *>(r + lay.off) : nullptr, r ? reinterpret_cast<int32_t *>(r + lay.clen) : nullptr,
                                            r ? cap_loci_ : 0, r ? cap_counts_ : 0, &info);
            if (rc == PG_OK) break;
            if (info.err_reason) { // where the reference panics: the line, as its message names it, and why
                const char *line = s + info.err_line_off;
                int64_t number = 1 + std::count(b, line, '\n');
                const char *le = static_cast<const char *>(std::memchr(line, '\n', (size_t)(e - line)));
                const std::string first(line, std::min<size_t>(20, (size_t)((le ? le : e) - line)));
                throw std::runtime_error("Input file error, i.e. '" + what + "' at line " + std::to_string(number) +
                                         " of the range read, with the first 20 characters as: " + first + ". " + pg_last_error(ctx_));
            }
            const int64_t need_counts = info.kept * info.n_pools * 6;
            if (attempt > 0 || (info.kept <= cap_loci_ && need_counts <= cap_counts_ && r)) throw std::runtime_error(std::string("vcf: ") + pg_last_error(ctx_));
            cap_loci_ = std::max<int64_t>(info.kept + info.kept / 8, 1024);
            cap_counts_ = std::max<int64_t>(need_counts + need_counts / 8, 1024);
            rows_dev_.reset(RowLayout(cap_loci_, cap_counts_).bytes, "the rows of a slab of VCF text");
        }
        if (chrom_line && info.chrom_line_off >= 0) {
            const char *line = s + info.chrom_line_off;
            const char *le = static_cast<const char *>(std::memchr(line, '\n', (size_t)(z - line)));
            le = le ? le : z;
            if (le > line && le[-1] == '\r' && le < z) --le;
            chrom_line->assign(line, le);
            std::string header;
            if (dev_writer && vcf_sync_header(*chrom_line, header)) dev_writer->set_header(header);
        }
        if (info.data_lines > 0) {
            if (n < 0) n = info.n_pools;
            else if (n != info.n_pools) throw std::runtime_error("Input file error, i.e. '" + what + "': the number of samples changes inside the file");
        }
        const int64_t k = info.kept;
        if (k > 0 && dev_writer) // --sync-writer gpu: the rows stay on the device, their text comes back
            dev_writer->append_rows(ctx_, text_dev_.get(), bytes, rows_dev_.get(), lay, k, n);
        else if (k > 0) {
            // the rows come back in one copy: everything the device wrote lies in front of lay.ref + k
            char *rows = static_cast<char *>(pin_rows_.reserve(lay.bytes));
            if (!rows) throw std::runtime_error("out of pinned memory for the rows of " + what);
            hip_ok(hipMemcpy(rows, rows_dev_.get(), lay.ref + (size_t)k, hipMemcpyDeviceToHost), "copy of the rows of a slab");
            append_parsed_rows(rows, lay, k, n, s, sb, counts, last, n_threads, sync_text);
        }
        s = z;
    }
    sb.n = n > 0 ? n : (int)f_.pool_sizes.size();
    sb.L = (int64_t)sb.pos.size();
    const size_t cbytes = sizeof(uint32_t) * counts.size();
    sb.counts = static_cast<uint32_t *>(alloc.alloc ? alloc.alloc(cbytes ? cbytes : 1) : std::malloc(cbytes ? cbytes : 1));
    if (alloc.alloc) sb.release = alloc.release ? alloc.release : [](void *) {};
    if (!sb.counts) throw std::runtime_error("out of memory for the allele counts of " + what);
    if (cbytes) std::memcpy(sb.counts, counts.data(), cbytes);
    return sb;
}

SyncBatch parse_vcf_file(int device, const std::string &fname, int n_threads, const PileupFilter &f, const SyncAlloc &alloc) {
    const MappedFile mf(fname);
    VcfReader reader(device, f);
    return reader.parse(mf.data(), mf.data() + mf.size(), alloc, fname, n_threads);
}

int64_t vcf_to_sync_file(int device, const std::string &fname, const PileupFilter &f, const std::string &out_fname, int n_threads,
                         bool gpu_writer) {
    const MappedFile mf(fname);
    VcfReader reader(device, f);
    std::string text, chrom_line, header;
    const char *no_names = "Pool names not found, please check the header line of the vcf file. Make sure `#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT...` header exists.";
    if (gpu_writer) { // the lines are formatted on the device and written slab by slab; an error on the way removes the file (DeviceSyncWriter)
        DeviceSyncWriter writer(out_fname);
        reader.parse(mf.data(), mf.data() + mf.size(), SyncAlloc(), fname, n_threads, nullptr, &chrom_line, &writer);
        if (!vcf_sync_header(chrom_line, header)) throw std::runtime_error(no_names);
        return writer.finish(header);
    }
    const SyncBatch sb = reader.parse(mf.data(), mf.data() + mf.size(), SyncAlloc(), fname, n_threads, &text, &chrom_line);
    // the pool names: fields 9.. of the last #CHROM line (vcf.rs:343-359)
    if (!vcf_sync_header(chrom_line, header)) throw std::runtime_error(no_names);
    const int ofd = ::open(out_fname.c_str(), O_WRONLY | O_CREAT | O_EXCL, 0644);
    if (ofd < 0) throw std::runtime_error("Unable to create file: " + out_fname + " (it must not exist)");
    FILE *fo = ::fdopen(ofd, "w");
    std::fwrite(header.data(), 1, header.size(), fo);
    std::fwrite(text.data(), 1, text.size(), fo);
    std::fclose(fo);
    return sb.L;
}

} // namespace pgh
