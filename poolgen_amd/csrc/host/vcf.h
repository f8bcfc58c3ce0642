// vcf.h -- VCF text -> allele counts, the `vcf2sync` front end (base/vcf.rs), with the text parsed on the GPU by
// pg_vcf_parse_dev: the host maps the file, cuts it at line starts, hands the slabs over from pinned memory, interns the
// chromosome names of the rows that come back and, for vcf2sync, writes their sync lines.
#pragma once
#include "../../../include/poolgen_hip.h"
#include "gpu_mem.h"
#include "host_util.h"
#include "pileup.h"
#include <string>
#include <vector>

namespace pgh {

class DeviceSyncWriter; // parsed_rows.h

// One reader per thread that parses: it owns a library context of its own on `device` (a parser thread runs beside the
// context that analyses the piece before), the pinned and device copies of a slab and the rows that come back.
class VcfReader {
public:
    VcfReader(int device, const PileupFilter &f); // of `f`: min_coverage_depth, min_coverage_breadth, min_allele_frequency, pool_sizes
    ~VcfReader();
    VcfReader(const VcfReader &) = delete;
    VcfReader &operator=(const VcfReader &) = delete;
    // [b, e) starts at a line start.  The counts of the kept loci in file order, at the column POSITIONS vcf_to_sync writes
    // (A:T:C:G:D:N, which the sync reader reads back as A,T,C,G,N,D: the quirk of pileup inputs), i.e. what parse_sync_buffer
    // returns for the sync text of these lines.  `what` names the input in messages; line numbers in them count from
    // `first_line`.  With `sync_text` the lines vcf2sync writes are appended to it (n_threads format them), and the text of
    // the last "#CHROM" line of the range replaces *chrom_line (when there is one).  With `dev_writer` (--sync-writer gpu) the rows
    // are not copied back: the device formats their sync lines, the writer appends them to its file and learns the header of every
    // "#CHROM" line on the way, and the batch returned is empty.
    SyncBatch parse(const char *b, const char *e, const SyncAlloc &alloc, const std::string &what, int n_threads = 1,
                    std::string *sync_text = nullptr, std::string *chrom_line = nullptr, DeviceSyncWriter *dev_writer = nullptr);

private:
    pg_ctx *ctx_ = nullptr;
    int device_;
    PileupFilter f_;
    size_t slab_bytes_;
    PinnedBuf pin_text_, pin_rows_;
    DeviceBuf<char> text_dev_;
    DeviceBuf<char> rows_dev_;
    int64_t cap_loci_ = 0, cap_counts_ = 0;
};

// Whole file (vcf.rs:306-425): header "#chr\tpos\tref\t" + the sample names of the last #CHROM line; refuses to overwrite,
// which the caller has probed before.  Returns the number of loci written.  gpu_writer (--sync-writer gpu): the lines are formatted
// on the device (pg_sync_format_rows_dev) instead of by n_threads host threads; the file is the same.
int64_t vcf_to_sync_file(int device, const std::string &fname, const PileupFilter &f, const std::string &out_fname, int n_threads,
                         bool gpu_writer = false);
SyncBatch parse_vcf_file(int device, const std::string &fname, int n_threads, const PileupFilter &f, const SyncAlloc &alloc);

} // namespace pgh
