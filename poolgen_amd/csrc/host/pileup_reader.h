// pileup_reader.h -- mpileup text -> allele counts with the text parsed on the GPU by pg_pileup_parse_dev (--pileup-parser gpu):
// the host maps the file, cuts it at line starts, hands the slabs over from pinned memory, interns the chromosome names of the
// rows that come back and, for pileup2sync, writes their sync lines.  The default, parse_pileup_buffer on the host's threads
// (pileup.h), gives the same rows.
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
class PileupReader {
public:
    PileupReader(int device, const PileupFilter &f);
    ~PileupReader(); // PGH_TIMING=1: where the reader's time went, on stderr
    PileupReader(const PileupReader &) = delete;
    PileupReader &operator=(const PileupReader &) = delete;
    // [b, e) starts at a line start.  The counts of the kept loci in file order at the column POSITIONS pileup_to_sync writes,
    // i.e. what parse_pileup_buffer returns.  `what` names the input in messages; line numbers in them count from `origin`
    // (the start of the file).  With `sync_text` the lines pileup2sync writes are appended to it (n_threads format them).  With
    // `dev_writer` (--sync-writer gpu) the rows are not copied back: the device formats their sync lines, the writer appends them
    // to its file, and the batch returned is empty.
    SyncBatch parse(const char *b, const char *e, const SyncAlloc &alloc, const char *origin, const std::string &what, int n_threads = 1,
                    std::string *sync_text = nullptr, DeviceSyncWriter *dev_writer = nullptr);

private:
    pg_ctx *ctx_ = nullptr;
    int device_;
    PileupFilter f_;
    size_t slab_bytes_;
    PinnedBuf pin_text_, pin_rows_;
    DeviceBuf<char> text_dev_;
    DeviceBuf<char> rows_dev_;
    int64_t cap_loci_ = 0, cap_counts_ = 0;
    double bytes_ = 0, t_h2d_ = 0, t_parse_ = 0, t_rows_ = 0;
    bool dev_written_ = false; // a DeviceSyncWriter took the rows: t_rows_ is its time
};

// Whole file: what pileup_to_sync_file writes (the same header, the same refusal to overwrite, which the caller has probed
// before), the lines formatted by append_sync_line on n_threads threads or, with gpu_writer (--sync-writer gpu), on the device by
// pg_sync_format_rows_dev.  Returns the number of loci written.
int64_t pileup_to_sync_file_gpu(int device, const std::string &fname, const std::vector<std::string> &pool_names, const PileupFilter &f,
                                const std::string &out_fname, int n_threads, bool gpu_writer = false);
SyncBatch parse_pileup_file_gpu(int device, const std::string &fname, int n_threads, const PileupFilter &f, const SyncAlloc &alloc);

} // namespace pgh
