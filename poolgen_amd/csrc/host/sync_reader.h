// sync_reader.h -- sync text -> allele counts with the text parsed on the GPU by pg_sync_parse_dev (--sync-parser gpu): the host
// copies the text of a slab into pinned memory and hands it over, interns the chromosome names of the rows that come back and
// keeps their positions; the counts stay on the device for the operators, or come back where the caller needs them on the host.
#pragma once
#include "../../../include/poolgen_hip.h"
#include "gpu_mem.h"
#include "host_util.h"
#include <string>
#include <vector>

namespace pgh {

// One reader per thread that parses: it owns a library context of its own on `device` (a parser thread runs beside the
// context that analyses the piece before), the pinned and device copies of a slab, the labels that come back and two device
// count buffers, for piece c and piece c + 1.
class SyncReader {
public:
    explicit SyncReader(int device);
    ~SyncReader(); // PGH_TIMING=1: where the reader's time went, on stderr
    SyncReader(const SyncReader &) = delete;
    SyncReader &operator=(const SyncReader &) = delete;
    // [b, e) starts at a line start and is taken as ONE slab.  What parse_sync_buffer returns for it, except that the counts
    // are 32-bit on the device: counts_dev of the batch points into count buffer `slot` (0 or 1) of this reader and holds until
    // the next call with the same slot.  expect_n as for parse_sync_buffer.  `what` names the input in messages; their line
    // numbers count from `origin` (the start of the file).  n_threads copy the text.
    SyncBatch parse_dev(const char *b, const char *e, int expect_n, int slot, const char *origin, const std::string &what, int n_threads);
    // the same for a range of any size, in slabs, with the counts copied back into memory from `alloc`: parse_sync_buffer's batch
    SyncBatch parse_host(const char *b, const char *e, int expect_n, const SyncAlloc &alloc, const char *origin, const std::string &what,
                         int n_threads);

private:
    // one slab: its labels are appended to `sb` (last: the chromosome of the row before), its counts are in count buffer `slot`
    pg_sync_info slab(const char *s, int64_t bytes, int expect_n, int slot, const char *origin, const std::string &what, int n_threads,
                      SyncBatch &sb, int &last);
    pg_ctx *ctx_ = nullptr;
    int device_;
    size_t slab_bytes_;
    PinnedBuf pin_text_, pin_rows_;
    DeviceBuf<char> text_dev_, rows_dev_;
    DeviceBuf<uint32_t> counts_dev_[2];
    int64_t cap_loci_ = 0, cap_counts_[2] = {0, 0};
    double t_pin_ = 0, t_h2d_ = 0, t_parse_ = 0, t_labels_ = 0, t_d2h_ = 0;
    int64_t bytes_ = 0;
};

// the whole file (parse_sync_file's batch, 32-bit counts in memory from `alloc`)
SyncBatch parse_sync_file_gpu(int device, const std::string &fname, int n_threads, const SyncAlloc &alloc);

} // namespace pgh
