// piece_reader.h -- an input that is read in PIECES: while the caller works on piece c, the worker threads already parse
// piece c + 1 into the other of two pinned buffers.
#pragma once
#include "gpu_mem.h"
#include "host_util.h"
#include "pileup.h"
#include "pileup_reader.h"
#include "sync_reader.h"
#include "vcf.h"
#include <cstdlib>
#include <future>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>
#include <sys/mman.h>
#include <unistd.h>

namespace pgh {

// The text of a piece is not looked at again once it is parsed: its pages leave the mapping here, on a thread of their own,
// instead of all at once when the process ends -- unmapping 27 GB of touched file pages (6.6 M page-table entries, one thread,
// inside exit) was 0.25 s per 5 GB of input AFTER the program's last line (profiles/r04_stream_*.log).  MADV_DONTNEED on a
// read-only private file mapping only drops the entries; the page cache keeps the file.  PGH_KEEP_MAPPED=1 leaves them.
// The helper threads belong to an object that lives SHORTER than the mapping (a member of the PieceReader, which is built on a
// MappedFile that outlives it): its destructor joins them, so that no madvise is still on its way when the mapping goes (an
// exception, the fall-back to the whole-file path) and the address range may already belong to something else -- where
// MADV_DONTNEED would discard live data.
class TextDropper {
    std::mutex m_;
    std::vector<std::thread> th_;
    const bool keep_ = std::getenv("PGH_KEEP_MAPPED") != nullptr;
public:
    TextDropper() = default;
    TextDropper(const TextDropper &) = delete;
    TextDropper &operator=(const TextDropper &) = delete;
    void operator()(const char *b, const char *e) {
        if (keep_) return;
        const uintptr_t pg = (uintptr_t)sysconf(_SC_PAGESIZE);
        const uintptr_t lo = ((uintptr_t)b + pg - 1) / pg * pg, hi = (uintptr_t)e / pg * pg;
        if (hi <= lo || hi - lo < ((uintptr_t)1 << 20)) return;
        std::lock_guard<std::mutex> g(m_);
        th_.emplace_back([lo, hi] { (void)::madvise(reinterpret_cast<void *>(lo), hi - lo, MADV_DONTNEED); });
    }
    ~TextDropper() {
        for (auto &t : th_) if (t.joinable()) t.join();
    }
};

// Pieces [c0, c1) of `mf` between `cuts`, in turn.  The counts of piece c live in pinned slot c & 1 (two buffers that grow on
// demand), so the batch next() returned is valid until next() is called again.  expect_n / compact16: see parse_sync_buffer; a
// pileup piece is converted in memory with `pf`, a VCF piece on the device with the thresholds of `pf`.  sync_gpu (a sync input
// only): the text of a piece is parsed on the rank's device; SyncOnGpu::device leaves the counts there (counts_dev of the batch,
// in device slot c & 1 of the reader), SyncOnGpu::host copies them back into the pinned slot.  pileup_gpu (a pileup input only): the
// text of a piece is parsed on the rank's device and the counts come back into the pinned slot.
enum class SyncOnGpu { no, device, host };

class PieceReader {
    const MappedFile &mf_;
    const std::vector<size_t> &cuts_;
    int c_;
    const int c1_, device_, threads_;
    const InputKind kind_;
    std::unique_ptr<VcfReader> vcf_; // a VCF piece is parsed on the rank's device, by a context of the parser's own
    std::unique_ptr<SyncReader> sync_; // --sync-parser gpu: a sync piece likewise
    std::unique_ptr<PileupReader> pileup_; // --pileup-parser gpu: a pileup piece likewise
    const SyncOnGpu sync_gpu_;
    const PileupFilter &pf_;
    const int expect_n_;
    const bool compact16_;
    PinnedBuf slot_[2];
    TextDropper drop_parsed_text_;
    std::future<SyncBatch> next_; // (last: its destructor waits for the parser, which uses the members above)

    SyncBatch parse(int c) {
        (void)hipSetDevice(device_); // the pinned allocator runs on the parser's thread
        const char *b = mf_.data() + cuts_[c], *e = mf_.data() + cuts_[c + 1];
        SyncAlloc al;
        al.alloc = [s = &slot_[c & 1]](size_t bytes) { return s->reserve(bytes); };
        al.release = [](void *) {};
        SyncBatch parsed = sync_ && sync_gpu_ == SyncOnGpu::device ? sync_->parse_dev(b, e, expect_n_, c & 1, mf_.data(), "the sync input", threads_)
                           : sync_                                  ? sync_->parse_host(b, e, expect_n_, al, mf_.data(), "the sync input", threads_)
                           : kind_ == InputKind::vcf      ? vcf_->parse(b, e, al, "the VCF input", threads_)
                           : pileup_                      ? pileup_->parse(b, e, al, mf_.data(), "the pileup input", threads_)
                           : kind_ == InputKind::pileup ? parse_pileup_buffer(b, e, threads_, pf_, al)
                                                        : parse_sync_buffer(b, e, threads_, expect_n_, al, compact16_);
        drop_parsed_text_(b, e);
        return parsed;
    }
    void start() { if (c_ < c1_) next_ = std::async(std::launch::async, [this, c = c_] { return parse(c); }); }
public:
    PieceReader(const MappedFile &mf, const std::vector<size_t> &cuts, int c0, int c1, int device, int threads, InputKind kind,
                const PileupFilter &pf, int expect_n, bool compact16, SyncOnGpu sync_gpu = SyncOnGpu::no, bool pileup_gpu = false)
        : mf_(mf), cuts_(cuts), c_(c0), c1_(c1), device_(device), threads_(threads), kind_(kind), sync_gpu_(sync_gpu), pf_(pf), expect_n_(expect_n),
          compact16_(compact16) {
        if (kind_ == InputKind::vcf) vcf_ = std::make_unique<VcfReader>(device_, pf_);
        if (kind_ == InputKind::sync && sync_gpu_ != SyncOnGpu::no) sync_ = std::make_unique<SyncReader>(device_);
        if (kind_ == InputKind::pileup && pileup_gpu) pileup_ = std::make_unique<PileupReader>(device_, pf_);
        start();
    }
    bool more() const { return c_ < c1_; }
    SyncBatch next() { // the current piece, parsed; the parse of the one after it has begun when this returns
        SyncBatch sb = next_.get();
        ++c_;
        start();
        return sb;
    }
};

} // namespace pgh
