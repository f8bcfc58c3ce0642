// parsed_rows.h -- the rows a text parser on the device (pg_vcf_parse_dev, pg_pileup_parse_dev) leaves for one slab, and what the
// host makes of them: one block of five arrays, copied back in one piece, appended to the batch of the range being read.
#pragma once
#include "host_util.h"
#include "pileup.h"
#include <algorithm>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

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

} // namespace pgh
