// pg_hostpileup.cpp -- pg_host_pileup_parse: the host twin of the device pileup parser (pg_pileup.hip).  Plain C++ over the
// rules of pg_pileup_line.h, a thread per share of the lines; no context, no GPU.  The checker of the device form and the
// baseline it is measured against.  Built with -ffp-contract=off: q is a sum of separately rounded products.
#include "pg_common.h"
#include "pg_pileup_line.h"
#include <algorithm>
#include <thread>

namespace {

struct PlRule {
    const double *sizes;
    int n_sizes;
    bool remove_ns, keep_lc;
    uint64_t depth;
    uint32_t breadth;
    double maf;
    PgPileupTables tab;
};

struct PlPart { // what one thread found in its share of the slab
    std::vector<uint32_t> counts;
    std::vector<uint64_t> pos;
    std::vector<uint8_t> ref;
    std::vector<int64_t> off;
    std::vector<int32_t> clen;
    int64_t lines = 0;
    uint64_t err = PG_PILEUP_NO_ERR;
    std::vector<int64_t> fs;       // scratch: a line's field starts
    std::vector<PgPileupPool> pl;  // scratch: a line's pools
};

enum { PL_DROP = 1, PL_KEEP = 2 }; // or minus a pg_pileup_reason

int pl_host_line(const PlRule &R, const unsigned char *line, int64_t len, int64_t off, PlPart &P) {
    if (len == 0) return -PG_PILEUP_E_FIELDS;
    if (len > 0x7fffffffLL) return -PG_PILEUP_E_LONG;
    std::vector<int64_t> &fs = P.fs;
    fs.clear();
    fs.push_back(0);
    for (int64_t i = 0; i < len; ++i)
        if (line[i] == '\t') fs.push_back(i + 1);
    const int64_t nfields = (int64_t)fs.size();
    fs.push_back(len + 1);
    if (nfields < 3) return -PG_PILEUP_E_FIELDS;
    uint64_t pos;
    unsigned char ref;
    int err = pg_pileup_head(line, fs[1], fs[2] - 1, fs[2], fs[3] - 1, &pos, &ref);
    const unsigned char refcls = pg_pileup_allele_class(ref, R.keep_lc);
    const int64_t npools = (nfields - 3 + 2) / 3;
    const int n = (int)std::min<int64_t>(npools, R.n_sizes);
    P.pl.resize(n);
    int64_t covered = 0;
    int phred = 0;
    for (int j = 0; j < n; ++j) {
        const int64_t f = 3 + 3 * (int64_t)j;
        const bool have_r = f + 1 < nfields, have_q = f + 2 < nfields;
        pg_pileup_pool(line, fs[f], fs[f + 1] - 1, have_r, have_r ? fs[f + 1] : 0, have_r ? fs[f + 2] - 1 : 0, have_q, have_q ? fs[f + 2] : 0,
                       have_q ? fs[f + 3] - 1 : 0, refcls, R.remove_ns, R.tab.cls, R.tab.qcls, &P.pl[j]);
        err = pg_pileup_min_code(err, P.pl[j].err);
        phred |= P.pl[j].phred;
        covered += (uint64_t)pg_pileup_depth(P.pl[j]) >= R.depth ? 1 : 0;
    }
    if (npools > R.n_sizes) err = pg_pileup_min_code(err, pg_pileup_tail(line, fs[3 + 3 * (int64_t)R.n_sizes], len, refcls, R.remove_ns, R.tab.cls, R.tab.qcls));
    if (err) return -err;
    if (npools != R.n_sizes || phred) return PL_DROP;
    if (covered < (int64_t)R.breadth) return PL_DROP;
    double q = 0.0;
    for (int j = 0; j < n; ++j) q += pg_pileup_q_term(P.pl[j].t, pg_pileup_depth(P.pl[j]), R.sizes[j]);
    if (!pg_pileup_maf_pass(q, R.maf)) return PL_DROP;
    for (int j = 0; j < n; ++j) {
        const PgPileupPool &s = P.pl[j];
        const uint32_t six[6] = {s.a, s.t, s.c, s.g, s.d, s.n};
        P.counts.insert(P.counts.end(), six, six + 6);
    }
    P.pos.push_back(pos);
    P.ref.push_back(ref);
    P.off.push_back(off);
    P.clen.push_back((int32_t)(fs[1] - 1));
    return PL_KEEP;
}

void pl_host_share(const PlRule &R, const unsigned char *text, int64_t bytes, int64_t lo, int64_t hi, PlPart &P) {
    auto line_start_at_or_after = [&](int64_t x) { // the first line start >= x
        if (x <= 0) return (int64_t)0;
        if (x >= bytes) return bytes;
        const void *nl = std::memchr(text + x - 1, '\n', (size_t)(bytes - (x - 1)));
        return nl ? (int64_t)(static_cast<const unsigned char *>(nl) - text) + 1 : bytes;
    };
    int64_t s = line_start_at_or_after(lo);
    const int64_t end = line_start_at_or_after(hi);
    bool bad = false;
    while (s < end) {
        const void *nl = std::memchr(text + s, '\n', (size_t)(bytes - s));
        const int64_t e = nl ? (int64_t)(static_cast<const unsigned char *>(nl) - text) : bytes;
        ++P.lines;
        if (!bad) { // (later lines of this share cannot come first; they are still counted)
            int64_t len = e - s;
            if (len > 0 && text[e - 1] == '\r') --len;
            const int st = pl_host_line(R, text + s, len, s, P);
            if (st < 0) {
                P.err = pg_pileup_err_key(s, -st);
                bad = true;
            }
        }
        s = e + 1;
    }
}

} // namespace

extern "C" int pg_host_pileup_parse(const char *text_, int64_t bytes, const double *pool_sizes, int n_sizes, int remove_ns,
                                    int keep_lowercase_reference, double max_base_error_rate, uint64_t min_coverage_depth,
                                    double min_coverage_breadth, double min_allele_frequency, uint32_t *counts, uint64_t *pos, uint8_t *ref,
                                    int64_t *line_off, int32_t *chrom_len, int64_t cap_loci, int64_t cap_counts, pg_pileup_info *info,
                                    int n_threads) {
    if (!info) return PG_ERR_INVALID;
    *info = pg_pileup_info{0, 0, -1, 0, 0};
    if (bytes < 0 || (bytes > 0 && !text_) || !pool_sizes || n_sizes < 1 || n_sizes > PG_PILEUP_MAX_POOLS || cap_loci < 0 || cap_counts < 0)
        return PG_ERR_INVALID;
    const unsigned char *text = reinterpret_cast<const unsigned char *>(text_);
    PlRule R;
    R.sizes = pool_sizes;
    R.n_sizes = n_sizes;
    R.remove_ns = remove_ns != 0;
    R.keep_lc = keep_lowercase_reference != 0;
    R.depth = min_coverage_depth;
    R.breadth = pg_pileup_breadth_threshold(min_coverage_breadth, n_sizes);
    R.maf = min_allele_frequency;
    pg_pileup_tables(R.keep_lc, max_base_error_rate, &R.tab);
    const int parts = (int)std::max<int64_t>(1, std::min<int64_t>(n_threads, bytes / 4096 + 1));
    const int64_t each = (bytes + parts - 1) / parts;
    std::vector<PlPart> P(parts);
    {
        std::vector<std::thread> th;
        for (int t = 1; t < parts; ++t)
            th.emplace_back([&, t] { pl_host_share(R, text, bytes, std::min(bytes, t * each), std::min(bytes, (t + 1) * each), P[t]); });
        pl_host_share(R, text, bytes, 0, std::min(bytes, each), P[0]);
        for (auto &x : th) x.join();
    }
    uint64_t err = PG_PILEUP_NO_ERR;
    for (int t = 0; t < parts; ++t) {
        err = std::min(err, P[t].err);
        info->lines += P[t].lines;
    }
    if (err != PG_PILEUP_NO_ERR) {
        info->err_line_off = (int64_t)(err >> 8);
        info->err_reason = (int32_t)(err & 0xff);
        return PG_ERR_INVALID;
    }
    int64_t kept = 0;
    for (int t = 0; t < parts; ++t) kept += (int64_t)P[t].pos.size();
    info->kept = kept;
    const int64_t need_counts = kept * n_sizes * 6;
    if (kept > cap_loci || need_counts > cap_counts) return PG_ERR_INVALID;
    if (kept == 0) return PG_OK;
    if (!counts || !pos || !ref || !line_off || !chrom_len) return PG_ERR_INVALID;
    int64_t at = 0;
    for (int t = 0; t < parts; ++t) {
        const int64_t k = (int64_t)P[t].pos.size();
        if (!k) continue;
        std::memcpy(pos + at, P[t].pos.data(), sizeof(uint64_t) * k);
        std::memcpy(ref + at, P[t].ref.data(), k);
        std::memcpy(line_off + at, P[t].off.data(), sizeof(int64_t) * k);
        std::memcpy(chrom_len + at, P[t].clen.data(), sizeof(int32_t) * k);
        std::memcpy(counts + at * n_sizes * 6, P[t].counts.data(), sizeof(uint32_t) * P[t].counts.size());
        at += k;
    }
    return PG_OK;
}
