// pg_hostvcf.cpp -- pg_host_vcf_parse: the host twin of the device VCF parser (pg_vcf.hip).  Plain C++ over the rules of
// pg_vcf_line.h, a thread per share of the lines; no context, no GPU.  The checker of the device form and the baseline it is
// measured against.
#include "pg_common.h"
#include "pg_vcf_line.h"
#include <algorithm>
#include <thread>

namespace {

struct VcfRule {
    const double *sizes;
    int n_sizes;
    uint64_t depth;
    uint32_t breadth;
    double maf, sizes_sum;
};

struct VcfPart { // what one thread found in its share of the slab
    std::vector<uint32_t> counts;
    std::vector<uint64_t> pos;
    std::vector<uint8_t> ref;
    std::vector<int64_t> off;
    std::vector<int32_t> clen;
    int64_t data_lines = 0, chrom_off = -1;
    uint64_t err = PG_VCF_NO_ERR;
    int first_n = -1;
    int64_t first_n_off = -1, other_n_off = -1; // the first line with sample fields, the first one with another number of them
    std::vector<int64_t> fs;                    // scratch: a line's field starts
    std::vector<PgVcfSample> smp;               // scratch: a line's samples
};

enum { VCF_SKIP = 0, VCF_DROP = 1, VCF_KEEP = 2 }; // or minus a pg_vcf_reason

int vcf_host_line(const VcfRule &R, const unsigned char *line, int64_t len, int64_t off, VcfPart &P) {
    if (len == 0) return -PG_VCF_E_EMPTY;
    if (line[0] == '#') {
        if (len >= 6 && std::memcmp(line, "#CHROM", 6) == 0) P.chrom_off = off;
        return VCF_SKIP;
    }
    ++P.data_lines;
    if (len < PG_VCF_MIN_LINE) return -PG_VCF_E_SHORT;
    if (len > 0x7fffffffLL) return -PG_VCF_E_LONG;
    std::vector<int64_t> &fs = P.fs;
    fs.clear();
    fs.push_back(0);
    for (int64_t i = 0; i < len; ++i)
        if (line[i] == '\t') fs.push_back(i + 1);
    const int64_t nfields = (int64_t)fs.size();
    fs.push_back(len + 1);
    if (nfields < PG_VCF_FIXED_FIELDS) return -PG_VCF_E_FIELDS;
    const int64_t n64 = nfields - PG_VCF_FIXED_FIELDS;
    const int n = (int)std::min<int64_t>(n64, PG_VCF_MAX_POOLS + 1);
    if (P.first_n < 0) { P.first_n = n; P.first_n_off = off; }
    else if (n != P.first_n && P.other_n_off < 0) P.other_n_off = off;
    PgVcfHead h;
    pg_vcf_head(line, fs[1], fs[2] - 1, fs[3], fs[4] - 1, fs[4], fs[5] - 1, fs[8], fs[9] - 1, &h);
    int err = h.err;
    if (n > R.n_sizes) err = pg_vcf_min_code(err, PG_VCF_E_POOLS);
    if (n > R.n_sizes || !h.ad_ok) return -err; // the samples cannot be read
    const int m = n > 0 ? pg_vcf_ad_count(line + fs[9], fs[10] - 1 - fs[9], h.ad_idx) : 0;
    P.smp.resize(n);
    int64_t covered = 0;
    bool ragged = false;
    for (int j = 0; j < n; ++j) {
        pg_vcf_sample(line + fs[9 + j], fs[10 + j] - 1 - fs[9 + j], h.ad_idx, m, h.map, &P.smp[j]);
        err = pg_vcf_min_code(err, P.smp[j].err);
        covered += P.smp[j].depth >= R.depth ? 1 : 0;
        ragged = ragged || P.smp[j].count < m;
    }
    if (err) return -err;
    if (!pg_vcf_breadth_pass(R.breadth, covered, n > 0 && P.smp[0].depth >= R.depth, n)) return VCF_DROP;
    if (n == 0) return -PG_VCF_E_NO_SAMPLES;
    if (ragged) return -PG_VCF_E_AD_RAGGED;
    if (m < 2) return VCF_DROP;
    double q = 0.0;
    for (int j = 0; j < n; ++j) q += pg_vcf_q_term(P.smp[j].v1, P.smp[j].row_sum, R.sizes[j], R.sizes_sum);
    if (!pg_vcf_maf_pass(q, R.maf)) return VCF_DROP;
    if (pg_vcf_map_out_of(h.map, m)) return -PG_VCF_E_ALLELE_OOB;
    for (int j = 0; j < n; ++j) {
        const PgVcfSample &s = P.smp[j];
        const uint32_t six[6] = {s.a, s.t, s.c, s.g, s.d, s.n};
        P.counts.insert(P.counts.end(), six, six + 6);
    }
    P.pos.push_back(h.pos);
    P.ref.push_back(h.ref);
    P.off.push_back(off);
    P.clen.push_back((int32_t)(fs[1] - 1));
    return VCF_KEEP;
}

void vcf_host_share(const VcfRule &R, const unsigned char *text, int64_t bytes, int64_t lo, int64_t hi, VcfPart &P) {
    auto line_start_at_or_after = [&](int64_t x) { // the first line start >= x
        if (x <= 0) return (int64_t)0;
        if (x >= bytes) return bytes;
        const void *nl = std::memchr(text + x - 1, '\n', (size_t)(bytes - (x - 1)));
        return nl ? (int64_t)(static_cast<const unsigned char *>(nl) - text) + 1 : bytes;
    };
    int64_t s = line_start_at_or_after(lo);
    const int64_t end = line_start_at_or_after(hi);
    while (s < end) {
        const void *nl = std::memchr(text + s, '\n', (size_t)(bytes - s));
        const int64_t e = nl ? (int64_t)(static_cast<const unsigned char *>(nl) - text) : bytes;
        int64_t len = e - s;
        if (nl && len > 0 && text[e - 1] == '\r') --len;
        const int st = vcf_host_line(R, text + s, len, s, P);
        if (st < 0) {
            P.err = std::min(P.err, pg_vcf_err_key(s, -st));
            return; // (later lines of this share cannot come first)
        }
        s = e + 1;
    }
}

} // namespace

extern "C" int pg_host_vcf_parse(const char *text_, int64_t bytes, const double *pool_sizes, int n_sizes, uint64_t min_coverage_depth,
                                 double min_coverage_breadth, double min_allele_frequency, uint32_t *counts, uint64_t *pos, uint8_t *ref,
                                 int64_t *line_off, int32_t *chrom_len, int64_t cap_loci, int64_t cap_counts, pg_vcf_info *info,
                                 int n_threads) {
    if (!info) return PG_ERR_INVALID;
    *info = pg_vcf_info{0, 0, -1, -1, 0, 0};
    if (bytes < 0 || (bytes > 0 && !text_) || !pool_sizes || n_sizes < 1 || n_sizes > PG_VCF_MAX_POOLS || cap_loci < 0 || cap_counts < 0)
        return PG_ERR_INVALID;
    const unsigned char *text = reinterpret_cast<const unsigned char *>(text_);
    VcfRule R{pool_sizes, n_sizes, min_coverage_depth, pg_vcf_breadth_threshold(min_coverage_breadth, n_sizes), min_allele_frequency, 0.0};
    for (int i = 0; i < n_sizes; ++i) R.sizes_sum += pool_sizes[i];
    const int parts = (int)std::max<int64_t>(1, std::min<int64_t>(n_threads, bytes / 4096 + 1));
    const int64_t each = (bytes + parts - 1) / parts;
    std::vector<VcfPart> P(parts);
    {
        std::vector<std::thread> th;
        for (int t = 1; t < parts; ++t)
            th.emplace_back([&, t] { vcf_host_share(R, text, bytes, std::min(bytes, t * each), std::min(bytes, (t + 1) * each), P[t]); });
        vcf_host_share(R, text, bytes, 0, std::min(bytes, each), P[0]);
        for (auto &x : th) x.join();
    }
    uint64_t err = PG_VCF_NO_ERR;
    int n = -1;
    for (int t = 0; t < parts; ++t) {
        err = std::min(err, P[t].err);
        info->data_lines += P[t].data_lines;
        info->chrom_line_off = std::max(info->chrom_line_off, P[t].chrom_off);
        if (P[t].first_n < 0) continue;
        if (n < 0) n = P[t].first_n;
        if (P[t].first_n != n) err = std::min(err, pg_vcf_err_key(P[t].first_n_off, PG_VCF_E_POOLS));
        else if (P[t].other_n_off >= 0) err = std::min(err, pg_vcf_err_key(P[t].other_n_off, PG_VCF_E_POOLS));
    }
    if (err != PG_VCF_NO_ERR) {
        info->err_line_off = (int64_t)(err >> 8);
        info->err_reason = (int32_t)(err & 0xff);
        return PG_ERR_INVALID;
    }
    int64_t kept = 0;
    for (int t = 0; t < parts; ++t) kept += (int64_t)P[t].pos.size();
    info->kept = kept;
    info->n_pools = n < 0 ? 0 : n;
    const int64_t need_counts = kept * info->n_pools * 6;
    if (kept > cap_loci || need_counts > cap_counts) return PG_ERR_INVALID;
    if (kept == 0) return PG_OK;
    if (!pos || !ref || !line_off || !chrom_len || (need_counts > 0 && !counts)) return PG_ERR_INVALID;
    int64_t at = 0;
    for (int t = 0; t < parts; ++t) {
        const int64_t k = (int64_t)P[t].pos.size();
        if (!k) continue;
        std::memcpy(pos + at, P[t].pos.data(), sizeof(uint64_t) * k);
        std::memcpy(ref + at, P[t].ref.data(), k);
        std::memcpy(line_off + at, P[t].off.data(), sizeof(int64_t) * k);
        std::memcpy(chrom_len + at, P[t].clen.data(), sizeof(int32_t) * k);
        if (!P[t].counts.empty()) std::memcpy(counts + at * info->n_pools * 6, P[t].counts.data(), sizeof(uint32_t) * P[t].counts.size());
        at += k;
    }
    return PG_OK;
}
