// pg_vcf.hip -- vcf2sync's reader on the device: a slab of VCF text to the allele counts of the loci that VcfLine::filter keeps
// (base/vcf.rs; the rules, shared with the host twin, are pg_vcf_line.h).  Four steps on the context's stream;
// the index, the scans and the lane-group steps are the shared ones of pg_text_steps.h:
//   index   PgLineIndex: k_text_index<false> (newlines per 4 KB of text: a lane reads one aligned 16-byte word) + k_scan_blocks
//           (64-bit exclusive scan of the workgroups' sums, 1024 per round) + k_text_index<true> (the same read again, a block scan,
//           and every newline writes the start of the line behind it): start[0 .. lines], no host work per line;
//   parse   k_vcf_parse<false>: a line is taken by a GROUP of lanes (8 .. 64, a power of two chosen from the number of pool sizes,
//           so that 5 pools have 8 lines in a wave and 200 pools one line across it).  The group walks its line in chunks of one
//           byte per lane; a ballot on '\t' and a popcount of the lower lanes give a byte's field index, and the field starts go
//           to LDS.  The fixed fields (POS, REF, ALT, FORMAT) are read by every lane alike -- a few bytes, the same address in all
//           lanes -- so nothing has to be passed round; then lane j takes samples j, j + lanes, ..: it steps over ':' to the AD
//           piece and reads the comma list.  The filter follows the reference's order of operations; q, the one fp64 sum, is
//           formed in pool order, the terms passing through lane shuffles one after the other (a tree would be faster and not
//           bit-equal).  One int per line comes out: kept, data line, number of samples; a line where the reference would
//           panic enters (offset, reason) into one 64-bit atomicMin;
//   scan    k_vcf_keep (scan_keep_flags: exclusive scan of 256 keep flags per workgroup, data lines counted; then, VCF's own, the
//           sample numbers compared with the first data line's) + k_scan_blocks: a kept line's rank is scan_rank(local, blockoff, line);
//   emit    k_vcf_parse<true>: the kept lines are split and read again (the text is in cache or cheap to fetch beside what a
//           staging copy of every line's counts would cost) and write their rows at their rank.
// No array is indexed at run time in a thread: a sample's numbers are the named members of PgVcfSample.
#include "pg_common.h"
#include "pg_text_steps.h"
#include "pg_vcf_line.h"

namespace {

constexpr int VCF_THREADS = 256;
constexpr int VCF_INFO_KEEP = PG_LINE_KEEP, VCF_INFO_DATA = PG_LINE_DATA, VCF_INFO_HAS_N = 4, VCF_INFO_N_SHIFT = 3;
constexpr int VCF_N_BITS = 12; // the first data line's (offset << 12 | samples): samples <= PG_VCF_MAX_POOLS + 1 < 4096

struct VcfCtl { // read back by the host
    PgLineCounts n;
    unsigned long long err;     // pg_vcf_err_key of the first bad line, PG_VCF_NO_ERR without one
    unsigned long long first_n; // (offset << VCF_N_BITS | samples) of the first line with sample fields, ~0 without one
    unsigned long long chrom_key; // 1 + the offset of the last line that begins with #CHROM, 0 without one
    int64_t kept, data_lines;
};

// ---- parse and emit --------------------------------------------------------------------------------------------------------
struct VcfRule {
    const double *sizes; // device
    int n_sizes;
    int F;               // field starts a group keeps: n_sizes + 10
    uint64_t depth;
    uint32_t breadth;
    double maf, sizes_sum;
};

struct VcfOut {
    uint32_t *counts;
    uint64_t *pos;
    uint8_t *ref;
    int64_t *line_off;
    int32_t *chrom_len;
    int n_pools;
};

enum { VCF_SKIP = 0, VCF_DROP = 1, VCF_KEEP = 2 }; // or minus a pg_vcf_reason

template <bool EMIT>
__global__ __launch_bounds__(VCF_THREADS) void k_vcf_parse(const PgText T, const int64_t *__restrict__ start, int64_t lines, const VcfRule R,
                                                           int shift, int32_t *__restrict__ info, VcfCtl *__restrict__ ctl,
                                                           const int32_t *__restrict__ local, const int64_t *__restrict__ blockoff,
                                                           const VcfOut O) {
    extern __shared__ int fs_all[];
    const int tid = threadIdx.x;
    const PgLaneGroup G = lane_group(tid, shift);
    const int lpr = G.lpr, g = G.g, gl = G.gl;
    int *fs = fs_all + g * R.F;
    const int64_t line = (int64_t)blockIdx.x * (VCF_THREADS >> shift) + g;
    bool active = line < lines; // uniform over the group, as is everything decided from the line alone
    if (EMIT && active) active = (info[line] & VCF_INFO_KEEP) != 0;
    int64_t s = 0;
    int res = VCF_SKIP, wlen = 0;
    bool data = false;
    if (active) {
        int64_t len;
        line_bounds(T, start, line, false, &s, &len); // a '\r' goes only with its newline (pg_hostvcf.cpp does the same)
        if (len == 0) res = -PG_VCF_E_EMPTY;
        else if (T.text[s] == '#') {
            if (!EMIT && gl == 0 && len >= 6 && T.text[s + 1] == 'C' && T.text[s + 2] == 'H' && T.text[s + 3] == 'R' && T.text[s + 4] == 'O' &&
                T.text[s + 5] == 'M')
                atomicMax(&ctl->chrom_key, (unsigned long long)s + 1ULL);
        } else {
            data = true;
            if (len < PG_VCF_MIN_LINE) res = -PG_VCF_E_SHORT;
            else if (len > PG_LINE_MAX) res = -PG_VCF_E_LONG;
            else wlen = (int)len;
        }
    }
    const unsigned char *L = T.text + s;
    // the field starts: fs[f] = where field f begins, for f < F
    const int ntabs = group_split_tabs(L, wlen, G, fs, R.F);
    if (gl == 0 && wlen > 0) fs[0] = 0;
    __syncthreads(); // every thread of the workgroup arrives: no path above returns
    int n = -1;
    if (wlen > 0) {
        const int nfields = ntabs + 1;
        if (nfields < PG_VCF_FIXED_FIELDS) res = -PG_VCF_E_FIELDS;
        else {
            n = min(nfields - PG_VCF_FIXED_FIELDS, PG_VCF_MAX_POOLS + 1);
            auto fend = [&](int f) { return f + 1 < nfields ? fs[f + 1] - 1 : wlen; }; // f + 1 < F wherever it is asked
            PgVcfHead h;
            pg_vcf_head(L, fs[1], fend(1), fs[3], fend(3), fs[4], fend(4), fs[8], fend(8), &h);
            int err = h.err;
            if (n > R.n_sizes) err = pg_vcf_min_code(err, PG_VCF_E_POOLS);
            if (n > R.n_sizes || !h.ad_ok) res = -err; // the samples cannot be read
            else {
                const int m = n > 0 ? pg_vcf_ad_count(L + fs[9], fend(9) - fs[9], h.ad_idx) : 0;
                int covered = 0, ragged = 0, cov0 = 0;
                double q = 0.0;
                int64_t rank = 0;
                if (EMIT) rank = scan_rank(local, blockoff, line);
                for (int j0 = 0; j0 < n; j0 += lpr) { // one trip count for the group
                    const int j = j0 + gl;
                    const bool have = j < n;
                    PgVcfSample sm{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
                    if (have) pg_vcf_sample(L + fs[9 + j], fend(9 + j) - fs[9 + j], h.ad_idx, m, h.map, &sm);
                    if (EMIT) {
                        if (have) {
                            uint32_t *dst = O.counts + (rank * O.n_pools + j) * 6; // rank < kept <= cap_loci, j < n_pools: inside cap_counts
                            dst[0] = sm.a; dst[1] = sm.t; dst[2] = sm.c; dst[3] = sm.g; dst[4] = sm.d; dst[5] = sm.n;
                        }
                        continue;
                    }
                    err = pg_vcf_min_code(err, sm.err);
                    const int cov = have && sm.depth >= R.depth ? 1 : 0;
                    covered += cov;
                    if (j == 0) cov0 = cov;
                    ragged |= have && sm.count < m ? 1 : 0;
                    const double term = have ? pg_vcf_q_term(sm.v1, sm.row_sum, R.sizes[j], R.sizes_sum) : 0.0;
                    const int in_round = min(lpr, n - j0);
                    for (int l = 0; l < in_round; ++l) q += __shfl(term, l, lpr); // pool order, one addition after the other
                }
                if (EMIT) {
                    if (gl == 0) {
                        O.pos[rank] = h.pos;
                        O.ref[rank] = h.ref;
                        O.line_off[rank] = s;
                        O.chrom_len[rank] = fs[1] - 1;
                    }
                } else {
                    for (int d = 1; d < lpr; d <<= 1) {
                        err = pg_vcf_min_code(err, __shfl_xor(err, d, lpr));
                        covered += __shfl_xor(covered, d, lpr);
                        ragged |= __shfl_xor(ragged, d, lpr);
                    }
                    cov0 = __shfl(cov0, 0, lpr);
                    if (err) res = -err;
                    else if (!pg_vcf_breadth_pass(R.breadth, covered, cov0 != 0, n)) res = VCF_DROP;
                    else if (n == 0) res = -PG_VCF_E_NO_SAMPLES;
                    else if (ragged) res = -PG_VCF_E_AD_RAGGED;
                    else if (m < 2) res = VCF_DROP;
                    else if (!pg_vcf_maf_pass(q, R.maf)) res = VCF_DROP;
                    else if (pg_vcf_map_out_of(h.map, m)) res = -PG_VCF_E_ALLELE_OOB;
                    else res = VCF_KEEP;
                }
            }
        }
    }
    if (!EMIT && active && gl == 0) {
        info[line] = (res == VCF_KEEP ? VCF_INFO_KEEP : 0) | (data ? VCF_INFO_DATA : 0) | (n >= 0 ? VCF_INFO_HAS_N | (n << VCF_INFO_N_SHIFT) : 0);
        if (n >= 0) atomicMin(&ctl->first_n, ((unsigned long long)s << VCF_N_BITS) | (unsigned long long)n);
        if (res < 0) atomicMin(&ctl->err, (unsigned long long)pg_vcf_err_key(s, -res));
    }
}

// ---- scan of the keep flags, and VCF's own tail: every line has the first data line's number of samples ---------------------
__global__ __launch_bounds__(PG_COUNT_ROWS) void k_vcf_keep(const int32_t *__restrict__ info, int64_t lines, const int64_t *__restrict__ start,
                                                            int32_t *__restrict__ local, int64_t *__restrict__ blocksum, VcfCtl *__restrict__ ctl) {
    const int64_t i = (int64_t)blockIdx.x * PG_COUNT_ROWS + threadIdx.x;
    const int v = scan_keep_flags(info, lines, local, blocksum, &ctl->data_lines);
    if ((v & VCF_INFO_HAS_N) && (v >> VCF_INFO_N_SHIFT) != (int)(ctl->first_n & ((1u << VCF_N_BITS) - 1u))) // (first_n is complete: the parse kernel is over)
        atomicMin(&ctl->err, (unsigned long long)pg_vcf_err_key(start[i], PG_VCF_E_POOLS));
}

const char *vcf_reason_text(int r) {
    switch (r) {
    case PG_VCF_E_EMPTY: return "an empty line";
    case PG_VCF_E_SHORT: return "a data line shorter than 20 bytes";
    case PG_VCF_E_LONG: return "a line of 2^31 bytes or more";
    case PG_VCF_E_FIELDS: return "fewer than 9 tab-separated fields";
    case PG_VCF_E_POS: return "the position is not a valid integer (u64)";
    case PG_VCF_E_HIGH_BYTE: return "a byte >= 0x80 in REF or ALT (not supported)";
    case PG_VCF_E_AD_KEY: return "FORMAT does not name exactly one AD (allele depths)";
    case PG_VCF_E_POOLS: return "more samples than pool sizes, or another number of samples than the first data line";
    case PG_VCF_E_SUBFIELDS: return "a sample has too few ':' fields to hold AD";
    case PG_VCF_E_AD_VALUE: return "an allele depth is not a valid integer (u64)";
    case PG_VCF_E_COUNT32: return "an allele depth above 4294967295 (not supported: the counts are 32-bit)";
    case PG_VCF_E_NO_SAMPLES: return "no samples";
    case PG_VCF_E_AD_RAGGED: return "a sample has fewer allele depths than the first sample";
    case PG_VCF_E_ALLELE_OOB: return "an allele without an allele depth in the first sample";
    }
    return "unknown";
}

} // namespace

extern "C" int pg_vcf_parse_dev(pg_ctx *ctx, const char *text_dev, int64_t bytes, const double *pool_sizes, int n_sizes,
                                uint64_t min_coverage_depth, double min_coverage_breadth, double min_allele_frequency,
                                uint32_t *counts_dev, uint64_t *pos_dev, uint8_t *ref_dev, int64_t *line_off_dev, int32_t *chrom_len_dev,
                                int64_t cap_loci, int64_t cap_counts, pg_vcf_info *info) {
    if (!ctx) return PG_ERR_INVALID;
    PG_CHECK(ctx, info != nullptr, "vcf_parse: null pointer");
    *info = pg_vcf_info{0, 0, -1, -1, 0, 0};
    PG_CHECK(ctx, bytes >= 0 && (bytes == 0 || text_dev) && pool_sizes && n_sizes >= 1 && cap_loci >= 0 && cap_counts >= 0,
             "vcf_parse: bad arguments bytes=%lld n_sizes=%d cap_loci=%lld cap_counts=%lld", (long long)bytes, n_sizes, (long long)cap_loci,
             (long long)cap_counts);
    PG_CHECK(ctx, n_sizes <= PG_VCF_MAX_POOLS, "vcf_parse: %d pool sizes, at most %d are supported", n_sizes, PG_VCF_MAX_POOLS);
    PG_CHECK(ctx, bytes < ((int64_t)1 << 40), "vcf_parse: a slab of %lld bytes; cut the text at line starts into slabs below 2^40", (long long)bytes);
    if (bytes == 0) return PG_OK;
    PG_HIP(ctx, hipSetDevice(ctx->device));
    const PgText T = pg_text(text_dev, bytes);
    const size_t o_sizes = pg_up16(sizeof(VcfCtl)), front_bytes = o_sizes + sizeof(double) * (size_t)n_sizes; // the front block: VcfCtl, the pool sizes
    VcfCtl init{};
    init.err = PG_VCF_NO_ERR;
    init.first_n = ~0ULL;
    auto front = [&](char *ws, auto count_lines) -> hipError_t {
        hipError_t e = hipMemcpyAsync(ws, &init, sizeof(VcfCtl), hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) return e;
        e = hipMemcpyAsync(ws + o_sizes, pool_sizes, sizeof(double) * (size_t)n_sizes, hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) return e;
        count_lines(PgNoHook());
        return hipGetLastError();
    };
    VcfCtl res{};
    PgLineIndex X;
    int rc = X.build(ctx, PG_K_VCF, "vcf_parse", T, front_bytes, front, &res);
    if (rc) return rc;
    const int64_t lines = X.lines;
    VcfCtl *ctl = reinterpret_cast<VcfCtl *>(X.ws);
    VcfRule R;
    R.sizes = reinterpret_cast<const double *>(X.ws + o_sizes);
    R.n_sizes = n_sizes;
    R.F = n_sizes + PG_VCF_FIXED_FIELDS + 1;
    R.depth = min_coverage_depth;
    R.breadth = pg_vcf_breadth_threshold(min_coverage_breadth, n_sizes);
    R.maf = min_allele_frequency;
    R.sizes_sum = 0.0;
    for (int i = 0; i < n_sizes; ++i) R.sizes_sum += pool_sizes[i];
    const int shift = pg_lpr_shift(n_sizes, 3); // so that 5 pools have 8 lines in a wave and 200 pools one line across it
    const int lines_per_block = VCF_THREADS >> shift;
    int64_t nbp;
    rc = X.parse_blocks(ctx, "vcf_parse", lines_per_block, &nbp);
    if (rc) return rc;
    const size_t lds = sizeof(int) * (size_t)lines_per_block * (size_t)R.F; // at most 32 x 18 or 4 x 2058 ints
    const VcfOut none{nullptr, nullptr, nullptr, nullptr, nullptr, 0};
    pg_prof_begin(ctx, PG_K_VCF | PG_PROF_CONT);
    hipLaunchKernelGGL(k_vcf_parse<false>, dim3((unsigned)nbp), dim3(VCF_THREADS), lds, ctx->stream, T, (const int64_t *)X.start, lines, R, shift, X.info,
                       ctl, (const int32_t *)nullptr, (const int64_t *)nullptr, none);
    hipLaunchKernelGGL(k_vcf_keep, dim3((unsigned)X.nbk), dim3(PG_COUNT_ROWS), 0, ctx->stream, (const int32_t *)X.info, lines, (const int64_t *)X.start,
                       X.local, X.bsk, ctl);
    X.scan_kept(ctx, &ctl->kept);
    pg_prof_end(ctx);
    PG_HIP(ctx, hipGetLastError());
    PG_HIP(ctx, hipMemcpyAsync(&res, ctl, sizeof(VcfCtl), hipMemcpyDeviceToHost, ctx->stream));
    PG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    info->data_lines = res.data_lines;
    info->chrom_line_off = (int64_t)res.chrom_key - 1;
    if (res.err != PG_VCF_NO_ERR) {
        info->err_line_off = (int64_t)(res.err >> 8);
        info->err_reason = (int32_t)(res.err & 0xff);
        return pg_fail(ctx, PG_ERR_INVALID, "vcf_parse: the line at byte %lld of the text: %s", (long long)info->err_line_off,
                       vcf_reason_text(info->err_reason));
    }
    info->kept = res.kept;
    info->n_pools = res.first_n == ~0ULL ? 0 : (int32_t)(res.first_n & ((1u << VCF_N_BITS) - 1u));
    const int64_t need_counts = res.kept * info->n_pools * 6;
    PG_CHECK(ctx, res.kept <= cap_loci && need_counts <= cap_counts, "vcf_parse: %lld loci of %d pools need %lld count elements, the buffers hold %lld loci and %lld",
             (long long)res.kept, (int)info->n_pools, (long long)need_counts, (long long)cap_loci, (long long)cap_counts);
    if (res.kept == 0) return PG_OK;
    PG_CHECK(ctx, pos_dev && ref_dev && line_off_dev && chrom_len_dev && (need_counts == 0 || counts_dev), "vcf_parse: null output buffer");
    const VcfOut O{counts_dev, pos_dev, ref_dev, line_off_dev, chrom_len_dev, (int)info->n_pools};
    pg_prof_begin(ctx, PG_K_VCF | PG_PROF_CONT);
    hipLaunchKernelGGL(k_vcf_parse<true>, dim3((unsigned)nbp), dim3(VCF_THREADS), lds, ctx->stream, T, (const int64_t *)X.start, lines, R, shift, X.info, ctl,
                       (const int32_t *)X.local, (const int64_t *)X.bok, O);
    pg_prof_end(ctx);
    PG_HIP(ctx, hipGetLastError());
    return PG_OK;
}
