// pg_pileup.hip -- pileup2sync's reader on the device: a slab of samtools mpileup text to the allele counts of the loci that
// PileupLine::filter keeps (base/pileup.rs; the rules, shared with the host twin, are pg_pileup_line.h).
// The steps of pg_vcf.hip on the context's stream; the index, the scans and the lane-group steps are the shared ones of
// pg_text_steps.h:
//   index   PgLineIndex: k_text_index<false> (newlines per 4 KB of text: a lane reads one aligned 16-byte word) + k_scan_blocks
//           (64-bit exclusive scan of the workgroups' sums) + k_text_index<true> (every newline writes the start of the line
//           behind it);
//   parse   k_pl_parse<false>: a line is taken by a GROUP of lanes (8 .. 64, a power of two chosen from the number of pool
//           sizes).  The group walks its line in chunks of one byte per lane; a ballot on '\t' and a popcount of the lower lanes
//           give a byte's field index, and the field starts go to LDS.  The first three fields are read by every lane alike;
//           then lane j takes pools j, j + lanes, ..: it walks that pool's read string and quality string together, byte by
//           byte, with six named counters (pg_pileup_pool).  q, the one fp64 sum, is formed in pool order, the terms passing
//           through lane shuffles one after the other.  Pools behind the n_sizes-th (the line is dropped, but only when it is
//           sound) are checked by the group's first lane, one after the other.  One int per line comes out: kept or not; a
//           line where the reference would panic enters (offset, reason) into one 64-bit atomicMin;
//   scan    k_scan_keep (exclusive scan of 256 keep flags per workgroup) + k_scan_blocks: a kept line's rank;
//   emit    k_pl_parse<true>: the kept lines are split and walked again and write their rows at their rank, adjacent pools
//           from adjacent lanes.
// No loop over the text can spin: each advances a cursor towards a field or line end (pg_pileup_line.h).  Every read of the
// text is a byte of [0, bytes) or an aligned 16-byte word that holds one.
#include "pg_common.h"
#include "pg_text_steps.h"
#include "pg_pileup_line.h"

namespace {

constexpr int PL_THREADS = 256;
constexpr size_t PL_LDS_BUDGET = 60 * 1024; // field starts of a workgroup's lines (beside the 512 bytes of tables)

struct PlCtl { // read back by the host
    PgLineCounts n;
    unsigned long long err; // pg_pileup_err_key of the first bad line, PG_PILEUP_NO_ERR without one
    int64_t kept;
};

// ---- parse and emit --------------------------------------------------------------------------------------------------------
struct PlRule {
    const double *sizes;          // device
    const unsigned char *tables;  // device: PgPileupTables
    int n_sizes;
    int F;   // field starts a group keeps: 3 n_sizes + 4 (the start of pool n_sizes' coverage is the last)
    int lpb; // lines a workgroup takes: as many groups as it has, or fewer where their field starts would not fit into LDS
    int remove_ns, keep_lc;
    uint64_t depth;
    uint32_t breadth;
    double maf;
};

struct PlOut {
    uint32_t *counts;
    uint64_t *pos;
    uint8_t *ref;
    int64_t *line_off;
    int32_t *chrom_len;
};

enum { PL_DROP = 1, PL_KEEP = 2 }; // or minus a pg_pileup_reason

template <bool EMIT>
__global__ __launch_bounds__(PL_THREADS) void k_pl_parse(const PgText T, const int64_t *__restrict__ start, int64_t lines, const PlRule R, int shift,
                                                         int32_t *__restrict__ keep, PlCtl *__restrict__ ctl, const int32_t *__restrict__ local,
                                                         const int64_t *__restrict__ blockoff, const PlOut O) {
    extern __shared__ int fs_all[];
    __shared__ unsigned char tab[sizeof(PgPileupTables)];
    const int tid = threadIdx.x;
    for (int i = tid; i < (int)sizeof(PgPileupTables); i += PL_THREADS) tab[i] = R.tables[i];
    const unsigned char *cls = tab, *qcls = tab + 256;
    const PgLaneGroup G = lane_group(tid, shift);
    const int lpr = G.lpr, g = G.g, gl = G.gl;
    int *fs = fs_all + (g < R.lpb ? g : 0) * R.F; // (groups without a line write nothing)
    const int64_t line = (int64_t)blockIdx.x * R.lpb + g;
    bool active = g < R.lpb && line < lines; // uniform over the group, as is everything decided from the line alone
    if (EMIT && active) active = keep[line] != 0;
    int64_t s = 0;
    int res = PL_DROP, wlen = 0;
    if (active) {
        int64_t len;
        line_bounds(T, start, line, true, &s, &len); // a '\r' goes from a last line without its newline too
        if (len == 0) res = -PG_PILEUP_E_FIELDS;
        else if (len > PG_LINE_MAX) res = -PG_PILEUP_E_LONG;
        else wlen = (int)len;
    }
    const unsigned char *L = T.text + s;
    // the field starts: fs[f] = where field f begins, for f < F
    const int ntabs = group_split_tabs(L, wlen, G, fs, R.F);
    if (gl == 0 && wlen > 0) fs[0] = 0;
    __syncthreads(); // every thread of the workgroup arrives: no path above returns
    if (wlen > 0) {
        const int nfields = ntabs + 1;
        if (nfields < 3) res = -PG_PILEUP_E_FIELDS;
        else {
            auto fend = [&](int f) { return f + 1 < nfields ? fs[f + 1] - 1 : wlen; }; // f + 1 < F wherever it is asked
            uint64_t pos;
            unsigned char ref;
            int err = pg_pileup_head(L, fs[1], fend(1), fs[2], fend(2), &pos, &ref);
            const unsigned char refcls = pg_pileup_allele_class(ref, R.keep_lc != 0);
            const int npools = (nfields - 3 + 2) / 3;
            const int n = min(npools, R.n_sizes); // the pools the lanes share; their fields are 3 + 3 j .. 5 + 3 j < F - 1
            int covered = 0, phred = 0;
            double q = 0.0;
            int64_t rank = 0;
            if (EMIT) rank = scan_rank(local, blockoff, line);
            for (int j0 = 0; j0 < n; j0 += lpr) { // one trip count for the group
                const int j = j0 + gl;
                const bool have = j < n;
                PgPileupPool P{0, 0, 0, 0, 0, 0, 0, 0};
                if (have) {
                    const int f = 3 + 3 * j;
                    const bool have_r = f + 1 < nfields, have_q = f + 2 < nfields;
                    pg_pileup_pool(L, fs[f], fend(f), have_r, have_r ? fs[f + 1] : 0, have_r ? fend(f + 1) : 0, have_q, have_q ? fs[f + 2] : 0,
                                   have_q ? fend(f + 2) : 0, refcls, R.remove_ns != 0, cls, qcls, &P);
                }
                if (EMIT) {
                    if (have) {
                        uint32_t *dst = O.counts + (rank * R.n_sizes + j) * 6; // rank < kept <= cap_loci, j < n_sizes: inside cap_counts
                        dst[0] = P.a; dst[1] = P.t; dst[2] = P.c; dst[3] = P.g; dst[4] = P.d; dst[5] = P.n;
                    }
                    continue;
                }
                err = pg_pileup_min_code(err, P.err);
                phred |= P.phred;
                const uint32_t depth = pg_pileup_depth(P);
                covered += have && (uint64_t)depth >= R.depth ? 1 : 0;
                const double term = have ? pg_pileup_q_term(P.t, depth, R.sizes[j]) : 0.0;
                const int in_round = min(lpr, n - j0);
                for (int l = 0; l < in_round; ++l) q += __shfl(term, l, lpr); // pool order, one addition after the other
            }
            if (EMIT) {
                if (gl == 0) {
                    O.pos[rank] = pos;
                    O.ref[rank] = ref;
                    O.line_off[rank] = s;
                    O.chrom_len[rank] = fs[1] - 1;
                }
            } else {
                if (npools > R.n_sizes && gl == 0) // fs[F - 1]: where pool n_sizes' coverage begins
                    err = pg_pileup_min_code(err, pg_pileup_tail(L, fs[R.F - 1], wlen, refcls, R.remove_ns != 0, cls, qcls));
                for (int d = 1; d < lpr; d <<= 1) {
                    err = pg_pileup_min_code(err, __shfl_xor(err, d, lpr));
                    covered += __shfl_xor(covered, d, lpr);
                    phred |= __shfl_xor(phred, d, lpr);
                }
                if (err) res = -err;
                else if (npools != R.n_sizes || phred) res = PL_DROP; // the reference's filter error and its Phred error both end as None
                else if ((uint32_t)covered < R.breadth) res = PL_DROP;
                else if (!pg_pileup_maf_pass(q, R.maf)) res = PL_DROP;
                else res = PL_KEEP;
            }
        }
    }
    if (!EMIT && active && gl == 0) {
        keep[line] = res == PL_KEEP ? PG_LINE_KEEP : 0;
        if (res < 0) atomicMin(&ctl->err, (unsigned long long)pg_pileup_err_key(s, -res));
    }
}

const char *pl_reason_text(int r) {
    switch (r) {
    case PG_PILEUP_E_LONG: return "a line of 2^31 bytes or more";
    case PG_PILEUP_E_FIELDS: return "fewer than three tab-separated fields";
    case PG_PILEUP_E_POS: return "position is not a valid integer (i.e. u64)";
    case PG_PILEUP_E_REF: return "the reference allele is not a valid single character";
    case PG_PILEUP_E_COV: return "coverage field/s is/are not valid integer/s (i.e. u64)";
    case PG_PILEUP_E_RAGGED: return "the coverages, number of read alleles and read qualities do not match (ragged pool)";
    case PG_PILEUP_E_INDEL: return "codes for insertions and deletion must be integers after '+' and '-'";
    case PG_PILEUP_E_MISMATCH: return "the coverages, number of read alleles and read qualities do not match";
    }
    return "unknown";
}

} // namespace

extern "C" int pg_pileup_parse_dev(pg_ctx *ctx, const char *text_dev, int64_t bytes, const double *pool_sizes, int n_sizes, int remove_ns,
                                   int keep_lowercase_reference, double max_base_error_rate, uint64_t min_coverage_depth,
                                   double min_coverage_breadth, double min_allele_frequency, uint32_t *counts_dev, uint64_t *pos_dev,
                                   uint8_t *ref_dev, int64_t *line_off_dev, int32_t *chrom_len_dev, int64_t cap_loci, int64_t cap_counts,
                                   pg_pileup_info *info) {
    if (!ctx) return PG_ERR_INVALID;
    PG_CHECK(ctx, info != nullptr, "pileup_parse: null pointer");
    *info = pg_pileup_info{0, 0, -1, 0, 0};
    PG_CHECK(ctx, bytes >= 0 && (bytes == 0 || text_dev) && pool_sizes && n_sizes >= 1 && cap_loci >= 0 && cap_counts >= 0,
             "pileup_parse: bad arguments bytes=%lld n_sizes=%d cap_loci=%lld cap_counts=%lld", (long long)bytes, n_sizes, (long long)cap_loci,
             (long long)cap_counts);
    PG_CHECK(ctx, n_sizes <= PG_PILEUP_MAX_POOLS, "pileup_parse: %d pool sizes, at most %d are supported", n_sizes, PG_PILEUP_MAX_POOLS);
    PG_CHECK(ctx, bytes < ((int64_t)1 << 40), "pileup_parse: a slab of %lld bytes; cut the text at line starts into slabs below 2^40", (long long)bytes);
    if (bytes == 0) return PG_OK;
    PG_HIP(ctx, hipSetDevice(ctx->device));
    const PgText T = pg_text(text_dev, bytes);
    PgPileupTables tables;
    pg_pileup_tables(keep_lowercase_reference != 0, max_base_error_rate, &tables); // (std::pow on the host, once per call)
    const size_t o_sizes = pg_up16(sizeof(PlCtl)), o_tab = pg_up16(o_sizes + sizeof(double) * (size_t)n_sizes);
    const size_t front_bytes = o_tab + sizeof(PgPileupTables); // the front block: PlCtl, the pool sizes, the tables
    PlCtl init{};
    init.err = PG_PILEUP_NO_ERR;
    auto front = [&](char *ws, auto count_lines) -> hipError_t {
        hipError_t e = hipMemcpyAsync(ws, &init, sizeof(PlCtl), hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) return e;
        e = hipMemcpyAsync(ws + o_sizes, pool_sizes, sizeof(double) * (size_t)n_sizes, hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) return e;
        e = hipMemcpyAsync(ws + o_tab, &tables, sizeof(PgPileupTables), hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) return e;
        count_lines(PgNoHook());
        return hipGetLastError();
    };
    PlCtl res{};
    PgLineIndex X;
    int rc = X.build(ctx, PG_K_PILEUP, "pileup_parse", T, front_bytes, front, &res);
    const int64_t lines = X.lines;
    info->lines = lines; // (0 until they are counted; reported even where the line tables could not be reserved)
    if (rc) return rc;
    PlCtl *ctl = reinterpret_cast<PlCtl *>(X.ws);
    int32_t *keep = X.info; // PG_LINE_KEEP or 0
    const int shift = pg_lpr_shift(n_sizes, 3);
    PlRule R;
    R.sizes = reinterpret_cast<const double *>(X.ws + o_sizes);
    R.tables = reinterpret_cast<const unsigned char *>(X.ws + o_tab);
    R.n_sizes = n_sizes;
    R.F = 3 * n_sizes + 4;
    R.lpb = (int)std::max<size_t>(1, std::min<size_t>((size_t)(PL_THREADS >> shift), PL_LDS_BUDGET / (sizeof(int) * (size_t)R.F)));
    R.remove_ns = remove_ns;
    R.keep_lc = keep_lowercase_reference;
    R.depth = min_coverage_depth;
    R.breadth = pg_pileup_breadth_threshold(min_coverage_breadth, n_sizes);
    R.maf = min_allele_frequency;
    int64_t nbp;
    rc = X.parse_blocks(ctx, "pileup_parse", R.lpb, &nbp);
    if (rc) return rc;
    const size_t lds = sizeof(int) * (size_t)R.lpb * (size_t)R.F; // at most 60 KB, or one line of 4096 pools: 49 168 bytes
    const PlOut none{nullptr, nullptr, nullptr, nullptr, nullptr};
    pg_prof_begin(ctx, PG_K_PILEUP | PG_PROF_CONT);
    hipLaunchKernelGGL(k_pl_parse<false>, dim3((unsigned)nbp), dim3(PL_THREADS), lds, ctx->stream, T, (const int64_t *)X.start, lines, R, shift, keep, ctl,
                       (const int32_t *)nullptr, (const int64_t *)nullptr, none);
    hipLaunchKernelGGL(k_scan_keep, dim3((unsigned)X.nbk), dim3(PG_COUNT_ROWS), 0, ctx->stream, (const int32_t *)keep, lines, X.local, X.bsk,
                       (int64_t *)nullptr);
    X.scan_kept(ctx, &ctl->kept);
    pg_prof_end(ctx);
    PG_HIP(ctx, hipGetLastError());
    PG_HIP(ctx, hipMemcpyAsync(&res, ctl, sizeof(PlCtl), hipMemcpyDeviceToHost, ctx->stream));
    PG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (res.err != PG_PILEUP_NO_ERR) {
        info->err_line_off = (int64_t)(res.err >> 8);
        info->err_reason = (int32_t)(res.err & 0xff);
        return pg_fail(ctx, PG_ERR_INVALID, "pileup_parse: the line at byte %lld of the text: %s", (long long)info->err_line_off,
                       pl_reason_text(info->err_reason));
    }
    info->kept = res.kept;
    const int64_t need_counts = res.kept * n_sizes * 6;
    PG_CHECK(ctx, res.kept <= cap_loci && need_counts <= cap_counts, "pileup_parse: %lld loci of %d pools need %lld count elements, the buffers hold %lld loci and %lld",
             (long long)res.kept, n_sizes, (long long)need_counts, (long long)cap_loci, (long long)cap_counts);
    if (res.kept == 0) return PG_OK;
    PG_CHECK(ctx, counts_dev && pos_dev && ref_dev && line_off_dev && chrom_len_dev, "pileup_parse: null output buffer");
    const PlOut O{counts_dev, pos_dev, ref_dev, line_off_dev, chrom_len_dev};
    pg_prof_begin(ctx, PG_K_PILEUP | PG_PROF_CONT);
    hipLaunchKernelGGL(k_pl_parse<true>, dim3((unsigned)nbp), dim3(PL_THREADS), lds, ctx->stream, T, (const int64_t *)X.start, lines, R, shift, keep, ctl,
                       (const int32_t *)X.local, (const int64_t *)X.bok, O);
    pg_prof_end(ctx);
    PG_HIP(ctx, hipGetLastError());
    return PG_OK;
}
