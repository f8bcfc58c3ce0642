// pg_pileup.hip -- pileup2sync's reader on the device: a slab of samtools mpileup text to the allele counts of the loci that
// PileupLine::filter keeps (base/pileup.rs; the rules, shared with the host twin, are pg_pileup_line.h).
// The steps of pg_vcf.hip, in a copy of their own, on the context's stream:
//   index   k_pl_index<false> (newlines per 4 KB of text: a lane reads one aligned 16-byte word) + k_pl_scan (64-bit exclusive
//           scan of the workgroups' sums) + k_pl_index<true> (every newline writes the start of the line behind it);
//   parse   k_pl_parse<false>: a line is taken by a GROUP of lanes (8 .. 64, a power of two chosen from the number of pool
//           sizes).  The group walks its line in chunks of one byte per lane; a ballot on '\t' and a popcount of the lower lanes
//           give a byte's field index, and the field starts go to LDS.  The first three fields are read by every lane alike;
//           then lane j takes pools j, j + lanes, ..: it walks that pool's read string and quality string together, byte by
//           byte, with six named counters (pg_pileup_pool).  q, the one fp64 sum, is formed in pool order, the terms passing
//           through lane shuffles one after the other.  Pools behind the n_sizes-th (the line is dropped, but only when it is
//           sound) are checked by the group's first lane, one after the other.  One int per line comes out: kept or not; a
//           line where the reference would panic enters (offset, reason) into one 64-bit atomicMin;
//   scan    k_pl_keep (exclusive scan of 256 keep flags per workgroup) + k_pl_scan: a kept line's rank;
//   emit    k_pl_parse<true>: the kept lines are split and walked again and write their rows at their rank, adjacent pools
//           from adjacent lanes.
// No loop over the text can spin: each advances a cursor towards a field or line end (pg_pileup_line.h).  Every read of the
// text is a byte of [0, bytes) or an aligned 16-byte word that holds one.
#include "pg_common.h"
#include "pg_pileup_line.h"

namespace {

constexpr int PL_THREADS = 256;
constexpr size_t PL_LDS_BUDGET = 60 * 1024; // field starts of a workgroup's lines (beside the 512 bytes of tables)

struct PlCtl { // read back by the host
    unsigned long long err; // pg_pileup_err_key of the first bad line, PG_PILEUP_NO_ERR without one
    long long newlines, lines, kept;
};

struct PlText {
    const unsigned char *text;
    int64_t bytes;
    int64_t head;    // text - head is 16-byte aligned
    int64_t nchunks; // aligned 16-byte words that hold a byte of the text
};

// lanes per line: the smallest power of two that holds the pools, from 8 lanes to a wave
int pl_lpr_shift(int n) {
    int s = 3;
    while (s < 6 && (1 << s) < n) ++s;
    return s;
}

// bit k = byte k of x is '\n'
__device__ __forceinline__ unsigned pl_nl4(unsigned x) {
    const unsigned y = x ^ 0x0A0A0A0Au;
    const unsigned z = ~(((y & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | y | 0x7F7F7F7Fu); // 0x80 in every byte of y that is zero
    return ((z >> 7) & 1u) | ((z >> 14) & 2u) | ((z >> 21) & 4u) | ((z >> 28) & 8u);
}

// the newlines among the bytes of aligned word c that belong to the text: bit k = position 16 c - head + k
__device__ __forceinline__ unsigned pl_nl_mask(const PlText &T, int64_t c) {
    if (c >= T.nchunks) return 0u;
    const uint4 w = *reinterpret_cast<const uint4 *>(T.text - T.head + 16 * c); // whole inside the aligned words the text touches
    unsigned m = pl_nl4(w.x) | (pl_nl4(w.y) << 4) | (pl_nl4(w.z) << 8) | (pl_nl4(w.w) << 12);
    const int64_t p0 = 16 * c - T.head;
    if (p0 < 0) m &= (0xffffu << (int)(-p0)) & 0xffffu;
    if (p0 + 16 > T.bytes) m &= (1u << (int)(T.bytes - p0)) - 1u;
    return m;
}

// ---- index ---------------------------------------------------------------------------------------------------------------
template <bool EMIT>
__global__ __launch_bounds__(PL_THREADS) void k_pl_index(const PlText T, int64_t *__restrict__ blocksum, const int64_t *__restrict__ blockoff,
                                                         const PlCtl *__restrict__ ctl, int64_t *__restrict__ start) {
    __shared__ int sc[PL_THREADS];
    const int tid = threadIdx.x;
    const int64_t c = (int64_t)blockIdx.x * PL_THREADS + tid;
    unsigned m = pl_nl_mask(T, c);
    const int cnt = __popc(m);
    sc[tid] = cnt;
    __syncthreads();
    for (int d = 1; d < PL_THREADS; d <<= 1) {
        const int v = tid >= d ? sc[tid - d] : 0;
        __syncthreads();
        sc[tid] += v;
        __syncthreads();
    }
    if (!EMIT) {
        if (tid == PL_THREADS - 1) blocksum[blockIdx.x] = sc[PL_THREADS - 1];
        return;
    }
    int64_t rank = blockoff[blockIdx.x] + (sc[tid] - cnt); // newlines in front of this word
    const int64_t p0 = 16 * c - T.head;
    while (m) {
        const int k = __ffs(m) - 1;
        m &= m - 1u;
        start[++rank] = p0 + k + 1; // rank + 1 <= newlines <= lines
    }
    if (c == 0) {
        start[0] = 0;
        if (ctl->lines > ctl->newlines) start[ctl->lines] = T.bytes + 1; // the last line lacks its newline: as if it stood at `bytes`
    }
}

// exclusive 64-bit scan of the workgroups' sums, 1024 per round; the total goes to *total, and with `text` the number of lines
// to *lines
__global__ __launch_bounds__(1024) void k_pl_scan(const int64_t *__restrict__ blocksum, int64_t nb, int64_t *__restrict__ blockoff,
                                                  long long *__restrict__ total, const unsigned char *__restrict__ text, int64_t bytes,
                                                  long long *__restrict__ lines) {
    __shared__ int64_t sc[1024];
    __shared__ int64_t carry;
    const int tid = threadIdx.x;
    if (tid == 0) carry = 0;
    __syncthreads();
    for (int64_t base = 0; base < nb; base += 1024) {
        const int64_t i = base + tid;
        const int64_t c = i < nb ? blocksum[i] : 0;
        sc[tid] = c;
        __syncthreads();
        for (int d = 1; d < 1024; d <<= 1) {
            const int64_t v = tid >= d ? sc[tid - d] : 0;
            __syncthreads();
            sc[tid] += v;
            __syncthreads();
        }
        if (i < nb) blockoff[i] = carry + sc[tid] - c;
        __syncthreads();
        if (tid == 1023) carry += sc[1023];
        __syncthreads();
    }
    if (tid == 0) {
        *total = carry;
        if (text) *lines = carry + (text[bytes - 1] != '\n' ? 1 : 0);
    }
}

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
__global__ __launch_bounds__(PL_THREADS) void k_pl_parse(const PlText T, const int64_t *__restrict__ start, int64_t lines, const PlRule R, int shift,
                                                         int32_t *__restrict__ keep, PlCtl *__restrict__ ctl, const int32_t *__restrict__ local,
                                                         const int64_t *__restrict__ blockoff, const PlOut O) {
    extern __shared__ int fs_all[];
    __shared__ unsigned char tab[sizeof(PgPileupTables)];
    const int tid = threadIdx.x;
    for (int i = tid; i < (int)sizeof(PgPileupTables); i += PL_THREADS) tab[i] = R.tables[i];
    const unsigned char *cls = tab, *qcls = tab + 256;
    const int lpr = 1 << shift;
    const int g = tid >> shift, gl = tid & (lpr - 1);
    const int gbase = (tid & 63) & ~(lpr - 1); // the group's first lane in its wave
    const uint64_t gmask = lpr == 64 ? ~0ULL : ((1ULL << lpr) - 1ULL);
    int *fs = fs_all + (g < R.lpb ? g : 0) * R.F; // (groups without a line write nothing)
    const int64_t line = (int64_t)blockIdx.x * R.lpb + g;
    bool active = g < R.lpb && line < lines; // uniform over the group, as is everything decided from the line alone
    if (EMIT && active) active = keep[line] != 0;
    int64_t s = 0;
    int res = PL_DROP, wlen = 0;
    if (active) {
        s = start[line];
        const int64_t e = start[line + 1] - 1; // the newline's place, or `bytes` for a last line without one
        int64_t len = e - s;
        if (len > 0 && T.text[e - 1] == '\r') --len;
        if (len == 0) res = -PG_PILEUP_E_FIELDS;
        else if (len > 0x7fffffffLL) res = -PG_PILEUP_E_LONG;
        else wlen = (int)len;
    }
    const unsigned char *L = T.text + s;
    // the field starts: fs[f] = where field f begins, for f < F
    int ntabs = 0;
    for (int off = 0; off < wlen; off += lpr) { // (one trip count for the group; other groups of the wave may leave earlier)
        const int idx = off + gl;
        const bool tabhere = idx < wlen && L[idx] == '\t';
        const uint64_t gb = ((uint64_t)__ballot(tabhere) >> gbase) & gmask;
        if (tabhere) {
            const int f = ntabs + __popcll(gb & ((1ULL << gl) - 1ULL)) + 1;
            if (f < R.F) fs[f] = idx + 1;
        }
        ntabs += __popcll(gb);
    }
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
            if (EMIT) rank = blockoff[line >> 8] + local[line];
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
        keep[line] = res == PL_KEEP ? 1 : 0;
        if (res < 0) atomicMin(&ctl->err, (unsigned long long)pg_pileup_err_key(s, -res));
    }
}

// ---- scan of the keep flags ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_pl_keep(const int32_t *__restrict__ keep, int64_t lines, int32_t *__restrict__ local,
                                                 int64_t *__restrict__ blocksum) {
    __shared__ int sc[256];
    const int tid = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * 256 + tid;
    const int c = i < lines ? keep[i] : 0;
    sc[tid] = c;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        const int a = tid >= d ? sc[tid - d] : 0;
        __syncthreads();
        sc[tid] += a;
        __syncthreads();
    }
    if (i < lines) local[i] = sc[tid] - c;
    if (tid == 255) blocksum[blockIdx.x] = sc[255];
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
    PlText T;
    T.text = reinterpret_cast<const unsigned char *>(text_dev);
    T.bytes = bytes;
    T.head = (int64_t)(reinterpret_cast<uintptr_t>(text_dev) & 15);
    T.nchunks = (bytes + T.head + 15) / 16;
    const int64_t nbi = (T.nchunks + PL_THREADS - 1) / PL_THREADS;
    PG_CHECK(ctx, nbi < ((int64_t)1 << 31), "pileup_parse: a slab of %lld bytes; cut the text into smaller slabs", (long long)bytes);
    PgPileupTables tables;
    pg_pileup_tables(keep_lowercase_reference != 0, max_base_error_rate, &tables); // (std::pow on the host, once per call)
    auto up16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
    size_t off = 0;
    const size_t o_ctl = off; off = up16(off + sizeof(PlCtl));
    const size_t o_sizes = off; off = up16(off + sizeof(double) * (size_t)n_sizes);
    const size_t o_tab = off; off = up16(off + sizeof(PgPileupTables));
    const size_t o_bsi = off; off = up16(off + 8 * (size_t)nbi);
    const size_t o_boi = off; off = up16(off + 8 * (size_t)nbi);
    const size_t front = off;
    int rc = pg_ws_reserve(ctx, front);
    if (rc) return rc;
    PlCtl init{};
    init.err = PG_PILEUP_NO_ERR;
    auto count_lines = [&]() -> hipError_t { // the control block, the pool sizes, the tables, the newlines of every 4 KB and their scan
        char *ws = static_cast<char *>(ctx->ws.get());
        hipError_t e = hipMemcpyAsync(ws + o_ctl, &init, sizeof(PlCtl), hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) return e;
        e = hipMemcpyAsync(ws + o_sizes, pool_sizes, sizeof(double) * (size_t)n_sizes, hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) return e;
        e = hipMemcpyAsync(ws + o_tab, &tables, sizeof(PgPileupTables), hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) return e;
        PlCtl *ctl = reinterpret_cast<PlCtl *>(ws + o_ctl);
        hipLaunchKernelGGL(k_pl_index<false>, dim3((unsigned)nbi), dim3(PL_THREADS), 0, ctx->stream, T, reinterpret_cast<int64_t *>(ws + o_bsi),
                           (const int64_t *)nullptr, (const PlCtl *)nullptr, (int64_t *)nullptr);
        hipLaunchKernelGGL(k_pl_scan, dim3(1), dim3(1024), 0, ctx->stream, reinterpret_cast<const int64_t *>(ws + o_bsi), nbi,
                           reinterpret_cast<int64_t *>(ws + o_boi), &ctl->newlines, T.text, bytes, &ctl->lines);
        return hipGetLastError();
    };
    PlCtl res{};
    pg_prof_begin(ctx, PG_K_PILEUP);
    PG_HIP(ctx, count_lines());
    pg_prof_end(ctx);
    PG_HIP(ctx, hipMemcpyAsync(&res, static_cast<char *>(ctx->ws.get()) + o_ctl, sizeof(PlCtl), hipMemcpyDeviceToHost, ctx->stream));
    PG_HIP(ctx, hipStreamSynchronize(ctx->stream)); // (the host copies of init, tables and the sizes have been read by now)
    const int64_t lines = res.lines;
    PG_CHECK(ctx, lines >= 1 && lines <= bytes && res.newlines <= lines, "pileup_parse: internal error, %lld lines in %lld bytes", (long long)lines, (long long)bytes);
    info->lines = lines;
    const int64_t nbk = (lines + 255) / 256;
    const size_t o_start = off; off = up16(off + 8 * (size_t)(lines + 2));
    const size_t o_keep = off; off = up16(off + 4 * (size_t)lines);
    const size_t o_local = off; off = up16(off + 4 * (size_t)lines);
    const size_t o_bsk = off; off = up16(off + 8 * (size_t)nbk);
    const size_t o_bok = off; off = up16(off + 8 * (size_t)nbk);
    const size_t before = ctx->ws.bytes();
    rc = pg_ws_reserve(ctx, off);
    if (rc) return rc;
    pg_prof_begin(ctx, PG_K_PILEUP | PG_PROF_CONT);
    if (ctx->ws.bytes() != before) PG_HIP(ctx, count_lines()); // the workspace was replaced by a larger block: its front part again (the same numbers)
    char *ws = static_cast<char *>(ctx->ws.get());
    PlCtl *ctl = reinterpret_cast<PlCtl *>(ws + o_ctl);
    int64_t *start = reinterpret_cast<int64_t *>(ws + o_start), *bsk = reinterpret_cast<int64_t *>(ws + o_bsk), *bok = reinterpret_cast<int64_t *>(ws + o_bok);
    int32_t *keep = reinterpret_cast<int32_t *>(ws + o_keep), *local = reinterpret_cast<int32_t *>(ws + o_local);
    hipLaunchKernelGGL(k_pl_index<true>, dim3((unsigned)nbi), dim3(PL_THREADS), 0, ctx->stream, T, (int64_t *)nullptr,
                       reinterpret_cast<const int64_t *>(ws + o_boi), (const PlCtl *)ctl, start);
    const int shift = pl_lpr_shift(n_sizes);
    PlRule R;
    R.sizes = reinterpret_cast<const double *>(ws + o_sizes);
    R.tables = reinterpret_cast<const unsigned char *>(ws + o_tab);
    R.n_sizes = n_sizes;
    R.F = 3 * n_sizes + 4;
    R.lpb = (int)std::max<size_t>(1, std::min<size_t>((size_t)(PL_THREADS >> shift), PL_LDS_BUDGET / (sizeof(int) * (size_t)R.F)));
    R.remove_ns = remove_ns;
    R.keep_lc = keep_lowercase_reference;
    R.depth = min_coverage_depth;
    R.breadth = pg_pileup_breadth_threshold(min_coverage_breadth, n_sizes);
    R.maf = min_allele_frequency;
    const int64_t nbp = (lines + R.lpb - 1) / R.lpb;
    PG_CHECK(ctx, nbp < ((int64_t)1 << 31), "pileup_parse: %lld lines in one slab; cut the text into smaller slabs", (long long)lines);
    const size_t lds = sizeof(int) * (size_t)R.lpb * (size_t)R.F; // at most 60 KB, or one line of 4096 pools: 49 168 bytes
    const PlOut none{nullptr, nullptr, nullptr, nullptr, nullptr};
    hipLaunchKernelGGL(k_pl_parse<false>, dim3((unsigned)nbp), dim3(PL_THREADS), lds, ctx->stream, T, (const int64_t *)start, lines, R, shift, keep, ctl,
                       (const int32_t *)nullptr, (const int64_t *)nullptr, none);
    hipLaunchKernelGGL(k_pl_keep, dim3((unsigned)nbk), dim3(256), 0, ctx->stream, (const int32_t *)keep, lines, local, bsk);
    hipLaunchKernelGGL(k_pl_scan, dim3(1), dim3(1024), 0, ctx->stream, (const int64_t *)bsk, nbk, bok, &ctl->kept, (const unsigned char *)nullptr,
                       (int64_t)0, (long long *)nullptr);
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
    hipLaunchKernelGGL(k_pl_parse<true>, dim3((unsigned)nbp), dim3(PL_THREADS), lds, ctx->stream, T, (const int64_t *)start, lines, R, shift, keep, ctl,
                       (const int32_t *)local, (const int64_t *)bok, O);
    pg_prof_end(ctx);
    PG_HIP(ctx, hipGetLastError());
    return PG_OK;
}
