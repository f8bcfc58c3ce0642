// pg_vcf.hip -- vcf2sync's reader on the device: a slab of VCF text to the allele counts of the loci that VcfLine::filter keeps
// (base/vcf.rs; the rules, shared with the host twin, are pg_vcf_line.h).  Four steps on the context's stream:
//   index   k_vcf_index<false> (newlines per 4 KB of text: a lane reads one aligned 16-byte word) + k_vcf_scan (64-bit exclusive
//           scan of the workgroups' sums, 1024 per round) + k_vcf_index<true> (the same read again, a block scan, and every
//           newline writes the start of the line behind it): start[0 .. lines], no host work per line;
//   parse   k_vcf_parse<false>: a line is taken by a GROUP of lanes (8 .. 64, a power of two chosen from the number of pool sizes,
//           so that 5 pools have 8 lines in a wave and 200 pools one line across it).  The group walks its line in chunks of one
//           byte per lane; a ballot on '\t' and a popcount of the lower lanes give a byte's field index, and the field starts go
//           to LDS.  The fixed fields (POS, REF, ALT, FORMAT) are read by every lane alike -- a few bytes, the same address in all
//           lanes -- so nothing has to be passed round; then lane j takes samples j, j + lanes, ..: it steps over ':' to the AD
//           piece and reads the comma list.  The filter follows the reference's order of operations; q, the one fp64 sum, is
//           formed in pool order, the terms passing through lane shuffles one after the other (a tree would be faster and not
//           bit-equal).  One int per line comes out: kept, data line, number of samples; a line where the reference would
//           panic enters (offset, reason) into one 64-bit atomicMin;
//   scan    k_vcf_keep (exclusive scan of 256 keep flags per workgroup, data lines counted, sample numbers compared with the first
//           data line's) + k_vcf_scan: a kept line's rank is blockoff[line >> 8] + local[line];
//   emit    k_vcf_parse<true>: the kept lines are split and read again (the text is in cache or cheap to fetch beside what a
//           staging copy of every line's counts would cost) and write their rows at their rank.
// No array is indexed at run time in a thread: a sample's numbers are the named members of PgVcfSample.
#include "pg_common.h"
#include "pg_vcf_line.h"

namespace {

constexpr int VCF_THREADS = 256;
constexpr int VCF_INFO_KEEP = 1, VCF_INFO_DATA = 2, VCF_INFO_HAS_N = 4, VCF_INFO_N_SHIFT = 3;
constexpr int VCF_N_BITS = 12; // the first data line's (offset << 12 | samples): samples <= PG_VCF_MAX_POOLS + 1 < 4096

struct VcfCtl { // read back by the host
    unsigned long long err;     // pg_vcf_err_key of the first bad line, PG_VCF_NO_ERR without one
    unsigned long long first_n; // (offset << VCF_N_BITS | samples) of the first line with sample fields, ~0 without one
    unsigned long long chrom_key; // 1 + the offset of the last line that begins with #CHROM, 0 without one
    long long newlines, lines, kept, data_lines;
};

struct VcfText {
    const unsigned char *text;
    int64_t bytes;
    int64_t head;    // text - head is 16-byte aligned
    int64_t nchunks; // aligned 16-byte words that hold a byte of the text
};

// lanes per line: the smallest power of two that holds the pools, from 8 lanes to a wave
int vcf_lpr_shift(int n) {
    int s = 3;
    while (s < 6 && (1 << s) < n) ++s;
    return s;
}

// bit k = byte k of x is '\n'
__device__ __forceinline__ unsigned vcf_nl4(unsigned x) {
    const unsigned y = x ^ 0x0A0A0A0Au;
    const unsigned z = ~(((y & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | y | 0x7F7F7F7Fu); // 0x80 in every byte of y that is zero
    return ((z >> 7) & 1u) | ((z >> 14) & 2u) | ((z >> 21) & 4u) | ((z >> 28) & 8u);
}

// the newlines among the bytes of aligned word c that belong to the text: bit k = position 16 c - head + k
__device__ __forceinline__ unsigned vcf_nl_mask(const VcfText &T, int64_t c) {
    if (c >= T.nchunks) return 0u;
    const uint4 w = *reinterpret_cast<const uint4 *>(T.text - T.head + 16 * c); // whole inside the aligned words the text touches
    unsigned m = vcf_nl4(w.x) | (vcf_nl4(w.y) << 4) | (vcf_nl4(w.z) << 8) | (vcf_nl4(w.w) << 12);
    const int64_t p0 = 16 * c - T.head;
    if (p0 < 0) m &= (0xffffu << (int)(-p0)) & 0xffffu;
    if (p0 + 16 > T.bytes) m &= (1u << (int)(T.bytes - p0)) - 1u;
    return m;
}

// ---- index ---------------------------------------------------------------------------------------------------------------
template <bool EMIT>
__global__ __launch_bounds__(VCF_THREADS) void k_vcf_index(const VcfText T, int64_t *__restrict__ blocksum, const int64_t *__restrict__ blockoff,
                                                           const VcfCtl *__restrict__ ctl, int64_t *__restrict__ start) {
    __shared__ int sc[VCF_THREADS];
    const int tid = threadIdx.x;
    const int64_t c = (int64_t)blockIdx.x * VCF_THREADS + tid;
    unsigned m = vcf_nl_mask(T, c);
    const int cnt = __popc(m);
    sc[tid] = cnt;
    __syncthreads();
    for (int d = 1; d < VCF_THREADS; d <<= 1) {
        const int v = tid >= d ? sc[tid - d] : 0;
        __syncthreads();
        sc[tid] += v;
        __syncthreads();
    }
    if (!EMIT) {
        if (tid == VCF_THREADS - 1) blocksum[blockIdx.x] = sc[VCF_THREADS - 1];
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

// exclusive 64-bit scan of the workgroups' sums (the pattern of k_csv_scan / k_load_scan, in a copy of its own); the total goes to
// *total, and with `text` the number of lines to *lines
__global__ __launch_bounds__(1024) void k_vcf_scan(const int64_t *__restrict__ blocksum, int64_t nb, int64_t *__restrict__ blockoff,
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
__global__ __launch_bounds__(VCF_THREADS) void k_vcf_parse(const VcfText T, const int64_t *__restrict__ start, int64_t lines, const VcfRule R,
                                                           int shift, int32_t *__restrict__ info, VcfCtl *__restrict__ ctl,
                                                           const int32_t *__restrict__ local, const int64_t *__restrict__ blockoff,
                                                           const VcfOut O) {
    extern __shared__ int fs_all[];
    const int tid = threadIdx.x;
    const int lpr = 1 << shift;
    const int g = tid >> shift, gl = tid & (lpr - 1);
    const int gbase = (tid & 63) & ~(lpr - 1); // the group's first lane in its wave
    const uint64_t gmask = lpr == 64 ? ~0ULL : ((1ULL << lpr) - 1ULL);
    int *fs = fs_all + g * R.F;
    const int64_t line = (int64_t)blockIdx.x * (VCF_THREADS >> shift) + g;
    bool active = line < lines; // uniform over the group, as is everything decided from the line alone
    if (EMIT && active) active = (info[line] & VCF_INFO_KEEP) != 0;
    int64_t s = 0;
    int res = VCF_SKIP, wlen = 0;
    bool data = false;
    if (active) {
        s = start[line];
        const int64_t e = start[line + 1] - 1; // the newline's place, or `bytes` for a last line without one
        int64_t len = e - s;
        if (e < T.bytes && len > 0 && T.text[e - 1] == '\r') --len;
        if (len == 0) res = -PG_VCF_E_EMPTY;
        else if (T.text[s] == '#') {
            if (!EMIT && gl == 0 && len >= 6 && T.text[s + 1] == 'C' && T.text[s + 2] == 'H' && T.text[s + 3] == 'R' && T.text[s + 4] == 'O' &&
                T.text[s + 5] == 'M')
                atomicMax(&ctl->chrom_key, (unsigned long long)s + 1ULL);
        } else {
            data = true;
            if (len < PG_VCF_MIN_LINE) res = -PG_VCF_E_SHORT;
            else if (len > 0x7fffffffLL) res = -PG_VCF_E_LONG;
            else wlen = (int)len;
        }
    }
    const unsigned char *L = T.text + s;
    // the field starts: fs[f] = where field f begins, for f < F
    int ntabs = 0;
    for (int off = 0; off < wlen; off += lpr) { // (one trip count for the group; other groups of the wave may leave earlier)
        const int idx = off + gl;
        const bool tab = idx < wlen && L[idx] == '\t';
        const uint64_t gb = ((uint64_t)__ballot(tab) >> gbase) & gmask;
        if (tab) {
            const int f = ntabs + __popcll(gb & ((1ULL << gl) - 1ULL)) + 1;
            if (f < R.F) fs[f] = idx + 1;
        }
        ntabs += __popcll(gb);
    }
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
                if (EMIT) rank = blockoff[line >> 8] + local[line];
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

// ---- scan of the keep flags (k_csv_count's pattern) -----------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_vcf_keep(const int32_t *__restrict__ info, int64_t lines, const int64_t *__restrict__ start,
                                                  int32_t *__restrict__ local, int64_t *__restrict__ blocksum, VcfCtl *__restrict__ ctl) {
    __shared__ int sc[256];
    __shared__ int sd[256];
    const int tid = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * 256 + tid;
    const int v = i < lines ? info[i] : 0;
    const int c = v & VCF_INFO_KEEP;
    sc[tid] = c;
    sd[tid] = (v & VCF_INFO_DATA) ? 1 : 0;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        const int a = tid >= d ? sc[tid - d] : 0;
        const int b = tid >= d ? sd[tid - d] : 0;
        __syncthreads();
        sc[tid] += a;
        sd[tid] += b;
        __syncthreads();
    }
    if (i < lines) local[i] = sc[tid] - c;
    if (tid == 255) {
        blocksum[blockIdx.x] = sc[255];
        if (sd[255]) atomicAdd(reinterpret_cast<unsigned long long *>(&ctl->data_lines), (unsigned long long)sd[255]);
    }
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
    VcfText T;
    T.text = reinterpret_cast<const unsigned char *>(text_dev);
    T.bytes = bytes;
    T.head = (int64_t)(reinterpret_cast<uintptr_t>(text_dev) & 15);
    T.nchunks = (bytes + T.head + 15) / 16;
    const int64_t nbi = (T.nchunks + VCF_THREADS - 1) / VCF_THREADS;
    auto up16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
    size_t off = 0;
    const size_t o_ctl = off; off = up16(off + sizeof(VcfCtl));
    const size_t o_sizes = off; off = up16(off + sizeof(double) * (size_t)n_sizes);
    const size_t o_bsi = off; off = up16(off + 8 * (size_t)nbi);
    const size_t o_boi = off; off = up16(off + 8 * (size_t)nbi);
    const size_t front = off;
    int rc = pg_ws_reserve(ctx, front);
    if (rc) return rc;
    VcfCtl init{};
    init.err = PG_VCF_NO_ERR;
    init.first_n = ~0ULL;
    auto count_lines = [&]() -> hipError_t { // the control block, the pool sizes, the newlines of every 4 KB and their scan
        char *ws = static_cast<char *>(ctx->ws.get());
        hipError_t e = hipMemcpyAsync(ws + o_ctl, &init, sizeof(VcfCtl), hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) return e;
        e = hipMemcpyAsync(ws + o_sizes, pool_sizes, sizeof(double) * (size_t)n_sizes, hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) return e;
        VcfCtl *ctl = reinterpret_cast<VcfCtl *>(ws + o_ctl);
        hipLaunchKernelGGL(k_vcf_index<false>, dim3((unsigned)nbi), dim3(VCF_THREADS), 0, ctx->stream, T, reinterpret_cast<int64_t *>(ws + o_bsi),
                           (const int64_t *)nullptr, (const VcfCtl *)nullptr, (int64_t *)nullptr);
        hipLaunchKernelGGL(k_vcf_scan, dim3(1), dim3(1024), 0, ctx->stream, reinterpret_cast<const int64_t *>(ws + o_bsi), nbi,
                           reinterpret_cast<int64_t *>(ws + o_boi), &ctl->newlines, T.text, bytes, &ctl->lines);
        return hipGetLastError();
    };
    VcfCtl res{};
    pg_prof_begin(ctx, PG_K_VCF);
    PG_HIP(ctx, count_lines());
    pg_prof_end(ctx);
    PG_HIP(ctx, hipMemcpyAsync(&res, static_cast<char *>(ctx->ws.get()) + o_ctl, sizeof(VcfCtl), hipMemcpyDeviceToHost, ctx->stream));
    PG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const int64_t lines = res.lines;
    PG_CHECK(ctx, lines >= 1 && lines <= bytes && res.newlines <= lines, "vcf_parse: internal error, %lld lines in %lld bytes", (long long)lines, (long long)bytes);
    const int64_t nbk = (lines + 255) / 256;
    const size_t o_start = off; off = up16(off + 8 * (size_t)(lines + 2));
    const size_t o_info = off; off = up16(off + 4 * (size_t)lines);
    const size_t o_local = off; off = up16(off + 4 * (size_t)lines);
    const size_t o_bsk = off; off = up16(off + 8 * (size_t)nbk);
    const size_t o_bok = off; off = up16(off + 8 * (size_t)nbk);
    const size_t before = ctx->ws.bytes();
    rc = pg_ws_reserve(ctx, off);
    if (rc) return rc;
    pg_prof_begin(ctx, PG_K_VCF | PG_PROF_CONT);
    if (ctx->ws.bytes() != before) PG_HIP(ctx, count_lines()); // the workspace was replaced by a larger block (wherever that one lies): its front part again (the same numbers)
    char *ws = static_cast<char *>(ctx->ws.get());
    VcfCtl *ctl = reinterpret_cast<VcfCtl *>(ws + o_ctl);
    int64_t *start = reinterpret_cast<int64_t *>(ws + o_start), *bsk = reinterpret_cast<int64_t *>(ws + o_bsk), *bok = reinterpret_cast<int64_t *>(ws + o_bok);
    int32_t *linfo = reinterpret_cast<int32_t *>(ws + o_info), *local = reinterpret_cast<int32_t *>(ws + o_local);
    hipLaunchKernelGGL(k_vcf_index<true>, dim3((unsigned)nbi), dim3(VCF_THREADS), 0, ctx->stream, T, (int64_t *)nullptr,
                       reinterpret_cast<const int64_t *>(ws + o_boi), (const VcfCtl *)ctl, start);
    VcfRule R;
    R.sizes = reinterpret_cast<const double *>(ws + o_sizes);
    R.n_sizes = n_sizes;
    R.F = n_sizes + PG_VCF_FIXED_FIELDS + 1;
    R.depth = min_coverage_depth;
    R.breadth = pg_vcf_breadth_threshold(min_coverage_breadth, n_sizes);
    R.maf = min_allele_frequency;
    R.sizes_sum = 0.0;
    for (int i = 0; i < n_sizes; ++i) R.sizes_sum += pool_sizes[i];
    const int shift = vcf_lpr_shift(n_sizes);
    const int lines_per_block = VCF_THREADS >> shift;
    const int64_t nbp = (lines + lines_per_block - 1) / lines_per_block;
    PG_CHECK(ctx, nbp < ((int64_t)1 << 31), "vcf_parse: %lld lines in one slab; cut the text into smaller slabs", (long long)lines);
    const size_t lds = sizeof(int) * (size_t)lines_per_block * (size_t)R.F; // at most 32 x 18 or 4 x 2058 ints
    const VcfOut none{nullptr, nullptr, nullptr, nullptr, nullptr, 0};
    hipLaunchKernelGGL(k_vcf_parse<false>, dim3((unsigned)nbp), dim3(VCF_THREADS), lds, ctx->stream, T, (const int64_t *)start, lines, R, shift, linfo,
                       ctl, (const int32_t *)nullptr, (const int64_t *)nullptr, none);
    hipLaunchKernelGGL(k_vcf_keep, dim3((unsigned)nbk), dim3(256), 0, ctx->stream, (const int32_t *)linfo, lines, (const int64_t *)start, local, bsk, ctl);
    hipLaunchKernelGGL(k_vcf_scan, dim3(1), dim3(1024), 0, ctx->stream, (const int64_t *)bsk, nbk, bok, &ctl->kept, (const unsigned char *)nullptr,
                       (int64_t)0, (long long *)nullptr);
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
    hipLaunchKernelGGL(k_vcf_parse<true>, dim3((unsigned)nbp), dim3(VCF_THREADS), lds, ctx->stream, T, (const int64_t *)start, lines, R, shift, linfo, ctl,
                       (const int32_t *)local, (const int64_t *)bok, O);
    pg_prof_end(ctx);
    PG_HIP(ctx, hipGetLastError());
    return PG_OK;
}
