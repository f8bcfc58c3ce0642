// pg_sync.hip -- the sync reader on the device: a slab of sync text to the counts of its loci (the rules, shared with the host
// twin, are pg_sync_line.h).  The index, the scans and the lane-group steps are the shared ones of
// pg_text_steps.h.  Steps on the context's stream:
//   index   PgLineIndex: k_text_index<false> (newlines per 4 KB of text: a lane reads one aligned 16-byte word; through
//           SyncFirstHook it also offers every line start whose first byte is not '#' to a minimum, the first data line) +
//           k_scan_blocks (64-bit exclusive scan of the workgroups' sums, 1024 per round) + k_sync_first (the tabs of that first
//           line: the pool count, from which the host sizes the lane groups) + k_text_index<true> (the same read again, a block
//           scan, and every newline writes the start of the line behind it): start[0 .. lines], no host work per line;
//   parse   k_sync_parse<false>: a line is taken by a GROUP of lanes (8 .. 64, a power of two chosen from the pool count, so that
//           5 pools have 8 lines in a wave and 200 pools one line across it).  The group walks its line in chunks of one byte per
//           lane; a ballot on '\t' and a popcount of the lower lanes give a byte's field index, and the field starts go to LDS.
//           The position is read by every lane alike; then lane j takes pools j, j + lanes, ..  One int per line comes out
//           (kept, data line); a line where the host parser would throw enters (offset, reason) into one 64-bit atomicMin;
//   scan    k_scan_keep (exclusive scan of 256 keep flags per workgroup, data lines counted) + k_scan_blocks: a kept line's rank
//           is scan_rank(local, blockoff, line);
//   emit    k_sync_parse<true>: the kept lines are split and read again and write their rows at their rank; adjacent lanes
//           write adjacent pools, so a wave's stores are one contiguous run.
// No array is indexed at run time in a thread: a pool's numbers are the named members of PgSyncPool.  Every read of the text
// is a byte inside [0, bytes) or a whole aligned 16-byte word that holds such a byte.
#include "pg_common.h"
#include "pg_text_steps.h"
#include "pg_sync_line.h"

namespace {

constexpr int SYNC_THREADS = 256;
constexpr int SYNC_INFO_KEEP = PG_LINE_KEEP, SYNC_INFO_DATA = PG_LINE_DATA;

struct SyncCtl { // read back by the host
    PgLineCounts n;
    unsigned long long err;   // pg_sync_err_key of the first bad line, PG_SYNC_NO_ERR without one
    unsigned long long first; // the offset of the first line that does not start with '#', ~0 without one
    long long first_tabs;     // the tabs of that line
    int64_t kept, data_lines;
};

// The index's hook: every line start whose first byte is not '#' is offered to a minimum, the first data line.
struct SyncFirstHook {
    unsigned long long *first; // SyncCtl::first
    __device__ void operator()(const PgText &T, int64_t c, int64_t p0, unsigned m) const {
        const unsigned hash = text_eq_mask(T, c, '#');
        // the line starts among this word's bytes: behind a newline of this word, behind one that ends the word before, at 0
        unsigned ls = (m << 1) & 0xffffu;
        if (p0 <= 0) ls |= 1u << (int)(-p0);
        else if (T.text[p0 - 1] == '\n') ls |= 1u; // 0 <= p0 - 1 < bytes
        if (p0 + 16 > T.bytes) ls &= (1u << (int)(T.bytes - p0)) - 1u; // `bytes` itself starts no line
        ls &= ~hash;
        if (ls) {
            const unsigned long long cand = (unsigned long long)(p0 + (__ffs(ls) - 1));
            if (cand < *reinterpret_cast<volatile unsigned long long *>(first)) atomicMin(first, cand); // (the value only falls)
        }
    }
};

// the tabs of the first line that does not start with '#' (one workgroup; 256 bytes a round, up to the line's newline)
__global__ __launch_bounds__(SYNC_THREADS) void k_sync_first(const PgText T, SyncCtl *__restrict__ ctl) {
    __shared__ int tabs[SYNC_THREADS];
    __shared__ int stop;
    const int tid = threadIdx.x;
    const unsigned long long first = ctl->first;
    if (first == ~0ULL) return; // (uniform)
    int mine = 0;
    for (int64_t base = (int64_t)first; base < T.bytes; base += SYNC_THREADS) {
        if (tid == 0) stop = SYNC_THREADS;
        __syncthreads();
        const int64_t p = base + tid;
        const unsigned char b = p < T.bytes ? T.text[p] : (unsigned char)'\n';
        if (b == '\n') atomicMin(&stop, tid);
        __syncthreads();
        const int end = stop;
        if (b == '\t' && tid < end) ++mine;
        __syncthreads(); // (stop is set again only behind this)
        if (end < SYNC_THREADS) break;
    }
    tabs[tid] = mine;
    __syncthreads();
    for (int d = SYNC_THREADS / 2; d > 0; d >>= 1) {
        if (tid < d) tabs[tid] += tabs[tid + d];
        __syncthreads();
    }
    if (tid == 0) ctl->first_tabs = tabs[0];
}

// ---- parse and emit --------------------------------------------------------------------------------------------------------
struct SyncOut {
    uint32_t *counts;
    uint64_t *pos;
    int64_t *line_off;
    int32_t *chrom_len;
};

template <bool EMIT>
__global__ __launch_bounds__(SYNC_THREADS) void k_sync_parse(const PgText T, const int64_t *__restrict__ start, int64_t lines, int n_ref, int F,
                                                             int shift, int32_t *__restrict__ info, SyncCtl *__restrict__ ctl,
                                                             const int32_t *__restrict__ local, const int64_t *__restrict__ blockoff, const SyncOut O) {
    extern __shared__ int fs_all[];
    const int tid = threadIdx.x;
    const PgLaneGroup G = lane_group(tid, shift);
    const int lpr = G.lpr, g = G.g, gl = G.gl;
    int *fs = fs_all + g * F;
    const int64_t line = (int64_t)blockIdx.x * (blockDim.x >> shift) + g;
    bool active = line < lines; // uniform over the group, as is everything decided from the line alone
    if (EMIT && active) active = (info[line] & SYNC_INFO_KEEP) != 0;
    int64_t s = 0;
    int res = 0, wlen = 0; // res: 0 skipped, 1 kept, or minus a pg_sync_reason
    bool data = false;
    if (active) {
        int64_t len;
        line_bounds(T, start, line, true, &s, &len); // a '\r' goes from a last line without its newline too
        if (len == 0) res = -PG_SYNC_E_EMPTY;
        else if (T.text[s] != '#') {
            data = true;
            if (len > PG_LINE_MAX) res = -PG_SYNC_E_LONG;
            else wlen = (int)len;
        }
    }
    const unsigned char *L = T.text + s;
    // the field starts: fs[f] = where field f begins, for 1 <= f < F
    const int ntabs = group_split_tabs(L, wlen, G, fs, F);
    __syncthreads(); // every thread of the workgroup arrives: no path above returns
    if (wlen > 0) {
        uint64_t pos = 0;
        const bool pos_ok = ntabs >= 2 && pg_sync_pos(L + fs[1], fs[2] - 1 - fs[1], &pos); // F >= 5: fs[1] and fs[2] are kept
        const int head = pg_sync_head(ntabs, pos_ok);
        res = head;
        if (head == 1) {
            const int m = ntabs - 2;            // the pools of this line: fields 3 .. ntabs
            const int mm = min(m, n_ref);       // those that are looked at; field 3 + j < F - 1 for j < mm
            int err = m != n_ref ? PG_SYNC_E_POOLS : 0;
            int64_t rank = 0;
            if (EMIT) rank = scan_rank(local, blockoff, line);
            for (int j0 = 0; j0 < mm; j0 += lpr) { // one trip count for the group
                const int j = j0 + gl;
                if (j < mm) {
                    const int f = 3 + j;
                    const int fe = f < ntabs ? fs[f + 1] - 1 : wlen; // f + 1 <= mm + 3 <= n_ref + 3 < F
                    PgSyncPool pl;
                    pg_sync_pool(L + fs[f], fe - fs[f], &pl);
                    if (EMIT) {
                        uint32_t *dst = O.counts + (rank * n_ref + j) * 6; // rank < kept <= cap_loci, j < n_pools: inside cap_counts
                        dst[0] = pl.c0; dst[1] = pl.c1; dst[2] = pl.c2; dst[3] = pl.c3; dst[4] = pl.c4; dst[5] = pl.c5;
                    } else
                        err = pg_sync_min_code(err, pl.err);
                }
            }
            if (EMIT) {
                if (gl == 0) {
                    O.pos[rank] = pos;
                    O.line_off[rank] = s;
                    O.chrom_len[rank] = fs[1] - 1;
                }
            } else {
                for (int d = 1; d < lpr; d <<= 1) err = pg_sync_min_code(err, __shfl_xor(err, d, lpr));
                if (err) res = -err;
            }
        }
    }
    if (!EMIT && active && gl == 0) {
        info[line] = (res == 1 ? SYNC_INFO_KEEP : 0) | (data ? SYNC_INFO_DATA : 0);
        if (res < 0) atomicMin(&ctl->err, (unsigned long long)pg_sync_err_key(s, -res));
    }
}

const char *sync_reason_text(int r) {
    switch (r) {
    case PG_SYNC_E_EMPTY: return "an empty line";
    case PG_SYNC_E_FIELDS: return "fewer than four tab-separated fields";
    case PG_SYNC_E_COUNT: return "the allele counts are not valid integers, or a pool has fewer than six";
    case PG_SYNC_E_COUNT32: return "an allele count above 4294967295";
    case PG_SYNC_E_POOLS: return "inconsistent number of pools";
    case PG_SYNC_E_LONG: return "a line of 2^31 bytes or more";
    }
    return "unknown";
}

} // namespace

extern "C" int pg_sync_parse_dev(pg_ctx *ctx, const char *text_dev, int64_t bytes, int expect_n, uint32_t *counts_dev, uint64_t *pos_dev,
                                 int64_t *line_off_dev, int32_t *chrom_len_dev, int64_t cap_loci, int64_t cap_counts, pg_sync_info *info) {
    if (!ctx) return PG_ERR_INVALID;
    PG_CHECK(ctx, info != nullptr, "sync_parse: null pointer");
    *info = pg_sync_info{0, 0, -1, 0, 0};
    PG_CHECK(ctx, bytes >= 0 && (bytes == 0 || text_dev) && expect_n >= 0 && cap_loci >= 0 && cap_counts >= 0,
             "sync_parse: bad arguments bytes=%lld expect_n=%d cap_loci=%lld cap_counts=%lld", (long long)bytes, expect_n, (long long)cap_loci,
             (long long)cap_counts);
    PG_CHECK(ctx, expect_n <= PG_SYNC_MAX_POOLS, "sync_parse: %d pools, at most %d are supported", expect_n, PG_SYNC_MAX_POOLS);
    PG_CHECK(ctx, bytes < ((int64_t)1 << 40), "sync_parse: a slab of %lld bytes; cut the text at line starts into slabs below 2^40", (long long)bytes);
    if (bytes == 0) return PG_OK;
    PG_HIP(ctx, hipSetDevice(ctx->device));
    const PgText T = pg_text(text_dev, bytes);
    SyncCtl init{};
    init.err = PG_SYNC_NO_ERR;
    init.first = ~0ULL;
    auto front = [&](char *ws, auto count_lines) -> hipError_t { // the front block is SyncCtl alone; behind the index, the first data line's tabs
        SyncCtl *ctl = reinterpret_cast<SyncCtl *>(ws);
        const hipError_t e = hipMemcpyAsync(ctl, &init, sizeof(SyncCtl), hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) return e;
        count_lines(SyncFirstHook{&ctl->first});
        hipLaunchKernelGGL(k_sync_first, dim3(1), dim3(SYNC_THREADS), 0, ctx->stream, T, ctl);
        return hipGetLastError();
    };
    SyncCtl res{};
    PgLineIndex X;
    int rc = X.build(ctx, PG_K_SYNC, "sync_parse", T, sizeof(SyncCtl), front, &res);
    if (rc) return rc;
    const int64_t lines = X.lines;
    SyncCtl *ctl = reinterpret_cast<SyncCtl *>(X.ws);
    // the first line that does not start with '#' fixes the pool count
    uint64_t first_err = PG_SYNC_NO_ERR;
    int n_first = 0;
    if (res.first != ~0ULL) {
        const int code = pg_sync_first_line((int)std::min<long long>(res.first_tabs, PG_SYNC_TAB_CAP), expect_n, &n_first);
        if (code) first_err = pg_sync_err_key((int64_t)res.first, code);
    }
    const int n_ref = expect_n > 0 ? expect_n : std::max(1, std::min(n_first, PG_SYNC_MAX_POOLS)); // what the lines are compared with
    const int F = n_ref + 4; // field starts a group keeps: 1 .. n_ref + 3
    const int shift = pg_lpr_shift(n_ref, 3); // so that 5 pools have 8 lines in a wave and 200 pools one line across it
    const int threads = n_ref > 1024 ? 64 : SYNC_THREADS; // one line per workgroup where a line's field starts take 4 KB or more
    const int lines_per_block = threads >> shift;
    int64_t nbp;
    rc = X.parse_blocks(ctx, "sync_parse", lines_per_block, &nbp);
    if (rc) return rc;
    const size_t lds = sizeof(int) * (size_t)lines_per_block * (size_t)F; // at most 32 x 12, 4 x 1028 or 1 x 4100 ints
    const SyncOut none{nullptr, nullptr, nullptr, nullptr};
    pg_prof_begin(ctx, PG_K_SYNC | PG_PROF_CONT);
    hipLaunchKernelGGL(k_sync_parse<false>, dim3((unsigned)nbp), dim3(threads), lds, ctx->stream, T, (const int64_t *)X.start, lines, n_ref, F, shift, X.info,
                       ctl, (const int32_t *)nullptr, (const int64_t *)nullptr, none);
    hipLaunchKernelGGL(k_scan_keep, dim3((unsigned)X.nbk), dim3(PG_COUNT_ROWS), 0, ctx->stream, (const int32_t *)X.info, lines, X.local, X.bsk,
                       &ctl->data_lines);
    X.scan_kept(ctx, &ctl->kept);
    pg_prof_end(ctx);
    PG_HIP(ctx, hipGetLastError());
    PG_HIP(ctx, hipMemcpyAsync(&res, ctl, sizeof(SyncCtl), hipMemcpyDeviceToHost, ctx->stream));
    PG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    info->data_lines = res.data_lines;
    const uint64_t err = std::min<uint64_t>(res.err, first_err);
    if (err != PG_SYNC_NO_ERR) {
        info->err_line_off = (int64_t)(err >> 8);
        info->err_reason = (int32_t)(err & 0xff);
        return pg_fail(ctx, PG_ERR_INVALID, "sync_parse: the line at byte %lld of the text: %s", (long long)info->err_line_off,
                       sync_reason_text(info->err_reason));
    }
    info->kept = res.kept;
    info->n_pools = n_first;
    const int64_t need_counts = res.kept * info->n_pools * 6;
    PG_CHECK(ctx, res.kept <= cap_loci && need_counts <= cap_counts, "sync_parse: %lld loci of %d pools need %lld count elements, the buffers hold %lld loci and %lld",
             (long long)res.kept, (int)info->n_pools, (long long)need_counts, (long long)cap_loci, (long long)cap_counts);
    if (res.kept == 0) return PG_OK;
    PG_CHECK(ctx, pos_dev && line_off_dev && chrom_len_dev && counts_dev, "sync_parse: null output buffer");
    const SyncOut O{counts_dev, pos_dev, line_off_dev, chrom_len_dev};
    pg_prof_begin(ctx, PG_K_SYNC | PG_PROF_CONT);
    hipLaunchKernelGGL(k_sync_parse<true>, dim3((unsigned)nbp), dim3(threads), lds, ctx->stream, T, (const int64_t *)X.start, lines, n_ref, F, shift, X.info, ctl,
                       (const int32_t *)X.local, (const int64_t *)X.bok, O);
    pg_prof_end(ctx);
    PG_HIP(ctx, hipGetLastError());
    return PG_OK;
}
