// pg_sync.hip -- the sync reader on the device: a slab of sync text to the counts of its loci (the rules, shared with the host
// twin, are pg_sync_line.h).  The index / scan pattern is pg_vcf.hip's, in a copy of its own.  Steps on
// the context's stream:
//   index   k_sync_index<false> (newlines per 4 KB of text: a lane reads one aligned 16-byte word; it also offers every line
//           start whose first byte is not '#' to a minimum, the first data line) + k_sync_scan (64-bit exclusive scan of the
//           workgroups' sums, 1024 per round) + k_sync_first (the tabs of that first line: the pool count, from which the host
//           sizes the lane groups) + k_sync_index<true> (the same read again, a block scan, and every newline writes the start
//           of the line behind it): start[0 .. lines], no host work per line;
//   parse   k_sync_parse<false>: a line is taken by a GROUP of lanes (8 .. 64, a power of two chosen from the pool count, so that
//           5 pools have 8 lines in a wave and 200 pools one line across it).  The group walks its line in chunks of one byte per
//           lane; a ballot on '\t' and a popcount of the lower lanes give a byte's field index, and the field starts go to LDS.
//           The position is read by every lane alike; then lane j takes pools j, j + lanes, ..  One int per line comes out
//           (kept, data line); a line where the host parser would throw enters (offset, reason) into one 64-bit atomicMin;
//   scan    k_sync_keep (exclusive scan of 256 keep flags per workgroup, data lines counted) + k_sync_scan: a kept line's rank
//           is blockoff[line >> 8] + local[line];
//   emit    k_sync_parse<true>: the kept lines are split and read again and write their rows at their rank; adjacent lanes
//           write adjacent pools, so a wave's stores are one contiguous run.
// No array is indexed at run time in a thread: a pool's numbers are the named members of PgSyncPool.  Every read of the text
// is a byte inside [0, bytes) or a whole aligned 16-byte word that holds such a byte.
#include "pg_common.h"
#include "pg_sync_line.h"

namespace {

constexpr int SYNC_THREADS = 256;
constexpr int SYNC_INFO_KEEP = 1, SYNC_INFO_DATA = 2;

struct SyncCtl { // read back by the host
    unsigned long long err;   // pg_sync_err_key of the first bad line, PG_SYNC_NO_ERR without one
    unsigned long long first; // the offset of the first line that does not start with '#', ~0 without one
    long long first_tabs;     // the tabs of that line
    long long newlines, lines, kept, data_lines;
};

struct SyncText {
    const unsigned char *text;
    int64_t bytes;
    int64_t head;    // text - head is 16-byte aligned
    int64_t nchunks; // aligned 16-byte words that hold a byte of the text
};

// lanes per line: the smallest power of two that holds the pools, from 8 lanes to a wave
int sync_lpr_shift(int n) {
    int s = 3;
    while (s < 6 && (1 << s) < n) ++s;
    return s;
}

// bit k = byte k of x equals the byte repeated in c4
__device__ __forceinline__ unsigned sync_eq4(unsigned x, unsigned c4) {
    const unsigned y = x ^ c4;
    const unsigned z = ~(((y & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | y | 0x7F7F7F7Fu); // 0x80 in every byte of y that is zero
    return ((z >> 7) & 1u) | ((z >> 14) & 2u) | ((z >> 21) & 4u) | ((z >> 28) & 8u);
}

// of the bytes of aligned word c that belong to the text: *nl bit k = position 16 c - head + k is '\n', *hash the same for '#'
__device__ __forceinline__ void sync_masks(const SyncText &T, int64_t c, unsigned *nl, unsigned *hash) {
    *nl = 0u;
    *hash = 0u;
    if (c >= T.nchunks) return;
    const uint4 w = *reinterpret_cast<const uint4 *>(T.text - T.head + 16 * c); // whole inside the aligned words the text touches
    unsigned m = sync_eq4(w.x, 0x0A0A0A0Au) | (sync_eq4(w.y, 0x0A0A0A0Au) << 4) | (sync_eq4(w.z, 0x0A0A0A0Au) << 8) | (sync_eq4(w.w, 0x0A0A0A0Au) << 12);
    unsigned h = sync_eq4(w.x, 0x23232323u) | (sync_eq4(w.y, 0x23232323u) << 4) | (sync_eq4(w.z, 0x23232323u) << 8) | (sync_eq4(w.w, 0x23232323u) << 12);
    const int64_t p0 = 16 * c - T.head;
    unsigned valid = 0xffffu;
    if (p0 < 0) valid &= (0xffffu << (int)(-p0)) & 0xffffu;
    if (p0 + 16 > T.bytes) valid &= (1u << (int)(T.bytes - p0)) - 1u;
    *nl = m & valid;
    *hash = h & valid;
}

// ---- index ---------------------------------------------------------------------------------------------------------------
template <bool EMIT>
__global__ __launch_bounds__(SYNC_THREADS) void k_sync_index(const SyncText T, int64_t *__restrict__ blocksum, const int64_t *__restrict__ blockoff,
                                                             SyncCtl *__restrict__ ctl, int64_t *__restrict__ start) {
    __shared__ int sc[SYNC_THREADS];
    const int tid = threadIdx.x;
    const int64_t c = (int64_t)blockIdx.x * SYNC_THREADS + tid;
    unsigned m, hash;
    sync_masks(T, c, &m, &hash);
    const int64_t p0 = 16 * c - T.head;
    if (!EMIT && c < T.nchunks) {
        // the line starts among this word's bytes: behind a newline of this word, behind one that ends the word before, at 0
        unsigned ls = (m << 1) & 0xffffu;
        if (p0 <= 0) ls |= 1u << (int)(-p0);
        else if (T.text[p0 - 1] == '\n') ls |= 1u; // 0 <= p0 - 1 < bytes
        if (p0 + 16 > T.bytes) ls &= (1u << (int)(T.bytes - p0)) - 1u; // `bytes` itself starts no line
        ls &= ~hash;
        if (ls) {
            const unsigned long long cand = (unsigned long long)(p0 + (__ffs(ls) - 1));
            if (cand < *reinterpret_cast<volatile unsigned long long *>(&ctl->first)) atomicMin(&ctl->first, cand); // (the value only falls)
        }
    }
    const int cnt = __popc(m);
    sc[tid] = cnt;
    __syncthreads();
    for (int d = 1; d < SYNC_THREADS; d <<= 1) {
        const int v = tid >= d ? sc[tid - d] : 0;
        __syncthreads();
        sc[tid] += v;
        __syncthreads();
    }
    if (!EMIT) {
        if (tid == SYNC_THREADS - 1) blocksum[blockIdx.x] = sc[SYNC_THREADS - 1];
        return;
    }
    int64_t rank = blockoff[blockIdx.x] + (sc[tid] - cnt); // newlines in front of this word
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

// exclusive 64-bit scan of the workgroups' sums (the pattern of k_vcf_scan / k_csv_scan, in a copy of its own); the total goes
// to *total, and with `text` the number of lines to *lines
__global__ __launch_bounds__(1024) void k_sync_scan(const int64_t *__restrict__ blocksum, int64_t nb, int64_t *__restrict__ blockoff,
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

// the tabs of the first line that does not start with '#' (one workgroup; 256 bytes a round, up to the line's newline)
__global__ __launch_bounds__(SYNC_THREADS) void k_sync_first(const SyncText T, SyncCtl *__restrict__ ctl) {
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
__global__ __launch_bounds__(SYNC_THREADS) void k_sync_parse(const SyncText T, const int64_t *__restrict__ start, int64_t lines, int n_ref, int F,
                                                             int shift, int32_t *__restrict__ info, SyncCtl *__restrict__ ctl,
                                                             const int32_t *__restrict__ local, const int64_t *__restrict__ blockoff, const SyncOut O) {
    extern __shared__ int fs_all[];
    const int tid = threadIdx.x;
    const int lpr = 1 << shift;
    const int g = tid >> shift, gl = tid & (lpr - 1);
    const int gbase = (tid & 63) & ~(lpr - 1); // the group's first lane in its wave
    const uint64_t gmask = lpr == 64 ? ~0ULL : ((1ULL << lpr) - 1ULL);
    int *fs = fs_all + g * F;
    const int64_t line = (int64_t)blockIdx.x * (blockDim.x >> shift) + g;
    bool active = line < lines; // uniform over the group, as is everything decided from the line alone
    if (EMIT && active) active = (info[line] & SYNC_INFO_KEEP) != 0;
    int64_t s = 0;
    int res = 0, wlen = 0; // res: 0 skipped, 1 kept, or minus a pg_sync_reason
    bool data = false;
    if (active) {
        s = start[line];
        const int64_t e = start[line + 1] - 1; // the newline's place, or `bytes` for a last line without one
        int64_t len = e - s;
        if (len > 0 && T.text[e - 1] == '\r') --len;
        if (len == 0) res = -PG_SYNC_E_EMPTY;
        else if (T.text[s] != '#') {
            data = true;
            if (len > 0x7fffffffLL) res = -PG_SYNC_E_LONG;
            else wlen = (int)len;
        }
    }
    const unsigned char *L = T.text + s;
    // the field starts: fs[f] = where field f begins, for 1 <= f < F
    int ntabs = 0;
    for (int off = 0; off < wlen; off += lpr) { // (one trip count for the group; other groups of the wave may leave earlier)
        const int idx = off + gl;
        const bool tab = idx < wlen && L[idx] == '\t';
        const uint64_t gb = ((uint64_t)__ballot(tab) >> gbase) & gmask;
        if (tab) {
            const int f = ntabs + __popcll(gb & ((1ULL << gl) - 1ULL)) + 1;
            if (f < F) fs[f] = idx + 1;
        }
        ntabs += __popcll(gb);
    }
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
            if (EMIT) rank = blockoff[line >> 8] + local[line];
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

// ---- scan of the keep flags (k_vcf_keep's pattern) -------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_sync_keep(const int32_t *__restrict__ info, int64_t lines, int32_t *__restrict__ local,
                                                   int64_t *__restrict__ blocksum, SyncCtl *__restrict__ ctl) {
    __shared__ int sc[256];
    __shared__ int sd[256];
    const int tid = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * 256 + tid;
    const int v = i < lines ? info[i] : 0;
    const int c = v & SYNC_INFO_KEEP;
    sc[tid] = c;
    sd[tid] = (v & SYNC_INFO_DATA) ? 1 : 0;
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
    SyncText T;
    T.text = reinterpret_cast<const unsigned char *>(text_dev);
    T.bytes = bytes;
    T.head = (int64_t)(reinterpret_cast<uintptr_t>(text_dev) & 15);
    T.nchunks = (bytes + T.head + 15) / 16;
    const int64_t nbi = (T.nchunks + SYNC_THREADS - 1) / SYNC_THREADS;
    auto up16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
    size_t off = 0;
    const size_t o_ctl = off; off = up16(off + sizeof(SyncCtl));
    const size_t o_bsi = off; off = up16(off + 8 * (size_t)nbi);
    const size_t o_boi = off; off = up16(off + 8 * (size_t)nbi);
    const size_t front = off;
    int rc = pg_ws_reserve(ctx, front);
    if (rc) return rc;
    SyncCtl init{};
    init.err = PG_SYNC_NO_ERR;
    init.first = ~0ULL;
    auto count_lines = [&]() -> hipError_t { // the control block, the newlines of every 4 KB, their scan, the first data line
        char *ws = static_cast<char *>(ctx->ws.get());
        hipError_t e = hipMemcpyAsync(ws + o_ctl, &init, sizeof(SyncCtl), hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) return e;
        SyncCtl *ctl = reinterpret_cast<SyncCtl *>(ws + o_ctl);
        hipLaunchKernelGGL(k_sync_index<false>, dim3((unsigned)nbi), dim3(SYNC_THREADS), 0, ctx->stream, T, reinterpret_cast<int64_t *>(ws + o_bsi),
                           (const int64_t *)nullptr, ctl, (int64_t *)nullptr);
        hipLaunchKernelGGL(k_sync_scan, dim3(1), dim3(1024), 0, ctx->stream, reinterpret_cast<const int64_t *>(ws + o_bsi), nbi,
                           reinterpret_cast<int64_t *>(ws + o_boi), &ctl->newlines, T.text, bytes, &ctl->lines);
        hipLaunchKernelGGL(k_sync_first, dim3(1), dim3(SYNC_THREADS), 0, ctx->stream, T, ctl);
        return hipGetLastError();
    };
    SyncCtl res{};
    pg_prof_begin(ctx, PG_K_SYNC);
    PG_HIP(ctx, count_lines());
    pg_prof_end(ctx);
    PG_HIP(ctx, hipMemcpyAsync(&res, static_cast<char *>(ctx->ws.get()) + o_ctl, sizeof(SyncCtl), hipMemcpyDeviceToHost, ctx->stream));
    PG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const int64_t lines = res.lines;
    PG_CHECK(ctx, lines >= 1 && lines <= bytes && res.newlines <= lines, "sync_parse: internal error, %lld lines in %lld bytes", (long long)lines, (long long)bytes);
    // the first line that does not start with '#' fixes the pool count
    uint64_t first_err = PG_SYNC_NO_ERR;
    int n_first = 0;
    if (res.first != ~0ULL) {
        const int code = pg_sync_first_line((int)std::min<long long>(res.first_tabs, PG_SYNC_TAB_CAP), expect_n, &n_first);
        if (code) first_err = pg_sync_err_key((int64_t)res.first, code);
    }
    const int n_ref = expect_n > 0 ? expect_n : std::max(1, std::min(n_first, PG_SYNC_MAX_POOLS)); // what the lines are compared with
    const int64_t nbk = (lines + 255) / 256;
    const size_t o_start = off; off = up16(off + 8 * (size_t)(lines + 2));
    const size_t o_info = off; off = up16(off + 4 * (size_t)lines);
    const size_t o_local = off; off = up16(off + 4 * (size_t)lines);
    const size_t o_bsk = off; off = up16(off + 8 * (size_t)nbk);
    const size_t o_bok = off; off = up16(off + 8 * (size_t)nbk);
    const size_t before = ctx->ws.bytes();
    rc = pg_ws_reserve(ctx, off);
    if (rc) return rc;
    pg_prof_begin(ctx, PG_K_SYNC | PG_PROF_CONT);
    if (ctx->ws.bytes() != before) PG_HIP(ctx, count_lines()); // the workspace was replaced by a larger block (wherever that one lies): its front part again (the same numbers)
    char *ws = static_cast<char *>(ctx->ws.get());
    SyncCtl *ctl = reinterpret_cast<SyncCtl *>(ws + o_ctl);
    int64_t *start = reinterpret_cast<int64_t *>(ws + o_start), *bsk = reinterpret_cast<int64_t *>(ws + o_bsk), *bok = reinterpret_cast<int64_t *>(ws + o_bok);
    int32_t *linfo = reinterpret_cast<int32_t *>(ws + o_info), *local = reinterpret_cast<int32_t *>(ws + o_local);
    hipLaunchKernelGGL(k_sync_index<true>, dim3((unsigned)nbi), dim3(SYNC_THREADS), 0, ctx->stream, T, (int64_t *)nullptr,
                       reinterpret_cast<const int64_t *>(ws + o_boi), ctl, start);
    const int F = n_ref + 4; // field starts a group keeps: 1 .. n_ref + 3
    const int shift = sync_lpr_shift(n_ref);
    const int threads = n_ref > 1024 ? 64 : SYNC_THREADS; // one line per workgroup where a line's field starts take 4 KB or more
    const int lines_per_block = threads >> shift;
    const int64_t nbp = (lines + lines_per_block - 1) / lines_per_block;
    PG_CHECK(ctx, nbp < ((int64_t)1 << 31), "sync_parse: %lld lines in one slab; cut the text into smaller slabs", (long long)lines);
    const size_t lds = sizeof(int) * (size_t)lines_per_block * (size_t)F; // at most 32 x 12, 4 x 1028 or 1 x 4100 ints
    const SyncOut none{nullptr, nullptr, nullptr, nullptr};
    hipLaunchKernelGGL(k_sync_parse<false>, dim3((unsigned)nbp), dim3(threads), lds, ctx->stream, T, (const int64_t *)start, lines, n_ref, F, shift, linfo,
                       ctl, (const int32_t *)nullptr, (const int64_t *)nullptr, none);
    hipLaunchKernelGGL(k_sync_keep, dim3((unsigned)nbk), dim3(256), 0, ctx->stream, (const int32_t *)linfo, lines, local, bsk, ctl);
    hipLaunchKernelGGL(k_sync_scan, dim3(1), dim3(1024), 0, ctx->stream, (const int64_t *)bsk, nbk, bok, &ctl->kept, (const unsigned char *)nullptr,
                       (int64_t)0, (long long *)nullptr);
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
    hipLaunchKernelGGL(k_sync_parse<true>, dim3((unsigned)nbp), dim3(threads), lds, ctx->stream, T, (const int64_t *)start, lines, n_ref, F, shift, linfo, ctl,
                       (const int32_t *)local, (const int64_t *)bok, O);
    pg_prof_end(ctx);
    PG_HIP(ctx, hipGetLastError());
    return PG_OK;
}
