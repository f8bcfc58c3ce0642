// pg_text_steps.h -- the steps that the device text paths share, written once: the parsers (pg_vcf.hip, pg_sync.hip,
// pg_pileup.hip) and the writers (pg_csv.hip, pg_syncfmt.hip, pg_resultfmt.hip, pg_tablefmt.hip); the loader of pg_locus_ops.hip takes the scan of
// the workgroups' sums.  Nothing here knows a format.  Header-only: everything is in an anonymous namespace, so every translation
// unit has its own instances (of the templates, those it launches).
//   text and index   PgText, text_eq_mask, k_text_index<EMIT, Hook>: start[0 .. lines] of a text without host work per line;
//   scans            block_scan (one workgroup over an LDS array), k_scan_blocks (64-bit scan of the workgroups' sums),
//                    k_scan_lengths (the writers' lengths), k_scan_keep (the parsers' keep flags), scan_rank / scan_off;
//   lane groups      pg_lpr_shift, PgLaneGroup, group_split_tabs, line_bounds: a line or row taken by 2^shift lanes of a wave;
//   tile flush       tile_flush: an LDS tile laid out like the 16-byte words of the output, copied out;
//   host side        PgLineIndex (the parsers' two-phase reservation and line index), PgLengthScan (the writers' offsets).
#pragma once
#include "pg_common.h"
#include <algorithm>
#include <cstddef>

namespace {

constexpr int PG_INDEX_THREADS = 256;                                  // aligned 16-byte words per workgroup of the index: 4 KB of text
constexpr int PG_COUNT_SHIFT = 8, PG_COUNT_ROWS = 1 << PG_COUNT_SHIFT; // elements per workgroup of a scan's first level
constexpr int PG_SCAN_WIDTH = 1024;                                    // workgroup sums per round of its second level
constexpr int PG_LINE_KEEP = 1, PG_LINE_DATA = 2;                      // the bits of a line's info word that k_scan_keep reads
constexpr int64_t PG_LINE_MAX = 0x7fffffffLL;                          // a longer line is refused: offsets inside a line are int

inline size_t pg_up16(size_t x) { return (x + 15) & ~(size_t)15; }

// ---- text and index ------------------------------------------------------------------------------------------------------
struct PgText {
    const unsigned char *text;
    int64_t bytes;
    int64_t head;    // text - head is 16-byte aligned
    int64_t nchunks; // aligned 16-byte words that hold a byte of the text
};

inline PgText pg_text(const char *text_dev, int64_t bytes) {
    PgText T;
    T.text = reinterpret_cast<const unsigned char *>(text_dev);
    T.bytes = bytes;
    T.head = (int64_t)(reinterpret_cast<uintptr_t>(text_dev) & 15);
    T.nchunks = (bytes + T.head + 15) / 16;
    return T;
}

struct PgLineCounts { // the first member of a parser's control struct: written by the index, read back by the host
    int64_t newlines, lines;
};

// bit k = byte k of x equals the byte repeated in c4
__device__ __forceinline__ unsigned text_eq4(unsigned x, unsigned c4) {
    const unsigned y = x ^ c4;
    const unsigned z = ~(((y & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | y | 0x7F7F7F7Fu); // 0x80 in every byte of y that is zero
    return ((z >> 7) & 1u) | ((z >> 14) & 2u) | ((z >> 21) & 4u) | ((z >> 28) & 8u);
}

// the bytes equal to `byte` among those of aligned word c that belong to the text: bit k = position 16 c - head + k
__device__ __forceinline__ unsigned text_eq_mask(const PgText &T, int64_t c, unsigned char byte) {
    if (c >= T.nchunks) return 0u;
    const uint4 w = *reinterpret_cast<const uint4 *>(T.text - T.head + 16 * c); // whole inside the aligned words the text touches
    const unsigned c4 = 0x01010101u * byte;
    unsigned m = text_eq4(w.x, c4) | (text_eq4(w.y, c4) << 4) | (text_eq4(w.z, c4) << 8) | (text_eq4(w.w, c4) << 12);
    const int64_t p0 = 16 * c - T.head;
    if (p0 < 0) m &= (0xffffu << (int)(-p0)) & 0xffffu;
    if (p0 + 16 > T.bytes) m &= (1u << (int)(T.bytes - p0)) - 1u;
    return m;
}

// inclusive scan of sc[0 .. W) in place by the W threads of a workgroup (Hillis-Steele); thread tid has written sc[tid], every
// thread calls
struct PgPlus {
    template <class V> __device__ V operator()(const V &a, const V &b) const { return a + b; }
};
template <int W, class V, class Op = PgPlus>
__device__ __forceinline__ void block_scan(V *sc, int tid, Op op = Op()) {
    __syncthreads();
    for (int d = 1; d < W; d <<= 1) {
        V v = sc[tid];
        if (tid >= d) v = op(sc[tid - d], v);
        __syncthreads();
        sc[tid] = v;
        __syncthreads();
    }
}

struct PgNoHook {
    __device__ void operator()(const PgText &, int64_t, int64_t, unsigned) const {}
};

// The line index: a lane reads one aligned 16-byte word.  EMIT = false: the newlines of every 4 KB of text to blocksum, and
// hook(T, c, p0, newlines) once per word of the text (p0 = the position of the word's first byte, negative in front of the text).
// EMIT = true, behind k_scan_blocks: the same read again, and every newline writes the start of the line behind it.
template <bool EMIT, class Hook>
__global__ __launch_bounds__(PG_INDEX_THREADS) void k_text_index(const PgText T, int64_t *__restrict__ blocksum, const int64_t *__restrict__ blockoff,
                                                                 const PgLineCounts *__restrict__ n, int64_t *__restrict__ start, const Hook hook) {
    __shared__ int sc[PG_INDEX_THREADS];
    const int tid = threadIdx.x;
    const int64_t c = (int64_t)blockIdx.x * PG_INDEX_THREADS + tid;
    unsigned m = text_eq_mask(T, c, '\n');
    const int64_t p0 = 16 * c - T.head;
    if (!EMIT && c < T.nchunks) hook(T, c, p0, m);
    const int cnt = __popc(m);
    sc[tid] = cnt;
    block_scan<PG_INDEX_THREADS>(sc, tid);
    if (!EMIT) {
        if (tid == PG_INDEX_THREADS - 1) blocksum[blockIdx.x] = sc[PG_INDEX_THREADS - 1];
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
        if (n->lines > n->newlines) start[n->lines] = T.bytes + 1; // the last line lacks its newline: as if it stood at `bytes`
    }
}

// ---- scans ---------------------------------------------------------------------------------------------------------------
// exclusive 64-bit scan of the workgroups' sums, PG_SCAN_WIDTH per round (one workgroup); the total goes to *total, and with
// `text` the number of lines to *lines
__global__ __launch_bounds__(PG_SCAN_WIDTH) void k_scan_blocks(const int64_t *__restrict__ blocksum, int64_t nb, int64_t *__restrict__ blockoff,
                                                               int64_t *__restrict__ total, const unsigned char *__restrict__ text, int64_t bytes,
                                                               int64_t *__restrict__ lines) {
    __shared__ int64_t sc[PG_SCAN_WIDTH];
    __shared__ int64_t carry;
    const int tid = threadIdx.x;
    if (tid == 0) carry = 0;
    __syncthreads();
    for (int64_t base = 0; base < nb; base += PG_SCAN_WIDTH) {
        const int64_t i = base + tid;
        const int64_t c = i < nb ? blocksum[i] : 0;
        sc[tid] = c;
        block_scan<PG_SCAN_WIDTH>(sc, tid);
        if (i < nb) blockoff[i] = carry + sc[tid] - c;
        __syncthreads();
        if (tid == PG_SCAN_WIDTH - 1) carry += sc[PG_SCAN_WIDTH - 1];
        __syncthreads();
    }
    if (tid == 0) {
        *total = carry;
        if (text) *lines = carry + (text[bytes - 1] != '\n' ? 1 : 0);
    }
}

inline void pg_scan_blocks(pg_ctx *ctx, const int64_t *blocksum, int64_t nb, int64_t *blockoff, int64_t *total) {
    hipLaunchKernelGGL(k_scan_blocks, dim3(1), dim3(PG_SCAN_WIDTH), 0, ctx->stream, blocksum, nb, blockoff, total, (const unsigned char *)nullptr,
                       (int64_t)0, (int64_t *)nullptr);
}

struct PgScanCtl { // a writer's scan results, read back by the host
    int64_t total;
    int32_t max; // the longest element
    int32_t bad; // the measure kernel's flags
};

// the writers' lengths: exclusive scan of PG_COUNT_ROWS lengths per workgroup, the workgroup's sum, the longest element
struct PgSumMax {
    int sum, max;
};
struct PgSumMaxOp {
    __device__ PgSumMax operator()(const PgSumMax &a, const PgSumMax &b) const { return PgSumMax{a.sum + b.sum, a.max > b.max ? a.max : b.max}; }
};
__global__ __launch_bounds__(PG_COUNT_ROWS) void k_scan_lengths(int32_t *__restrict__ local, int64_t count, int64_t *__restrict__ blocksum,
                                                                PgScanCtl *__restrict__ ctl) {
    __shared__ PgSumMax sc[PG_COUNT_ROWS];
    const int tid = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * PG_COUNT_ROWS + tid;
    const int c = i < count ? local[i] : 0; // in: the element's length; out (same element, same thread): its offset inside the block
    sc[tid] = PgSumMax{c, c};
    block_scan<PG_COUNT_ROWS>(sc, tid, PgSumMaxOp());
    if (i < count) local[i] = sc[tid].sum - c;
    if (tid == PG_COUNT_ROWS - 1) {
        blocksum[blockIdx.x] = sc[PG_COUNT_ROWS - 1].sum;
        atomicMax(&ctl->max, sc[PG_COUNT_ROWS - 1].max);
    }
}

// the parsers' keep flags: exclusive scan of the PG_LINE_KEEP bits of PG_COUNT_ROWS lines per workgroup and the workgroup's sum;
// with `data_lines`, the PG_LINE_DATA bits are counted into it.  Returns the thread's info word (0 behind the last line).  Both
// counts are at most 256, so they share one int: the data lines from bit 16.
__device__ __forceinline__ int scan_keep_flags(const int32_t *__restrict__ info, int64_t lines, int32_t *__restrict__ local,
                                               int64_t *__restrict__ blocksum, int64_t *__restrict__ data_lines) {
    __shared__ int sc[PG_COUNT_ROWS];
    const int tid = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * PG_COUNT_ROWS + tid;
    const int v = i < lines ? info[i] : 0;
    const int c = v & PG_LINE_KEEP;
    sc[tid] = c | ((v & PG_LINE_DATA) ? 1 << 16 : 0);
    block_scan<PG_COUNT_ROWS>(sc, tid);
    if (i < lines) local[i] = (sc[tid] & 0xffff) - c;
    if (tid == PG_COUNT_ROWS - 1) {
        blocksum[blockIdx.x] = sc[PG_COUNT_ROWS - 1] & 0xffff;
        const int d = sc[PG_COUNT_ROWS - 1] >> 16;
        if (data_lines && d) atomicAdd(reinterpret_cast<unsigned long long *>(data_lines), (unsigned long long)d);
    }
    return v;
}

__global__ __launch_bounds__(PG_COUNT_ROWS) void k_scan_keep(const int32_t *__restrict__ info, int64_t lines, int32_t *__restrict__ local,
                                                             int64_t *__restrict__ blocksum, int64_t *__restrict__ data_lines) {
    scan_keep_flags(info, lines, local, blocksum, data_lines);
}

// element i's place behind both levels of a scan: a kept line's rank, a row's offset
__device__ __forceinline__ int64_t scan_rank(const int32_t *__restrict__ local, const int64_t *__restrict__ blockoff, int64_t i) {
    return blockoff[i >> PG_COUNT_SHIFT] + local[i];
}
// .. or the total at the end
__device__ __forceinline__ int64_t scan_off(const int32_t *__restrict__ local, const int64_t *__restrict__ blockoff, const PgScanCtl *ctl, int64_t i,
                                            int64_t count) {
    return i < count ? scan_rank(local, blockoff, i) : ctl->total;
}

// ---- lane groups ---------------------------------------------------------------------------------------------------------
// lanes per line or row: the smallest power of two that holds n, from 2^min_shift lanes to a wave
inline int pg_lpr_shift(int n, int min_shift) {
    int s = min_shift;
    while (s < 6 && (1 << s) < n) ++s;
    return s;
}

struct PgLaneGroup {
    int lpr;        // lanes of a group
    int g, gl;      // the thread's group in its workgroup, its lane in the group
    int gbase;      // the group's first lane in its wave
    uint64_t gmask; // lpr ones
};

__device__ __forceinline__ PgLaneGroup lane_group(int tid, int shift) {
    PgLaneGroup G;
    G.lpr = 1 << shift;
    G.g = tid >> shift;
    G.gl = tid & (G.lpr - 1);
    G.gbase = (tid & 63) & ~(G.lpr - 1);
    G.gmask = G.lpr == 64 ? ~0ULL : ((1ULL << G.lpr) - 1ULL);
    return G;
}

// The field starts of the line L[0 .. wlen) by the lanes of a group: fs[f] = where field f begins, for 1 <= f < F; returns the
// line's tabs.  The group walks the line in chunks of one byte per lane; a ballot on '\t' and a popcount of the lower lanes give
// a byte's field index.  Every lane of the group calls with the same wlen (0 for a group without a line: nothing is read or
// written); there is no barrier inside, the caller's follows.
__device__ __forceinline__ int group_split_tabs(const unsigned char *L, int wlen, const PgLaneGroup &G, int *fs, int F) {
    int ntabs = 0;
    for (int off = 0; off < wlen; off += G.lpr) { // (one trip count for the group; other groups of the wave may leave earlier)
        const int idx = off + G.gl;
        const bool tab = idx < wlen && L[idx] == '\t';
        const uint64_t gb = ((uint64_t)__ballot(tab) >> G.gbase) & G.gmask;
        if (tab) {
            const int f = ntabs + __popcll(gb & ((1ULL << G.gl) - 1ULL)) + 1;
            if (f < F) fs[f] = idx + 1;
        }
        ntabs += __popcll(gb);
    }
    return ntabs;
}

// line `line` of the index: *s = its first byte, *len = its length without the newline and without a '\r' in front of it.  A last
// line without a newline ends at `bytes`; its '\r' goes only with strip_cr_without_newline (the formats differ: their host
// parsers do).
__device__ __forceinline__ void line_bounds(const PgText &T, const int64_t *__restrict__ start, int64_t line, bool strip_cr_without_newline,
                                            int64_t *s, int64_t *len) {
    *s = start[line];
    const int64_t e = start[line + 1] - 1; // the newline's place, or `bytes` for a last line without one
    *len = e - *s;
    if ((strip_cr_without_newline || e < T.bytes) && *len > 0 && T.text[e - 1] == '\r') --*len;
}

// ---- tile flush ----------------------------------------------------------------------------------------------------------
// tile[head + i] is byte i of out[0 .. nbytes), and out + i is 16-byte aligned where head + i is: whole words by 16-byte stores
// (a lane a word, consecutive lanes consecutive words), the ragged head and tail by byte stores.  Two workgroups meet inside a
// word only with byte stores.  Behind the barrier that ends the writes to the tile; nthreads >= 16.
__device__ __forceinline__ void tile_flush(const unsigned char *tile, int head, unsigned char *out, int nbytes, int tid, int nthreads) {
    const int h = min(nbytes, (16 - head) & 15);                      // bytes in front of the first whole word
    const int body = (nbytes - h) & ~15;                              // whole 16-byte words
    if (tid < h) out[tid] = tile[head + tid];
    for (int i = tid * 16; i < body; i += nthreads * 16)              // head + h is 0 or 16 whenever body > 0
        *reinterpret_cast<uint4 *>(out + h + i) = *reinterpret_cast<const uint4 *>(tile + head + h + i);
    const int tail = nbytes - h - body;                               // < 16
    if (tid < tail) out[h + body + tid] = tile[head + h + body + tid];
}

// ---- host side -----------------------------------------------------------------------------------------------------------
// The parsers' line index in the context's workspace, which is laid out in two phases because the line tables can be sized only
// when the lines are counted: [the caller's front block][blocksum, blockoff of the index] first, behind them
// [start: lines + 2][info][local][blocksum, blockoff of the keep scan].  The caller's front block begins with its control struct
// Ctl, whose first member is `PgLineCounts n`.  front(ws, count_lines) uploads the front block to ws and calls
// count_lines(hook) once, in stream order between what the hook needs in front of it and what reads the hook's results; it
// returns a hipError_t.  It is called again when the second reservation replaced the workspace (wherever the new block lies):
// the same numbers come out.  Device time goes to `kid`; the caller's own brackets continue it with PG_PROF_CONT.
struct PgLineIndex {
    int64_t lines = 0, nbk = 0; // lines of the text, workgroups of the keep scan
    char *ws = nullptr;         // the workspace behind both reservations: the front block
    int64_t *start = nullptr, *bsk = nullptr, *bok = nullptr;
    int32_t *info = nullptr, *local = nullptr;

    template <class Ctl, class Front>
    int build(pg_ctx *ctx, int kid, const char *who, const PgText &T, size_t front_bytes, Front front, Ctl *res) {
        static_assert(offsetof(Ctl, n) == 0, "the control struct begins with its PgLineCounts");
        const int64_t nbi = (T.nchunks + PG_INDEX_THREADS - 1) / PG_INDEX_THREADS;
        PG_CHECK(ctx, nbi < ((int64_t)1 << 31), "%s: a slab of %lld bytes; cut the text into smaller slabs", who, (long long)T.bytes);
        size_t off = pg_up16(front_bytes);
        const size_t o_bsi = off; off = pg_up16(off + 8 * (size_t)nbi);
        const size_t o_boi = off; off = pg_up16(off + 8 * (size_t)nbi);
        int rc = pg_ws_reserve(ctx, off);
        if (rc) return rc;
        auto front_part = [&]() -> hipError_t {
            char *w = static_cast<char *>(ctx->ws.get());
            PgLineCounts *n = reinterpret_cast<PgLineCounts *>(w);
            return front(w, [&](auto hook) { // the newlines of every 4 KB and their scan
                hipLaunchKernelGGL((k_text_index<false, decltype(hook)>), dim3((unsigned)nbi), dim3(PG_INDEX_THREADS), 0, ctx->stream, T,
                                   reinterpret_cast<int64_t *>(w + o_bsi), (const int64_t *)nullptr, (const PgLineCounts *)nullptr, (int64_t *)nullptr,
                                   hook);
                hipLaunchKernelGGL(k_scan_blocks, dim3(1), dim3(PG_SCAN_WIDTH), 0, ctx->stream, reinterpret_cast<const int64_t *>(w + o_bsi), nbi,
                                   reinterpret_cast<int64_t *>(w + o_boi), &n->newlines, T.text, T.bytes, &n->lines);
            });
        };
        pg_prof_begin(ctx, kid);
        PG_HIP(ctx, front_part());
        pg_prof_end(ctx);
        PG_HIP(ctx, hipMemcpyAsync(res, ctx->ws.get(), sizeof(Ctl), hipMemcpyDeviceToHost, ctx->stream));
        PG_HIP(ctx, hipStreamSynchronize(ctx->stream)); // (the host copies that front() uploaded have been read by now)
        const int64_t counted = res->n.lines;
        PG_CHECK(ctx, counted >= 1 && counted <= T.bytes && res->n.newlines <= counted, "%s: internal error, %lld lines in %lld bytes", who,
                 (long long)counted, (long long)T.bytes);
        lines = counted; // (known from here on, whatever fails below)
        nbk = (lines + PG_COUNT_ROWS - 1) / PG_COUNT_ROWS;
        const size_t o_start = off; off = pg_up16(off + 8 * (size_t)(lines + 2));
        const size_t o_info = off; off = pg_up16(off + 4 * (size_t)lines);
        const size_t o_local = off; off = pg_up16(off + 4 * (size_t)lines);
        const size_t o_bsk = off; off = pg_up16(off + 8 * (size_t)nbk);
        const size_t o_bok = off; off = pg_up16(off + 8 * (size_t)nbk);
        const size_t before = ctx->ws.bytes();
        rc = pg_ws_reserve(ctx, off);
        if (rc) return rc;
        pg_prof_begin(ctx, kid | PG_PROF_CONT);
        hipError_t e = ctx->ws.bytes() != before ? front_part() : hipSuccess; // the workspace was replaced by a larger block: its front part again
        ws = static_cast<char *>(ctx->ws.get());
        start = reinterpret_cast<int64_t *>(ws + o_start);
        info = reinterpret_cast<int32_t *>(ws + o_info);
        local = reinterpret_cast<int32_t *>(ws + o_local);
        bsk = reinterpret_cast<int64_t *>(ws + o_bsk);
        bok = reinterpret_cast<int64_t *>(ws + o_bok);
        if (e == hipSuccess) {
            hipLaunchKernelGGL((k_text_index<true, PgNoHook>), dim3((unsigned)nbi), dim3(PG_INDEX_THREADS), 0, ctx->stream, T, (int64_t *)nullptr,
                               reinterpret_cast<const int64_t *>(ws + o_boi), reinterpret_cast<const PgLineCounts *>(ws), start, PgNoHook());
            e = hipGetLastError();
        }
        pg_prof_end(ctx);
        PG_HIP(ctx, e);
        return PG_OK;
    }

    // workgroups of a parse kernel that takes lines_per_block lines each
    int parse_blocks(pg_ctx *ctx, const char *who, int lines_per_block, int64_t *nbp) const {
        *nbp = (lines + lines_per_block - 1) / lines_per_block;
        PG_CHECK(ctx, *nbp < ((int64_t)1 << 31), "%s: %lld lines in one slab; cut the text into smaller slabs", who, (long long)lines);
        return PG_OK;
    }

    // the ranks of the kept lines: local and bok for scan_rank, the number of kept lines to *kept
    void scan_kept(pg_ctx *ctx, int64_t *kept) const { pg_scan_blocks(ctx, bsk, nbk, bok, kept); }
};

// The writers' offsets in the context's workspace: [local: count x i32][blocksum][blockoff][ctl].  prepare() lays them out and
// clears ctl; the caller's measure kernel writes the lengths to local and its flags to ctl->bad; scan() turns the lengths into
// offsets (scan_off) in the caller's profile bracket; read() brings ctl to the host.
struct PgLengthScan {
    int64_t count = 0, nb = 0;
    int32_t *local = nullptr;
    int64_t *bsum = nullptr, *boff = nullptr;
    PgScanCtl *ctl = nullptr;

    int prepare(pg_ctx *ctx, int64_t n) {
        count = n;
        nb = (n + PG_COUNT_ROWS - 1) / PG_COUNT_ROWS;
        size_t off = 0;
        const size_t o_local = off; off = pg_up16(off + sizeof(int32_t) * (size_t)n);
        const size_t o_bsum = off; off = pg_up16(off + 8 * (size_t)nb);
        const size_t o_boff = off; off = pg_up16(off + 8 * (size_t)nb);
        const size_t o_ctl = off; off = pg_up16(off + sizeof(PgScanCtl));
        const int rc = pg_ws_reserve(ctx, off);
        if (rc) return rc;
        char *ws = static_cast<char *>(ctx->ws.get());
        local = reinterpret_cast<int32_t *>(ws + o_local);
        bsum = reinterpret_cast<int64_t *>(ws + o_bsum);
        boff = reinterpret_cast<int64_t *>(ws + o_boff);
        ctl = reinterpret_cast<PgScanCtl *>(ws + o_ctl);
        PG_HIP(ctx, hipMemsetAsync(ctl, 0, sizeof(PgScanCtl), ctx->stream));
        return PG_OK;
    }
    void scan(pg_ctx *ctx) const {
        hipLaunchKernelGGL(k_scan_lengths, dim3((unsigned)nb), dim3(PG_COUNT_ROWS), 0, ctx->stream, local, count, bsum, ctl);
        pg_scan_blocks(ctx, bsum, nb, boff, &ctl->total);
    }
    int read(pg_ctx *ctx, PgScanCtl *res) const {
        PG_HIP(ctx, hipGetLastError());
        PG_HIP(ctx, hipMemcpyAsync(res, ctl, sizeof(PgScanCtl), hipMemcpyDeviceToHost, ctx->stream));
        PG_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return PG_OK;
    }
};

} // namespace
