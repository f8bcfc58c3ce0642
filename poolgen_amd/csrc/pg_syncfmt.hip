// pg_syncfmt.hip -- the sync writer of pileup2sync and vcf2sync: the rows a text parser left on the device (pg_vcf_parse_dev,
// pg_pileup_parse_dev, pg_sync_parse_dev) as the bytes of their sync lines (append_sync_line, host/pileup.h; pileup.rs:348-371,
// vcf.rs:212-229), formatted on the device.
//
// One line per row: the chromosome's name (a piece of the slab the row was parsed from), '\t', the position, '\t', the reference
// byte, per pool '\t' and its six counts joined by ':', '\n' (pg_sync_fmt.h).  The structure is pg_csv.hip's, three steps on the
// context's stream:
//   measure  k_syncfmt_measure: the byte length of every row (int32), a flag for a name outside the slab and for a row that is
//            too long;
//   scan     PgLengthScan (pg_text_steps.h): k_scan_lengths (exclusive scan of PG_COUNT_ROWS = 256 lengths per workgroup, the longest
//            row) + k_scan_blocks (64-bit exclusive scan of the workgroups' sums, PG_SCAN_WIDTH = 1024 per round): a row's offset is
//            scan_off(r);
//   emit     k_syncfmt_emit<SF_STAGED>: a workgroup takes `rpb` consecutive rows -- one contiguous byte range of the output --
//            formats them into an LDS tile laid out like the 16-byte words of the output, then copies the tile out (tile_flush): whole
//            words by 16-byte stores (a lane a word, consecutive lanes consecutive words), the ragged head and tail by byte stores.  Two
//            workgroups meet inside a word only with byte stores; nothing is read back; nothing at or past the total is written.
//            k_syncfmt_emit<SF_DIRECT>: a row longer than the tile goes to the output by byte stores, a wave per row.
// A row is formatted by a GROUP of lpr lanes (1 .. 64, a power of two: the smallest that holds n_pools): lane j of the group takes
// pools j, j + lpr, ..; a pool's place in the row is the group's running sum of the pools' text lengths, an inclusive scan by lane
// shuffles.  A pool's six counts stay in registers and every digit goes straight to its byte: no array, no scratch.
#include "pg_common.h"
#include "pg_text_steps.h"
#include "pg_sync_fmt.h"

namespace {

constexpr int SF_THREADS = 256;
constexpr int SF_TILE = 16384; // bytes of text a workgroup stages (plus up to 15 in front of them: the word it starts in)
constexpr int SF_BAD_NAME = 1, SF_BAD_LONG = 2;
// The two widths of the shared scan (pg_text_steps.h) under this file's names: tests/test_gpu_syncfmt.py reads them from this
// source to place its row counts on both sides of a scan level.  They cannot drift from what the kernels are built with.
constexpr int SF_COUNT_ROWS = 256, SF_SCAN_WIDTH = 1024;
static_assert(SF_COUNT_ROWS == PG_COUNT_ROWS && SF_SCAN_WIDTH == PG_SCAN_WIDTH, "the scan widths of pg_text_steps.h");

struct SfRows { // what a row is made of
    const unsigned char *slab;
    int64_t slab_bytes;
    const uint32_t *counts;
    const uint64_t *pos;
    const uint8_t *ref;
    const int64_t *line_off;
    const int32_t *chrom_len;
    int n;
};

__device__ __forceinline__ void sf_load_pool(const uint32_t *__restrict__ p, uint32_t (&c)[6]) {
#pragma unroll
    for (int i = 0; i < 6; ++i) c[i] = p[i];
}

// ---- measure -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SF_THREADS) void k_syncfmt_measure(const SfRows R, int64_t rows, int lpr_shift, int32_t *__restrict__ rowlen,
                                                                PgScanCtl *__restrict__ ctl) {
    const int lpr = 1 << lpr_shift;
    const int64_t gid = (int64_t)blockIdx.x * SF_THREADS + threadIdx.x;
    const int64_t r = gid >> lpr_shift;
    const int gl = (int)(gid & (lpr - 1));
    const bool have_row = r < rows; // uniform over the group
    int pools = 0;                  // at most 66 n < PG_SYNCFMT_MAX_ROW
    if (have_row) {
        const uint32_t *row = R.counts + r * R.n * 6;
        for (int j = gl; j < R.n; j += lpr) {
            uint32_t c[6];
            sf_load_pool(row + j * 6, c);
            pools += pg_syncfmt_pool_len(c);
        }
    }
    for (int d = 1; d < lpr; d <<= 1) pools += __shfl_xor(pools, d, 64); // (lanes without a row carry 0; groups are aligned blocks of lanes)
    if (have_row && gl == 0) {
        int bad = 0;
        const int32_t clen = R.chrom_len[r];
        int64_t len = 0;
        if (!pg_syncfmt_name_ok(R.line_off[r], clen, R.slab_bytes)) bad = SF_BAD_NAME;
        else {
            len = pg_syncfmt_row_len(clen, R.pos[r], pools);
            if (len > PG_SYNCFMT_MAX_ROW) { bad = SF_BAD_LONG; len = 0; }
        }
        rowlen[r] = (int32_t)len;
        if (bad) atomicOr(&ctl->bad, bad);
    }
}

// ---- emit --------------------------------------------------------------------------------------------------------------
// One row by the lpr lanes of a group (all of them call, `active` or not: the shuffles need the whole group); dst = the row's
// first byte, in LDS or in the output.  Only rows the measure step has passed come here: the name lies inside the slab.
__device__ __forceinline__ void sf_format_row(const SfRows &R, int64_t r, bool active, int gl, int lpr, unsigned char *dst) {
    int o = 0;
    const uint32_t *row = R.counts;
    if (active) {
        row = R.counts + r * R.n * 6;
        const int clen = R.chrom_len[r];
        const unsigned char *name = R.slab + R.line_off[r];
        for (int i = gl; i < clen; i += lpr) dst[i] = name[i];
        const uint64_t pos = R.pos[r];
        if (gl == 0) pg_syncfmt_put_pos_ref(dst + clen, pos, R.ref[r]);
        o = (int)pg_syncfmt_prefix_len(clen, pos);
    }
    for (int j0 = 0; j0 < R.n; j0 += lpr) { // uniform trip count
        const int j = j0 + gl;
        const bool have = active && j < R.n;
        uint32_t c[6] = {0, 0, 0, 0, 0, 0};
        if (have) sf_load_pool(row + j * 6, c);
        const int len = have ? pg_syncfmt_pool_len(c) : 0;
        int s = len; // inclusive scan over the group
        for (int d = 1; d < lpr; d <<= 1) {
            const int v = __shfl_up(s, d, lpr);
            if (gl >= d) s += v;
        }
        if (have) {
            pg_syncfmt_put_pool(dst + o + s - len, c);
            if (j == R.n - 1) dst[o + s] = '\n';
        }
        o += __shfl(s, lpr - 1, lpr);
    }
}

enum { SF_STAGED = 0, SF_DIRECT = 1 }; // how k_syncfmt_emit takes its rows (the dispatch rule: pg_sync_format_rows_dev)

template <int MODE>
__global__ __launch_bounds__(SF_THREADS) void k_syncfmt_emit(const SfRows R, int64_t rows, int lpr_shift, int rpb,
                                                             const int32_t *__restrict__ local, const int64_t *__restrict__ blockoff,
                                                             const PgScanCtl *__restrict__ ctl, unsigned char *__restrict__ text) {
    const int tid = threadIdx.x;
    if (MODE == SF_DIRECT) { // a wave per row, straight to the output
        const int64_t r = (int64_t)blockIdx.x * (SF_THREADS / 64) + (tid >> 6);
        const bool active = r < rows;
        sf_format_row(R, r, active, tid & 63, 64, text + (active ? scan_off(local, blockoff, ctl, r, rows) : 0));
        return;
    }
    __shared__ __attribute__((aligned(16))) unsigned char tile[SF_TILE + 16];
    const int lpr = 1 << lpr_shift, ng = SF_THREADS >> lpr_shift;
    const int g = tid >> lpr_shift, gl = tid & (lpr - 1);
    const int64_t r_lo = (int64_t)blockIdx.x * rpb, r_hi = r_lo + rpb < rows ? r_lo + rpb : rows;
    const int64_t B = scan_off(local, blockoff, ctl, r_lo, rows), E = scan_off(local, blockoff, ctl, r_hi, rows);
    const int head = (int)((reinterpret_cast<uintptr_t>(text) + (uint64_t)B) & 15); // tile[head + i] is byte B + i of the output
    for (int64_t r0 = r_lo; r0 < r_hi; r0 += ng) {                                  // uniform trip count
        const int64_t r = r0 + g;
        const bool active = r < r_hi;
        const int at = active ? (int)(scan_off(local, blockoff, ctl, r, rows) - B) : 0;
        sf_format_row(R, r, active, gl, lpr, tile + head + at);
    }
    __syncthreads();
    const int nbytes = (int)(E - B);                                  // <= SF_TILE: rpb rows of at most the longest row's length
    tile_flush(tile, head, text + B, nbytes, tid, SF_THREADS);
}

} // namespace

extern "C" int pg_sync_format_rows_dev(pg_ctx *ctx, const char *slab_dev, int64_t slab_bytes, const uint32_t *counts_dev,
                                       const uint64_t *pos_dev, const uint8_t *ref_dev, const int64_t *line_off_dev,
                                       const int32_t *chrom_len_dev, int n_pools, int64_t rows, char *text_dev, int64_t cap,
                                       int64_t *bytes) {
    if (!ctx) return PG_ERR_INVALID;
    PG_CHECK(ctx, bytes != nullptr, "sync_format_rows: null pointer");
    *bytes = 0;
    PG_CHECK(ctx, n_pools >= 1 && n_pools <= PG_SYNCFMT_MAX_POOLS, "sync_format_rows: %d pools (1 to %d are formatted)", n_pools,
             PG_SYNCFMT_MAX_POOLS);
    PG_CHECK(ctx, slab_bytes >= 0 && rows >= 0 && rows <= ((int64_t)1 << 31) && cap >= 0,
             "sync_format_rows: bad shape slab_bytes=%lld rows=%lld cap=%lld", (long long)slab_bytes, (long long)rows, (long long)cap);
    PG_CHECK(ctx, cap == 0 || text_dev, "sync_format_rows: null text buffer");
    if (rows == 0) return PG_OK;
    PG_CHECK(ctx, (slab_dev || slab_bytes == 0) && counts_dev && pos_dev && ref_dev && line_off_dev && chrom_len_dev,
             "sync_format_rows: null pointer");
    PG_HIP(ctx, hipSetDevice(ctx->device));
    PgLengthScan S;
    int rc = S.prepare(ctx, rows);
    if (rc) return rc;
    const SfRows R{reinterpret_cast<const unsigned char *>(slab_dev), slab_bytes, counts_dev, pos_dev, ref_dev, line_off_dev, chrom_len_dev, n_pools};
    const int lpr_shift = pg_lpr_shift(n_pools, 0);
    const int64_t measure_blocks = ((rows << lpr_shift) + SF_THREADS - 1) / SF_THREADS;
    pg_prof_begin(ctx, PG_K_SYNCFMT);
    hipLaunchKernelGGL(k_syncfmt_measure, dim3((unsigned)measure_blocks), dim3(SF_THREADS), 0, ctx->stream, R, rows, lpr_shift, S.local, S.ctl);
    S.scan(ctx);
    pg_prof_end(ctx);
    PgScanCtl res{};
    rc = S.read(ctx, &res);
    if (rc) return rc;
    PG_CHECK(ctx, !(res.bad & SF_BAD_NAME), "sync_format_rows: a row's chromosome name (line_off, chrom_len) lies outside the slab");
    PG_CHECK(ctx, !(res.bad & SF_BAD_LONG), "sync_format_rows: a line of text is longer than %d bytes", PG_SYNCFMT_MAX_ROW);
    *bytes = res.total;
    PG_CHECK(ctx, res.total <= cap, "sync_format_rows: the text needs %lld bytes, the buffer holds %lld", (long long)res.total, (long long)cap);
    unsigned char *text = reinterpret_cast<unsigned char *>(text_dev);
    pg_prof_begin(ctx, PG_K_SYNCFMT | PG_PROF_CONT);
    if (res.max > SF_TILE) { // the direct path: a row does not fit the tile
        const int64_t blocks = (rows + SF_THREADS / 64 - 1) / (SF_THREADS / 64);
        hipLaunchKernelGGL(k_syncfmt_emit<SF_DIRECT>, dim3((unsigned)blocks), dim3(SF_THREADS), 0, ctx->stream, R, rows, 6, 0, S.local, S.boff, S.ctl, text);
    } else {
        const int rpb = SF_TILE / std::max(1, res.max); // rows per workgroup: rpb rows of at most the longest row's length fit the tile
        const int64_t blocks = (rows + rpb - 1) / rpb;
        hipLaunchKernelGGL(k_syncfmt_emit<SF_STAGED>, dim3((unsigned)blocks), dim3(SF_THREADS), 0, ctx->stream, R, rows, lpr_shift, rpb, S.local, S.boff, S.ctl, text);
    }
    pg_prof_end(ctx);
    PG_HIP(ctx, hipGetLastError());
    return PG_OK;
}
