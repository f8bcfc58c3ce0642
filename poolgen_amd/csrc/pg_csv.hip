// pg_csv.hip -- sync2csv's writer: the rows of the loaded matrix as the bytes of the allele-frequency CSV
// (FileSyncPhen::write_csv, base/sync.rs:1182-1262), formatted on the device.
//
// One line per row of G: "chromosome,position,allele," + the n cells joined by ',' + '\n'; a cell's text is pg_csv_cell's
// (pg_csv_cell.h: parse_f64_roundup_and_own(x, 6) restricted to frequencies).  Three steps on the context's stream:
//   measure  k_csv_measure: the byte length of every row (int32), a flag for cells that are no frequency and for labels out
//            of range;
//   scan     PgLengthScan (pg_text_steps.h): k_scan_lengths (exclusive scan of 256 lengths per workgroup, the longest row) +
//            k_scan_blocks (64-bit exclusive scan of the workgroups' sums, 1024 per round): a row's offset is scan_off(r);
//   emit     k_csv_emit<CSV_STAGED>: a workgroup takes `rpb` consecutive rows -- one contiguous byte range of the file -- formats them
//            into an LDS tile laid out like the 16-byte words of the output, then copies the tile out (tile_flush): whole words by
//            16-byte stores (a lane a word, consecutive lanes consecutive words), the ragged head and tail by byte stores.  Two
//            workgroups meet inside a word only with byte stores; nothing is read back; nothing at or past the total is written.
//            With fewer rows than waves in a tile (rows above 4 KB) the whole workgroup formats row after row together.
//            k_csv_emit<CSV_DIRECT>: a row longer than the tile goes from registers to the output by byte stores, a wave per row.
// A row is formatted by a GROUP of lpr lanes (1 .. 64, a power of two: the smallest that holds n, so that n = 5 has 8 rows in a
// wave and n = 200 one row across it): lane j of the group takes cells j, j + lpr, ..; a cell's place in the row is the
// group's running sum of (length + 1), an inclusive scan by lane shuffles.  A cell's text stays in a 64-bit register and
// leaves by (predicated) byte stores at constant shifts: no array, no scratch.
#include "pg_common.h"
#include "pg_text_steps.h"
#include "pg_csv_cell.h"

namespace {

constexpr int CSV_THREADS = 256;
constexpr int CSV_TILE = 16384;       // bytes of text a workgroup stages (plus up to 15 in front of them: the word it starts in)
constexpr int CSV_MAX_ROW = 1 << 22;  // bytes: 256 rows of this length still sum in an int32
constexpr int CSV_BAD_CELL = 1, CSV_BAD_LABEL = 2, CSV_BAD_LONG = 4;

struct CsvRows { // what a row is made of (the pointers of the call, already moved to its first row)
    const double *G;
    int64_t ld;
    int n;
    const int64_t *col_locus;
    const int32_t *col_allele;
    const int32_t *locus_chrom;
    const uint64_t *locus_pos;
    const unsigned char *chrom_text;
    const int32_t *chrom_off;
    int n_chrom;
};

struct CsvPrefix {
    int name0, name_len, nd, al;
    uint64_t pos;
    bool ok;
};

__device__ __forceinline__ CsvPrefix csv_prefix(const CsvRows &R, int64_t r) {
    CsvPrefix p;
    const int64_t loc = R.col_locus[r];
    p.al = R.col_allele[r];
    const int cid = loc >= 0 ? R.locus_chrom[loc] : -1;
    p.ok = loc >= 0 && cid >= 0 && cid < R.n_chrom && p.al >= 0 && p.al < 6;
    p.pos = p.ok ? R.locus_pos[loc] : 0;
    p.name0 = p.ok ? R.chrom_off[cid] : 0;
    p.name_len = p.ok ? R.chrom_off[cid + 1] - p.name0 : 0;
    if (p.name_len < 0) { p.ok = false; p.name_len = 0; }
    p.nd = pg_csv_pos_digits(p.pos);
    return p;
}

// ---- measure -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CSV_THREADS) void k_csv_measure(const CsvRows R, int64_t rows, int lpr_shift, int32_t *__restrict__ rowlen,
                                                             PgScanCtl *__restrict__ ctl) {
    const int lpr = 1 << lpr_shift;
    const int64_t gid = (int64_t)blockIdx.x * CSV_THREADS + threadIdx.x;
    const int64_t r = gid >> lpr_shift;
    const int gl = (int)(gid & (lpr - 1));
    const bool have_row = r < rows; // uniform over the group
    int bad = 0, cells = 0; // cells: at most 9 n < CSV_MAX_ROW
    if (have_row) {
        const double *row = R.G + r * R.ld;
        for (int j = gl; j < R.n; j += lpr) {
            uint64_t text;
            cells += pg_csv_cell(row[j], &text, &bad) + 1;
        }
    }
    for (int d = 1; d < lpr; d <<= 1) cells += __shfl_xor(cells, d, 64); // (lanes without a row carry 0; groups are aligned blocks of lanes)
    if (have_row && gl == 0) {
        const CsvPrefix p = csv_prefix(R, r);
        if (!p.ok) bad |= CSV_BAD_LABEL;
        int64_t len = (int64_t)cells + p.name_len + p.nd + 4;
        if (len > CSV_MAX_ROW) { bad |= CSV_BAD_LONG; len = 0; }
        rowlen[r] = (int32_t)len;
    }
    if (bad) atomicOr(&ctl->bad, bad);
}

// ---- emit --------------------------------------------------------------------------------------------------------------
// `len` bytes of `text` (first byte lowest), then `sep`, to dst[0 .. len]
__device__ __forceinline__ void csv_store_cell(unsigned char *dst, uint64_t text, int len, unsigned char sep) {
#pragma unroll
    for (int i = 0; i < PG_CSV_CELL_MAX; ++i)
        if (i < len) dst[i] = (unsigned char)(text >> (8 * i));
    dst[len] = sep;
}

// "chromosome,position,allele," of row r by lanes gl, gl + lpr, .. of the lanes that format it; returns its length
__device__ __forceinline__ int csv_write_prefix(const CsvRows &R, int64_t r, int gl, int lpr, unsigned char *dst) {
    const CsvPrefix p = csv_prefix(R, r);
    for (int i = gl; i < p.name_len; i += lpr) dst[i] = R.chrom_text[p.name0 + i];
    if (gl == 0) {
        unsigned char *q = dst + p.name_len;
        q[0] = ',';
        uint64_t v = p.pos;
        for (int i = p.nd; i >= 1; --i) {
            const uint64_t w = v / 10;
            q[i] = (unsigned char)('0' + (int)(v - w * 10));
            v = w;
        }
        q[p.nd + 1] = ',';
        q[p.nd + 2] = pg_csv_allele(p.al);
        q[p.nd + 3] = ',';
    }
    return p.name_len + p.nd + 4;
}

// One row by the lpr lanes of a group (all of them call, `active` or not: the shuffles need the whole group); dst = the row's
// first byte, in LDS or in the output.
__device__ __forceinline__ void csv_format_row(const CsvRows &R, int64_t r, bool active, int gl, int lpr, unsigned char *dst) {
    int o = 0;
    const double *row = R.G;
    if (active) {
        row = R.G + r * R.ld;
        o = csv_write_prefix(R, r, gl, lpr, dst);
    }
    for (int j0 = 0; j0 < R.n; j0 += lpr) { // uniform trip count
        const int j = j0 + gl;
        const bool have = active && j < R.n;
        uint64_t text = 0;
        int bad = 0, len = 0;
        if (have) len = pg_csv_cell(row[j], &text, &bad);
        const int l1 = have ? len + 1 : 0;
        int s = l1; // inclusive scan over the group
        for (int d = 1; d < lpr; d <<= 1) {
            const int v = __shfl_up(s, d, lpr);
            if (gl >= d) s += v;
        }
        if (have) csv_store_cell(dst + o + s - l1, text, len, j == R.n - 1 ? '\n' : ',');
        o += __shfl(s, lpr - 1, lpr);
    }
}

// One row by the whole workgroup (every thread calls, with the same row): 256 cells per turn, the place of a cell from the
// scan inside its wave plus the sums of the waves in front of it, which cross in `wsum` (two sets of one int per wave, used in
// turn: a wave that runs ahead writes the other set, and cannot reach this set again before everyone has left this turn's barrier).
__device__ __forceinline__ void csv_format_row_wg(const CsvRows &R, int64_t r, int tid, unsigned char *dst, int (*wsum)[CSV_THREADS / 64]) {
    constexpr int NW = CSV_THREADS / 64;
    const double *row = R.G + r * R.ld;
    int o = csv_write_prefix(R, r, tid, CSV_THREADS, dst);
    const int lane = tid & 63, wv = tid >> 6;
    int turn = 0;
    for (int j0 = 0; j0 < R.n; j0 += CSV_THREADS, turn ^= 1) { // uniform trip count
        const int j = j0 + tid;
        const bool have = j < R.n;
        uint64_t text = 0;
        int bad = 0, len = 0;
        if (have) len = pg_csv_cell(row[j], &text, &bad);
        const int l1 = have ? len + 1 : 0;
        int s = l1;
        for (int d = 1; d < 64; d <<= 1) {
            const int v = __shfl_up(s, d, 64);
            if (lane >= d) s += v;
        }
        if (lane == 63) wsum[turn][wv] = s;
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            const int t = wsum[turn][w];
            before += w < wv ? t : 0;
            total += t;
        }
        if (have) csv_store_cell(dst + o + before + s - l1, text, len, j == R.n - 1 ? '\n' : ',');
        o += total;
    }
}

enum { CSV_STAGED = 0, CSV_STAGED_WG = 1, CSV_DIRECT = 2 }; // how k_csv_emit takes its rows (the dispatch rules: pg_csv_freq_rows_dev)

template <int MODE>
__global__ __launch_bounds__(CSV_THREADS) void k_csv_emit(const CsvRows R, int64_t rows, int lpr_shift, int rpb,
                                                          const int32_t *__restrict__ local, const int64_t *__restrict__ blockoff,
                                                          const PgScanCtl *__restrict__ ctl, unsigned char *__restrict__ text) {
    const int tid = threadIdx.x;
    if (MODE == CSV_DIRECT) { // a wave per row, straight to the output
        const int64_t r = (int64_t)blockIdx.x * (CSV_THREADS / 64) + (tid >> 6);
        const bool active = r < rows;
        csv_format_row(R, r, active, tid & 63, 64, text + (active ? scan_off(local, blockoff, ctl, r, rows) : 0));
        return;
    }
    __shared__ __attribute__((aligned(16))) unsigned char tile[CSV_TILE + 16];
    const int lpr = 1 << lpr_shift, ng = CSV_THREADS >> lpr_shift;
    const int g = tid >> lpr_shift, gl = tid & (lpr - 1);
    const int64_t r_lo = (int64_t)blockIdx.x * rpb, r_hi = r_lo + rpb < rows ? r_lo + rpb : rows;
    const int64_t B = scan_off(local, blockoff, ctl, r_lo, rows), E = scan_off(local, blockoff, ctl, r_hi, rows);
    const int head = (int)((reinterpret_cast<uintptr_t>(text) + (uint64_t)B) & 15); // tile[head + i] is byte B + i of the output
    if (MODE == CSV_STAGED_WG) { // fewer rows than waves: the workgroup formats row after row together
        __shared__ int wsum[2][CSV_THREADS / 64];
        for (int64_t r = r_lo; r < r_hi; ++r) {
            csv_format_row_wg(R, r, tid, tile + head + (int)(scan_off(local, blockoff, ctl, r, rows) - B), wsum);
            __syncthreads(); // (the next row starts on set 0 of wsum again)
        }
    } else
    for (int64_t r0 = r_lo; r0 < r_hi; r0 += ng) {                                  // uniform trip count
        const int64_t r = r0 + g;
        const bool active = r < r_hi;
        const int at = active ? (int)(scan_off(local, blockoff, ctl, r, rows) - B) : 0;
        csv_format_row(R, r, active, gl, lpr, tile + head + at);
    }
    __syncthreads();
    const int nbytes = (int)(E - B);                                  // <= CSV_TILE: rpb rows of at most the longest row's length
    tile_flush(tile, head, text + B, nbytes, tid, CSV_THREADS);
}

} // namespace

extern "C" int pg_csv_freq_rows_dev(pg_ctx *ctx, const double *G_dev, int64_t ld, int n, int64_t row0, int64_t rows,
                                    const int64_t *col_locus_dev, const int32_t *col_allele_dev, const int32_t *locus_chrom_dev,
                                    const uint64_t *locus_pos_dev, const char *chrom_text_dev, const int32_t *chrom_off_dev, int n_chrom,
                                    char *text_dev, int64_t cap, int64_t *bytes) {
    if (!ctx) return PG_ERR_INVALID;
    PG_CHECK(ctx, bytes != nullptr, "csv_freq_rows: null pointer");
    *bytes = 0;
    PG_CHECK(ctx, n >= 1 && ld >= n && row0 >= 0 && rows >= 0 && rows <= ((int64_t)1 << 31) && cap >= 0 && n_chrom >= 1,
             "csv_freq_rows: bad shape n=%d ld=%lld row0=%lld rows=%lld cap=%lld n_chrom=%d", n, (long long)ld, (long long)row0,
             (long long)rows, (long long)cap, n_chrom);
    PG_CHECK(ctx, (int64_t)n * (PG_CSV_CELL_MAX + 1) < CSV_MAX_ROW, "csv_freq_rows: too many pools (%d) for one row of text", n);
    PG_CHECK(ctx, cap == 0 || text_dev, "csv_freq_rows: null text buffer");
    if (rows == 0) return PG_OK;
    PG_CHECK(ctx, G_dev && col_locus_dev && col_allele_dev && locus_chrom_dev && locus_pos_dev && chrom_text_dev && chrom_off_dev,
             "csv_freq_rows: null pointer");
    PG_HIP(ctx, hipSetDevice(ctx->device));
    PgLengthScan S;
    int rc = S.prepare(ctx, rows);
    if (rc) return rc;
    const CsvRows R{G_dev + row0 * ld, ld, n, col_locus_dev + row0, col_allele_dev + row0, locus_chrom_dev, locus_pos_dev,
                    reinterpret_cast<const unsigned char *>(chrom_text_dev), chrom_off_dev, n_chrom};
    const int lpr_shift = pg_lpr_shift(n, 0); // so that n = 5 has 8 rows in a wave and n = 200 one row across it
    const int64_t measure_blocks = ((rows << lpr_shift) + CSV_THREADS - 1) / CSV_THREADS;
    pg_prof_begin(ctx, PG_K_CSV);
    hipLaunchKernelGGL(k_csv_measure, dim3((unsigned)measure_blocks), dim3(CSV_THREADS), 0, ctx->stream, R, rows, lpr_shift, S.local, S.ctl);
    S.scan(ctx);
    pg_prof_end(ctx);
    PgScanCtl res{};
    rc = S.read(ctx, &res);
    if (rc) return rc;
    PG_CHECK(ctx, !(res.bad & CSV_BAD_LABEL), "csv_freq_rows: a row's locus, chromosome id or allele is out of range");
    PG_CHECK(ctx, !(res.bad & CSV_BAD_LONG), "csv_freq_rows: a row of text is longer than %d bytes", CSV_MAX_ROW);
    *bytes = res.total;
    PG_CHECK(ctx, !(res.bad & CSV_BAD_CELL), "csv_freq_rows: a cell is no allele frequency (outside [0, 1] and not NaN)");
    PG_CHECK(ctx, res.total <= cap, "csv_freq_rows: the text needs %lld bytes, the buffer holds %lld", (long long)res.total, (long long)cap);
    unsigned char *text = reinterpret_cast<unsigned char *>(text_dev);
    pg_prof_begin(ctx, PG_K_CSV | PG_PROF_CONT);
    if (res.max > CSV_TILE) { // the direct path: a row does not fit the tile
        const int64_t blocks = (rows + CSV_THREADS / 64 - 1) / (CSV_THREADS / 64);
        hipLaunchKernelGGL(k_csv_emit<CSV_DIRECT>, dim3((unsigned)blocks), dim3(CSV_THREADS), 0, ctx->stream, R, rows, 6, 0, S.local, S.boff, S.ctl, text);
    } else {
        const int rpb = CSV_TILE / std::max(1, res.max); // rows per workgroup: rpb rows of at most the longest row's length fit the tile
        const int64_t blocks = (rows + rpb - 1) / rpb;
        if (rpb < CSV_THREADS / 64) // fewer rows than waves (rows above 4 KB): a workgroup per row
            hipLaunchKernelGGL(k_csv_emit<CSV_STAGED_WG>, dim3((unsigned)blocks), dim3(CSV_THREADS), 0, ctx->stream, R, rows, 6, rpb, S.local, S.boff, S.ctl, text);
        else
            hipLaunchKernelGGL(k_csv_emit<CSV_STAGED>, dim3((unsigned)blocks), dim3(CSV_THREADS), 0, ctx->stream, R, rows, lpr_shift, rpb, S.local, S.boff, S.ctl, text);
    }
    pg_prof_end(ctx);
    PG_HIP(ctx, hipGetLastError());
    return PG_OK;
}
