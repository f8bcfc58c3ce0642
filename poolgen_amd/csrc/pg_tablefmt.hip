// pg_tablefmt.hip -- the popgen writer's table: rows of a strided fp64 table as CSV text, formatted on the device, one lane per
// CELL (pg_table_cells.h).  The row formatters (pg_resultfmt.hip) take a lane per row and refuse a row above 2^22 bytes; a
// window row of fst has n^2 cells (0.9 MB at 200 pools, 5.5 MB at 500) and there are only some 1 500 of them, so here the unit
// of work and of the scan is the element: one cell with the byte behind it, in column 0 with the row's label in front of it.
// Three steps on the context's stream, none of which reads the text back:
//   measure  k_tf_measure: the byte length of every element (int32), a flag for a bad label;
//   scan     PgLengthScan (pg_text_steps.h): k_scan_lengths over TF_CELLS = PG_COUNT_ROWS = 256 elements per workgroup,
//            k_scan_blocks (64-bit) over the workgroups' sums;
//   emit     k_tf_emit: a workgroup takes the 256 elements of one workgroup of the scan, so its byte range is
//            [blockoff[b], blockoff[b + 1]) and an element's place in it is its stored local offset.  A lane converts its cell
//            again (the conversion lives in registers; storing digits, exponent and count per cell in the measure pass would
//            be 24 bytes of traffic each way against a few hundred integer instructions) and writes it into an LDS tile laid
//            out like the 16-byte words of the output; tile_flush copies the tile out.  256 cells of ordinary length are
//            some 5 KB, one pass.  Where the range is longer than the tile (long cells, long labels) the workgroup walks it in
//            passes of whole elements, as many as fit; an element that alone exceeds the tile (a label above 16 KB) goes through
//            the tile in pieces, all lanes copying.  Passes meet like workgroups do: inside a word only with byte stores.
// There is no limit on a row; a label is at most PG_TABLE_LABEL_MAX bytes; the total is 64-bit.
#include "pg_common.h"
#include "pg_text_steps.h"
#include "pg_table_cells.h"
#include <algorithm>

namespace {

constexpr int TF_CELLS = PG_COUNT_ROWS; // elements, and lanes, per workgroup: a workgroup of the scan
constexpr int TF_TILE = 16384;          // bytes of text a pass stages (plus up to 15 in front of them: the word it starts in)
constexpr int TF_BAD_LABEL = 1;
static_assert(PG_F64_TEXT_MAX_LEN + 1 <= TF_TILE, "an element without its label fits the tile");
static_assert((int64_t)TF_CELLS * (PG_TABLE_LABEL_MAX + PG_F64_TEXT_MAX_LEN + 1) < ((int64_t)1 << 31), "a workgroup's lengths sum in an int32");

// element e of the call -> its row of the table and its column
__device__ __forceinline__ void tf_place(int64_t e, int64_t cols, int64_t row0, int64_t *r, int64_t *c) {
    const int64_t q = e / cols;
    *r = row0 + q;
    *c = e - q * cols;
}

__global__ __launch_bounds__(TF_CELLS) void k_tf_measure(const PgTable T, int64_t row0, int64_t count, int32_t *__restrict__ len,
                                                         PgScanCtl *__restrict__ ctl) {
    const int64_t e = (int64_t)blockIdx.x * TF_CELLS + threadIdx.x;
    if (e >= count) return;
    int64_t r, c;
    tf_place(e, T.cols, row0, &r, &c);
    int64_t n = 0;
    if (c == 0) {
        n = T.label_len(r);
        if (n < 0) {
            atomicOr(&ctl->bad, TF_BAD_LABEL);
            len[e] = 0;
            return;
        }
    }
    len[e] = (int32_t)(n + pg_f64_len(T.cell(r, c)) + 1);
}

__global__ __launch_bounds__(TF_CELLS) void k_tf_emit(const PgTable T, int64_t row0, int64_t count, const int32_t *__restrict__ local,
                                                      const int64_t *__restrict__ blockoff, const PgScanCtl *__restrict__ ctl,
                                                      unsigned char *__restrict__ text) {
    __shared__ __attribute__((aligned(16))) unsigned char tile[TF_TILE + 16];
    __shared__ int loc[TF_CELLS + 1]; // the elements' offsets in the workgroup's range, and its length behind them
    const int tid = threadIdx.x;
    const int64_t e0 = (int64_t)blockIdx.x * TF_CELLS, e = e0 + tid;
    const int nc = (int)(count - e0 < TF_CELLS ? count - e0 : TF_CELLS);
    const int64_t B = blockoff[blockIdx.x];
    const int64_t E = e0 + TF_CELLS < count ? blockoff[blockIdx.x + 1] : ctl->total;
    if (tid < nc) loc[tid] = local[e];
    if (tid == 0) loc[nc] = (int)(E - B);
    int64_t r = 0, c = 0;
    pg_f64_parts_t parts = pg_f64_parts(0.0);
    int lab = 0; // the bytes of the label in front of this lane's cell
    if (tid < nc) {
        tf_place(e, T.cols, row0, &r, &c);
        parts = T.cell(r, c);
        if (c == 0) lab = (int)T.label_len(r);
    }
    __syncthreads();
    for (int c0 = 0; c0 < nc;) { // (c0, and with it the whole loop, is the same in every lane)
        int c1 = c0, hi = nc; // the most whole elements that fit the tile: the last c1 with loc[c1] - loc[c0] <= TF_TILE
        while (c1 < hi) {
            const int mid = (c1 + hi + 1) >> 1;
            if (loc[mid] - loc[c0] <= TF_TILE) c1 = mid;
            else hi = mid - 1;
        }
        unsigned char *out = text + B + loc[c0];
        if (c1 > c0) {
            const int head = (int)(reinterpret_cast<uintptr_t>(out) & 15); // tile[head + i] is byte i behind `out`
            if (tid >= c0 && tid < c1) {
                PgPutSink s{tile + head + (loc[tid] - loc[c0])};
                if (lab > 0) s.bytes(T.label + T.label_off[r], lab);
                T.write_cell(parts, c, s);
            }
            __syncthreads();
            tile_flush(tile, head, out, loc[c1] - loc[c0], tid, TF_CELLS);
            __syncthreads();
            c0 = c1;
            continue;
        }
        // element c0 alone is longer than the tile: its label in pieces of a tile by all lanes, then its cell
        const int64_t row = row0 + (e0 + c0) / T.cols; // (column 0: nothing but a label is that long)
        const unsigned char *src = T.label + T.label_off[row];
        const int total = loc[c0 + 1] - loc[c0];
        const int label_bytes = (int)(T.label_off[row + 1] - T.label_off[row]);
        for (int k = 0; k < label_bytes; k += TF_TILE) {
            const int nb = label_bytes - k < TF_TILE ? label_bytes - k : TF_TILE;
            const int head = (int)(reinterpret_cast<uintptr_t>(out + k) & 15);
            for (int i = tid; i < nb; i += TF_CELLS) tile[head + i] = src[k + i];
            __syncthreads();
            tile_flush(tile, head, out + k, nb, tid, TF_CELLS);
            __syncthreads();
        }
        const int head = (int)(reinterpret_cast<uintptr_t>(out + label_bytes) & 15);
        if (tid == c0) {
            PgPutSink s{tile + head};
            T.write_cell(parts, c, s);
        }
        __syncthreads();
        tile_flush(tile, head, out + label_bytes, total - label_bytes, tid, TF_CELLS);
        __syncthreads();
        c0 += 1;
    }
}

} // namespace

extern "C" int pg_f64_table_dev(pg_ctx *ctx, const double *x_dev, int64_t rows, int64_t cols, int64_t row_stride, int64_t col_stride, int64_t row0,
                                int64_t n_rows, int n_digits, int first_col_digits, const char *label_text_dev, const int64_t *label_off_dev,
                                char *text_dev, int64_t cap, int64_t *bytes) {
    if (!ctx) return PG_ERR_INVALID;
    PG_CHECK(ctx, bytes != nullptr, "f64_table: null pointer");
    *bytes = 0;
    PG_CHECK(ctx, rows >= 0 && cols >= 1 && row_stride >= 0 && col_stride >= 0 && cap >= 0, "f64_table: bad shape rows=%lld cols=%lld strides=%lld,%lld cap=%lld",
             (long long)rows, (long long)cols, (long long)row_stride, (long long)col_stride, (long long)cap);
    PG_CHECK(ctx, row0 >= 0 && n_rows >= 0 && row0 <= rows && n_rows <= rows - row0, "f64_table: rows [%lld, %lld) of %lld", (long long)row0,
             (long long)(row0 + n_rows), (long long)rows);
    PG_CHECK(ctx, n_digits <= PG_F64_MAX_ROUND_DIGITS && first_col_digits <= PG_F64_MAX_ROUND_DIGITS,
             "f64_table: n_digits=%d, first_col_digits=%d (at most %d; negative prints the value as it is)", n_digits, first_col_digits,
             PG_F64_MAX_ROUND_DIGITS);
    PG_CHECK(ctx, cap == 0 || text_dev, "f64_table: null text buffer");
    PG_CHECK(ctx, n_rows <= (((int64_t)1 << 39) - 1) / cols, "f64_table: %lld x %lld cells in one call; format the table in slabs of rows", (long long)n_rows,
             (long long)cols);
    if (n_rows == 0) return PG_OK;
    PG_CHECK(ctx, x_dev != nullptr && (label_off_dev == nullptr || label_text_dev != nullptr), "f64_table: null pointer");
    PG_HIP(ctx, hipSetDevice(ctx->device));
    const PgTable T{x_dev, cols, row_stride, col_stride, n_digits < 0 ? -1 : n_digits, first_col_digits < 0 ? -1 : first_col_digits,
                    reinterpret_cast<const unsigned char *>(label_text_dev), label_off_dev};
    const int64_t count = n_rows * cols;
    PgLengthScan S;
    int rc = S.prepare(ctx, count);
    if (rc) return rc;
    pg_prof_begin(ctx, PG_K_RESULTFMT);
    hipLaunchKernelGGL(k_tf_measure, dim3((unsigned)S.nb), dim3(TF_CELLS), 0, ctx->stream, T, row0, count, S.local, S.ctl);
    S.scan(ctx);
    pg_prof_end(ctx);
    PgScanCtl res{};
    rc = S.read(ctx, &res);
    if (rc) return rc;
    PG_CHECK(ctx, !(res.bad & TF_BAD_LABEL), "f64_table: a label's offsets decrease, or the label is longer than %d bytes", PG_TABLE_LABEL_MAX);
    *bytes = res.total;
    PG_CHECK(ctx, res.total <= cap, "f64_table: the text needs %lld bytes, the buffer holds %lld", (long long)res.total, (long long)cap);
    pg_prof_begin(ctx, PG_K_RESULTFMT | PG_PROF_CONT);
    hipLaunchKernelGGL(k_tf_emit, dim3((unsigned)S.nb), dim3(TF_CELLS), 0, ctx->stream, T, row0, count, S.local, S.boff, S.ctl,
                       reinterpret_cast<unsigned char *>(text_dev));
    pg_prof_end(ctx);
    PG_HIP(ctx, hipGetLastError());
    return PG_OK;
}
