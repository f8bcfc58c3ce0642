// pg_table_cells.h -- the table of the popgen writer, shared by the device formatter (pg_tablefmt.hip) and its host twin
// (pg_hosttablefmt.cpp): what an ELEMENT of text is made of and how it is written, once, for both sides.
//
// Row r of the table is  label_r, the cells joined by ',', '\n'.  The element is the CELL, not the row (a window row of fst has
// n^2 cells and there are few rows): element (r, c) is the text of x[r * row_stride + c * col_stride] and the byte behind it --
// ',' or, in the last column, '\n' -- and the element of column 0 begins with the row's label.  The elements follow each other
// in row-major order, so the text is their concatenation.  The number cells are pg_f64_text.h's: display for nd < 0,
// roundup_own(x, nd) otherwise; column 0 has a digit count of its own (nd0).
#pragma once
#include "pg_result_rows.h"

constexpr int PG_TABLE_LABEL_MAX = 1 << 22; // bytes of one label (a longer one is refused): 256 elements still sum in an int32

struct PgTable {
    const double *x;
    int64_t cols, row_stride, col_stride;
    int nd, nd0;
    const unsigned char *label; // the labels' bytes and rows + 1 offsets into them; label_off == nullptr: no labels
    const int64_t *label_off;

    // the length of row r's label; -1 for offsets that decrease (or are negative) and for a label above the limit
    PG_F64_HD int64_t label_len(int64_t r) const {
        if (!label_off) return 0;
        const int64_t a = label_off[r], b = label_off[r + 1];
        return a < 0 || b < a || b - a > PG_TABLE_LABEL_MAX ? -1 : b - a;
    }
    PG_F64_HD pg_f64_parts_t cell(int64_t r, int64_t c) const { return pg_f64_cell(x[r * row_stride + c * col_stride], c == 0 ? nd0 : nd); }
    PG_F64_HD unsigned char behind(int64_t c) const { return c + 1 < cols ? ',' : '\n'; }
    // the element without its label
    template <class Sink>
    PG_F64_HD void write_cell(const pg_f64_parts_t &p, int64_t c, Sink &s) const {
        s.f64(p);
        s.ch(behind(c));
    }
    // the whole element; the label has been checked
    template <class Sink>
    PG_F64_HD void write(int64_t r, int64_t c, Sink &s) const {
        if (c == 0 && label_off) s.bytes(label + label_off[r], (int)(label_off[r + 1] - label_off[r]));
        write_cell(cell(r, c), c, s);
    }
};
