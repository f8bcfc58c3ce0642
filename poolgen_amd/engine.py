"""Engine: torch-facing wrapper over one pg_ctx (one GPU, one stream).

Method names follow the reference operators they stand in for:
  ols_with_covariate   gwas::ols_with_covariate      (gwas/ols.rs:278-436)
  ols_iterate          gwas::ols_iterate             (gwas/ols.rs:201-276)
  correlation          gwas::correlation             (gwas/correlation_test.rs:73-129)
  chisq                tables::chisq                 (tables/chisq_test.rs:5-47)
  fisher               tables::fisher                (tables/fisher_exact_test.rs:32-130)
  gwalpha              gwas::gwalpha_ls / gwalpha_ml (gwas/gwalpha.rs:281-380)
  gp_ols               gp::ols                       (gp/ols.rs:8-101)
  gudmc                popgen::gudmc                 (popgen/gudmc.rs:64-462)
  freq_csv             FileSyncPhen::write_csv's rows (base/sync.rs:1182-1262)
  impute               imputation::impute_mean / impute_aLDkNN (imputation/*.rs)
All heavy arguments are torch CUDA tensors (device memory owned by torch); results are
torch CUDA tensors.  Everything is computed by libpoolgen_hip.so.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass

import numpy as np
import torch

from ._native import KERNEL_IDS, NativeError, PgFilter, PgPileupInfo, PgSyncInfo, PgVcfInfo, load_library

ALLELES = "ATCGND"  # base/sync.rs:134 reader order


@dataclass
class Filter:
    """FilterStats subset (base/structs_and_traits.rs:68-78) with the CLI defaults (main.rs:44-58)."""
    remove_ns: bool = True
    min_coverage_depth: int = 1
    min_allele_frequency: float = 0.001
    max_missingness_rate: float = 0.0

    def to_c(self) -> PgFilter:
        return PgFilter(int(self.remove_ns), 0, int(self.min_coverage_depth),
                        float(self.min_allele_frequency), float(self.max_missingness_rate))


def _sensible_round(x: float, digits: int) -> float:
    """sensible_round (base/helpers.rs): round half away from zero at `digits` decimals"""
    f = 10.0 ** digits
    return math.copysign(math.floor(abs(x) * f + 0.5), x) / f


def _host_f64(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64))


def _chrom_table(chrom_names):
    """The distinct chromosome names as one byte string plus len + 1 int32 offsets."""
    names = [c.encode() if isinstance(c, str) else bytes(c) for c in chrom_names]
    off = np.zeros(len(names) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(c) for c in names])
    text = np.frombuffer(b"".join(names) or b"\0", dtype=np.uint8).copy()
    return text, off


def freq_csv_host(G, col_locus, col_allele, chrom_ids, pos, chrom_names, n=None, row0=0, rows=None, n_threads=1, out=None):
    """Engine.freq_csv on the host (pg_host_csv_freq_rows: plain C++, no GPU): the same arguments as numpy arrays, the text
    as bytes.  The checker of the device form and the baseline it is measured against.  With `out` (a uint8 array that is large
    enough) the text is formatted into it by one call, without the size query, and the filled part of `out` is returned."""
    lib = load_library()
    G = np.asarray(G, dtype=np.float64)
    if G.ndim != 2 or not G.flags.c_contiguous:
        raise ValueError("G must be a C-contiguous p x ld array")
    p, ld = G.shape
    n = ld if n is None else int(n)
    rows = p - row0 if rows is None else int(rows)
    if not (0 <= row0 and 0 <= rows and row0 + rows <= p):
        raise ValueError("freq_csv_host: rows out of range")
    cl = np.ascontiguousarray(col_locus, dtype=np.int64); ca = np.ascontiguousarray(col_allele, dtype=np.int32)
    ch = np.ascontiguousarray(chrom_ids, dtype=np.int32); po = np.ascontiguousarray(pos, dtype=np.uint64)
    if len(cl) != p or len(ca) != p or len(ch) != len(po):
        raise ValueError("freq_csv_host: label arrays do not match")
    text, off = _chrom_table(chrom_names)
    args = [G.ctypes.data, ld, n, int(row0), rows, cl.ctypes.data, ca.ctypes.data, ch.ctypes.data, po.ctypes.data,
            text.ctypes.data, off.ctypes.data, len(off) - 1]
    need = C.c_int64()
    if out is not None:
        if out.dtype != np.uint8 or not out.flags.c_contiguous:
            raise ValueError("freq_csv_host: out must be a contiguous uint8 array")
        rc = lib.pg_host_csv_freq_rows(*args, out.ctypes.data, out.size, C.byref(need), int(n_threads))
        if rc != 0:
            raise NativeError(f"pg_host_csv_freq_rows failed ({rc}): the text needs {need.value} bytes, out holds {out.size}"
                              if need.value > out.size else f"pg_host_csv_freq_rows failed ({rc})")
        return out[:need.value]
    rc = lib.pg_host_csv_freq_rows(*args, None, 0, C.byref(need), int(n_threads))
    if rc != 0 and need.value == 0:
        raise NativeError(f"pg_host_csv_freq_rows failed ({rc}): a label is out of range")
    out = np.empty(max(need.value, 1), dtype=np.uint8)
    rc = lib.pg_host_csv_freq_rows(*args, out.ctypes.data, need.value, C.byref(need), int(n_threads))
    if rc != 0:   # the buffer has the size asked for, so:
        raise NativeError(f"pg_host_csv_freq_rows failed ({rc}): a cell is no allele frequency (outside [0, 1] and not NaN)")
    return out[:need.value].tobytes()


VCF_REASONS = {1: "empty line", 2: "data line under 20 bytes", 3: "line of 2^31 bytes or more", 4: "fewer than 9 fields", 5: "POS is no u64",
               6: "byte >= 0x80 in REF or ALT", 7: "not exactly one AD in FORMAT", 8: "number of samples", 9: "sample without an AD piece",
               10: "AD value is no u64", 11: "AD value above 2^32 - 1", 12: "no samples", 13: "fewer AD values than pool 0",
               14: "allele without an AD column"}


class VcfError(NativeError):
    """A VCF line at which the reference's vcf2sync panics (or one of the documented deviations): `offset` is the byte offset of
    the first such line of the text, `reason` a pg_vcf_reason."""

    def __init__(self, what, offset, reason):
        super().__init__(f"{what}: the line at byte {offset} of the text: {VCF_REASONS.get(reason, reason)}")
        self.offset, self.reason = int(offset), int(reason)


def _vcf_result(info, counts, pos, ref, off, clen):
    k, n = info.kept, info.n_pools
    return {"counts": counts[:k * n * 6].reshape(k, n, 6), "pos": pos[:k], "ref": ref[:k], "line_off": off[:k], "chrom_len": clen[:k],
            "data_lines": int(info.data_lines), "n_pools": int(n), "chrom_line_off": int(info.chrom_line_off)}


def vcf_parse_host(text, pool_sizes, min_coverage_depth=1, min_coverage_breadth=1.0, min_allele_frequency=0.001, n_threads=1):
    """Engine.vcf_parse on the host (pg_host_vcf_parse: plain C++, no GPU): the same dictionary, of numpy arrays."""
    lib = load_library()
    t = np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray, memoryview)) else np.ascontiguousarray(text, dtype=np.uint8)
    ps = _host_f64(pool_sizes)
    info = PgVcfInfo()
    args = [t.ctypes.data if t.size else None, t.size, ps.ctypes.data, len(ps), int(min_coverage_depth), float(min_coverage_breadth),
            float(min_allele_frequency)]
    rc = lib.pg_host_vcf_parse(*args, None, None, None, None, None, 0, 0, C.byref(info), int(n_threads))
    if info.err_reason:
        raise VcfError("pg_host_vcf_parse", info.err_line_off, info.err_reason)
    k, n = info.kept, info.n_pools
    if rc != 0 and k == 0:
        raise NativeError(f"pg_host_vcf_parse failed ({rc}): bad arguments")
    counts = np.empty(k * n * 6, dtype=np.uint32); pos = np.empty(k, dtype=np.uint64); ref = np.empty(k, dtype=np.uint8)
    off = np.empty(k, dtype=np.int64); clen = np.empty(k, dtype=np.int32)
    if k:
        rc = lib.pg_host_vcf_parse(*args, counts.ctypes.data, pos.ctypes.data, ref.ctypes.data, off.ctypes.data, clen.ctypes.data, k,
                                   counts.size, C.byref(info), int(n_threads))
        if rc != 0:
            raise NativeError(f"pg_host_vcf_parse failed ({rc})")
    return _vcf_result(info, counts, pos, ref, off, clen)


SYNC_REASONS = {1: "empty line", 2: "fewer than four tab-separated fields", 3: "a count is no valid integer, or a pool has fewer than six",
                4: "count above 2^32 - 1", 5: "number of pools", 6: "line of 2^31 bytes or more"}


class SyncError(NativeError):
    """A sync line at which the CLI's host parser throws: `offset` is the byte offset of the first such line of the text,
    `reason` a pg_sync_reason."""

    def __init__(self, what, offset, reason):
        super().__init__(f"{what}: the line at byte {offset} of the text: {SYNC_REASONS.get(reason, reason)}")
        self.offset, self.reason = int(offset), int(reason)


def _sync_result(info, counts, pos, off, clen):
    k, n = info.kept, info.n_pools
    return {"counts": counts[:k * n * 6].reshape(k, n, 6), "pos": pos[:k], "line_off": off[:k], "chrom_len": clen[:k],
            "data_lines": int(info.data_lines), "n_pools": int(n)}


def sync_parse_host(text, expect_n=0, n_threads=1):
    """Engine.sync_parse on the host (pg_host_sync_parse: plain C++, no GPU): the same dictionary, of numpy arrays."""
    lib = load_library()
    t = np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray, memoryview)) else np.ascontiguousarray(text, dtype=np.uint8)
    info = PgSyncInfo()
    args = [t.ctypes.data if t.size else None, t.size, int(expect_n)]
    rc = lib.pg_host_sync_parse(*args, None, None, None, None, 0, 0, C.byref(info), int(n_threads))
    if info.err_reason:
        raise SyncError("pg_host_sync_parse", info.err_line_off, info.err_reason)
    k, n = info.kept, info.n_pools
    if rc != 0 and k == 0:
        raise NativeError(f"pg_host_sync_parse failed ({rc}): bad arguments")
    counts = np.empty(k * n * 6, dtype=np.uint32); pos = np.empty(k, dtype=np.uint64)
    off = np.empty(k, dtype=np.int64); clen = np.empty(k, dtype=np.int32)
    if k:
        rc = lib.pg_host_sync_parse(*args, counts.ctypes.data, pos.ctypes.data, off.ctypes.data, clen.ctypes.data, k, counts.size,
                                    C.byref(info), int(n_threads))
        if rc != 0:
            raise NativeError(f"pg_host_sync_parse failed ({rc})")
    return _sync_result(info, counts, pos, off, clen)


PILEUP_REASONS = {1: "line of 2^31 bytes or more", 2: "fewer than three tab-separated fields", 3: "position is no number",
                  4: "reference allele is not one byte below 0x80", 5: "a pool's coverage is no number",
                  6: "a pool without its read or quality field", 7: "non-digit where an indel length must start",
                  8: "reads, quality bytes and coverage do not match"}


class PileupError(NativeError):
    """A pileup line at which the reference's pileup2sync panics: `offset` is the byte offset of the first such line of the
    text, `reason` a pg_pileup_reason."""

    def __init__(self, what, offset, reason):
        super().__init__(f"{what}: the line at byte {offset} of the text: {PILEUP_REASONS.get(reason, reason)}")
        self.offset, self.reason = int(offset), int(reason)


def _pileup_result(info, n, counts, pos, ref, off, clen):
    k = info.kept
    return {"counts": counts[:k * n * 6].reshape(k, n, 6), "pos": pos[:k], "ref": ref[:k], "line_off": off[:k], "chrom_len": clen[:k],
            "lines": int(info.lines), "n_pools": int(n)}


def _pileup_args(pool_sizes, remove_ns, keep_lowercase_reference, max_base_error_rate, min_coverage_depth, min_coverage_breadth,
                 min_allele_frequency):
    ps = _host_f64(pool_sizes)
    return ps, [ps.ctypes.data, len(ps), int(bool(remove_ns)), int(bool(keep_lowercase_reference)), float(max_base_error_rate),
                int(min_coverage_depth), float(min_coverage_breadth), float(min_allele_frequency)]


def pileup_parse_host(text, pool_sizes, remove_ns=True, keep_lowercase_reference=False, max_base_error_rate=0.01, min_coverage_depth=1,
                      min_coverage_breadth=1.0, min_allele_frequency=0.001, n_threads=1):
    """Engine.pileup_parse on the host (pg_host_pileup_parse: plain C++, no GPU): the same dictionary, of numpy arrays."""
    lib = load_library()
    t = np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray, memoryview)) else np.ascontiguousarray(text, dtype=np.uint8)
    ps, rule = _pileup_args(pool_sizes, remove_ns, keep_lowercase_reference, max_base_error_rate, min_coverage_depth, min_coverage_breadth,
                            min_allele_frequency)
    info = PgPileupInfo()
    args = [t.ctypes.data if t.size else None, t.size] + rule
    rc = lib.pg_host_pileup_parse(*args, None, None, None, None, None, 0, 0, C.byref(info), int(n_threads))
    if info.err_reason:
        raise PileupError("pg_host_pileup_parse", info.err_line_off, info.err_reason)
    k, n = info.kept, len(ps)
    if rc != 0 and k == 0:
        raise NativeError(f"pg_host_pileup_parse failed ({rc}): bad arguments")
    counts = np.empty(k * n * 6, dtype=np.uint32); pos = np.empty(k, dtype=np.uint64); ref = np.empty(k, dtype=np.uint8)
    off = np.empty(k, dtype=np.int64); clen = np.empty(k, dtype=np.int32)
    if k:
        rc = lib.pg_host_pileup_parse(*args, counts.ctypes.data, pos.ctypes.data, ref.ctypes.data, off.ctypes.data, clen.ctypes.data, k,
                                      counts.size, C.byref(info), int(n_threads))
        if rc != 0:
            raise NativeError(f"pg_host_pileup_parse failed ({rc})")
    return _pileup_result(info, n, counts, pos, ref, off, clen)


def sync_format_host(counts, pos, ref, line_off, chrom_len, slab, n_threads=1):
    """Engine.sync_format on the host (pg_host_sync_format_rows: plain C++, no GPU): the rows of a parser's dictionary as NumPy
    arrays plus the text they were parsed from, to the bytes of their sync lines.  The checker of the device form and the
    baseline it is measured against."""
    lib = load_library()
    c = np.ascontiguousarray(counts).view(np.uint32) if np.asarray(counts).dtype == np.int32 else np.ascontiguousarray(counts, dtype=np.uint32)
    if c.ndim != 3 or c.shape[2] != 6:
        raise ValueError("sync_format_host: counts must be rows x n_pools x 6")
    k, n = c.shape[0], c.shape[1]
    po = np.ascontiguousarray(pos).view(np.uint64) if np.asarray(pos).dtype == np.int64 else np.ascontiguousarray(pos, dtype=np.uint64)
    rf = np.ascontiguousarray(ref, dtype=np.uint8); off = np.ascontiguousarray(line_off, dtype=np.int64)
    cl = np.ascontiguousarray(chrom_len, dtype=np.int32)
    if not (len(po) == len(rf) == len(off) == len(cl) == k):
        raise ValueError("sync_format_host: the row arrays do not match")
    t = np.frombuffer(slab, dtype=np.uint8) if isinstance(slab, (bytes, bytearray, memoryview)) else np.ascontiguousarray(slab, dtype=np.uint8)
    args = [t.ctypes.data if t.size else None, t.size, c.ctypes.data, po.ctypes.data, rf.ctypes.data, off.ctypes.data, cl.ctypes.data, n, k]
    need = C.c_int64()
    rc = lib.pg_host_sync_format_rows(*args, None, 0, C.byref(need), int(n_threads))
    if rc != 0 and need.value == 0:
        raise NativeError(f"pg_host_sync_format_rows failed ({rc}): bad arguments, or a row's chromosome name lies outside the slab")
    out = np.empty(max(need.value, 1), dtype=np.uint8)
    if need.value:
        rc = lib.pg_host_sync_format_rows(*args, out.ctypes.data, need.value, C.byref(need), int(n_threads))
        if rc != 0:
            raise NativeError(f"pg_host_sync_format_rows failed ({rc})")
    return out[:need.value].tobytes()


RESULT_OPS = {"fisher_exact_test": 0, "chisq_test": 1, "gwalpha": 2, "pearson_corr": 3, "ols_iter": 4}   # enum pg_result_op


def name_table(names):
    """Chromosome names -> (one uint8 array of their bytes, int32 offsets: len(names) + 1), the form the row formatters take."""
    raw = [n if isinstance(n, (bytes, bytearray)) else str(n).encode() for n in names]
    off = np.zeros(len(raw) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(b) for b in raw], dtype=np.int64)
    return np.frombuffer(b"".join(raw), dtype=np.uint8).copy(), off


def _host_text_call(fn, what, args, n_threads):
    """size query, then the text: the two-call pattern of the host twins -> bytes"""
    need = C.c_int64()
    rc = fn(*args, None, 0, C.byref(need), int(n_threads))
    if rc != 0 and need.value == 0:
        raise NativeError(f"{what} failed ({rc}): bad arguments, a label out of range or a row above the row limit")
    out = np.empty(max(need.value, 1), dtype=np.uint8)
    if need.value:
        rc = fn(*args, out.ctypes.data, need.value, C.byref(need), int(n_threads))
        if rc != 0:
            raise NativeError(f"{what} failed ({rc})")
    return out[:need.value].tobytes()


def f64_text_host(x, n_digits: int = -1, n_threads: int = 1) -> bytes:
    """Engine.f64_text on the host (pg_host_f64_text: plain C++, no GPU): one line per value, Rust's `{}` of the double for
    n_digits < 0, parse_f64_roundup_and_own(x, n_digits) otherwise."""
    a = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
    return _host_text_call(load_library().pg_host_f64_text, "pg_host_f64_text", [a.ctypes.data if a.size else None, a.size, int(n_digits)], n_threads)


def _u64(a):
    a = np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint64) if a.dtype == np.int64 else np.ascontiguousarray(a, dtype=np.uint64)


def result_rows_host(op, n_out, allele_ids, mean_freq, stat, pval, locus_chrom, locus_pos, chrom_names, k: int = 1, n_threads: int = 1) -> bytes:
    """Engine.result_rows on the host (pg_host_result_rows): the slot-major outputs of a per-locus operator as NumPy arrays,
    chromosome id and position per locus and the list of chromosome names, to the bytes of the analysis' CSV rows."""
    no = np.ascontiguousarray(n_out, dtype=np.int32); L = no.size
    ids = np.ascontiguousarray(allele_ids, dtype=np.int32)
    mf = None if mean_freq is None else np.ascontiguousarray(mean_freq, dtype=np.float64)
    st = np.ascontiguousarray(stat, dtype=np.float64)
    pv = None if pval is None else np.ascontiguousarray(pval, dtype=np.float64)
    ch = np.ascontiguousarray(locus_chrom, dtype=np.int32); po = _u64(locus_pos)
    text, off = name_table(chrom_names)
    args = [RESULT_OPS[op] if isinstance(op, str) else int(op), L, int(k), no.ctypes.data, ids.ctypes.data, None if mf is None else mf.ctypes.data,
            st.ctypes.data, None if pv is None else pv.ctypes.data, ch.ctypes.data, po.ctypes.data, text.ctypes.data if text.size else None,
            off.ctypes.data, len(off) - 1]
    return _host_text_call(load_library().pg_host_result_rows, "pg_host_result_rows", args, n_threads)


def kinship_rows_host(beta, pval, col_chrom, col_pos, col_allele, chrom_names, row0: int = 0, rows: int | None = None, n_threads: int = 1) -> bytes:
    """Engine.kinship_rows on the host (pg_host_kinship_rows): beta and pval as p x k arrays, the labels of the matrix'
    columns, to rows [row0, row0 + rows) of the kinship analyses' CSV (trait-major, the reference's label shift kept)."""
    b = np.ascontiguousarray(beta, dtype=np.float64); pv = np.ascontiguousarray(pval, dtype=np.float64)
    b = b.reshape(b.shape[0], -1); p, k = b.shape
    ch = np.ascontiguousarray(col_chrom, dtype=np.int32); po = _u64(col_pos); al = np.ascontiguousarray(col_allele, dtype=np.int32)
    text, off = name_table(chrom_names)
    rows = p * k - row0 if rows is None else rows
    args = [p, k, int(row0), int(rows), b.ctypes.data, pv.ctypes.data, ch.ctypes.data, po.ctypes.data, al.ctypes.data,
            text.ctypes.data if text.size else None, off.ctypes.data, len(off) - 1]
    return _host_text_call(load_library().pg_host_kinship_rows, "pg_host_kinship_rows", args, n_threads)


def label_table(labels):
    """Row labels -> (one uint8 array of their bytes, int64 offsets: len(labels) + 1), the form the table formatter takes."""
    raw = [s if isinstance(s, (bytes, bytearray)) else str(s).encode() for s in labels]
    off = np.zeros(len(raw) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(b) for b in raw], dtype=np.int64)
    return np.frombuffer(b"".join(raw), dtype=np.uint8).copy(), off


def _table_view(shape, strides, itemsize=8):
    """(rows, cols, row_stride, col_stride) in elements of a 2-D view: strided views (a transpose) are taken as they are"""
    if len(shape) != 2:
        raise ValueError("f64_table: expected a 2-D table")
    if any(s % itemsize or s < 0 for s in strides):
        raise ValueError("f64_table: the view's strides must be non-negative multiples of 8 bytes")
    return int(shape[0]), int(shape[1]), int(strides[0] // itemsize), int(strides[1] // itemsize)


def f64_table_host(x, labels=None, n_digits: int = -1, first_col_digits: int | None = None, row0: int = 0, n_rows: int | None = None,
                   n_threads: int = 1) -> bytes:
    """Engine.f64_table on the host (pg_host_f64_table): rows [row0, row0 + n_rows) of a 2-D float64 array (any strides: a
    transposed view is printed without a copy) as CSV text, row r = labels[r] (as given, no separator added) + the cells
    joined by ',' + '\\n'.  n_digits < 0 prints Rust's `{}`, 0..22 parse_f64_roundup_and_own; first_col_digits (default:
    n_digits) applies to column 0."""
    a = np.asarray(x, dtype=np.float64)
    rows, cols, rs, cs = _table_view(a.shape, a.strides)
    n_rows = rows - row0 if n_rows is None else n_rows
    text, off = (None, None) if labels is None else label_table(labels)
    if off is not None and len(off) != rows + 1:
        raise ValueError("f64_table: one label per row of the table")
    args = [a.ctypes.data if a.size else None, rows, cols, rs, cs, int(row0), int(n_rows), int(n_digits),
            int(n_digits if first_col_digits is None else first_col_digits), None if text is None else text.ctypes.data,
            None if off is None else off.ctypes.data]
    return _host_text_call(load_library().pg_host_f64_table, "pg_host_f64_table", args, n_threads)


GUDMC_ROW_KEYS = ("rows", "d_mean", "d_sd", "fst_mean", "fst_sd", "window", "d", "width", "width_dev", "width_p", "fst_delta", "fst_p")


def gudmc_rows_host(res, win_chr, win_ini, win_fin, pool_names, chrom_names, row0: int = 0, rows: int | None = None, n_threads: int = 1) -> bytes:
    """Engine.gudmc_rows on the host (pg_host_gudmc_rows): `res` is the dict of Engine.gudmc_from_tables as NumPy arrays."""
    keep = [np.ascontiguousarray(res[k], dtype=np.int64 if k in ("rows", "window") else np.float64) for k in GUDMC_ROW_KEYS]
    n = keep[0].size; w = keep[5].size // max(n * n, 1)
    ch = np.ascontiguousarray(win_chr, dtype=np.int32); ini = _u64(win_ini); fin = _u64(win_fin)
    ptext, poff = name_table(pool_names); ctext, coff = name_table(chrom_names)
    rows = int(keep[0].sum()) * n - row0 if rows is None else rows
    args = [n, w, int(row0), int(rows)] + [k.ctypes.data for k in keep] + [ch.ctypes.data, ini.ctypes.data, fin.ctypes.data,
            ptext.ctypes.data if ptext.size else None, poff.ctypes.data, ctext.ctypes.data if ctext.size else None, coff.ctypes.data, len(coff) - 1]
    return _host_text_call(load_library().pg_host_gudmc_rows, "pg_host_gudmc_rows", args, n_threads)


class Engine:
    def __init__(self, device: int | None = None, use_torch_stream: bool = True):
        self._lib = load_library()
        if not torch.cuda.is_available():
            raise NativeError("no GPU visible to torch: poolgen_amd needs an MI355X (gfx950) device")
        self.device = torch.cuda.current_device() if device is None else int(device)
        torch.cuda.set_device(self.device)
        stream = torch.cuda.current_stream(self.device).cuda_stream if use_torch_stream else 0
        ctx = C.c_void_p()
        rc = self._lib.pg_create(C.byref(ctx), self.device, C.c_void_p(stream))
        if rc != 0:
            raise NativeError(f"pg_create failed ({rc}): {self._lib.pg_last_error(None).decode()}")
        self._ctx = ctx
        self._comm_ready = False   # True while this context holds an RCCL communicator (comm_init .. comm_destroy)

    def close(self):
        self._comm_ready = False
        if getattr(self, "_ctx", None):
            self._lib.pg_destroy(self._ctx)
            self._ctx = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int, what: str):
        if rc != 0:
            raise NativeError(f"{what} failed ({rc}): {self._lib.pg_last_error(self._ctx).decode()}")

    def _dev(self, t: torch.Tensor, dtype) -> int:
        if not (t.is_cuda and t.dtype == dtype and t.is_contiguous() and t.device.index == self.device):
            raise ValueError(f"expected a contiguous {dtype} tensor on cuda:{self.device}")
        return t.data_ptr()

    # ---- profiling ---------------------------------------------------------------------
    def profile(self, on: bool = True):
        self._check(self._lib.pg_profile_enable(self._ctx, int(on)), "pg_profile_enable")

    def profile_reset(self):
        self._check(self._lib.pg_profile_reset(self._ctx), "pg_profile_reset")

    def profile_get(self, kernel: str):
        ms, n = C.c_double(), C.c_int64()
        self._check(self._lib.pg_profile_get(self._ctx, KERNEL_IDS[kernel], C.byref(ms), C.byref(n)),
                    "pg_profile_get")
        return ms.value, n.value

    def synchronize(self):
        self._check(self._lib.pg_synchronize(self._ctx), "pg_synchronize")

    # ---- multi-GPU: RCCL inside the library (pg_comm.cpp) ------------------------------------
    def comm_unique_id(self) -> bytes:
        """ncclGetUniqueId through the library; one rank calls it and hands the bytes to the others."""
        buf = C.create_string_buffer(128)
        self._check(self._lib.pg_comm_unique_id(buf), "pg_comm_unique_id")
        return buf.raw

    def comm_init(self, unique_id: bytes, nranks: int, rank: int):
        """Collective: every rank of the node calls it with the same id (ncclCommInitRank on this engine's GPU)."""
        assert len(unique_id) == 128
        self._check(self._lib.pg_comm_init_rank(self._ctx, C.c_char_p(unique_id), int(nranks), int(rank)), "pg_comm_init_rank")
        self._comm_ready = True

    def comm_destroy(self):
        self._comm_ready = False   # allreduce_sum would be the identity from here on: callers must fall back
        self._check(self._lib.pg_comm_destroy(self._ctx), "pg_comm_destroy")

    @property
    def comm_size(self) -> int:
        return int(self._lib.pg_comm_size(self._ctx))

    @property
    def comm_rank(self) -> int:
        return int(self._lib.pg_comm_rank(self._ctx))

    def comm_version(self) -> int:
        v = C.c_int()
        self._check(self._lib.pg_comm_version(C.byref(v)), "pg_comm_version")
        return v.value

    def allreduce_sum(self, t: torch.Tensor) -> torch.Tensor:
        """In-place sum over the ranks of this engine's communicator (identity without one), on the engine's stream."""
        self._check(self._lib.pg_allreduce_sum_dev(self._ctx, self._dev(t, torch.float64), t.numel()), "pg_allreduce_sum_dev")
        return t

    def ols_with_covariate_sharded(self, G: torch.Tensor, p_total: int, Y, var_explained: float = 0.75, force_m: int = -1,
                                   n: int | None = None, out=None, want_K: bool = False):
        """One rank's share of ols_iter_with_kinship in ONE library call (pg_ols_kinship_sharded_dev): partial kinship,
        RCCL all-reduce, n x n step with p_total, sweep of the own slab.  Returns (m, K or None, beta, var, pval)."""
        p, ld, n = self._g_dims(G, n)
        Yh = _host_f64(Y).reshape(n, -1)
        k = Yh.shape[1]
        if out is None:
            out = torch.empty((3, p, k), dtype=torch.float64, device=G.device)
        K = np.empty((n, n)) if want_K else None
        m = C.c_int()
        self._check(self._lib.pg_ols_kinship_sharded_dev(self._ctx, self._dev(G, torch.float64), p, int(p_total), n, ld,
                                                         Yh.ctypes.data, k, float(var_explained), int(force_m), C.byref(m),
                                                         K.ctypes.data if want_K else None, out[0].data_ptr(),
                                                         out[1].data_ptr(), out[2].data_ptr()),
                    "pg_ols_kinship_sharded_dev")
        return m.value, K, out[0], out[1], out[2]

    # ---- kinship path ---------------------------------------------------------------------
    @staticmethod
    def _g_dims(G: torch.Tensor, n: int | None):
        p, ld = G.shape
        return int(p), int(ld), int(ld if n is None else n)

    def set_phenotypes(self, Y, n: int | None = None):
        """Announce Y before kinship_partial so the kinship pass can pre-compute the m = 0 fits."""
        if Y is None:
            self._check(self._lib.pg_set_phenotypes(self._ctx, 0, None, 0), "pg_set_phenotypes")
            return
        Yh = _host_f64(Y)
        Yh = Yh.reshape(len(Yh) if n is None else n, -1)
        self._check(self._lib.pg_set_phenotypes(self._ctx, Yh.shape[0], Yh.ctypes.data, Yh.shape[1]),
                    "pg_set_phenotypes")

    def kinship_partial(self, G: torch.Tensor, n: int | None = None) -> torch.Tensor:
        """Unscaled sum_l g_l g_l^T (n x n) over the loci of G (p x ld, locus-major)."""
        p, ld, n = self._g_dims(G, n)
        S = torch.empty((n, n), dtype=torch.float64, device=G.device)
        self._check(self._lib.pg_kinship_partial_dev(self._ctx, self._dev(G, torch.float64), p, n, ld,
                                                     self._dev(S, torch.float64)), "pg_kinship_partial_dev")
        return S

    def kinship_set(self, S: torch.Tensor, p_total: int, Y, var_explained: float = 0.75,
                    force_m: int = -1, want_evals: bool = False, want_K: bool = True):
        """K = S / p_total, eigen rule, covariates, projected phenotypes.  Returns (m, K, evals);
        evals is None unless want_evals (asking for them forces the full eigen-decomposition); K is None
        unless want_K."""
        n = S.shape[0]
        Yh = _host_f64(Y).reshape(n, -1)
        K = np.empty((n, n)) if want_K else None; m = C.c_int()
        ev = np.empty(n) if want_evals else None
        self._check(self._lib.pg_kinship_set(self._ctx, self._dev(S, torch.float64), int(p_total), n,
                                             Yh.ctypes.data, Yh.shape[1], float(var_explained),
                                             int(force_m), C.byref(m), K.ctypes.data if want_K else None,
                                             ev.ctypes.data if want_evals else None),
                    "pg_kinship_set")
        return m.value, K, ev

    def covariates_set(self, n: int, Cmat, Y):
        Yh = _host_f64(Y).reshape(n, -1)
        if Cmat is None or np.size(Cmat) == 0:
            m, cptr = 0, None
        else:
            Ch = _host_f64(Cmat).reshape(n, -1)
            m, cptr = Ch.shape[1], Ch.ctypes.data
        self._check(self._lib.pg_covariates_set(self._ctx, n, cptr, m, Yh.ctypes.data, Yh.shape[1]),
                    "pg_covariates_set")
        self._k = Yh.shape[1]

    def ols_sweep(self, G: torch.Tensor, k: int, n: int | None = None, out=None):
        p, ld, n = self._g_dims(G, n)
        if out is None:
            out = torch.empty((3, p, k), dtype=torch.float64, device=G.device)
        self._check(self._lib.pg_ols_sweep_dev(self._ctx, self._dev(G, torch.float64), p, n, ld,
                                               out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr()),
                    "pg_ols_sweep_dev")
        return out[0], out[1], out[2]

    def ols_with_covariate(self, G: torch.Tensor, Y, var_explained: float = 0.75, force_m: int = -1,
                           n: int | None = None, out=None, want_K: bool = True):
        """Single-GPU ols_iter_with_kinship numeric core.  Returns (m, K, beta, var, pval).  want_K=False passes K_out = NULL:
        the library may then decide m = 0 from a bound that needs no kinship matrix (the lazy route, include/poolgen_hip.h)."""
        p, ld, n = self._g_dims(G, n)
        Yh = _host_f64(Y).reshape(n, -1)
        k = Yh.shape[1]
        if out is None:
            out = torch.empty((3, p, k), dtype=torch.float64, device=G.device)
        K = np.empty((n, n)) if want_K else None
        m = C.c_int()
        self._check(self._lib.pg_ols_kinship_dev(self._ctx, self._dev(G, torch.float64), p, n, ld,
                                                 Yh.ctypes.data, k, float(var_explained), int(force_m),
                                                 C.byref(m), K.ctypes.data if want_K else None, out[0].data_ptr(),
                                                 out[1].data_ptr(), out[2].data_ptr()),
                    "pg_ols_kinship_dev")
        return m.value, K, out[0], out[1], out[2]

    def mle_with_covariate(self, G: torch.Tensor, Y, var_explained: float = 0.75, force_m: int = -1, n: int | None = None):
        """gwas::mle_with_covariate (gwas/mle.rs:307-463), numeric core; parity unpinned (see include/poolgen_hip.h).
        Returns (m, K, beta, var, pval)."""
        p, ld, n = self._g_dims(G, n)
        Yh = _host_f64(Y).reshape(n, -1)
        k = Yh.shape[1]
        out = torch.empty((3, p, k), dtype=torch.float64, device=G.device)
        K = np.empty((n, n)); m = C.c_int()
        self._check(self._lib.pg_mle_kinship_dev(self._ctx, self._dev(G, torch.float64), p, n, ld, Yh.ctypes.data, k,
                                                 float(var_explained), int(force_m), C.byref(m), K.ctypes.data,
                                                 out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr()), "pg_mle_kinship_dev")
        return m.value, K, out[0], out[1], out[2]

    # ---- sync-derived batch operators -------------------------------------------------------
    # The library's outputs are SLOT-MAJOR (include/poolgen_hip.h): element (slot r, locus l) of allele_ids / mean_freq at
    # r * L + l, of stat / pval at (r * L + l) * k + trait; slots r >= n_out[l] are unspecified.  raw=True hands those arrays
    # out as they are ((5, L) / (5, L, k): what bench.py times); the default returns locus-major (L, 5[, k]) copies with the
    # unspecified slots filled with -1 / NaN, which is what the parity tests index.
    def _batch(self, fn, name, counts: torch.Tensor, pool_sizes, flt: Filter, Y, raw: bool = False):
        L, n, six = counts.shape
        assert six == 6
        ps = _host_f64(pool_sizes)
        Yh = _host_f64(Y).reshape(n, -1)
        k = Yh.shape[1]
        dev = counts.device
        n_out = torch.empty(L, dtype=torch.int32, device=dev)
        ids = torch.empty((5, L), dtype=torch.int32, device=dev)
        mf = torch.empty((5, L), dtype=torch.float64, device=dev)
        stat = torch.empty((5, L, k), dtype=torch.float64, device=dev)
        pv = torch.empty((5, L, k), dtype=torch.float64, device=dev)
        f = flt.to_c()
        self._check(fn(self._ctx, self._dev(counts, torch.int32), L, n, ps.ctypes.data, C.byref(f),
                       Yh.ctypes.data, k, n_out.data_ptr(), ids.data_ptr(), mf.data_ptr(),
                       stat.data_ptr(), pv.data_ptr()), name)
        if raw:
            return n_out, ids, mf, stat, pv
        live = torch.arange(5, device=dev)[None, :] < n_out[:, None]
        nan = torch.tensor(float("nan"), dtype=torch.float64, device=dev)
        return (n_out, torch.where(live, ids.T, torch.tensor(-1, dtype=torch.int32, device=dev)), torch.where(live, mf.T, nan),
                torch.where(live[:, :, None], stat.permute(1, 0, 2), nan), torch.where(live[:, :, None], pv.permute(1, 0, 2), nan))

    def ols_iterate(self, counts, pool_sizes, flt: Filter, Y, raw: bool = False):
        return self._batch(self._lib.pg_ols_iter_batch_dev, "pg_ols_iter_batch_dev", counts,
                           pool_sizes, flt, Y, raw)

    def correlation(self, counts, pool_sizes, flt: Filter, Y, raw: bool = False):
        return self._batch(self._lib.pg_pearson_batch_dev, "pg_pearson_batch_dev", counts,
                           pool_sizes, flt, Y, raw)

    def chisq(self, counts, pool_sizes, flt: Filter, raw: bool = False):
        L, n, _ = counts.shape
        ps = _host_f64(pool_sizes)
        dev = counts.device
        n_out = torch.empty(L, dtype=torch.int32, device=dev)
        ids = torch.empty((5, L), dtype=torch.int32, device=dev)   # the surviving alleles of the row in the slots below n_out
        chi2 = torch.empty(L, dtype=torch.float64, device=dev)
        pv = torch.empty(L, dtype=torch.float64, device=dev)
        f = flt.to_c()
        self._check(self._lib.pg_chisq_batch_dev(self._ctx, self._dev(counts, torch.int32), L, n, ps.ctypes.data,
                                                 C.byref(f), n_out.data_ptr(), ids.data_ptr(),
                                                 chi2.data_ptr(), pv.data_ptr()), "pg_chisq_batch_dev")
        if raw:
            return n_out, ids, chi2, pv
        live = torch.arange(5, device=dev)[None, :] < n_out[:, None]
        return n_out, torch.where(live, ids.T, torch.tensor(-1, dtype=torch.int32, device=dev)), chi2, pv

    def fisher(self, counts, pool_sizes, flt: Filter, raw: bool = False):
        """tables::fisher: n_out, ids, p_observed, pval (= p_observed + p_extremes) per locus; a locus' result depends on
        its own counts, the filter and n only."""
        L, n, _ = counts.shape
        ps = _host_f64(pool_sizes)
        dev = counts.device
        n_out = torch.empty(L, dtype=torch.int32, device=dev)
        ids = torch.empty((5, L), dtype=torch.int32, device=dev)   # the surviving alleles of the row in the slots below n_out
        pobs = torch.empty(L, dtype=torch.float64, device=dev)
        pv = torch.empty(L, dtype=torch.float64, device=dev)
        f = flt.to_c()
        self._check(self._lib.pg_fisher_batch_dev(self._ctx, self._dev(counts, torch.int32), L, n, ps.ctypes.data,
                                                  C.byref(f), n_out.data_ptr(), ids.data_ptr(),
                                                  pobs.data_ptr(), pv.data_ptr()), "pg_fisher_batch_dev")
        if raw:
            return n_out, ids, pobs, pv
        live = torch.arange(5, device=dev)[None, :] < n_out[:, None]
        return n_out, torch.where(live, ids.T, torch.tensor(-1, dtype=torch.int32, device=dev)), pobs, pv

    def gwalpha(self, counts, bins, q, sig: float, min: float, max: float, flt: Filter, method: str = "ML", raw: bool = False):
        """gwas::gwalpha_ls / gwalpha_ml per row (= locus, kept allele): n_out, ids, mean_freq, alpha, shapes (4 per row), cost,
        iters.  bins: the pools' shares (also the filter's pool sizes); q: column 1 of the reference's phenotype matrix as handed
        over.  Any method other than "LS" means ML (main.rs:337-356).  A row's result depends on the row alone."""
        L, n, six = counts.shape
        assert six == 6
        bh, qh = _host_f64(bins), _host_f64(q)
        if bh.shape != (n,) or qh.shape != (n,):
            raise ValueError(f"gwalpha: bins and q need one entry per pool ({n})")
        dev = counts.device
        n_out = torch.empty(L, dtype=torch.int32, device=dev)
        ids = torch.empty((5, L), dtype=torch.int32, device=dev)
        mf = torch.empty((5, L), dtype=torch.float64, device=dev)
        alpha = torch.empty((5, L), dtype=torch.float64, device=dev)
        shapes = torch.empty((5, L, 4), dtype=torch.float64, device=dev)
        cost = torch.empty((5, L), dtype=torch.float64, device=dev)
        iters = torch.empty((5, L), dtype=torch.int32, device=dev)
        f = flt.to_c()
        self._check(self._lib.pg_gwalpha_batch_dev(self._ctx, self._dev(counts, torch.int32), L, n, bh.ctypes.data, qh.ctypes.data,
                                                   float(sig), float(min), float(max), C.byref(f), 0 if method == "LS" else 1,
                                                   n_out.data_ptr(), ids.data_ptr(), mf.data_ptr(), alpha.data_ptr(),
                                                   shapes.data_ptr(), cost.data_ptr(), iters.data_ptr()), "pg_gwalpha_batch_dev")
        if raw:
            return n_out, ids, mf, alpha, shapes, cost, iters
        live = torch.arange(5, device=dev)[None, :] < n_out[:, None]
        nan = torch.tensor(float("nan"), dtype=torch.float64, device=dev)
        m1 = torch.tensor(-1, dtype=torch.int32, device=dev)
        return (n_out, torch.where(live, ids.T, m1), torch.where(live, mf.T, nan), torch.where(live, alpha.T, nan),
                torch.where(live[:, :, None], shapes.permute(1, 0, 2), nan), torch.where(live, cost.T, nan),
                torch.where(live, iters.T, m1))

    def beta_reg(self, a, b, x) -> torch.Tensor:
        """Beta(a, b).cdf(x) elementwise as the gwalpha fit evaluates it (statrs' beta_reg behind Beta::cdf's guards)."""
        dev = torch.device("cuda", self.device)
        t = [torch.as_tensor(np.ascontiguousarray(np.asarray(v, dtype=np.float64))).to(dev) if not isinstance(v, torch.Tensor) else v
             for v in (a, b, x)]
        if not (t[0].shape == t[1].shape == t[2].shape):
            raise ValueError("beta_reg: a, b and x need one shape")
        out = torch.empty_like(t[0])
        if out.numel() == 0:
            return out
        self._check(self._lib.pg_beta_reg_dev(self._ctx, self._dev(t[0], torch.float64), self._dev(t[1], torch.float64),
                                              self._dev(t[2], torch.float64), t[0].numel(), out.data_ptr()), "pg_beta_reg_dev")
        return out

    def last_listed(self):
        """(loci, listed) of the last batch operator call: how many loci its streaming pass handed to the second pass."""
        a, b = C.c_int64(), C.c_int64()
        self._check(self._lib.pg_locus_op_stats(self._ctx, C.byref(a), C.byref(b)), "pg_locus_op_stats")
        return a.value, b.value

    def last_listed_fraction(self) -> float:
        loci, listed = self.last_listed()
        return listed / loci if loci else 0.0

    def load_frequencies(self, counts, pool_sizes, flt: Filter, keep_p_minus_1: bool = False, order=None,
                         pool_keep=None, ld: int | None = None, coverages: bool = False):
        """The reference loader (base/sync.rs:972-1180) on a counts batch in HBM: filter, frequencies over the
        surviving alleles, optionally drop the major allele; one column of G per surviving allele.  Returns
        (G [p x ld], col_locus [p], col_allele [p]); `pool_keep` (bool per pool) selects the rows written.
        coverages=True appends cov [p x ld]: per column row the pools' depths over the locus' surviving alleles."""
        L, n, _ = counts.shape
        ps = _host_f64(pool_sizes)
        dev = counts.device
        f = flt.to_c()
        p = C.c_int64()
        optr = None
        if order is not None:
            order = order.to(device=dev, dtype=torch.int64).contiguous()
            optr = order.data_ptr()
        self._check(self._lib.pg_load_plan_dev(self._ctx, self._dev(counts, torch.int32), L, n, ps.ctypes.data,
                                               C.byref(f), int(keep_p_minus_1), optr, C.byref(p)), "pg_load_plan_dev")
        if pool_keep is None:
            pmap, n_out = None, n
        else:
            keep = np.asarray(pool_keep, dtype=bool)
            pmap = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)
            n_out = int(keep.sum())
        ld = (n_out + (n_out & 1)) if ld is None else int(ld)
        G = torch.empty((p.value, ld), dtype=torch.float64, device=dev)
        col_locus = torch.empty(p.value, dtype=torch.int64, device=dev)
        col_allele = torch.empty(p.value, dtype=torch.int32, device=dev)
        if coverages:
            cov = torch.empty((p.value, ld), dtype=torch.float64, device=dev)
            self._check(self._lib.pg_load_emit_cov_dev(self._ctx, pmap.ctypes.data if pmap is not None else None, n_out,
                                                       G.data_ptr(), ld, col_locus.data_ptr(), col_allele.data_ptr(),
                                                       cov.data_ptr()), "pg_load_emit_cov_dev")
            return G, col_locus, col_allele, cov
        self._check(self._lib.pg_load_emit_dev(self._ctx, pmap.ctypes.data if pmap is not None else None, n_out,
                                               G.data_ptr(), ld, col_locus.data_ptr(), col_allele.data_ptr()),
                    "pg_load_emit_dev")
        return G, col_locus, col_allele

    def freq_csv(self, G, col_locus, col_allele, chrom_ids, pos, chrom_names, n: int | None = None, row0: int = 0,
                 rows: int | None = None, out: torch.Tensor | None = None, validate: bool = True) -> torch.Tensor:
        """The rows [row0, row0 + rows) of load_frequencies' matrix as the text of sync2csv's file (FileSyncPhen::write_csv,
        base/sync.rs:1182-1262; no header line), formatted on the GPU: a torch.uint8 tensor on G's device.  chrom_ids / pos:
        per locus (what col_locus indexes) the chromosome's index into chrom_names and the position.  With `out` (a uint8
        tensor on the device that is large enough: a slab's buffer) one call formats into it, without the size query, and the
        filled part of `out` is returned.  validate=False skips the check that col_locus stays inside chrom_ids / pos (two
        reductions and a synchronisation per call: the library cannot know their length); a caller that formats slab after
        slab of one table checks once.  The name table of the last call stays on the device for the next one."""
        p, ld, n = self._g_dims(G, n)
        rows = p - row0 if rows is None else int(rows)
        if not (0 <= row0 and 0 <= rows and row0 + rows <= p):
            raise ValueError("freq_csv: rows out of range")
        dev = G.device
        if col_locus.numel() != p or col_allele.numel() != p:
            raise ValueError("freq_csv: col_locus / col_allele do not match G")
        ch = torch.as_tensor(np.ascontiguousarray(chrom_ids, dtype=np.int32)).to(dev) if not isinstance(chrom_ids, torch.Tensor) else chrom_ids
        # (torch has no uint64 arithmetic; the bits are what the kernel reads)
        po = torch.as_tensor(np.ascontiguousarray(pos, dtype=np.uint64).view(np.int64)).to(dev) if not isinstance(pos, torch.Tensor) else pos
        if ch.numel() != po.numel():
            raise ValueError("freq_csv: chrom_ids / pos do not match")
        if validate and rows and not (0 <= int(col_locus[row0:row0 + rows].min()) and int(col_locus[row0:row0 + rows].max()) < ch.numel()):
            raise ValueError("freq_csv: col_locus points outside chrom_ids / pos")   # (the library cannot know their length)
        key = (tuple(chrom_names), dev)
        if getattr(self, "_csv_names", (None,))[0] != key:
            text, off = _chrom_table(chrom_names)
            self._csv_names = (key, torch.as_tensor(text).to(dev), torch.as_tensor(off).to(dev))
        _, text_dev, off_dev = self._csv_names
        args = [self._ctx, self._dev(G, torch.float64), ld, n, int(row0), rows, self._dev(col_locus, torch.int64),
                self._dev(col_allele, torch.int32), self._dev(ch, torch.int32), self._dev(po, torch.int64), text_dev.data_ptr(),
                off_dev.data_ptr(), off_dev.numel() - 1]
        need = C.c_int64()
        if out is not None:
            self._check(self._lib.pg_csv_freq_rows_dev(*args, self._dev(out, torch.uint8), out.numel(), C.byref(need)),
                        "pg_csv_freq_rows_dev")
            return out[:need.value]
        rc = self._lib.pg_csv_freq_rows_dev(*args, None, 0, C.byref(need))
        if rc != 0 and need.value == 0:
            self._check(rc, "pg_csv_freq_rows_dev")
        out = torch.empty(need.value, dtype=torch.uint8, device=dev)
        if need.value:
            self._check(self._lib.pg_csv_freq_rows_dev(*args, out.data_ptr(), need.value, C.byref(need)), "pg_csv_freq_rows_dev")
        return out

    def vcf_parse(self, text, pool_sizes, min_coverage_depth: int = 1, min_coverage_breadth: float = 1.0,
                  min_allele_frequency: float = 0.001):
        """A slab of VCF text -- bytes, a NumPy uint8 array or a torch uint8 tensor (on the device it is parsed in place); it starts
        at a line start, its last line may lack the newline -- to what vcf2sync keeps of it (base/vcf.rs), parsed on the GPU.
        A dictionary: counts (kept x n_pools x 6, the six in the order vcf_to_sync writes them; the uint32 bits as int32, as the
        loader takes them), pos (the uint64 bits as int64: torch has no uint64 arithmetic), ref (uint8), line_off (int64), chrom_len (int32) as tensors on the device, and
        the integers data_lines, n_pools, chrom_line_off.  A line at which the reference panics raises VcfError."""
        dev = torch.device("cuda", self.device)
        if isinstance(text, torch.Tensor):
            t = text.to(dev)
            if t.dtype != torch.uint8 or not t.is_contiguous():
                raise ValueError("vcf_parse: text must be a contiguous uint8 tensor")
        else:
            a = np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray, memoryview)) else np.ascontiguousarray(text, dtype=np.uint8)
            t = torch.from_numpy(a.copy()).to(dev)
        ps = _host_f64(pool_sizes)
        info = PgVcfInfo()
        args = [self._ctx, t.data_ptr() if t.numel() else None, t.numel(), ps.ctypes.data, len(ps), int(min_coverage_depth),
                float(min_coverage_breadth), float(min_allele_frequency)]
        rc = self._lib.pg_vcf_parse_dev(*args, None, None, None, None, None, 0, 0, C.byref(info))
        if info.err_reason:
            raise VcfError("pg_vcf_parse_dev", info.err_line_off, info.err_reason)
        k, n = info.kept, info.n_pools
        if rc != 0 and k == 0:
            self._check(rc, "pg_vcf_parse_dev")
        counts = torch.empty(k * n * 6, dtype=torch.int32, device=dev)
        pos = torch.empty(k, dtype=torch.int64, device=dev); ref = torch.empty(k, dtype=torch.uint8, device=dev)
        off = torch.empty(k, dtype=torch.int64, device=dev); clen = torch.empty(k, dtype=torch.int32, device=dev)
        if k:
            self._check(self._lib.pg_vcf_parse_dev(*args, counts.data_ptr(), pos.data_ptr(), ref.data_ptr(), off.data_ptr(), clen.data_ptr(),
                                                   k, counts.numel(), C.byref(info)), "pg_vcf_parse_dev")
        return _vcf_result(info, counts, pos, ref, off, clen)

    def pileup_parse(self, text, pool_sizes, remove_ns: bool = True, keep_lowercase_reference: bool = False,
                     max_base_error_rate: float = 0.01, min_coverage_depth: int = 1, min_coverage_breadth: float = 1.0,
                     min_allele_frequency: float = 0.001):
        """A slab of samtools mpileup text -- bytes, a NumPy uint8 array or a torch uint8 tensor (on the device it is parsed in
        place); it starts at a line start, its last line may lack the newline -- to what pileup2sync keeps of it (base/pileup.rs),
        parsed on the GPU.  A dictionary: counts (kept x n_pools x 6 at the positions pileup_to_sync writes, A:T:C:G:D:N; the
        uint32 bits as int32, as the loader takes them), pos (the uint64 bits as int64), ref (uint8), line_off (int64), chrom_len
        (int32) as tensors on the device, and the integers lines, n_pools.  A line at which the reference panics raises
        PileupError."""
        dev = torch.device("cuda", self.device)
        if isinstance(text, torch.Tensor):
            t = text.to(dev)
            if t.dtype != torch.uint8 or not t.is_contiguous():
                raise ValueError("pileup_parse: text must be a contiguous uint8 tensor")
        else:
            a = np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray, memoryview)) else np.ascontiguousarray(text, dtype=np.uint8)
            t = torch.from_numpy(a.copy()).to(dev)
        ps, rule = _pileup_args(pool_sizes, remove_ns, keep_lowercase_reference, max_base_error_rate, min_coverage_depth,
                                min_coverage_breadth, min_allele_frequency)
        info = PgPileupInfo()
        args = [self._ctx, t.data_ptr() if t.numel() else None, t.numel()] + rule
        rc = self._lib.pg_pileup_parse_dev(*args, None, None, None, None, None, 0, 0, C.byref(info))
        if info.err_reason:
            raise PileupError("pg_pileup_parse_dev", info.err_line_off, info.err_reason)
        k, n = info.kept, len(ps)
        if rc != 0 and k == 0:
            self._check(rc, "pg_pileup_parse_dev")
        counts = torch.empty(k * n * 6, dtype=torch.int32, device=dev)
        pos = torch.empty(k, dtype=torch.int64, device=dev); ref = torch.empty(k, dtype=torch.uint8, device=dev)
        off = torch.empty(k, dtype=torch.int64, device=dev); clen = torch.empty(k, dtype=torch.int32, device=dev)
        if k:
            self._check(self._lib.pg_pileup_parse_dev(*args, counts.data_ptr(), pos.data_ptr(), ref.data_ptr(), off.data_ptr(),
                                                      clen.data_ptr(), k, counts.numel(), C.byref(info)), "pg_pileup_parse_dev")
        return _pileup_result(info, n, counts, pos, ref, off, clen)

    def sync_parse(self, text, expect_n: int = 0):
        """A slab of sync text -- bytes, a NumPy uint8 array or a torch uint8 tensor (on the device it is parsed in place); it starts
        at a line start, its last line may lack the newline -- to the counts of its loci, parsed on the GPU.  expect_n: the pool
        count every line must have (0: that of the first data line).  A dictionary: counts (kept x n_pools x 6, the uint32 bits as
        int32, as the loader takes them), pos (the uint64 bits as int64), line_off (int64), chrom_len (int32) as tensors on the
        device, and the integers data_lines, n_pools.  A line at which the CLI's host parser throws raises SyncError."""
        dev = torch.device("cuda", self.device)
        if isinstance(text, torch.Tensor):
            t = text.to(dev)
            if t.dtype != torch.uint8 or not t.is_contiguous():
                raise ValueError("sync_parse: text must be a contiguous uint8 tensor")
        else:
            a = np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray, memoryview)) else np.ascontiguousarray(text, dtype=np.uint8)
            t = torch.from_numpy(a.copy()).to(dev)
        info = PgSyncInfo()
        args = [self._ctx, t.data_ptr() if t.numel() else None, t.numel(), int(expect_n)]
        rc = self._lib.pg_sync_parse_dev(*args, None, None, None, None, 0, 0, C.byref(info))
        if info.err_reason:
            raise SyncError("pg_sync_parse_dev", info.err_line_off, info.err_reason)
        k, n = info.kept, info.n_pools
        if rc != 0 and k == 0:
            self._check(rc, "pg_sync_parse_dev")
        counts = torch.empty(k * n * 6, dtype=torch.int32, device=dev)
        pos = torch.empty(k, dtype=torch.int64, device=dev)
        off = torch.empty(k, dtype=torch.int64, device=dev); clen = torch.empty(k, dtype=torch.int32, device=dev)
        if k:
            self._check(self._lib.pg_sync_parse_dev(*args, counts.data_ptr(), pos.data_ptr(), off.data_ptr(), clen.data_ptr(), k, counts.numel(),
                                                    C.byref(info)), "pg_sync_parse_dev")
        return _sync_result(info, counts, pos, off, clen)

    def sync_format(self, counts, pos, ref, line_off, chrom_len, slab, out: torch.Tensor | None = None) -> torch.Tensor:
        """The rows vcf_parse / pileup_parse / sync_parse return (tensors on the device; sync_parse has no `ref`: supply one) plus
        the text they were parsed from (`slab`: a uint8 tensor on the device, or bytes / a NumPy array that is copied there) as the
        bytes of their sync lines (pileup_to_sync, pileup.rs:348-371; vcf_to_sync, vcf.rs:212-229), formatted on the GPU: a
        torch.uint8 tensor on the device.  With `out` (a uint8 tensor on the device that is large enough) one call formats into
        it, without the size query, and the filled part of `out` is returned."""
        dev = torch.device("cuda", self.device)
        if counts.dim() != 3 or counts.shape[2] != 6:
            raise ValueError("sync_format: counts must be rows x n_pools x 6")
        k, n = int(counts.shape[0]), int(counts.shape[1])
        if not (pos.numel() == ref.numel() == line_off.numel() == chrom_len.numel() == k):
            raise ValueError("sync_format: the row arrays do not match")
        if isinstance(slab, torch.Tensor):
            t = slab.to(dev)
            if t.dtype != torch.uint8 or not t.is_contiguous():
                raise ValueError("sync_format: slab must be a contiguous uint8 tensor")
        else:
            a = np.frombuffer(slab, dtype=np.uint8) if isinstance(slab, (bytes, bytearray, memoryview)) else np.ascontiguousarray(slab, dtype=np.uint8)
            t = torch.from_numpy(a.copy()).to(dev)
        args = [self._ctx, t.data_ptr() if t.numel() else None, t.numel(), self._dev(counts, torch.int32), self._dev(pos, torch.int64),
                self._dev(ref, torch.uint8), self._dev(line_off, torch.int64), self._dev(chrom_len, torch.int32), n, k]
        need = C.c_int64()
        if out is not None:
            self._check(self._lib.pg_sync_format_rows_dev(*args, self._dev(out, torch.uint8), out.numel(), C.byref(need)),
                        "pg_sync_format_rows_dev")
            return out[:need.value]
        rc = self._lib.pg_sync_format_rows_dev(*args, None, 0, C.byref(need))
        if rc != 0 and need.value == 0:
            self._check(rc, "pg_sync_format_rows_dev")
        out = torch.empty(need.value, dtype=torch.uint8, device=dev)
        if need.value:
            self._check(self._lib.pg_sync_format_rows_dev(*args, out.data_ptr(), need.value, C.byref(need)), "pg_sync_format_rows_dev")
        return out

    # ---- the result writer (pg_resultfmt.hip) ----------------------------------------------------
    def _text_call(self, fn, what, args, out):
        """size query, then the text (or one call into `out`) -> a uint8 tensor on the device"""
        need = C.c_int64()
        if out is not None:
            self._check(fn(*args, self._dev(out, torch.uint8), out.numel(), C.byref(need)), what)
            return out[:need.value]
        rc = fn(*args, None, 0, C.byref(need))
        if rc != 0 and need.value == 0:
            self._check(rc, what)
        out = torch.empty(need.value, dtype=torch.uint8, device=torch.device("cuda", self.device))
        if need.value:
            self._check(fn(*args, out.data_ptr(), need.value, C.byref(need)), what)
        return out

    def _names_dev(self, chrom_names):
        dev = torch.device("cuda", self.device)
        text, off = name_table(chrom_names)
        return torch.from_numpy(text).to(dev), torch.from_numpy(off).to(dev)

    def f64_text(self, x: torch.Tensor, n_digits: int = -1, out: torch.Tensor | None = None) -> torch.Tensor:
        """One line per value of `x` (float64, on the device), formatted on the GPU: Rust's `{}` of the double -- the shortest
        digits that round-trip, fixed notation -- for n_digits < 0, parse_f64_roundup_and_own(x, n_digits) otherwise.  Returns a
        uint8 tensor on the device; with `out` one call formats into it."""
        x = x.reshape(-1)
        args = [self._ctx, self._dev(x, torch.float64) if x.numel() else None, x.numel(), int(n_digits)]
        return self._text_call(self._lib.pg_f64_text_dev, "pg_f64_text_dev", args, out)

    def result_rows(self, op, n_out, allele_ids, mean_freq, stat, pval, locus_chrom, locus_pos, chrom_names, k: int = 1,
                    out: torch.Tensor | None = None) -> torch.Tensor:
        """The CSV rows of a per-locus analysis (`op`: fisher_exact_test, chisq_test, gwalpha, pearson_corr, ols_iter) from the
        slot-major tensors its batch operator left on the device, formatted on the GPU.  locus_chrom (int32) and locus_pos
        (int64) are per locus, chrom_names the list of names.  Equal to the host writer's bytes whenever every printed
        |value| < 2^53; above that it prints what the reference prints (see include/poolgen_hip.h)."""
        names, off = self._names_dev(chrom_names)
        args = [self._ctx, RESULT_OPS[op] if isinstance(op, str) else int(op), n_out.numel(), int(k), self._dev(n_out, torch.int32),
                self._dev(allele_ids, torch.int32), None if mean_freq is None else self._dev(mean_freq, torch.float64),
                self._dev(stat, torch.float64), None if pval is None else self._dev(pval, torch.float64), self._dev(locus_chrom, torch.int32),
                self._dev(locus_pos, torch.int64), names.data_ptr() if names.numel() else None, off.data_ptr(), off.numel() - 1]
        return self._text_call(self._lib.pg_result_rows_dev, "pg_result_rows_dev", args, out)

    def kinship_rows(self, beta, pval, col_chrom, col_pos, col_allele, chrom_names, row0: int = 0, rows: int | None = None,
                     out: torch.Tensor | None = None) -> torch.Tensor:
        """Rows [row0, row0 + rows) of the CSV of ols_iter_with_kinship / mle_iter_with_kinship from beta and pval (p x k, on the
        device) and the labels of the matrix' columns, formatted on the GPU: trait-major, the reference's label shift kept."""
        p = int(beta.shape[0]); k = int(beta.numel() // max(p, 1))
        names, off = self._names_dev(chrom_names)
        rows = p * k - row0 if rows is None else rows
        args = [self._ctx, p, k, int(row0), int(rows), self._dev(beta, torch.float64), self._dev(pval, torch.float64),
                self._dev(col_chrom, torch.int32), self._dev(col_pos, torch.int64), self._dev(col_allele, torch.int32),
                names.data_ptr() if names.numel() else None, off.data_ptr(), off.numel() - 1]
        return self._text_call(self._lib.pg_kinship_rows_dev, "pg_kinship_rows_dev", args, out)

    # ---- the popgen writer (pg_tablefmt.hip, pg_resultfmt.hip) -----------------------------------
    def f64_table(self, x: torch.Tensor, labels=None, n_digits: int = -1, first_col_digits: int | None = None, row0: int = 0,
                  n_rows: int | None = None, out: torch.Tensor | None = None) -> torch.Tensor:
        """Rows [row0, row0 + n_rows) of a 2-D float64 tensor on the device (any non-negative strides: a transposed view is
        printed without a copy) as CSV text, formatted on the GPU one lane per cell: row r = labels[r] (as given, no separator
        added) + the cells joined by ',' + '\\n'.  n_digits < 0 prints Rust's `{}`, 0..22 parse_f64_roundup_and_own;
        first_col_digits (default: n_digits) applies to column 0.  `labels`: a list of names, or a (uint8 bytes, int64 offsets)
        pair of tensors already on the device.  Returns a uint8 tensor on the device; with `out` one call formats into it."""
        dev = torch.device("cuda", self.device)
        if x.dtype != torch.float64 or x.device != dev:
            raise ValueError("f64_table: expected a float64 tensor on this engine's GPU")
        rows, cols, rs, cs = _table_view(tuple(x.shape), tuple(s * 8 for s in x.stride()))
        n_rows = rows - row0 if n_rows is None else n_rows
        if labels is None:
            text = off = None
        elif isinstance(labels, tuple):
            text, off = labels
        else:
            t, o = label_table(labels)
            text, off = torch.from_numpy(t).to(dev), torch.from_numpy(o).to(dev)
        if off is not None and off.numel() != rows + 1:
            raise ValueError("f64_table: one label per row of the table")
        args = [self._ctx, x.data_ptr() if x.numel() else None, rows, cols, rs, cs, int(row0), int(n_rows), int(n_digits),
                int(n_digits if first_col_digits is None else first_col_digits),
                None if text is None else (self._dev(text, torch.uint8) if text.numel() else self._dev(off, torch.int64)),
                None if off is None else self._dev(off, torch.int64)]
        return self._text_call(self._lib.pg_f64_table_dev, "pg_f64_table_dev", args, out)

    def gudmc_rows(self, res: dict, win_chr, win_ini, win_fin, pool_names, chrom_names, row0: int = 0, rows: int | None = None,
                   out: torch.Tensor | None = None) -> torch.Tensor:
        """Rows [row0, row0 + rows) of gudmc's file from the dict gudmc_from_tables returns (its tensors stay on the device; only
        rows[n] is read back), the windows' chromosome ids, first and last positions, the pool names and the chromosome names
        (by id), formatted on the GPU.  Returns a uint8 tensor on the device."""
        dev = torch.device("cuda", self.device)
        n = res["rows"].numel(); w = res["window"].numel() // max(n * n, 1)
        ch = torch.as_tensor(np.ascontiguousarray(win_chr, dtype=np.int32)).to(dev)
        ini = torch.as_tensor(_u64(win_ini).view(np.int64)).to(dev); fin = torch.as_tensor(_u64(win_fin).view(np.int64)).to(dev)
        ptext, poff = self._names_dev(pool_names); ctext, coff = self._names_dev(chrom_names)
        rows = int(res["rows"].sum().item()) * n - row0 if rows is None else rows
        args = [self._ctx, n, w, int(row0), int(rows)] + \
               [self._dev(res[k], torch.int64 if k in ("rows", "window") else torch.float64) for k in GUDMC_ROW_KEYS] + \
               [ch.data_ptr(), ini.data_ptr(), fin.data_ptr(), ptext.data_ptr() if ptext.numel() else None, poff.data_ptr(),
                ctext.data_ptr() if ctext.numel() else None, coff.data_ptr(), coff.numel() - 1]
        return self._text_call(self._lib.pg_gudmc_rows_dev, "pg_gudmc_rows_dev", args, out)

    # ---- imputation (src/imputation/) ------------------------------------------------------------
    def _impute_args(self, M, locus_col, n):
        p, ld, n = self._g_dims(M, n)
        lc = np.ascontiguousarray(locus_col, dtype=np.int64)
        return p, ld, n, lc, len(lc) - 1

    def set_missing_by_depth(self, G, cov, locus_col, min_depth: float = 5.0, n: int | None = None):
        """set_missing_by_depth (filtering_missing.rs:15-44), in place on G and cov (cov laid out like G, as load_frequencies
        returns it): cov < min_depth -> NaN coverage and NaN frequencies; the last locus keeps its frequencies, as written."""
        p, ld, n, lc, L = self._impute_args(G, locus_col, n)
        assert cov.shape == G.shape
        self._check(self._lib.pg_set_missing_by_depth_dev(self._ctx, self._dev(G, torch.float64), self._dev(cov, torch.float64),
                                                          p, n, ld, lc.ctypes.data, L, float(min_depth)), "pg_set_missing_by_depth_dev")

    def missingness(self, G, cov, locus_col, n: int | None = None):
        """(NaN frequencies per pool [n], NaN coverages per locus [L]): what the two filters sort by (:53-61, :136-144)."""
        p, ld, n, lc, L = self._impute_args(G, locus_col, n)
        assert cov.shape == G.shape
        pool_nan = np.empty(n, dtype=np.int64); locus_nan = np.empty(L, dtype=np.int64)
        self._check(self._lib.pg_missingness_dev(self._ctx, self._dev(G, torch.float64), self._dev(cov, torch.float64), p, n, ld,
                                                 lc.ctypes.data, L, pool_nan.ctypes.data, locus_nan.ctypes.data), "pg_missingness_dev")
        return pool_nan, locus_nan

    @staticmethod
    def top_missing_keep(nan_count, frac: float, what: str = "pools") -> np.ndarray:
        """The keep rule of filter_out_top_missing_pools / _loci (:63-86, :146-170) from NaN counts: the kept indices,
        ascending.  An empty result is the reference's error."""
        counts = np.ascontiguousarray(nan_count, dtype=np.int64)
        keep = np.empty(max(len(counts), 1), dtype=np.int64)
        left = load_library().pg_host_top_missing_keep(counts.ctypes.data, len(counts), float(frac), keep.ctypes.data)
        if left < 0:
            raise ValueError("top_missing_keep: bad argument")
        if left == 0:
            raise NativeError(f"No {what} left after filtering, please reduce 'frac_top_missing_{what}'")
        return keep[:left].copy()

    def impute_compact(self, G, cov, locus_col, keep_pools, keep_loci, col_locus=None, col_allele=None, n: int | None = None):
        """G, cov and the column labels of the kept pools and loci -> (G, cov, locus_col, col_locus, col_allele) of the kept
        part (labels None where none were given)."""
        p, ld, n, lc, L = self._impute_args(G, locus_col, n)
        kp = np.ascontiguousarray(keep_pools, dtype=np.int64); kl = np.ascontiguousarray(keep_loci, dtype=np.int64)
        if len(kl) == 0 or len(kp) == 0 or kl.min() < 0 or kl.max() >= L:
            raise ValueError("impute_compact: nothing kept, or a locus out of range")
        p_out = int((lc[kl + 1] - lc[kl]).sum())
        n_out = len(kp)
        ld_out = n_out + (n_out & 1)
        dev = G.device
        G2 = torch.empty((p_out, ld_out), dtype=torch.float64, device=dev)
        cov2 = torch.empty((p_out, ld_out), dtype=torch.float64, device=dev) if cov is not None else None
        cl2 = torch.empty(p_out, dtype=torch.int64, device=dev) if col_locus is not None else None
        ca2 = torch.empty(p_out, dtype=torch.int32, device=dev) if col_allele is not None else None
        lc2 = np.empty(len(kl) + 1, dtype=np.int64)
        ptr = lambda t, dt: self._dev(t, dt) if t is not None else None
        self._check(self._lib.pg_impute_compact_dev(self._ctx, self._dev(G, torch.float64), ptr(cov, torch.float64), p, n, ld,
                                                    ptr(col_locus, torch.int64), ptr(col_allele, torch.int32), lc.ctypes.data, L,
                                                    kp.ctypes.data, n_out, kl.ctypes.data, len(kl), G2.data_ptr(),
                                                    ptr(cov2, torch.float64), ld_out, ptr(cl2, torch.int64), ptr(ca2, torch.int32),
                                                    lc2.ctypes.data), "pg_impute_compact_dev")
        return G2, cov2, lc2, cl2, ca2

    def impute_mean(self, G, locus_col, n: int | None = None):
        """mean_imputation (mean_imputation.rs:6-41), in place."""
        p, ld, n, lc, L = self._impute_args(G, locus_col, n)
        self._check(self._lib.pg_impute_mean_dev(self._ctx, self._dev(G, torch.float64), p, n, ld, lc.ctypes.data, L), "pg_impute_mean_dev")

    def impute_aldknn(self, G, locus_col, win_head, win_tail, n_loci_to_estimate_distance: int = 10, k_neighbours: int = 5,
                      scratch_bytes: int = 0, n: int | None = None) -> torch.Tensor:
        """adaptive_ld_knn_imputation (adaptive_ld_knn_imputation.rs:174-341) -> the imputed copy of G.  scratch_bytes bounds
        the device memory of one batch of windows (0: 1 GiB)."""
        p, ld, n, lc, L = self._impute_args(G, locus_col, n)
        wh = np.ascontiguousarray(win_head, dtype=np.int64); wt = np.ascontiguousarray(win_tail, dtype=np.int64)
        out = torch.empty_like(G)
        self._check(self._lib.pg_impute_aldknn_dev(self._ctx, self._dev(G, torch.float64), p, n, ld, lc.ctypes.data, L, wh.ctypes.data,
                                                   wt.ctypes.data, len(wh), int(n_loci_to_estimate_distance), int(k_neighbours),
                                                   int(scratch_bytes), out.data_ptr()), "pg_impute_aldknn_dev")
        return out

    def impute_mark_cov(self, cov, locus_col, n: int | None = None):
        """NaN coverages of the loci that have a coverage at all become +inf (mean_imputation.rs:42-59), in place."""
        p, ld, n, lc, L = self._impute_args(cov, locus_col, n)
        self._check(self._lib.pg_impute_mark_cov_dev(self._ctx, self._dev(cov, torch.float64), p, n, ld, lc.ctypes.data, L),
                    "pg_impute_mark_cov_dev")

    def impute(self, G, cov, locus_col, chrom_ids=None, pos=None, method: str = "mean", min_depth_set_to_missing: float = 5.0,
               frac_top_missing_pools: float = 0.1, frac_top_missing_loci: float = 0.1, window_size_bp: int = 100,
               window_slide_size_bp: int = 50, min_loci_per_window: int = 10, n_loci_to_estimate_distance: int = 10,
               k_neighbours: int = 5, col_locus=None, col_allele=None, scratch_bytes: int = 0, n: int | None = None):
        """impute_mean / impute_aLDkNN (mean_imputation.rs:65-162, adaptive_ld_knn_imputation.rs:371-477) from the loaded
        matrix to the table the writer prints: missing by depth, the sparsest pools and loci out, the imputation, the coverage
        mark, the loci still missing everywhere out.  G and cov are not modified.  chrom_ids / pos: per locus, for the windows
        of "aLD-kNNi".  Returns a dict: G, cov (imputed, kept part), pools and loci (kept indices into the input), locus_col,
        col_locus / col_allele (labels of the kept columns when given), missing_rate (percent after every step, as the
        reference prints them)."""
        if method not in ("mean", "aLD-kNNi"):
            raise ValueError("impute: method must be 'mean' or 'aLD-kNNi'")
        rates = []

        def note(G_, cov_, lc_):
            ln = self.missingness(G_, cov_, lc_, n=n_now)[1]
            rates.append(_sensible_round(float(ln.sum()) * 100.0 / float(n_now * len(ln)), 2))
            return ln

        n_now = self._g_dims(G, n)[2]
        G = G.clone(); cov = cov.clone()
        lc = np.ascontiguousarray(locus_col, dtype=np.int64)
        note(G, cov, lc)
        self.set_missing_by_depth(G, cov, lc, min_depth_set_to_missing, n=n_now)
        pool_nan, locus_nan = self.missingness(G, cov, lc, n=n_now)
        rates.append(_sensible_round(float(locus_nan.sum()) * 100.0 / float(n_now * len(locus_nan)), 2))
        pools = self.top_missing_keep(pool_nan, frac_top_missing_pools, "pools")
        all_loci = np.arange(len(lc) - 1, dtype=np.int64)
        G, cov, lc, col_locus, col_allele = self.impute_compact(G, cov, lc, pools, all_loci, col_locus, col_allele, n=n_now)
        n_now = len(pools)
        locus_nan = note(G, cov, lc)
        loci = self.top_missing_keep(locus_nan, frac_top_missing_loci, "loci")
        G, cov, lc, col_locus, col_allele = self.impute_compact(G, cov, lc, np.arange(n_now), loci, col_locus, col_allele, n=n_now)
        note(G, cov, lc)
        if method == "mean":
            self.impute_mean(G, lc, n=n_now)
        else:
            if chrom_ids is None or pos is None:
                raise ValueError("impute: aLD-kNNi needs chrom_ids and pos of the loci")
            ch = np.ascontiguousarray(chrom_ids, dtype=np.int32)[loci]; po = np.ascontiguousarray(pos, dtype=np.uint64)[loci]
            head, tail = self.sliding_windows(ch, po, window_size_bp, window_slide_size_bp, min_loci_per_window)
            G = self.impute_aldknn(G, lc, head, tail, n_loci_to_estimate_distance, k_neighbours, scratch_bytes, n=n_now)
        self.impute_mark_cov(cov, lc, n=n_now)
        locus_nan = note(G, cov, lc)
        keep2 = self.top_missing_keep(locus_nan, 1.0, "loci")
        G, cov, lc, col_locus, col_allele = self.impute_compact(G, cov, lc, np.arange(n_now), keep2, col_locus, col_allele, n=n_now)
        note(G, cov, lc)
        return dict(G=G, cov=cov, pools=pools, loci=loci[keep2], locus_col=lc, col_locus=col_locus, col_allele=col_allele,
                    missing_rate=rates)

    # ---- popgen -------------------------------------------------------------------------------
    def sliding_windows(self, chrom_ids, pos, window_size_bp: int, window_slide_size_bp: int, min_loci_per_window: int):
        """define_sliding_windows (base/helpers.rs:294-403) -> (head, tail) inclusive locus index ranges."""
        ch = np.ascontiguousarray(chrom_ids, dtype=np.int32)
        po = np.ascontiguousarray(pos, dtype=np.uint64)
        head = np.empty(max(len(ch), 1), dtype=np.int64); tail = np.empty(max(len(ch), 1), dtype=np.int64)
        nw = self._lib.pg_host_sliding_windows(ch.ctypes.data, po.ctypes.data, len(ch), int(window_size_bp),
                                               int(window_slide_size_bp), int(min_loci_per_window), head.ctypes.data,
                                               tail.ctypes.data)
        return head[:nw].copy(), tail[:nw].copy()

    def _popgen_args(self, G, cov, locus_col, win_head, win_tail, n):
        p, ld, n = self._g_dims(G, n)
        assert cov.shape == G.shape
        lc = np.ascontiguousarray(locus_col, dtype=np.int64)
        wh = np.ascontiguousarray(win_head, dtype=np.int64); wt = np.ascontiguousarray(win_tail, dtype=np.int64)
        return p, ld, n, lc, wh, wt

    def watterson_windows(self, chrom_ids, pos, window_size_bp: int, window_slide_size_bp: int, min_loci_per_window: int):
        """theta_watterson's own window loop (popgen/watterson_theta.rs:56-164) -> (head, tail, cov, seed, slot): head/tail
        as sliding_windows; cov, seed, slot describe the reference's segregating-site count (include/poolgen_hip.h)."""
        ch = np.ascontiguousarray(chrom_ids, dtype=np.int32)
        po = np.ascontiguousarray(pos, dtype=np.uint64)
        out = [np.empty(max(len(ch), 1), dtype=np.int64) for _ in range(5)]
        nw = self._lib.pg_host_watterson_windows(ch.ctypes.data, po.ctypes.data, len(ch), int(window_size_bp),
                                                 int(window_slide_size_bp), int(min_loci_per_window),
                                                 *[o.ctypes.data for o in out])
        return tuple(o[:nw].copy() for o in out)

    @staticmethod
    def _count_args(count, nw):
        """count = None: counted mode (three NULLs); else (cov, seed, slot) per window: the reference's count."""
        if count is None:
            return [None, None, None], []
        keep = [np.ascontiguousarray(c, dtype=np.int64) for c in count]
        if len(keep) != 3 or any(len(c) != nw for c in keep):
            raise ValueError("count must be (cov, seed, slot), one entry per window each")
        return [c.ctypes.data for c in keep], keep

    # One marshalling per statistic, shared by its two forms: `fn` names the C entry point, `new(shape, dtype)` allocates an
    # output -- _on_host for the host forms (numpy), _on_device for the tables forms: the same arguments, the same bits, but
    # the results are CUDA tensors that never touched the host.
    _on_host = staticmethod(np.empty)

    def _on_device(self, shape, dtype=np.float64):
        return torch.empty(shape, dtype=torch.float64 if dtype is np.float64 else torch.int64, device=torch.device("cuda", self.device))

    @staticmethod
    def _ptr(a):
        return a.data_ptr() if isinstance(a, torch.Tensor) else a.ctypes.data

    def _theta_pi(self, fn, new, G, cov, locus_col, win_head, win_tail, n):
        p, ld, n, lc, wh, wt = self._popgen_args(G, cov, locus_col, win_head, win_tail, n)
        win = new((len(wh), n)); mean = new((n,))
        self._check(getattr(self._lib, fn)(self._ctx, self._dev(G, torch.float64), self._dev(cov, torch.float64), p, n, ld,
                                           lc.ctypes.data, len(lc) - 1, wh.ctypes.data, wt.ctypes.data, len(wh),
                                           self._ptr(win), self._ptr(mean)), fn)
        return win, mean

    def _fst(self, fn, new, G, cov, locus_col, win_head, win_tail, n):
        p, ld, n, lc, wh, wt = self._popgen_args(G, cov, locus_col, win_head, win_tail, n)
        mean = new((n, n)); win = new((len(wh), n * n))
        self._check(getattr(self._lib, fn)(self._ctx, self._dev(G, torch.float64), self._dev(cov, torch.float64), p, n, ld,
                                           lc.ctypes.data, len(lc) - 1, wh.ctypes.data, wt.ctypes.data, len(wh),
                                           self._ptr(mean), self._ptr(win) if len(wh) else None), fn)
        return mean, win

    def _diversity(self, fn, new, G, cov, locus_col, win_head, win_tail, pool_sizes, count, n):
        """theta_watterson (cov is None: the entry point takes no coverages) and tajima_d"""
        p, ld, n, lc, wh, wt = self._popgen_args(G, G if cov is None else cov, locus_col, win_head, win_tail, n)
        ps = _host_f64(pool_sizes)
        assert len(ps) == n
        cptr, keep = self._count_args(count, len(wh))
        matrix = [self._dev(G, torch.float64)] + ([] if cov is None else [self._dev(cov, torch.float64)])
        win = (len(wh), n)  # D, mean, theta_W, pi -- or theta_W, mean, S
        out = [new(win), new((n,))] + ([new(win, np.int64)] if cov is None else [new(win), new(win)])
        self._check(getattr(self._lib, fn)(self._ctx, *matrix, p, n, ld, lc.ctypes.data, len(lc) - 1, wh.ctypes.data, wt.ctypes.data,
                                           *cptr, len(wh), ps.ctypes.data, *[self._ptr(o) for o in out]), fn)
        return tuple(out)

    def theta_pi(self, G, cov, locus_col, win_head, win_tail, n: int | None = None):
        """popgen::theta_pi (popgen/pi.rs:10-113): (pi per window [n_windows x n], mean across windows [n])."""
        return self._theta_pi("pg_pi_dev", self._on_host, G, cov, locus_col, win_head, win_tail, n)

    def theta_pi_tables(self, G, cov, locus_col, win_head, win_tail, n: int | None = None):
        """theta_pi with its results left on the device (pg_pi_tables_dev): (pi per window [n_windows x n], mean [n])."""
        return self._theta_pi("pg_pi_tables_dev", self._on_device, G, cov, locus_col, win_head, win_tail, n)

    def fst(self, G, cov, locus_col, win_head, win_tail, n: int | None = None):
        """popgen::fst (popgen/fst.rs:10-115, :158-200): (genome-wide mean [n x n], per window [n_windows x n*n])."""
        return self._fst("pg_fst_dev", self._on_host, G, cov, locus_col, win_head, win_tail, n)

    def fst_tables(self, G, cov, locus_col, win_head, win_tail, n: int | None = None):
        """fst with its results left on the device (pg_fst_tables_dev): (genome-wide mean [n x n], per window [n_windows x n*n])."""
        return self._fst("pg_fst_tables_dev", self._on_device, G, cov, locus_col, win_head, win_tail, n)

    def theta_watterson(self, G, locus_col, win_head, win_tail, pool_sizes, count=None, n: int | None = None):
        """popgen::theta_watterson (popgen/watterson_theta.rs:36-188): (theta_W per window [n_windows x n], mean across
        windows [n], segregating sites per window [n_windows x n]).  count = (cov, seed, slot) of watterson_windows
        reproduces the reference's count; None counts the polymorphic loci of each window.  pool_sizes are used as given."""
        return self._diversity("pg_watterson_dev", self._on_host, G, None, locus_col, win_head, win_tail, pool_sizes, count, n)

    def theta_watterson_tables(self, G, locus_col, win_head, win_tail, pool_sizes, count=None, n: int | None = None):
        """theta_watterson with its results left on the device (pg_watterson_tables_dev): (theta_W per window, mean, S per window)."""
        return self._diversity("pg_watterson_tables_dev", self._on_device, G, None, locus_col, win_head, win_tail, pool_sizes, count, n)

    def tajima_d(self, G, cov, locus_col, win_head, win_tail, pool_sizes, count=None, n: int | None = None):
        """popgen::tajima_d (popgen/tajima_d.rs:10-96) in one pass over G: (D per window [n_windows x n], mean across
        windows [n], theta_W per window, pi per window).  count as for theta_watterson."""
        return self._diversity("pg_tajima_d_dev", self._on_host, G, cov, locus_col, win_head, win_tail, pool_sizes, count, n)

    def tajima_d_tables(self, G, cov, locus_col, win_head, win_tail, pool_sizes, count=None, n: int | None = None):
        """tajima_d with its results left on the device (pg_tajima_d_tables_dev): (D per window, mean, theta_W, pi per window)."""
        return self._diversity("pg_tajima_d_tables_dev", self._on_device, G, cov, locus_col, win_head, win_tail, pool_sizes, count, n)

    def _table(self, a) -> torch.Tensor:
        """a 2-D fp64 table (numpy or torch) as a contiguous tensor on this engine's GPU"""
        dev = torch.device("cuda", self.device)
        t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.array(a, dtype=np.float64, order="C"))  # a copy: writable
        t = t.to(device=dev, dtype=torch.float64).contiguous()
        if t.dim() != 2:
            raise ValueError("expected a 2-D table")
        return t

    def normal_fit(self, table):
        """The normal fit of popgen::gudmc (ml_normal_1d, popgen/gudmc.rs:39-60) to every column of a rows x cols table over
        its non-NaN entries: (mu [cols], sd [cols], count [cols] int64, iters [cols] int32), CUDA tensors."""
        t = self._table(table)
        rows, cols = t.shape
        if cols < 1:
            raise ValueError("normal_fit: the table has no columns")
        mu = torch.empty(cols, dtype=torch.float64, device=t.device); sd = torch.empty_like(mu)
        count = torch.empty(cols, dtype=torch.int64, device=t.device)
        iters = torch.empty(cols, dtype=torch.int32, device=t.device)
        self._check(self._lib.pg_normal_fit_dev(self._ctx, t.data_ptr() if rows else None, rows, cols, cols, mu.data_ptr(),
                                                sd.data_ptr(), count.data_ptr(), iters.data_ptr()), "pg_normal_fit_dev")
        return mu, sd, count, iters

    def gudmc_from_tables(self, d_win, fst_win, win_chr, win_ini, win_fin, sigma_threshold: float = 2.0,
                          recombination_rate_cM_per_Mb: float = 0.73) -> dict:
        """popgen::gudmc (popgen/gudmc.rs:64-462) from D per window [w x n] and Fst per window [w x n*n] (tajima_d's and
        fst's tables) and the windows' chromosome ids, first and last positions.  Returns CUDA tensors: rows [n], d_mean,
        d_sd [n]; fst_mean, fst_sd, width_mean, width_sd [n*n]; and per (pair, row) [n*n x w], specified for
        row < rows[pair % n]: window, d, width, width_dev, width_p, fst_delta, fst_p."""
        d = self._table(d_win); f = self._table(fst_win)
        w, n = d.shape
        if f.shape != (w, n * n):
            raise ValueError("gudmc: fst_win must be w x n*n for a w x n d_win")
        ch = np.ascontiguousarray(win_chr, dtype=np.int32)
        ini = np.ascontiguousarray(win_ini, dtype=np.uint64); fin = np.ascontiguousarray(win_fin, dtype=np.uint64)
        if not (len(ch) == len(ini) == len(fin) == w):
            raise ValueError("gudmc: win_chr, win_ini and win_fin need one entry per window")
        dev = d.device
        f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
        out = dict(rows=torch.empty(n, dtype=torch.int64, device=dev), d_mean=f64(n), d_sd=f64(n), fst_mean=f64(n * n),
                   fst_sd=f64(n * n), width_mean=f64(n * n), width_sd=f64(n * n),
                   window=torch.empty((n * n, w), dtype=torch.int64, device=dev), d=f64(n * n, w), width=f64(n * n, w),
                   width_dev=f64(n * n, w), width_p=f64(n * n, w), fst_delta=f64(n * n, w), fst_p=f64(n * n, w))
        self._check(self._lib.pg_gudmc_dev(self._ctx, d.data_ptr(), f.data_ptr(), w, n, ch.ctypes.data, ini.ctypes.data,
                                           fin.ctypes.data, float(sigma_threshold), float(recombination_rate_cM_per_Mb),
                                           *[t.data_ptr() for t in out.values()]), "pg_gudmc_dev")
        return out

    def gudmc(self, G, cov, locus_col, win_head, win_tail, win_chr, win_ini, win_fin, pool_sizes,
              sigma_threshold: float = 2.0, recombination_rate_cM_per_Mb: float = 0.73, count=None, n: int | None = None) -> dict:
        """tajima_d_tables, fst_tables and gudmc_from_tables in one call; count as for tajima_d.  The two tables stay on the
        device from the kernels that write them to the one that reads them."""
        d_win = self.tajima_d_tables(G, cov, locus_col, win_head, win_tail, pool_sizes, count=count, n=n)[0]
        fst_win = self.fst_tables(G, cov, locus_col, win_head, win_tail, n=n)[1]
        return self.gudmc_from_tables(d_win, fst_win, win_chr, win_ini, win_fin, sigma_threshold, recombination_rate_cM_per_Mb)

    # ---- genomic prediction -------------------------------------------------------------------
    def gp_xxt(self, G: torch.Tensor, n: int | None = None) -> torch.Tensor:
        p, ld, n = self._g_dims(G, n)
        S = torch.empty((n, n), dtype=torch.float64, device=G.device)
        self._check(self._lib.pg_gp_xxt_dev(self._ctx, self._dev(G, torch.float64), p, n, ld,
                                            S.data_ptr()), "pg_gp_xxt_dev")
        return S

    def gp_ols(self, G: torch.Tensor, Y, row_idx, XXt=None, n: int | None = None):
        p, ld, n = self._g_dims(G, n)
        Yh = _host_f64(Y).reshape(n, -1)
        k = Yh.shape[1]
        ri = np.ascontiguousarray(np.asarray(row_idx, dtype=np.int64))
        beta = torch.empty((p + 1, k), dtype=torch.float64, device=G.device)
        xptr = None
        if XXt is not None:
            XXt = _host_f64(XXt)
            xptr = XXt.ctypes.data
        self._check(self._lib.pg_gp_ols_dev(self._ctx, self._dev(G, torch.float64), p, n, ld,
                                            Yh.ctypes.data, k, ri.ctypes.data, len(ri), xptr,
                                            beta.data_ptr()), "pg_gp_ols_dev")
        return beta

    def gp_predict(self, G: torch.Tensor, beta: torch.Tensor, n: int | None = None) -> np.ndarray:
        """yhat = [1 | G^T] beta for every pool (n x k on the host)."""
        p, ld, n = self._g_dims(G, n)
        k = beta.shape[1]
        yhat = np.empty((n, k))
        self._check(self._lib.pg_gp_predict_dev(self._ctx, self._dev(G, torch.float64), p, n, ld,
                                                self._dev(beta, torch.float64), k, yhat.ctypes.data), "pg_gp_predict_dev")
        return yhat

    def gp_penalised(self, G: torch.Tensor, Y, row_idx, fold_of, n_folds: int, alpha: float, iterative_proxy: bool = False,
                     lambda_step: float = 0.1, n: int | None = None, XXt=None):
        """Every model behind penalised_lambda_path_with_k_fold_cross_validation (gp/penalise.rs:461-669): alpha in
        [0, 1] one lambda path, alpha < 0 the alpha x lambda grid of penalise_glmnet, iterative_proxy the
        *_with_iterative_proxy_norms variants.  Returns (beta (1+p) x k on the device, alphas[k], lambdas[k],
        perf[n_reps, n_folds, A, L, k])."""
        p, ld, n = self._g_dims(G, n)
        Yh = _host_f64(Y).reshape(n, -1)
        k = Yh.shape[1]
        ri = np.ascontiguousarray(np.asarray(row_idx, dtype=np.int64))
        fo = np.ascontiguousarray(np.asarray(fold_of, dtype=np.int32)).reshape(-1, len(ri))
        L = int(round(1.0 / lambda_step)) + 1
        A = 1 if alpha >= 0 else L
        beta = torch.empty((p + 1, k), dtype=torch.float64, device=G.device)
        al, lam = np.empty(k), np.empty(k)
        perf = np.empty((fo.shape[0], n_folds, A, L, k))
        xh = None if XXt is None else _host_f64(XXt)   # kept alive across the call
        self._check(self._lib.pg_gp_penalised_dev(self._ctx, self._dev(G, torch.float64), p, n, ld, Yh.ctypes.data, k,
                                                  ri.ctypes.data, len(ri), fo.ctypes.data, fo.shape[0], int(n_folds),
                                                  float(alpha), int(bool(iterative_proxy)), float(lambda_step),
                                                  beta.data_ptr(), al.ctypes.data, lam.ctypes.data, perf.ctypes.data,
                                                  None if xh is None else xh.ctypes.data),
                    "pg_gp_penalised_dev")
        return beta, al, lam, perf

    def gp_proxy(self, G: torch.Tensor, Y, row_idx, n: int | None = None) -> torch.Tensor:
        """ols_iterative_with_kinship_pca_covariate (gp/ols.rs:104-199): (1+p) x k on the device."""
        p, ld, n = self._g_dims(G, n)
        Yh = _host_f64(Y).reshape(n, -1)
        k = Yh.shape[1]
        ri = np.ascontiguousarray(np.asarray(row_idx, dtype=np.int64))
        out = torch.empty((p + 1, k), dtype=torch.float64, device=G.device)
        self._check(self._lib.pg_gp_proxy_dev(self._ctx, self._dev(G, torch.float64), p, n, ld, Yh.ctypes.data, k,
                                              ri.ctypes.data, len(ri), None, out.data_ptr()), "pg_gp_proxy_dev")
        return out

    def gp_ridge(self, G: torch.Tensor, Y, row_idx, fold_of, n_folds: int, alpha: float = 0.0,
                 lambda_step: float = 0.1, n: int | None = None):
        """penalise_ridge_like (gp/penalise.rs:133-159) with explicit folds: fold_of is (n_reps, len(row_idx)).
        Returns (beta (1+p) x k on the device, lambdas[k], perf[n_reps, n_folds, L, k])."""
        p, ld, n = self._g_dims(G, n)
        Yh = _host_f64(Y).reshape(n, -1)
        k = Yh.shape[1]
        ri = np.ascontiguousarray(np.asarray(row_idx, dtype=np.int64))
        fo = np.ascontiguousarray(np.asarray(fold_of, dtype=np.int32)).reshape(-1, len(ri))
        L = int(round(1.0 / lambda_step)) + 1
        beta = torch.empty((p + 1, k), dtype=torch.float64, device=G.device)
        lam = np.empty(k)
        perf = np.empty((fo.shape[0], n_folds, L, k))
        self._check(self._lib.pg_gp_ridge_dev(self._ctx, self._dev(G, torch.float64), p, n, ld, Yh.ctypes.data, k,
                                              ri.ctypes.data, len(ri), fo.ctypes.data, fo.shape[0], int(n_folds),
                                              float(alpha), float(lambda_step), beta.data_ptr(), lam.ctypes.data,
                                              perf.ctypes.data), "pg_gp_ridge_dev")
        return beta, lam, perf
