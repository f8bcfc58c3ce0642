"""pg_host_result_rows and pg_host_kinship_rows, the plain C++ twins of the device result writer (pg_result_rows_dev,
pg_kinship_rows_dev): against the restatement of the rows (tests/resultfmt_ref.py over tests/rustfmt.py), against hand-written
bytes for each of the six row kinds, their buffer contract, their refusals, thread-count independence -- and the host translation
unit on its own under the address and undefined-behaviour sanitizers.  Runs without a GPU."""
import ctypes as C
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

import f64_corpus as FC
import resultfmt_ref as RR

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "poolgen_amd" / "csrc"
PG_OK, PG_ERR_INVALID = 0, -1


def host_rows(g, n_threads=1):
    from poolgen_amd import result_rows_host
    op, n_out, ids, freq, stat, pval, chrom, pos, names, k = RR.args_of(g)
    return result_rows_host(op, n_out, ids, freq, stat, pval, chrom, pos, names, k=k, n_threads=n_threads)


def host_kinship(g, row0=0, rows=None, n_threads=1):
    from poolgen_amd import kinship_rows_host
    return kinship_rows_host(*RR.kinship_args_of(g), row0=row0, rows=rows, n_threads=n_threads)


@pytest.fixture(scope="module")
def cases():
    """(inputs, the restatement's text) per row kind and trait count, computed once"""
    out = []
    for i, op in enumerate(RR.OPS):
        for k in ((1, 2, 3) if op in ("pearson_corr", "ols_iter") else (1,)):
            g = RR.generated(op, 700, k, seed=300 + 10 * i + k)
            out.append((g, RR.result_rows(*RR.args_of(g))))
    return out


# ---- hand-written bytes for each of the six row kinds -------------------------------------------------------------------------
def lit(op, k=1):
    """two loci (the first with two alleles kept, the second dropped) and a third with one"""
    L = 3
    n_out = np.array([2, 0, 1], dtype=np.int32)
    ids = np.zeros(5 * L, dtype=np.int32); ids[0] = 0; ids[L] = 3; ids[2] = 2          # locus 0: A, G; locus 2: C
    freq = np.zeros(5 * L); freq[0] = 0.123456789; freq[L] = 0.25; freq[2] = 2.0 / 3.0
    per_locus = op in ("fisher_exact_test", "chisq_test")
    if per_locus:
        stat = np.array([12.3456789, 0.0, 0.1]); pval = np.array([0.5223146158470686, 0.0, 1e-300])
    else:
        stat = np.zeros(5 * L * k); pval = np.zeros(5 * L * k)
        for e, base in ((0, 1.23456789), (L, -0.000001234), (2, 1e23)):
            for j in range(k):
                stat[e * k + j] = base * (j + 1); pval[e * k + j] = (0.7797774084757156, 7.797774084757156e-08)[j]
    return dict(op=op, k=k, n_out=n_out, ids=ids, freq=None if per_locus else freq, stat=stat, pval=None if op == "gwalpha" else pval,
                chrom=np.array([0, 0, 1], dtype=np.int32), pos=np.array([456, 457, 18446744073709551615], dtype=np.uint64), names=["chr1", "X"])


ROW_LITERALS = [
    (lit("fisher_exact_test"), b"chr1,456,AG,12.3456789,0.5223146158470686\n" b"X,18446744073709551615,C,0.1,0." + b"0" * 299 + b"1\n"),
    (lit("chisq_test"), b"chr1,456,AG,12.345679,0.5223146158470686\n" b"X,18446744073709551615,C,0.1,0." + b"0" * 299 + b"1\n"),
    (lit("gwalpha"), b"chr1,456,A,0.123457,Pheno_0,1.234568,Unknown\n" b"chr1,456,G,0.25,Pheno_0,-0.000001,Unknown\n"
                     b"X,18446744073709551615,C,0.666667,Pheno_0,100000000000000000000000,Unknown\n"),
    (lit("pearson_corr", 2), b"chr1,456,A,0.123456789,Pheno_0,1.234568,0.7797774084757156\n" b"chr1,456,A,0.123456789,Pheno_1,2.469136,0.00000007797774084757156\n"
                             b"chr1,456,G,0.25,Pheno_0,-0.000001,0.7797774084757156\n" b"chr1,456,G,0.25,Pheno_1,-0.000002,0.00000007797774084757156\n"
                             b"X,18446744073709551615,C,0.6666666666666666,Pheno_0,100000000000000000000000,0.7797774084757156\n"
                             b"X,18446744073709551615,C,0.6666666666666666,Pheno_1,200000000000000000000000,0.00000007797774084757156\n"),
    (lit("ols_iter", 2), b"chr1,456,A,0.12345679,Pheno_0,1.234568,0.779777408476\n" b"chr1,456,A,0.12345679,Pheno_1,2.469136,0.000000077978\n"
                         b"chr1,456,G,0.25,Pheno_0,-0.000001,0.779777408476\n" b"chr1,456,G,0.25,Pheno_1,-0.000002,0.000000077978\n"
                         b"X,18446744073709551615,C,0.66666667,Pheno_0,100000000000000000000000,0.779777408476\n"
                         b"X,18446744073709551615,C,0.66666667,Pheno_1,200000000000000000000000,0.000000077978\n"),
]
KIN_LITERAL = (dict(beta=np.array([[1.5, -2.0], [0.001, 1e22], [3.0, 0.1]]), pval=np.array([[0.5, 1.0], [1e-10, 0.0], [float("nan"), 0.25]]),
                    col_chrom=np.array([1, 0], dtype=np.int32), col_pos=np.array([77, 5], dtype=np.uint64), col_allele=np.array([5, 1], dtype=np.int32),
                    names=["a", "chrB"]),
               b"intercept,0,intercept,Pheno_0,1.5,0.5\n" b"chrB,77,D,Pheno_0,0.001,0.0000000001\n" b"a,5,T,Pheno_0,3,NaN\n"
               b"intercept,0,intercept,Pheno_1,-2,1\n" b"chrB,77,D,Pheno_1,10000000000000000000000,0\n" b"a,5,T,Pheno_1,0.1,0.25\n")


def test_literals(native):
    for g, want in ROW_LITERALS:
        assert RR.result_rows(*RR.args_of(g)) == want, g["op"]               # the restatement against the hand-written bytes
        assert host_rows(g) == want, g["op"]                                  # the host twin against them
    g, want = KIN_LITERAL
    assert RR.kinship_rows(*RR.kinship_args_of(g)) == want and host_kinship(g) == want
    assert host_kinship(g, 1, 3) == b"".join(want.splitlines(True)[1:4])      # the last column's label (a second "a" row) never appears


def test_host_twin_equals_restatement_on_any_number_of_threads(native, cases):
    for g, want in cases:
        assert len(want) > 20_000
        for threads in (1, 3, 16):
            assert host_rows(g, threads) == want, (g["op"], g["k"], threads)


def test_kinship_rows_equal_restatement_and_parts_concatenate(native):
    for p, k in ((1, 1), (1, 3), (2, 1), (2, 2), (7, 3), (1000, 2)):
        g = RR.generated_kinship(p, k, seed=50 + p + k)
        want = RR.kinship_rows(*RR.kinship_args_of(g))
        for threads in (1, 3, 16):
            assert host_kinship(g, n_threads=threads) == want, (p, k, threads)
        assert want.startswith(b"intercept,0,intercept,Pheno_0,") and want.count(b"intercept,0,intercept") == k
    g = RR.generated_kinship(4, 3, seed=9)
    whole = host_kinship(g)
    lines = whole.splitlines(True)
    for row0 in range(13):
        for rows in range(13 - row0):
            assert host_kinship(g, row0, rows, n_threads=2) == b"".join(lines[row0:row0 + rows]), (row0, rows)


def raw_rows(native, g, buf, cap, threads=2, **change):
    """the C entry point itself -> (rc, bytes); `change` replaces arguments by name"""
    from poolgen_amd.engine import RESULT_OPS, name_table
    text, off = name_table(g["names"])
    a = dict(op=RESULT_OPS[g["op"]], L=len(g["n_out"]), k=g["k"], n_out=g["n_out"], ids=g["ids"], freq=g["freq"], stat=g["stat"], pval=g["pval"],
             chrom=g["chrom"], pos=g["pos"], text=text, off=off, n_chrom=len(off) - 1)
    a.update(change)
    ptr = lambda v: None if v is None else v.ctypes.data
    need = C.c_int64(-7)
    rc = native.pg_host_result_rows(a["op"], a["L"], a["k"], ptr(a["n_out"]), ptr(a["ids"]), ptr(a["freq"]), ptr(a["stat"]), ptr(a["pval"]), ptr(a["chrom"]),
                                    ptr(a["pos"]), ptr(a["text"]), ptr(a["off"]), a["n_chrom"], ptr(buf), cap, C.byref(need), threads)
    return rc, need.value


def test_size_query_exact_capacity_one_short_canary_and_alignment(native, cases):
    for g, want in cases[::2]:
        assert raw_rows(native, g, None, 0) == (PG_ERR_INVALID, len(want))          # the size query (the text needs more than 0 bytes)
        buf = np.full(len(want) + 64, 0xAA, dtype=np.uint8)
        assert raw_rows(native, g, buf, len(want) - 1) == (PG_ERR_INVALID, len(want)) and (buf == 0xAA).all()
        for cap in (len(want), len(want) + 64):
            buf[:] = 0xAA
            assert raw_rows(native, g, buf, cap) == (PG_OK, len(want))
            assert buf[:len(want)].tobytes() == want and (buf[len(want):] == 0xAA).all()
    g, want = cases[0]
    for off in range(16):
        b = np.full(len(want) + 32, 0xAA, dtype=np.uint8)
        v = b[off:]
        assert raw_rows(native, g, v, len(want)) == (PG_OK, len(want))
        assert v[:len(want)].tobytes() == want and (b[:off] == 0xAA).all() and (v[len(want):] == 0xAA).all()


def test_refused_inputs(native):
    g = RR.generated("ols_iter", 40, 2, seed=4, realistic=True)
    g["n_out"] = np.maximum(g["n_out"], 1); g["ids"] = np.minimum(g["ids"], 5)   # every locus kept (the junk ids of dropped loci made valid)
    want = RR.result_rows(*RR.args_of(g))
    buf = np.full(len(want) + 8, 0xAA, dtype=np.uint8)

    def refused(**change):
        buf[:] = 0xAA
        assert raw_rows(native, g, buf, buf.size, **change) == (PG_ERR_INVALID, 0) and (buf == 0xAA).all(), change

    def altered(key, index, value):
        a = g[key].copy(); a[index] = value
        return {key: a}

    assert raw_rows(native, g, buf, buf.size) == (PG_OK, len(want))
    refused(**altered("chrom", 7, -1))
    refused(**altered("chrom", 7, len(g["names"])))                          # one past the name table
    refused(**altered("ids", 7, 6))                                           # slot 0 of locus 7
    refused(**altered("ids", 7, -1))
    from poolgen_amd.engine import name_table
    off = name_table(g["names"])[1].copy(); off[2] = off[1] - 1               # offsets that decrease
    refused(off=off)
    off = name_table(g["names"])[1].copy(); off[0] = -1
    refused(off=off)
    for change in (dict(op=-1), dict(op=5), dict(L=-1), dict(k=0), dict(k=4097), dict(n_chrom=-1), dict(n_out=None), dict(ids=None), dict(freq=None),
                   dict(stat=None), dict(pval=None), dict(chrom=None), dict(pos=None), dict(off=None), dict(text=None)):
        refused(**change)
    assert raw_rows(native, g, buf, -1) == (PG_ERR_INVALID, 0)
    assert raw_rows(native, g, None, 5) == (PG_ERR_INVALID, 0)                # a capacity without a buffer
    # a label of a dropped locus is never read: out of range there is fine
    ok = dict(g); n0 = g["n_out"].copy(); n0[7] = 0; ok["n_out"] = n0
    ok.update(altered("chrom", 7, 99))
    assert raw_rows(native, ok, buf, buf.size)[0] == PG_OK
    # L = 0: PG_OK, bytes = 0, whatever the pointers
    buf[:] = 0xAA
    assert raw_rows(native, g, buf, buf.size, L=0) == (PG_OK, 0) and (buf == 0xAA).all()
    # gwalpha needs no pval, the per-locus kinds no freq
    gw = RR.generated("gwalpha", 30, 1, seed=2)
    assert gw["pval"] is None and host_rows(gw) == RR.result_rows(*RR.args_of(gw))
    # the row limit: a locus whose text passes 2^22 bytes (a name of 2^22 bytes) is refused, without a size
    long = dict(g); long["names"] = ["n" * RR.UNIT_MAX] + g["names"][1:]
    assert raw_rows(native, long, None, 0) == (PG_ERR_INVALID, 0)
    # kinship: rows outside k * p, p < 1, k out of range
    kg = RR.generated_kinship(5, 2, seed=1)
    from poolgen_amd import NativeError, kinship_rows_host
    for row0, rows in ((0, 11), (10, 1), (-1, 2), (3, -1)):
        with pytest.raises(NativeError):
            kinship_rows_host(*RR.kinship_args_of(kg), row0=row0, rows=rows)
    assert host_kinship(kg, 10, 0) == b""
    bad = dict(kg); a = kg["col_allele"].copy(); a[0] = 6; bad["col_allele"] = a
    with pytest.raises(NativeError):
        host_kinship(bad)
    assert host_kinship(bad, 0, 1).startswith(b"intercept")                   # the bad label is not among the rows asked for
    last = dict(kg); a = kg["col_chrom"].copy(); a[-1] = 99; last["col_chrom"] = a
    assert host_kinship(last) == host_kinship(kg)                             # the last column's label is never read


# ---- the host translation unit on its own, under the address and undefined-behaviour sanitizers ------------------------------------
SANITIZER_MAIN = r"""
#include "poolgen_hip.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
// input: cases as raw little-endian blocks (written by the test); every buffer is a heap block of exactly the size stated, so that a
// byte read or written outside one is an error the sanitizer reports
static FILE *f;
static long long i64() { long long v; if (std::fread(&v, 8, 1, f) != 1) std::exit(2); return v; }
static void *block(long long bytes) {
    void *p = std::malloc(bytes ? bytes : 1);
    if (bytes && std::fread(p, 1, bytes, f) != (size_t)bytes) std::exit(2);
    return p;
}
template <class Call> static int check(Call call, const char *want, long long want_bytes) {
    for (int threads : {1, 3}) {
        int64_t need = -7;
        int rc = call(nullptr, 0, &need, threads);
        if (need != want_bytes || (rc != PG_OK) != (want_bytes > 0)) { std::fprintf(stderr, "size %lld, want %lld\n", (long long)need, want_bytes); return 1; }
        char *text = (char *)std::malloc(want_bytes ? want_bytes : 1);   // sized exactly
        rc = call(text, want_bytes, &need, threads);
        if (rc != PG_OK || need != want_bytes || std::memcmp(text, want, want_bytes) != 0) { std::fprintf(stderr, "text differs\n"); return 1; }
        std::free(text);
        if (want_bytes > 1) {                                           // one byte short: nothing written (the block is one byte smaller too)
            char *small = (char *)std::malloc(want_bytes - 1);
            rc = call(small, want_bytes - 1, &need, threads);
            if (rc == PG_OK || need != want_bytes) return 1;
            std::free(small);
        }
    }
    return 0;
}
int main(int argc, char **argv) {
    if (argc != 2 || !(f = std::fopen(argv[1], "rb"))) return 2;
    const long long cases = i64();
    for (long long c = 0; c < cases; ++c) {
        const long long kind = i64();
        int bad = 0;
        if (kind == 0) {
            const long long nd = i64(), count = i64(), want_bytes = i64();
            double *x = (double *)block(8 * count);
            char *want = (char *)block(want_bytes);
            bad = check([&](char *t, int64_t cap, int64_t *need, int th) { return pg_host_f64_text(x, count, (int)nd, t, cap, need, th); }, want, want_bytes);
            std::free(x); std::free(want);
        } else if (kind == 1) {
            const long long op = i64(), L = i64(), k = i64(), n_chrom = i64(), has_freq = i64(), has_pval = i64(), stat_count = i64(), names_bytes = i64(),
                            want_bytes = i64();
            int32_t *n_out = (int32_t *)block(4 * L), *ids = (int32_t *)block(4 * 5 * L);
            double *freq = has_freq ? (double *)block(8 * 5 * L) : nullptr, *stat = (double *)block(8 * stat_count);
            double *pval = has_pval ? (double *)block(8 * stat_count) : nullptr;
            int32_t *chrom = (int32_t *)block(4 * L);
            uint64_t *pos = (uint64_t *)block(8 * L);
            int32_t *off = (int32_t *)block(4 * (n_chrom + 1));
            char *names = (char *)block(names_bytes), *want = (char *)block(want_bytes);
            bad = check([&](char *t, int64_t cap, int64_t *need, int th) {
                return pg_host_result_rows((int)op, L, (int)k, n_out, ids, freq, stat, pval, chrom, pos, names, off, (int)n_chrom, t, cap, need, th); }, want, want_bytes);
            std::free(n_out); std::free(ids); std::free(freq); std::free(stat); std::free(pval); std::free(chrom); std::free(pos); std::free(off);
            std::free(names); std::free(want);
        } else {
            const long long p = i64(), k = i64(), m = i64(), n_chrom = i64(), names_bytes = i64(), row0 = i64(), rows = i64(), want_bytes = i64();
            double *beta = (double *)block(8 * p * k), *pval = (double *)block(8 * p * k);
            int32_t *cc = (int32_t *)block(4 * m);
            uint64_t *cp = (uint64_t *)block(8 * m);
            int32_t *ca = (int32_t *)block(4 * m), *off = (int32_t *)block(4 * (n_chrom + 1));
            char *names = (char *)block(names_bytes), *want = (char *)block(want_bytes);
            bad = check([&](char *t, int64_t cap, int64_t *need, int th) {
                return pg_host_kinship_rows(p, (int)k, row0, rows, beta, pval, cc, cp, ca, names, off, (int)n_chrom, t, cap, need, th); }, want, want_bytes);
            std::free(beta); std::free(pval); std::free(cc); std::free(cp); std::free(ca); std::free(off); std::free(names); std::free(want);
        }
        if (bad) { std::fprintf(stderr, "case %lld (kind %lld)\n", c, kind); return 1; }
    }
    std::fclose(f);
    std::printf("ok %lld\n", cases);
    return 0;
}
"""


def write_cases(path, cases):
    from poolgen_amd.engine import RESULT_OPS, name_table
    q = lambda *v: struct.pack("<%dq" % len(v), *v)
    with open(path, "wb") as f:
        f.write(q(len(cases)))
        for kind, g, want in cases:
            if kind == 0:
                nd, x = g
                f.write(q(0, nd, len(x), len(want)) + np.ascontiguousarray(x).tobytes() + want)
            elif kind == 1:
                text, off = name_table(g["names"])
                f.write(q(1, RESULT_OPS[g["op"]], len(g["n_out"]), g["k"], len(off) - 1, g["freq"] is not None, g["pval"] is not None, len(g["stat"]),
                          len(text), len(want)))
                for a in (g["n_out"], g["ids"], g["freq"], g["stat"], g["pval"], g["chrom"], g["pos"], off, text):
                    if a is not None:
                        f.write(np.ascontiguousarray(a).tobytes())
                f.write(want)
            else:
                inputs, row0, rows = g
                text, off = name_table(inputs["names"])
                p, k = inputs["beta"].shape
                f.write(q(2, p, k, len(inputs["col_chrom"]), len(off) - 1, len(text), row0, rows, len(want)))
                for a in (inputs["beta"], inputs["pval"], inputs["col_chrom"], inputs["col_pos"], inputs["col_allele"], off, text):
                    f.write(np.ascontiguousarray(a).tobytes())
                f.write(want)


def test_host_translation_unit_under_sanitizers(tmp_path):
    """pg_hostresultfmt.cpp alone (with the shared headers) plus a small program with its own main, built with
    -fsanitize=address,undefined: the whole corpus through pg_host_f64_text, generated rows of every kind through the two row
    twins, on buffers sized exactly.  No Python and no preloaded runtime in that process."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler here")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-O1", "-std=c++17", "-ffp-contract=off"]
    if subprocess.run([cxx, *flags, str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0 \
            or subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the address / undefined-behaviour sanitizer runtime is not installed here")
    cases = [(0, (-1, FC.corpus()), FC.expected(-1))] + [(0, (nd, FC.corpus()), FC.expected(nd)) for nd in (0, 6, 12, 22)]
    for i, op in enumerate(RR.OPS):
        g = RR.generated(op, 300, 3, seed=700 + i)
        cases.append((1, g, RR.result_rows(*RR.args_of(g))))
    cases += [(1, g, want) for g, want in ROW_LITERALS]
    for p, k, row0, rows in ((1, 1, 0, 1), (2, 2, 1, 3), (300, 3, 0, 900), (300, 3, 299, 302)):
        g = RR.generated_kinship(p, k, seed=20 + p)
        cases.append((2, (g, row0, rows), RR.kinship_rows(*RR.kinship_args_of(g), row0=row0, rows=rows)))
    data = tmp_path / "cases.bin"
    write_cases(data, cases)
    main = tmp_path / "main.cpp"
    main.write_text(SANITIZER_MAIN)
    exe = tmp_path / "resultfmt_asan"
    subprocess.check_call([cxx, *flags, "-Wall", "-I", str(ROOT / "include"), str(main), str(CSRC / "pg_hostresultfmt.cpp"), "-o", str(exe), "-lpthread"])
    r = subprocess.run([str(exe), str(data)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == f"ok {len(cases)}", r.stdout + r.stderr
