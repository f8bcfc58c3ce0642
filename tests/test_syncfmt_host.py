"""pg_host_sync_format_rows, the plain C++ twin of the device sync writer (pg_sync_format_rows_dev): against the literal
restatement of append_sync_line (tests/syncfmt_ref.py) and hand-written bytes (tests/syncfmt_corpus.py), its buffer contract,
its refusals, and round trips through the host twins of the three parsers.  Runs without a GPU."""
import ctypes as C
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import syncfmt_corpus as SC
import syncfmt_ref as SR

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
CSRC = ROOT / "poolgen_amd" / "csrc"
PG_OK, PG_ERR_INVALID = 0, -1


def host_text(rows, n_threads=1):
    from poolgen_amd import sync_format_host
    return sync_format_host(*SC.args_of(rows), n_threads=n_threads)


def raw_call(native, rows, buf, cap, n_pools=None, n_rows=None, slab_bytes=None, n_threads=2):
    """the C entry point itself -> (rc, bytes)"""
    slab = np.frombuffer(rows["slab"], dtype=np.uint8)
    c = np.ascontiguousarray(rows["counts"], dtype=np.uint32)
    need = C.c_int64(-7)
    rc = native.pg_host_sync_format_rows(slab.ctypes.data if slab.size else None, slab.size if slab_bytes is None else slab_bytes, c.ctypes.data,
                                         rows["pos"].ctypes.data, rows["ref"].ctypes.data, rows["line_off"].ctypes.data,
                                         rows["chrom_len"].ctypes.data, c.shape[1] if n_pools is None else n_pools,
                                         c.shape[0] if n_rows is None else n_rows, buf.ctypes.data if buf is not None else None, cap,
                                         C.byref(need), n_threads)
    return rc, need.value


@pytest.fixture(scope="module")
def mixed():
    """(rows, the restatement's text) of generated shapes, computed once"""
    out = []
    for n, k in [(1, 40), (2, 33), (5, 70), (9, 17), (64, 9), (65, 7), (200, 5)]:
        rows = SC.generated(n, k, seed=100 + n)
        out.append((rows, SR.rows_text(*SC.args_of(rows))))
    return out


def test_literals(native):
    for name, rows, want in SC.LITERALS:
        assert SR.rows_text(*SC.args_of(rows)) == want, name             # the restatement against the hand-written bytes
        assert host_text(rows) == want, name                              # the host twin against them


def test_host_twin_equals_restatement_on_any_number_of_threads(native, mixed):
    for rows, want in mixed:
        for threads in (1, 3, 16):
            assert host_text(rows, threads) == want, (rows["counts"].shape, threads)


def test_every_reference_byte_position_edge_and_name_place(native):
    rows = SC.generated(3, 256 + 96, seed=5)
    assert set(rows["ref"].tolist()) == set(range(256)) and set(SC.POS_EDGES) <= set(int(p) for p in rows["pos"])
    slab, places = SC.name_slab()
    assert {(o % 16, l) for o, l in places} >= {(r, l) for r in range(16) for l in SC.NAME_LENGTHS}
    assert any(o + l == len(slab) and l == 17 for o, l in places)
    assert host_text(rows, 4) == SR.rows_text(*SC.args_of(rows))


def test_size_query_exact_capacity_one_short_and_canary(native, mixed):
    for rows, want in mixed[:4]:
        rc, need = raw_call(native, rows, None, 0)
        assert rc == PG_ERR_INVALID and need == len(want)                 # the size query (the text needs more than 0 bytes)
        buf = np.full(need + 64, 0xAA, dtype=np.uint8)
        rc, got = raw_call(native, rows, buf, need - 1)
        assert rc == PG_ERR_INVALID and got == need and (buf == 0xAA).all()   # one short: the size, and nothing written
        rc, got = raw_call(native, rows, buf, need)
        assert rc == PG_OK and got == need and buf[:need].tobytes() == want and (buf[need:] == 0xAA).all()
        buf[:] = 0xAA
        rc, got = raw_call(native, rows, buf, need + 64)                  # room to spare: still nothing at or behind text[bytes]
        assert rc == PG_OK and got == need and buf[:need].tobytes() == want and (buf[need:] == 0xAA).all()


def test_refused_inputs(native):
    rows = SC.generated(4, 12, seed=9)
    want = SR.rows_text(*SC.args_of(rows))
    buf = np.full(len(want) + 8, 0xAA, dtype=np.uint8)

    def refused(**change):
        r = dict(rows)
        kw = {}
        for key, v in change.items():
            if key in ("n_pools", "n_rows", "slab_bytes"):
                kw[key] = v
            else:
                a = r[key].copy(); a[7] = v; r[key] = a
        buf[:] = 0xAA
        rc, got = raw_call(native, r, buf, buf.size, **kw)
        assert rc == PG_ERR_INVALID and got == 0 and (buf == 0xAA).all(), change

    refused(line_off=-1)
    refused(chrom_len=-1)
    refused(line_off=len(rows["slab"]), chrom_len=1)                     # one byte past the slab
    refused(line_off=len(rows["slab"]) - 3, chrom_len=4)
    refused(line_off=2 ** 62, chrom_len=2 ** 31 - 1)                     # (no overflow in the check)
    refused(slab_bytes=int(rows["line_off"].max()) - 1)                  # a slab that ends in front of a (here empty) name
    refused(slab_bytes=-1)
    refused(n_pools=0)
    refused(n_pools=-3)
    refused(n_pools=SR.MAX_POOLS + 1)
    refused(n_rows=-1)
    rc, got = raw_call(native, rows, buf, -1)
    assert rc == PG_ERR_INVALID and got == 0
    rc, got = raw_call(native, rows, None, 5)                            # a capacity without a buffer
    assert rc == PG_ERR_INVALID and got == 0
    assert native.pg_host_sync_format_rows(None, 0, None, None, None, None, None, 4, 0, None, 0, None, 1) == PG_ERR_INVALID   # no `bytes`
    # a name that ends exactly at the slab's end is fine, and so is the empty name behind the last byte
    ok = dict(rows); a = rows["line_off"].copy(); a[7] = len(rows["slab"]); ok["line_off"] = a
    b = rows["chrom_len"].copy(); b[7] = 0; ok["chrom_len"] = b
    assert raw_call(native, ok, buf, buf.size)[0] == PG_OK
    # rows = 0: PG_OK, bytes = 0, whatever the pointers
    buf[:] = 0xAA
    rc, got = raw_call(native, rows, buf, buf.size, n_rows=0)
    assert rc == PG_OK and got == 0 and (buf == 0xAA).all()
    need = C.c_int64(-7)
    assert native.pg_host_sync_format_rows(None, 0, None, None, None, None, None, 4, 0, None, 0, C.byref(need), 1) == PG_OK and need.value == 0


def test_the_largest_row_and_the_line_limit(native):
    """4096 pools of ten-digit counts are 66 x 4096 + a short prefix; a name that takes the line past 2^22 bytes is refused."""
    rows = SC.generated(SR.MAX_POOLS, 2, seed=3, digits=10, names=False)
    want = SR.rows_text(*SC.args_of(rows))
    assert len(want) > 2 * 66 * SR.MAX_POOLS and host_text(rows, 2) == want
    slab = b"n" * (SR.MAX_ROW + 8)
    for clen, ok in ((SR.MAX_ROW - 17, True), (SR.MAX_ROW - 16, False)):   # + "\t0\tA" + "\t0:0:0:0:0:0" + "\n" = clen + 17 bytes
        r = SC.rows_of(slab, [(0, clen, 0, ord("A"), [[0] * 6])])
        rc, got = raw_call(native, r, None, 0)
        assert rc == PG_ERR_INVALID and got == (SR.MAX_ROW if ok else 0)


# ---- round trips through the parsers' host twins ------------------------------------------------------------------------------
VCF_THRESHOLDS = [(1, 1.0, 0.001), (1, 1.0, 0.0), (10, 1.0, 0.0), (5, 0.5, 0.05)]   # the four sets of test_vcf_host.py / test_gpu_vcf.py


def ref_bytes_of_sync_text(text):
    """the third field of every data line of a sync text"""
    return np.array([l.split(b"\t")[2][0] for l in text.split(b"\n") if l and not l.startswith(b"#")], dtype=np.uint8)


@pytest.mark.parametrize("depth,breadth,maf", VCF_THRESHOLDS)
def test_vcf_round_trip(native, depth, breadth, maf):
    import vcf_ref
    from poolgen_amd import sync_format_host, sync_parse_host, vcf_parse_host
    text = (GOLDEN / "test.vcf").read_bytes()
    sizes = [0.1] * 10
    want = vcf_ref.vcf2sync_bytes(text, sizes, depth, breadth, maf)      # the file the host path writes, as vcf_ref.py restates it
    header, body = want[:want.index(b"\n") + 1], want[want.index(b"\n") + 1:]
    p = vcf_parse_host(text, sizes, depth, breadth, maf, n_threads=3)
    got = sync_format_host(p["counts"], p["pos"], p["ref"], p["line_off"], p["chrom_len"], text, n_threads=3)
    assert got == body and (len(body) > 0) == (p["counts"].shape[0] > 0)
    if (depth, breadth, maf) == (1, 1.0, 0.0):
        assert len(body) > 0
    # sync text -> the sync parser's rows -> the same text
    s = sync_parse_host(header + body, n_threads=2)
    again = sync_format_host(s["counts"], s["pos"], ref_bytes_of_sync_text(body), s["line_off"], s["chrom_len"], header + body, n_threads=2)
    assert again == body


def test_pileup_round_trip(native):
    import pileup_corpus
    import pileup_ref
    from poolgen_amd import pileup_parse_host, sync_format_host, sync_parse_host
    seen = 0
    for name, text, sizes, rule in pileup_corpus.texts():
        want_rows = pileup_ref.parse_ref(text, sizes, **rule)
        lines = dict(pileup_ref.text_lines(text))
        want = b"".join(pileup_ref.sync_line(lines[int(o)], ("K", int(l), int(p), int(r), c)) + b"\n"
                        for o, l, p, r, c in zip(want_rows["line_off"], want_rows["chrom_len"], want_rows["pos"], want_rows["ref"], want_rows["counts"]))
        p = pileup_parse_host(text, sizes, n_threads=2, **rule)
        got = sync_format_host(p["counts"], p["pos"], p["ref"], p["line_off"], p["chrom_len"], text, n_threads=2)
        assert got == want, name
        if not got:
            continue
        seen += 1
        s = sync_parse_host(got, n_threads=2)
        assert s["counts"].shape[0] == p["counts"].shape[0], name
        assert sync_format_host(s["counts"], s["pos"], ref_bytes_of_sync_text(got), s["line_off"], s["chrom_len"], got) == got, name
    assert seen > 20


# ---- the host translation unit on its own, under the address and undefined-behaviour sanitizers ------------------------------------
SANITIZER_MAIN = r"""
#include "poolgen_hip.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
// input: rows as text (written by the test); every buffer is a heap block of exactly the size stated, so that a byte read or written
// outside one is an error the sanitizer reports
int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    long long cases = 0;
    if (std::fscanf(f, "%lld", &cases) != 1) return 2;
    for (long long c = 0; c < cases; ++c) {
        long long slab_bytes, n, rows, want_bytes;
        if (std::fscanf(f, "%lld %lld %lld %lld", &slab_bytes, &n, &rows, &want_bytes) != 4) return 2;
        std::fgetc(f);
        char *slab = (char *)std::malloc(slab_bytes ? slab_bytes : 1);
        if (slab_bytes && std::fread(slab, 1, slab_bytes, f) != (size_t)slab_bytes) return 2;
        uint32_t *counts = (uint32_t *)std::malloc(sizeof(uint32_t) * rows * n * 6 + 1);
        uint64_t *pos = (uint64_t *)std::malloc(sizeof(uint64_t) * rows + 1);
        uint8_t *ref = (uint8_t *)std::malloc(rows + 1);
        int64_t *off = (int64_t *)std::malloc(sizeof(int64_t) * rows + 1);
        int32_t *clen = (int32_t *)std::malloc(sizeof(int32_t) * rows + 1);
        for (long long r = 0; r < rows; ++r) {
            unsigned long long p; long long o; int l, rf;
            if (std::fscanf(f, "%llu %d %lld %d", &p, &rf, &o, &l) != 4) return 2;
            pos[r] = p; ref[r] = (uint8_t)rf; off[r] = o; clen[r] = l;
            for (long long j = 0; j < n * 6; ++j) { unsigned v; if (std::fscanf(f, "%u", &v) != 1) return 2; counts[r * n * 6 + j] = v; }
        }
        std::fgetc(f);
        char *want = (char *)std::malloc(want_bytes ? want_bytes : 1);
        if (want_bytes && std::fread(want, 1, want_bytes, f) != (size_t)want_bytes) return 2;
        for (int threads : {1, 3}) {
            int64_t need = -7;
            int rc = pg_host_sync_format_rows(slab, slab_bytes, counts, pos, ref, off, clen, (int)n, rows, nullptr, 0, &need, threads);
            if (need != want_bytes || (rc != PG_OK) != (want_bytes > 0)) { std::fprintf(stderr, "case %lld: size %lld, want %lld\n", c, (long long)need, want_bytes); return 1; }
            char *text = (char *)std::malloc(want_bytes ? want_bytes : 1);   // sized exactly
            rc = pg_host_sync_format_rows(slab, slab_bytes, counts, pos, ref, off, clen, (int)n, rows, text, want_bytes, &need, threads);
            if (rc != PG_OK || need != want_bytes || std::memcmp(text, want, want_bytes) != 0) { std::fprintf(stderr, "case %lld: text differs\n", c); return 1; }
            if (want_bytes > 1) {                                           // one byte short: nothing written (the block is one byte smaller too)
                char *small = (char *)std::malloc(want_bytes - 1);
                rc = pg_host_sync_format_rows(slab, slab_bytes, counts, pos, ref, off, clen, (int)n, rows, small, want_bytes - 1, &need, threads);
                if (rc == PG_OK || need != want_bytes) return 1;
                std::free(small);
            }
            std::free(text);
        }
        std::free(slab); std::free(counts); std::free(pos); std::free(ref); std::free(off); std::free(clen); std::free(want);
    }
    std::fclose(f);
    std::printf("ok %lld\n", cases);
    return 0;
}
"""


def test_host_translation_unit_under_sanitizers(tmp_path):
    """pg_hostsyncfmt.cpp alone plus a small program with its own main, built with -fsanitize=address,undefined: the corpus and
    generated rows on buffers sized exactly.  No Python and no preloaded runtime in that process."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler here")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-O1", "-std=c++17"]
    if subprocess.run([cxx, *flags, str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0 \
            or subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the address / undefined-behaviour sanitizer runtime is not installed here")
    cases = [rows for _, rows, _ in SC.LITERALS]
    cases += [SC.generated(n, k, seed=40 + n) for n, k in [(1, 130), (3, 90), (64, 5), (65, 5), (200, 3)]]
    cases += [SC.generated(SR.MAX_POOLS, 2, seed=41, digits=10, names=False)]
    data = tmp_path / "rows.bin"
    with open(data, "wb") as f:
        f.write(b"%d\n" % len(cases))
        for rows in cases:
            want = SR.rows_text(*SC.args_of(rows))
            k, n = rows["counts"].shape[:2]
            f.write(b"%d %d %d %d\n" % (len(rows["slab"]), n, k, len(want)))
            f.write(rows["slab"])
            for r in range(k):
                f.write(b"\n%d %d %d %d " % (int(rows["pos"][r]), int(rows["ref"][r]), int(rows["line_off"][r]), int(rows["chrom_len"][r])))
                f.write(" ".join(map(str, rows["counts"][r].reshape(-1).tolist())).encode())
            f.write(b"\n")
            f.write(want)
    main = tmp_path / "main.cpp"
    main.write_text(SANITIZER_MAIN)
    exe = tmp_path / "syncfmt_asan"
    subprocess.check_call([cxx, *flags, "-Wall", "-I", str(ROOT / "include"), str(main), str(CSRC / "pg_hostsyncfmt.cpp"), "-o", str(exe), "-lpthread"])
    r = subprocess.run([str(exe), str(data)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == f"ok {len(cases)}", r.stdout + r.stderr
