#!/usr/bin/env python3
"""The pileup parser on synthetic mpileup text (200 pools at depth 30 and 5 pools at depth 100; every pool a coverage, a read
string of '.', ',' and bases and a quality string, no indels): the text parsed on the GPU (pg_pileup_parse_dev) against the copy
of the same bytes over the link and against the same text parsed on the host (pg_host_pileup_parse, 16 threads).  One JSON line
per leg and shape, appended to profiles/pileup_ops.jsonl: the median of the rounds (the legs alternate inside a round, after a
warm-up of each):
  parse_dev       the kernels of one call (index, parse + scan, emit: kernel id "pileup" sums the stages), by device events
  h2d             the copy of the same bytes from pinned host memory alone: the link rate of this run
  parse_dev_h2d   that copy + the call (capacities known: one call), host clock around a device synchronise; the rows stay on
                  the device
  parse_host      the host twin on the text in host memory
  cli_host, cli_gpu   with --cli-rounds N: `poolgen chisq_test` on a file of the same text, --pileup-parser host (the existing
                  parse_pileup_buffer path) and gpu in turn, the wall clock of the process
with the text's size and bytes of text per second; parse_dev_h2d also carries its ratio to parse_host, cli_gpu to cli_host.

    python tools/bench_pileup.py [--shapes 200x30x20000,5x100x300000] [--rounds 7] [--threads 16] [--cli-rounds 7] [--dir /tmp]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from poolgen_amd import Engine
from poolgen_amd._native import PgPileupInfo

CLI = ROOT / "poolgen_amd" / "csrc" / "poolgen"
RULE = (1, 0, 0.01, 1, 1.0, 0.0)   # remove_ns, keep_lowercase_reference, max_base_error_rate, depth, breadth, frequency: every line is kept


def synthetic_pileup(loci, pools, depth, seed=1):
    """fixed-width lines, so that the text is made by array operations: 'chrC <9-digit pos> A' and per pool '<depth> <reads>
    <qualities>'; returns the text and the counts (loci x pools x 6, uint32)"""
    rng = np.random.default_rng(seed)
    head = b"chr0\t000000000\tA\t"
    cov = b"%d\t" % depth
    field = cov + b"." * depth + b"\t" + b"I" * depth + b"\t"
    line = np.frombuffer(head + field * pools, dtype=np.uint8)
    text = np.tile(line, (loci, 1))
    text[:, -1] = ord("\n")
    text[:, 3] = ord("1") + (np.arange(loci) * 5 // loci).astype(np.uint8)
    pos = np.arange(1, loci + 1)
    for d in range(9):
        text[:, 5 + 8 - d] = ord("0") + (pos // 10 ** d % 10).astype(np.uint8)
    f = text[:, len(head):].reshape(loci, pools, len(field))
    codes = np.frombuffer(b"..,,..,,..,,TtCGa*", dtype=np.uint8)                    # two reads in three are the reference
    reads = codes[rng.integers(0, len(codes), size=(loci, pools, depth), dtype=np.uint8)]
    f[:, :, len(cov):len(cov) + depth] = reads
    quals = np.frombuffer(b"IIIIIIIJJJ6?FFF#", dtype=np.uint8)                      # one in sixteen is below the error rate: gone
    q = quals[rng.integers(0, len(quals), size=(loci, pools, depth), dtype=np.uint8)]
    f[:, :, len(cov) + depth + 1:len(cov) + 2 * depth + 1] = q
    good = q != ord("#")
    counts = np.zeros((loci, pools, 6), dtype=np.uint32)
    for col, members in ((0, b".,a"), (1, b"Tt"), (2, b"C"), (3, b"G"), (4, b"*")):
        counts[:, :, col] = (np.isin(reads, np.frombuffer(members, dtype=np.uint8)) & good).sum(axis=2)
    return text.reshape(-1), counts


def bench(eng, n, depth, L, rounds, threads, out):
    print(f"bench_pileup: {n} pools of depth {depth} x {L} loci: making the text", file=sys.stderr, flush=True)
    text, want = synthetic_pileup(L, n, depth)
    size = text.size
    print(f"bench_pileup: {size} bytes of text; timing", file=sys.stderr, flush=True)
    text_pin = torch.from_numpy(text).pin_memory()
    text_dev = torch.empty(size, dtype=torch.uint8, device="cuda")
    counts = torch.empty(L * n * 6, dtype=torch.int32, device="cuda")
    pos = torch.empty(L, dtype=torch.int64, device="cuda"); off = torch.empty(L, dtype=torch.int64, device="cuda")
    clen = torch.empty(L, dtype=torch.int32, device="cuda"); ref = torch.empty(L, dtype=torch.uint8, device="cuda")
    sizes = np.full(n, 1.0 / n)
    info = PgPileupInfo()

    def call():
        rc = eng._lib.pg_pileup_parse_dev(eng._ctx, text_dev.data_ptr(), size, sizes.ctypes.data, n, *RULE, counts.data_ptr(), pos.data_ptr(), ref.data_ptr(),
                                          off.data_ptr(), clen.data_ptr(), L, counts.numel(), C.byref(info))
        if rc != 0:
            sys.exit(f"bench_pileup: pg_pileup_parse_dev failed ({rc})")

    def parse_dev():
        eng.profile_reset()
        call()
        return eng.profile_get("pileup")[0] * 1e-3

    def parse_dev_h2d():
        t0 = time.perf_counter()
        text_dev.copy_(text_pin, non_blocking=True)
        call()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def h2d():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        text_dev.copy_(text_pin, non_blocking=True)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    h_counts = np.empty(L * n * 6, dtype=np.uint32); h_pos = np.empty(L, dtype=np.uint64); h_ref = np.empty(L, dtype=np.uint8)
    h_off = np.empty(L, dtype=np.int64); h_clen = np.empty(L, dtype=np.int32)
    h_info = PgPileupInfo()

    def parse_host():                                        # capacities known, as for the device: one call
        t0 = time.perf_counter()
        rc = eng._lib.pg_host_pileup_parse(text.ctypes.data, size, sizes.ctypes.data, n, *RULE, h_counts.ctypes.data, h_pos.ctypes.data, h_ref.ctypes.data,
                                           h_off.ctypes.data, h_clen.ctypes.data, L, h_counts.size, C.byref(h_info), threads)
        if rc != 0:
            sys.exit(f"bench_pileup: pg_host_pileup_parse failed ({rc})")
        return time.perf_counter() - t0

    text_dev.copy_(text_pin)
    legs = {"parse_dev": parse_dev, "h2d": h2d, "parse_dev_h2d": parse_dev_h2d, "parse_host": parse_host}
    eng.profile(True)
    for fn in legs.values():                                 # the warm-up of each, and the check of the rows
        fn()
    if info.kept != L or h_info.kept != L or not np.array_equal(counts.cpu().numpy().view(np.uint32).reshape(L, n, 6), want) \
            or not np.array_equal(h_counts.reshape(L, n, 6), want) or not np.array_equal(pos.cpu().numpy(), np.arange(1, L + 1)):
        sys.exit("bench_pileup: the rows differ from the counts the text was made of")
    t = {k: [] for k in legs}
    for _ in range(rounds):                                  # alternating: the legs see the same neighbours on the machine
        for k, fn in legs.items():
            t[k].append(fn())
    eng.profile(False)
    common = {"pools": n, "depth": depth, "loci": L, "text_bytes": int(size), "host_threads": threads}
    med = {k: statistics.median(v) for k, v in t.items()}
    with open(out, "a") as f:
        for k, v in t.items():
            rec = {"op": "pileup_" + k, **common, "rounds": len(v), "ms": med[k] * 1e3, "ms_min": min(v) * 1e3, "ms_max": max(v) * 1e3,
                   "text_bytes_per_s": size / med[k]}
            if k == "parse_dev":
                rec["share_of_h2d"] = med[k] / med["h2d"]
            if k == "parse_dev_h2d":
                rec["speedup_over_parse_host"] = med["parse_host"] / med[k]
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")
    return text


def bench_cli(text, n, depth, L, rounds, threads, workdir, out):
    work = Path(tempfile.mkdtemp(prefix="bench_pileup_", dir=workdir))
    pileup, phen = work / "synthetic.pileup", work / "phen.csv"
    text.tofile(pileup)
    size = int(text.size)
    rng = np.random.default_rng(2)
    phen.write_text("#pop,size,trait\n" + "".join(f"Pool{i},20.0,{rng.random():.6f}\n" for i in range(n)))
    env = dict(os.environ, PGH_TIMING="1")
    t = {"host": [], "gpu": []}
    laps, sizes = {}, {}
    for r in range(rounds):                                  # alternating: host, gpu, host, gpu ..
        print(f"bench_pileup: the CLI, round {r + 1} of {rounds}", file=sys.stderr, flush=True)
        for pp in ("host", "gpu"):
            o = work / f"chisq_{pp}_{r}.csv"
            t0 = time.perf_counter()
            p = subprocess.run([str(CLI), "chisq_test", "-f", str(pileup), "-p", str(phen), "-o", str(o), "--n-threads", str(threads),
                                "--min-allele-frequency", "0.0", "--pileup-parser", pp], capture_output=True, text=True, env=env)
            t[pp].append(time.perf_counter() - t0)
            if p.returncode != 0:
                sys.exit(f"bench_pileup: chisq_test --pileup-parser {pp} failed: {p.stderr}")
            laps[pp] = p.stderr
            sizes[pp] = o.stat().st_size
            o.unlink()
    pileup.unlink(); phen.unlink(); os.rmdir(work)
    if sizes["host"] != sizes["gpu"]:
        sys.exit(f"bench_pileup: the outputs differ in size: {sizes}")
    med = {pp: statistics.median(v) for pp, v in t.items()}
    common = {"pools": n, "depth": depth, "loci": L, "text_bytes": size, "host_threads": threads, "analysis": "chisq_test"}
    with open(out, "a") as f:
        for pp, v in t.items():
            rec = {"op": "pileup_cli_" + pp, **common, "rounds": len(v), "ms": med[pp] * 1e3, "ms_min": min(v) * 1e3, "ms_max": max(v) * 1e3,
                   "text_bytes_per_s": size / med[pp]}
            if pp == "gpu":
                rec["speedup_over_cli_host"] = med["host"] / med["gpu"]
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")
    for pp in ("host", "gpu"):
        print(f"---- laps of the last run: chisq_test --pileup-parser {pp}\n{laps[pp]}", file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="200x30x20000,5x100x300000", help="pools x depth x loci, comma-separated")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--cli-rounds", type=int, default=7)
    ap.add_argument("--dir", default=tempfile.gettempdir())
    ap.add_argument("--out", default=str(ROOT / "profiles" / "pileup_ops.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_pileup: no GPU (a time from a CPU would say nothing)")
    for shape in a.shapes.split(","):
        n, depth, L = (int(x) for x in shape.split("x"))
        eng = Engine(0)
        text = bench(eng, n, depth, L, a.rounds, a.threads, a.out)
        del eng
        torch.cuda.empty_cache()
        if a.cli_rounds > 0:
            bench_cli(text, n, depth, L, a.cli_rounds, a.threads, a.dir, a.out)


if __name__ == "__main__":
    main()
