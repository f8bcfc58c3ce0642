#!/usr/bin/env python3
"""The sync parser on synthetic sync text (200 pools x 1 M loci and 5 pools x 10 M loci, about 14 bytes a pool): the text parsed
on the GPU (pg_sync_parse_dev) against the copy of the same bytes over the link and against the same text parsed on the host
(pg_host_sync_parse, 16 threads).  One JSON line per leg and shape, appended to profiles/sync_ops.jsonl: the median of the
rounds (the legs alternate inside a round, after a warm-up of each):
  parse_dev       the kernels of one call (index, parse + scan, emit: kernel id "sync" sums the stages), by device events
  parse_dev_h2d   the copy of the text from pinned host memory + the call (capacities known: one call), host clock around a
                  device synchronise; the rows stay on the device
  h2d             the copy of the same bytes alone: the link rate of this run, the yardstick of parse_dev (a parse that takes
                  longer than the copy of the next piece cannot hide behind it)
  parse_host      the host twin on the text in host memory
with the text's size and bytes of text per second; parse_dev also carries its time as a share of h2d's.
With --cli-rounds N the CLI runs too, from a file of the first shape: `poolgen ols_iter` and the streamed
`poolgen ols_iter_with_kinship`, --sync-parser host and gpu in turn under PGH_TIMING=1, N times each; the wall clock of every
run, the medians, their ratio and the laps of the last run of each go to profiles/sync_e2e.txt.

    python tools/bench_sync.py [--shapes 200x1000000,5x10000000] [--rounds 7] [--threads 16] [--cli-rounds 0] [--dir /tmp]
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
from poolgen_amd._native import PgSyncInfo

CLI = ROOT / "poolgen_amd" / "csrc" / "poolgen"


def synthetic_sync(loci, pools, seed=1):
    """fixed-width lines, so that the text is made by array operations: 'chrC <9-digit pos> N' and per pool 'AA:BB:C:D:0:0' (a
    leading zero is a valid count); returns the text and the counts (loci x pools x 6, uint32)"""
    rng = np.random.default_rng(seed)
    head = b"chr0\t000000000\tN\t"
    field = b"00:00:0:0:0:0\t"
    line = np.frombuffer(head + field * pools, dtype=np.uint8)
    text = np.tile(line, (loci, 1))
    text[:, -1] = ord("\n")
    text[:, 3] = ord("1") + (np.arange(loci) * 5 // loci).astype(np.uint8)
    pos = np.arange(1, loci + 1)
    for d in range(9):
        text[:, 5 + 8 - d] = ord("0") + (pos // 10 ** d % 10).astype(np.uint8)
    f = text[:, len(head):].reshape(loci, pools, len(field))
    counts = np.zeros((loci, pools, 6), dtype=np.uint32)
    for col, digits, at in ((0, 2, 0), (1, 2, 3), (2, 1, 6), (3, 1, 8)):
        v = rng.integers(0, 10 ** digits, size=(loci, pools), dtype=np.int32)
        counts[:, :, col] = v
        for d in range(digits):
            f[:, :, at + digits - 1 - d] = (v // 10 ** d % 10 + ord("0")).astype(np.uint8)
    return text.reshape(-1), counts


def bench(eng, n, L, rounds, threads, out):
    print(f"bench_sync: {n} pools x {L} loci: making the text", file=sys.stderr, flush=True)
    text, want = synthetic_sync(L, n)
    size = text.size
    print(f"bench_sync: {size} bytes of text; timing", file=sys.stderr, flush=True)
    text_pin = torch.from_numpy(text).pin_memory()
    text_dev = torch.empty(size, dtype=torch.uint8, device="cuda")
    counts = torch.empty(L * n * 6, dtype=torch.int32, device="cuda")
    pos = torch.empty(L, dtype=torch.int64, device="cuda"); off = torch.empty(L, dtype=torch.int64, device="cuda")
    clen = torch.empty(L, dtype=torch.int32, device="cuda")
    info = PgSyncInfo()

    def call():
        rc = eng._lib.pg_sync_parse_dev(eng._ctx, text_dev.data_ptr(), size, n, counts.data_ptr(), pos.data_ptr(), off.data_ptr(), clen.data_ptr(), L,
                                        counts.numel(), C.byref(info))
        if rc != 0:
            sys.exit(f"bench_sync: pg_sync_parse_dev failed ({rc})")

    def parse_dev():
        eng.profile_reset()
        call()
        return eng.profile_get("sync")[0] * 1e-3

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

    h_counts = np.empty(L * n * 6, dtype=np.uint32); h_pos = np.empty(L, dtype=np.uint64)
    h_off = np.empty(L, dtype=np.int64); h_clen = np.empty(L, dtype=np.int32)
    h_info = PgSyncInfo()

    def parse_host():                                        # capacities known, as for the device: one call
        t0 = time.perf_counter()
        rc = eng._lib.pg_host_sync_parse(text.ctypes.data, size, n, h_counts.ctypes.data, h_pos.ctypes.data, h_off.ctypes.data, h_clen.ctypes.data, L,
                                         h_counts.size, C.byref(h_info), threads)
        if rc != 0:
            sys.exit(f"bench_sync: pg_host_sync_parse failed ({rc})")
        return time.perf_counter() - t0

    text_dev.copy_(text_pin)
    legs = {"parse_dev": parse_dev, "parse_dev_h2d": parse_dev_h2d, "h2d": h2d, "parse_host": parse_host}
    eng.profile(True)
    for fn in legs.values():                                 # the warm-up of each, and the check of the rows
        fn()
    if info.kept != L or not np.array_equal(counts.cpu().numpy().view(np.uint32).reshape(L, n, 6), want) \
            or not np.array_equal(h_counts.reshape(L, n, 6), want) or not np.array_equal(pos.cpu().numpy(), np.arange(1, L + 1)):
        sys.exit("bench_sync: the rows differ from the counts the text was made of")
    t = {k: [] for k in legs}
    for _ in range(rounds):                                  # alternating: the legs see the same neighbours on the machine
        for k, fn in legs.items():
            t[k].append(fn())
    eng.profile(False)
    common = {"pools": n, "loci": L, "text_bytes": int(size), "host_threads": threads}
    med = {k: statistics.median(v) for k, v in t.items()}
    with open(out, "a") as f:
        for k, v in t.items():
            rec = {"op": "sync_" + k, **common, "rounds": len(v), "ms": med[k] * 1e3, "ms_min": min(v) * 1e3, "ms_max": max(v) * 1e3,
                   "text_bytes_per_s": size / med[k]}
            if k == "parse_dev":
                rec["share_of_h2d"] = med[k] / med["h2d"]
            if k == "parse_dev_h2d":
                rec["speedup_over_parse_host"] = med["parse_host"] / med[k]
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")


def bench_cli(n, L, rounds, threads, workdir, out):
    work = Path(tempfile.mkdtemp(prefix="bench_sync_", dir=workdir))
    sync, phen = work / "synthetic.sync", work / "phen.csv"
    text, _ = synthetic_sync(L, n)
    text.tofile(sync)
    size = int(text.size)
    del text
    rng = np.random.default_rng(2)
    phen.write_text("#pop,size,trait\n" + "".join(f"Pool{i},20.0,{rng.random():.6f}\n" for i in range(n)))
    env = dict(os.environ, PGH_TIMING="1")
    legs = [(an, ps) for an in ("ols_iter", "ols_iter_with_kinship") for ps in ("host", "gpu")]
    t = {leg: [] for leg in legs}
    laps, sizes = {}, {}
    for r in range(rounds):                                  # alternating: host, gpu, host, gpu ..
        print(f"bench_sync: the CLI, round {r + 1} of {rounds}", file=sys.stderr, flush=True)
        for an, ps in legs:
            o = work / f"{an}_{ps}_{r}.csv"
            t0 = time.perf_counter()
            p = subprocess.run([str(CLI), an, "-f", str(sync), "-p", str(phen), "-o", str(o), "--n-threads", str(threads), "--sync-parser", ps],
                               capture_output=True, text=True, env=env)
            t[(an, ps)].append(time.perf_counter() - t0)
            if p.returncode != 0:
                sys.exit(f"bench_sync: {an} --sync-parser {ps} failed: {p.stderr}")
            laps[(an, ps)] = p.stderr
            sizes[(an, ps)] = o.stat().st_size
            o.unlink()
    sync.unlink(); phen.unlink(); os.rmdir(work)
    with open(out, "w") as f:
        f.write(f"poolgen <analysis> --n-threads {threads} --sync-parser <host|gpu> on {n} pools x {L} loci of synthetic sync text ({size} bytes), PGH_TIMING=1;\n"
                f"wall clock of the process, {rounds} runs each, host and gpu in turn\n\n")
        for an in ("ols_iter", "ols_iter_with_kinship"):
            med = {ps: statistics.median(t[(an, ps)]) for ps in ("host", "gpu")}
            for ps in ("host", "gpu"):
                f.write(f"{an} --sync-parser {ps}: median {med[ps]:.3f} s  (" + " ".join(f"{x:.3f}" for x in t[(an, ps)]) + f")  output {sizes[(an, ps)]} bytes\n")
            f.write(f"{an}: host / gpu = {med['host'] / med['gpu']:.3f}\n\n")
        for leg in legs:
            f.write(f"---- laps of the last run: {leg[0]} --sync-parser {leg[1]}\n{laps[leg]}\n")
    print(Path(out).read_text(), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="200x1000000,5x10000000", help="pools x loci, comma-separated")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--cli-rounds", type=int, default=0)
    ap.add_argument("--dir", default=tempfile.gettempdir())
    ap.add_argument("--out", default=str(ROOT / "profiles" / "sync_ops.jsonl"))
    ap.add_argument("--cli-out", default=str(ROOT / "profiles" / "sync_e2e.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_sync: no GPU (a time from a CPU would say nothing)")
    eng = Engine(0)
    for shape in a.shapes.split(","):
        n, L = (int(x) for x in shape.split("x"))
        if a.rounds > 0:
            bench(eng, n, L, a.rounds, a.threads, a.out)
    if a.cli_rounds > 0:
        del eng
        torch.cuda.empty_cache()
        n, L = (int(x) for x in a.shapes.split(",")[0].split("x"))
        bench_cli(n, L, a.cli_rounds, a.threads, a.dir, a.cli_out)


if __name__ == "__main__":
    main()
