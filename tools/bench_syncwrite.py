#!/usr/bin/env python3
"""The sync writer: the rows a parser left on the device formatted there (pg_sync_format_rows_dev) against today's route, the rows
copied back and formatted by the host twin (pg_host_sync_format_rows, 16 threads), and the CLI's conversions with
`--sync-writer host` and `--sync-writer gpu`.  One JSON line per leg, appended to profiles/syncwrite_ops.jsonl: the median of the
rounds (the legs of a shape alternate inside a round, after a warm-up of each).  Per shape (pools x loci; two-digit depths as in
tools/bench_vcf.py, names chr1 .. chr5, positions 1 .. loci):
  format_dev        the kernels of one call (measure, scan, emit: kernel id "syncfmt" sums them), by device events: ms, bytes of
                    text written per second, and the useful bytes (counts and labels read + text written) as a share of the
                    8 TB/s HBM peak
  d2d_copy          a device-to-device copy of as many bytes as the text has, by device events: the floor the kernels are judged
                    against (format_dev carries the ratio)
  format_dev_d2h    the call (capacity known: one call) + the copy of the text into pinned host memory, host clock around a
                    device synchronise
  format_host_d2h   the copy of the five row arrays into pinned host memory + the host twin on them: today's route
                    (format_dev_d2h carries the speed-up over it)
and through the CLI, wall clock of the process, alternating host, gpu (and, with --parent-cli, the build of the commit before,
whose vcf2sync is today's yardstick):
  cli_vcf2sync_*    `poolgen vcf2sync` on tools/bench_vcf.py's synthetic file
  cli_pileup2sync_* `poolgen pileup2sync --pileup-parser gpu` on tools/bench_pileup.py's 200-pool file
The phase split of the last run of each (PGH_TIMING=1) goes to stderr.

    python tools/bench_syncwrite.py [--shapes 200x500000,5x10000000,4096x10000] [--rounds 7] [--cli-rounds 7] [--threads 16]
                                    [--cli vcf,pileup] [--parent-cli <poolgen of the parent commit>] [--dir /tmp]
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
sys.path.insert(0, str(ROOT / "tools"))
from poolgen_amd import Engine

HBM_PEAK = 8e12
CLI = ROOT / "poolgen_amd" / "csrc" / "poolgen"


def synthetic_rows(pools, loci, seed=1):
    rng = np.random.default_rng(seed)
    counts = np.zeros((loci, pools, 6), dtype=np.uint32)
    counts[:, :, 0] = rng.integers(0, 100, size=(loci, pools), dtype=np.uint32)
    counts[:, :, 1] = rng.integers(0, 100, size=(loci, pools), dtype=np.uint32)
    slab = np.frombuffer(b"chr1\tchr2\tchr3\tchr4\tchr5\t", dtype=np.uint8).copy()
    off = (np.arange(loci, dtype=np.int64) * 5 // loci) * 5
    return {"slab": slab, "counts": counts, "pos": np.arange(1, loci + 1, dtype=np.uint64), "ref": np.full(loci, ord("A"), dtype=np.uint8),
            "line_off": off, "chrom_len": np.full(loci, 4, dtype=np.int32)}


def emit(out, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    with open(out, "a") as f:
        f.write(line + "\n")


def bench_shape(eng, n, L, rounds, threads, out):
    rows = synthetic_rows(n, L)
    keys = ("counts", "pos", "ref", "line_off", "chrom_len")
    dev = {k: torch.from_numpy(rows[k].view(np.int32) if k == "counts" else rows[k].view(np.int64) if k == "pos" else rows[k]).cuda() for k in keys}
    slab = torch.from_numpy(rows["slab"]).cuda()
    pin = {k: torch.empty(dev[k].shape, dtype=dev[k].dtype).pin_memory() for k in keys}
    need = C.c_int64()

    def call(buf, cap):
        return eng._lib.pg_sync_format_rows_dev(eng._ctx, slab.data_ptr(), slab.numel(), dev["counts"].data_ptr(), dev["pos"].data_ptr(),
                                                dev["ref"].data_ptr(), dev["line_off"].data_ptr(), dev["chrom_len"].data_ptr(), n, L, buf, cap,
                                                C.byref(need))

    call(None, 0)
    size = need.value
    text_dev = torch.empty(size, dtype=torch.uint8, device="cuda")
    copy_dev = torch.empty(size, dtype=torch.uint8, device="cuda")
    text_pin = torch.empty(size, dtype=torch.uint8).pin_memory()
    text_host = np.empty(size, dtype=np.uint8)
    rows_bytes = sum(dev[k].numel() * dev[k].element_size() for k in keys)

    def format_dev():
        eng.profile_reset()
        if call(text_dev.data_ptr(), size) != 0:
            sys.exit("bench_syncwrite: pg_sync_format_rows_dev failed")
        return eng.profile_get("syncfmt")[0] * 1e-3

    def d2d_copy():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        copy_dev.copy_(text_dev)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e-3

    def format_dev_d2h():
        t0 = time.perf_counter()
        if call(text_dev.data_ptr(), size) != 0:
            sys.exit("bench_syncwrite: pg_sync_format_rows_dev failed")
        text_pin.copy_(text_dev, non_blocking=True)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def format_host_d2h():
        t0 = time.perf_counter()
        for k in keys:
            pin[k].copy_(dev[k], non_blocking=True)
        torch.cuda.synchronize()
        h = {k: pin[k].numpy() for k in keys}
        got = C.c_int64()
        rc = eng._lib.pg_host_sync_format_rows(rows["slab"].ctypes.data, rows["slab"].size, h["counts"].ctypes.data, h["pos"].ctypes.data,
                                               h["ref"].ctypes.data, h["line_off"].ctypes.data, h["chrom_len"].ctypes.data, n, L,
                                               text_host.ctypes.data, size, C.byref(got), threads)
        if rc != 0 or got.value != size:
            sys.exit("bench_syncwrite: pg_host_sync_format_rows failed")
        return time.perf_counter() - t0

    legs = {"format_dev": format_dev, "d2d_copy": d2d_copy, "format_dev_d2h": format_dev_d2h, "format_host_d2h": format_host_d2h}
    eng.profile(True)
    for fn in legs.values():                                  # warm-up of each
        fn()
    if not np.array_equal(text_pin.numpy(), text_host):
        sys.exit("bench_syncwrite: the device's text and the host's differ")
    t = {k: [] for k in legs}
    for _ in range(rounds):                                   # alternating: the legs see the same neighbours on the machine
        for k, fn in legs.items():
            t[k].append(fn())
    eng.profile(False)
    med = {k: statistics.median(v) for k, v in t.items()}
    common = {"pools": n, "loci": L, "text_bytes": int(size), "rows_bytes": int(rows_bytes), "host_threads": threads}
    for k, v in t.items():
        rec = {"op": "syncwrite_" + k, **common, "rounds": len(v), "ms": med[k] * 1e3, "ms_min": min(v) * 1e3, "ms_max": max(v) * 1e3,
               "text_bytes_per_s": size / med[k]}
        if k == "format_dev":
            rec["frac_of_hbm_peak_useful_bytes"] = (rows_bytes + size) / med[k] / HBM_PEAK
            rec["times_the_d2d_copy"] = med[k] / med["d2d_copy"]
            rec["mean_row_bytes"] = size / L
        if k == "format_dev_d2h":
            rec["speedup_over_format_host_d2h"] = med["format_host_d2h"] / med[k]
        emit(out, rec)


def bench_cli(name, args_of_writer, file_bytes, rounds, out, common):
    """args_of_writer: label -> the command line; alternating runs, the median wall clock of each"""
    env = dict(os.environ, PGH_TIMING="1")
    t = {k: [] for k in args_of_writer}
    laps, sizes = {}, {}
    for r in range(rounds):
        print(f"bench_syncwrite: {name}, round {r + 1} of {rounds}", file=sys.stderr, flush=True)
        for k, (cmd, o) in args_of_writer.items():
            t0 = time.perf_counter()
            p = subprocess.run(cmd, capture_output=True, text=True, env=env)
            t[k].append(time.perf_counter() - t0)
            if p.returncode != 0:
                sys.exit(f"bench_syncwrite: {name} {k} failed: {p.stderr}")
            laps[k] = p.stderr
            sizes[k] = o.stat().st_size
            o.unlink()
    if len(set(sizes.values())) != 1:
        sys.exit(f"bench_syncwrite: the outputs differ in size: {sizes}")
    med = {k: statistics.median(v) for k, v in t.items()}
    for k, v in t.items():
        rec = {"op": f"syncwrite_cli_{name}_{k}", **common, "input_bytes": int(file_bytes), "output_bytes": int(sizes[k]), "rounds": len(v),
               "ms": med[k] * 1e3, "ms_min": min(v) * 1e3, "ms_max": max(v) * 1e3}
        if k != "host":
            rec["speedup_over_host"] = med["host"] / med[k]
        emit(out, rec)
    for k in t:
        print(f"---- phases of the last run: {name} {k}\n{laps[k]}", file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="200x500000,5x10000000,4096x10000", help="pools x loci, comma-separated; empty: none")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--cli-rounds", type=int, default=7)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--cli", default="vcf,pileup", help="the conversions to run through the CLI; empty: none")
    ap.add_argument("--parent-cli", default="", help="the poolgen binary of the parent commit: its vcf2sync is run too")
    ap.add_argument("--vcf-loci", type=int, default=500_000)
    ap.add_argument("--pileup-shape", default="200x30x20000", help="pools x depth x loci of the pileup file")
    ap.add_argument("--dir", default=tempfile.gettempdir())
    ap.add_argument("--out", default=str(ROOT / "profiles" / "syncwrite_ops.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_syncwrite: no GPU (a time from a CPU would say nothing)")
    eng = Engine(0)
    for shape in filter(None, a.shapes.split(",")):
        n, L = map(int, shape.split("x"))
        bench_shape(eng, n, L, a.rounds, a.threads, a.out)
        torch.cuda.empty_cache()
    eng.close()
    which = set(filter(None, a.cli.split(",")))
    if not which:
        return
    work = Path(tempfile.mkdtemp(prefix="bench_syncwrite_", dir=a.dir))
    rng = np.random.default_rng(2)
    if "vcf" in which:
        from bench_vcf import synthetic_vcf
        n = 200
        text = synthetic_vcf(a.vcf_loci, n)
        vcf, phen = work / "synthetic.vcf", work / "phen.csv"
        text.tofile(vcf)
        phen.write_text("#pop,size,trait\n" + "".join(f"Pool{i},20.0,{rng.random():.6f}\n" for i in range(n)))
        runs = {}
        for k, exe, extra in (("host", CLI, ["--sync-writer", "host"]), ("gpu", CLI, ["--sync-writer", "gpu"]), ("parent", a.parent_cli, [])):
            if exe:
                o = work / f"vcf2sync_{k}.sync"
                runs[k] = ([str(exe), "vcf2sync", "-f", str(vcf), "-p", str(phen), "-o", str(o), "--n-threads", str(a.threads), *extra], o)
        bench_cli("vcf2sync", runs, text.size, a.cli_rounds, a.out, {"pools": n, "loci": a.vcf_loci, "host_threads": a.threads})
        vcf.unlink(); phen.unlink()
        del text
    if "pileup" in which:
        from bench_pileup import synthetic_pileup
        n, depth, L = map(int, a.pileup_shape.split("x"))
        text, _ = synthetic_pileup(L, n, depth)
        pileup, phen = work / "synthetic.pileup", work / "phen.csv"
        text.tofile(pileup)
        phen.write_text("#pop,size,trait\n" + "".join(f"Pool{i},20.0,{rng.random():.6f}\n" for i in range(n)))
        runs = {}
        for k in ("host", "gpu"):
            o = work / f"pileup2sync_{k}.sync"
            runs[k] = ([str(CLI), "pileup2sync", "-f", str(pileup), "-p", str(phen), "-o", str(o), "--n-threads", str(a.threads),
                        "--min-allele-frequency", "0.0", "--pileup-parser", "gpu", "--sync-writer", k], o)
        bench_cli("pileup2sync", runs, text.size, a.cli_rounds, a.out, {"pools": n, "depth": depth, "loci": L, "host_threads": a.threads})
        pileup.unlink(); phen.unlink()
    os.rmdir(work)


if __name__ == "__main__":
    main()
